"""An independent fp64 statement of cmf_gemm, written from the contract in include/cmflow_hip.h (the cmf_gemm comment) in plain
torch, usable on the CPU and on the GPU.  tests/test_gemm_ref_host.py pins it against torch.nn.functional and autograd;
tests/test_gpu_gemm_matrix.py judges the HIP kernel by it.

Operands are the LOGICAL matrices A (M,K) and B (K,N): storage layout (a_t / b_t, row strides) is the caller's business.

    A' = relu(pro_a[k] * A + pro_c[k])          B' = relu(prob_a[n] * B + prob_c[n])          acc = A' @ B'
    forward:   C = act(acc + bias[n])                         act: 0 none / 1 relu / 2 leaky(0.1) / 3 sigmoid
    mode 1:    C = acc * [ea[n] * Z + ec[n] > 0]              mode 2: C = acc * (Z > 0 ? 1 : 0.1)      mode 3: C = acc * [Z > 0]
    prior:     C = prior + C                                  (the `accumulate` flag)

Mask predicates are evaluated exactly as written (strict `>`: an exact zero is masked / takes the 0.1 slope).  Fed with the
grid-valued inputs of grid() below, ea * Z + ec is exact in fp32 as well (fused or not), so fp32 and fp64 decide every element alike
and a comparison never has to exclude one.
"""
import types

import torch

EPS32 = 2.0 ** -24                                # unit roundoff of fp32 (round to nearest)


def grid(shape, lo, hi, gen, device="cpu"):
    """Multiples of 1/4 in [lo, hi], uniformly, as float32 (exactly representable; exact zeros where lo <= 0 <= hi)."""
    q = torch.randint(int(round(lo * 4)), int(round(hi * 4)) + 1, tuple(shape), generator=gen)
    return (q.to(torch.float32) / 4).to(device)


def _d(t):
    return None if t is None else t.double()


def gemm_ref(A, B, pro=None, prob=None, bias=None, act=0, bwd=None, dxyz=None, prior=None):
    """Returns a namespace, everything float64:
      C       (M,N)  the result
      P       (M,N)  |A'| @ |B'| (+ |prior|): the magnitude the accumulation error of an element scales with
      factor  (M,N)  what the epilogue multiplies the accumulator by: the mask, the slope, or the activation's Lipschitz constant
      terms   list of (M,N) per-row terms of the statistics sums (2, or 5 with dxyz); an entry is None where the contract leaves
              the row unspecified (row 1 of modes 2 / 3).  Sum them over any row range.
      gains   list like terms: |d term / d C| per element (the square's 2|x| is its first-order gain)
    bwd = (mode, Z, ea, ec, mean, invstd); modes 2 / 3 read only Z."""
    A, B = _d(A), _d(B)
    if pro is not None:
        A = torch.relu(_d(pro[0])[None, :] * A + _d(pro[1])[None, :])
    if prob is not None:
        B = torch.relu(_d(prob[0])[None, :] * B + _d(prob[1])[None, :])
    acc = A @ B
    P = A.abs() @ B.abs()
    one = torch.ones_like(acc)
    mode = bwd[0] if bwd is not None else 0
    if mode == 0:
        pre = acc if bias is None else acc + _d(bias)[None, :]
        if act == 0:
            C, factor = pre, one
        elif act == 1:
            C, factor = torch.where(pre > 0, pre, torch.zeros_like(pre)), one
        elif act == 2:
            C, factor = torch.where(pre > 0, pre, 0.1 * pre), one
        elif act == 3:
            C, factor = 1.0 / (1.0 + torch.exp(-pre)), 0.25 * one
        else:
            raise ValueError(act)
        terms, gains = [C, C * C], [one, 2 * C.abs()]
    else:
        assert bias is None and act == 0
        Z = _d(bwd[1])
        if mode == 1:
            ea, ec, mean, invstd = (_d(t) for t in bwd[2:6])
            factor = ((ea[None, :] * Z + ec[None, :]) > 0).double()
            zhat = (Z - mean[None, :]) * invstd[None, :]
            C = acc * factor
            terms, gains = [C, C * zhat], [one, zhat.abs()]
        elif mode in (2, 3):
            factor = torch.where(Z > 0, one, (0.1 if mode == 2 else 0.0) * one)
            C = acc * factor
            terms, gains = [C, None], [one, None]
        else:
            raise ValueError(mode)
        if dxyz is not None:
            d = _d(dxyz)
            for k in range(3):
                terms.append(C * d[:, k:k + 1])
                gains.append(d[:, k:k + 1].abs().expand_as(C))
    if prior is not None:
        C = _d(prior) + C
        P = P + _d(prior).abs()
    return types.SimpleNamespace(C=C, P=P, factor=factor, terms=terms, gains=gains, act=act, mode=mode)


def elem_bound(ref, tol):
    """|C - C_ref| <= factor * (tol * P + 1e-6).  Sigmoid: 2e-5 * (1 + |C_ref|), the project's rtol = atol for it (__expf has
    no derivable bound)."""
    if ref.mode == 0 and ref.act == 3:
        return 2e-5 * (1.0 + ref.C.abs())
    return ref.factor * (tol * ref.P + 1e-6)


def stat_bound(ref, which, tol, rows):
    """Per-element share of the bound of statistics sum `which` for a partial covering `rows` rows: sum the result over the same
    rows as the term.  = propagated element bound + (rows + 3) * 2^-24 * |term| (sequential fp32 summation, and the up to three
    roundings that form the term)."""
    eb = elem_bound(ref, tol)
    prop = eb * ref.gains[which]
    if ref.mode == 0 and which == 1:
        prop = prop + eb * eb                      # (x + e)^2 - x^2 = 2 x e + e^2
    return prop + (rows + 3) * EPS32 * ref.terms[which].abs()
