"""CPU: pins tests/setconv_ref.py, the plain reference tests/test_gpu_setconv_chain.py judges the register-chain kernels by.

* Against oracle.cmflow_oracle.PointLocalFeature (the reference's op sequence: query_and_group, concat, six Conv2d + BatchNorm2d +
  ReLU, max) in eval mode with the same weights and the oracle's ball query, outputs and every gradient, in fp64 and in fp32 -- so
  the reference is anchored to something that is neither a kernel nor itself.
* The preconditions of the GPU cases: for every small case and its fixed seed the fp32 and the fp64 evaluation of the reference
  take the same side of every ReLU and select the same source point at every max, and no BatchNorm output of the three slot-level
  layers lies within 1e-5 of its ReLU's kink -- so a gradient difference on the GPU is a rounding difference, not another branch."""
import pytest
import torch

from oracle import cmflow_oracle as O, ops
from setconv_chain_case import (DEAD_CHANNELS, EDGE, INFER, LARGE, PER_LAYER_UNDER_GRAD, SMALL, TRAIN, Yardstick, block_grads,
                                block_params, blocks_per_wave, init_block, make_inputs, walk, MLP, MLP2)
from setconv_ref import max_err, set_conv_ref, ulp32


@pytest.fixture
def generic_ops(monkeypatch):
    """The oracle's grouping runs in C on fp32; fp64 tensors take torch.gather / scatter_add (same definition), the ball query
    always sees the fp32 coordinates (tests/grad_noise_floor.py does the same)."""
    bq0, gp0, gpg0 = ops.ball_query, ops.group_points, ops.group_points_grad

    def gp(points, idx):
        if points.dtype == torch.float32:
            return gp0(points, idx)
        B, C, N = points.shape
        _, P, S = idx.shape
        return torch.gather(points, 2, idx.long().view(B, 1, P * S).expand(-1, C, -1)).view(B, C, P, S)

    def gpg(go, idx, N):
        if go.dtype == torch.float32:
            return gpg0(go, idx, N)
        B, C, P, S = go.shape
        out = torch.zeros(B, C, N, dtype=go.dtype)
        return out.scatter_add_(2, idx.long().view(B, 1, P * S).expand(-1, C, -1), go.reshape(B, C, P * S))

    monkeypatch.setattr(ops, "ball_query", lambda r, ns, xyz, new: bq0(r, ns, xyz.float(), new.float()))
    monkeypatch.setattr(ops, "group_points", gp)
    monkeypatch.setattr(ops, "group_points_grad", gpg)


@pytest.mark.parametrize("B,N,S,radius", [(3, 40, 8, 4.0), (2, 24, 16, 2.0), (2, 16, 4, 50.0)])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-5)])
def test_reference_equals_the_oracle_block(generic_ops, B, N, S, radius, dtype, tol):
    """Bounds, as a fraction of each tensor's largest entry: fp64 1e-12 (both sides fp64, sums of <= 64 + S N terms: ~1e-15 with three
    decades to spare); fp32 2e-5 -- two fp32 evaluations of one function that order their sums differently (the oracle convolves
    the concatenated 6 channels, the reference adds the hoisted halves; BatchNorm folded or not): tests/grad_noise_floor.py
    measures 1e-4 .. 1e-3 for whole-model gradients, one block of six layers sits a decade below, and a transcription error (a
    swapped channel, a wrong neighbour, eps left out: 1e-5 of var ~ 1, i.e. 5e-6 of every activation, summed coherently) does not."""
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + S)
    mod = init_block(O.PointLocalFeature(radius, S, in_channel=3, mlp=MLP, mlp2=MLP2), g).to(dtype)
    xyz = torch.rand(B, N, 3, generator=g) * torch.tensor([12.0, 12.0, 2.0])
    feats = torch.randn(B, N, 3, generator=g)
    dout = torch.randn(B, N, 64, generator=g).to(dtype)
    mod.trace = []
    pts = feats.to(dtype).transpose(1, 2).contiguous().requires_grad_(True)
    out = mod(xyz.to(dtype).transpose(1, 2).contiguous(), pts)                      # (B,64,N)
    out.backward(dout.transpose(1, 2))
    idx = mod.trace[0]
    assert idx.shape == (B, N, S)

    params, buffers = block_params(mod)
    wf = mod.mlp_convs[0].weight.detach().view(32, 6)[:, 3:]
    ref = set_conv_ref(xyz, feats.to(dtype) @ wf.t(), idx, params, buffers, dtype)
    grads = ref.grads(dout)
    def close(a, b, what):
        a, b = a.detach(), b.detach()
        err, top = float((a - b).abs().max()), float(b.abs().max())
        assert err <= tol * top, "%s: %.3g of %.3g" % (what, err, top)
    close(ref.out, out.detach().transpose(1, 2), "out")
    dy = grads[0]
    close(dy @ wf, pts.grad.transpose(1, 2), "d feats")                             # y = feats Wf^T: the chain rule by hand
    w1g = mod.mlp_convs[0].weight.grad.view(32, 6)
    close(torch.einsum("bno,bnc->oc", dy, feats.to(dtype)), w1g[:, 3:], "d Wf")
    for name, a, b in zip(["wx"] + [None] * 17, grads[1:], block_grads(mod)):
        close(a, b, name or "param")
    assert len(grads) == 19


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_small_cases_are_flip_free_between_fp32_and_fp64(case):
    mod, xyz, y, dout = make_inputs(case, O.PointLocalFeature)
    idx = ops.ball_query(case.radius, case.S, xyz, xyz)
    params, buffers = block_params(mod)
    yd = Yardstick(case, xyz, y, idx, dout, params, buffers)
    flips = sum(int((a != b).sum()) for a, b in zip(yd.r32.masks(), yd.r64.masks()))
    moved = int((yd.r32.argmax_src != yd.r64.argmax_src).sum())
    min_u = min(float(u.detach().abs().min()) for u in yd.r64.u[:3])
    g_rel = max(e / float(r.abs().max()) for e, r in zip(yd.g_yard, yd.g64) if float(r.abs().max()) > 0)
    print("%-16s rows %5d  flips %d  argmax moved %d  min|u| %.2g  fp32 out err %.2g  grad err / max %.2g"
          % (case.name, case.B * case.N * case.S, flips, moved, min_u, yd.out_yard, g_rel))
    assert flips == 0 and moved == 0
    assert min_u >= 1e-5
    if case.radius < 0.1:                                   # every ball holds its centre only: all slots repeat it
        assert bool((idx == torch.arange(case.N, dtype=idx.dtype).view(1, case.N, 1)).all())
        assert float(yd.g64[1].abs().max()) == 0.0          # d Wx: the offsets are exactly zero
    if case.radius > 20:
        assert all(len(set(row.tolist())) == min(case.S, case.N) for row in idx.view(-1, case.S))       # every ball is full
    if case.dead:
        assert float(yd.r64.u[2].detach()[..., DEAD_CHANNELS].max()) < -50.0
        assert float(yd.g64[7][DEAD_CHANNELS].abs().max()) == 0.0 and float(yd.g32[7][DEAD_CHANNELS].abs().max()) == 0.0


def test_case_table_reaches_what_it_is_meant_to():
    """The block-walk arithmetic behind the shapes (csrc/setconv_chain.hip: a wave walks max(4, min(16 | 32, ceil(blocks / 3072 | 2048)))
    blocks of 32 rows, four waves per workgroup): computed, so that a change of the table cannot silently move a case."""
    by = {c.name: c for c in INFER}
    assert walk(by["1x8x4"], False) == (1, 4, 1, 1, 1, 1)                    # one block; waves 1-3 of the workgroup idle
    assert [walk(by[n], False)[3] for n in ("5x8x4", "3x16x4", "7x8x4")] == [1, 2, 3]       # the prefetch tails
    assert all(c.N * c.S == 32 for c in (by["5x8x4"], by["7x8x4"], by["1x8x4"]))             # a sample boundary at every block
    assert sorted({c.S for c in INFER}) == [4, 8, 16, 32]
    assert walk(by["17x8x32"], False)[4:] == (9, 2)                          # nine workgroups, two working waves in the last
    assert all((c.B * c.N * c.S) % 128 == 0 for c in TRAIN + EDGE) and (PER_LAYER_UNDER_GRAD.B * 8 * 4) % 128 != 0
    assert walk(LARGE, True) == (8448, 5, 1690, 3, 423, 2)                   # backward: five blocks per wave, tail of three
    assert blocks_per_wave(8192, True) == 4 and blocks_per_wave(8193, True) == 5
    assert ulp32(1.0) == 2.0 ** -23 and ulp32(3.9) == 2.0 ** -22 and ulp32(0.0) == 0.0
