"""Reference and fixtures of tests/test_gpu_ema.py and tests/test_ema_host.py (not a test): the averaged weights' recurrence in
float64 with a derived rounding bound, and a module whose parameter tensors straddle the optimizer kernel's 1024-element chunks in
every way (next to ``grad_guard_ref.small_module``)."""
import numpy as np
import torch

U = 2.0 ** -24                                                     # the unit roundoff of fp32 (round to nearest)
ODD_SIZES = (1, 3, 1023, 1025, 2049)                               # offsets 0, 1, 4, 1027, 2052 | total 4101: every chunk boundary (1024, 2048,
ODD_TOTAL = sum(ODD_SIZES)                                         # 3072, 4096) inside a tensor, every tensor boundary inside a chunk


def ema_recurrence(p_seq, e0, decay):
    """The averaged weights after the parameter vectors ``p_seq`` (the ones the kernel itself produced, fp32), from ``e0``, in float64:

        e <- e + omd * (p - e),   omd = fl32(1 - decay)            (the kernel's own rounded coefficient, exact in float64)

    -> (e, b), float64 arrays: the reference and an element-wise bound on |kernel's ema - e|.

    The bound.  The kernel computes, in fp32, d = fl(p - e~) and e~' = fl(omd * d + e~) -- one explicit fma, so two roundings a step:
    d = (p - e~)(1 + d1), e~' = (e~ + omd * d)(1 + d2), |d1|, |d2| <= 2^-24.  With err = e~ - e and decay_f = 1 - omd,

        err' = decay_f * err  +  omd * (p - e~) * d1  +  d2 * (e~ + omd * d)

    so   |err'| <= decay_f * |err| + 2^-24 * omd * |p - e~| + 2^-24 * |e~'| / (1 - 2^-24).  The previous error is carried by the
    factor decay_f < 1: it is damped, never amplified.  The right-hand side is evaluated on the REFERENCE's values (e for e~); what
    that neglects is of second order -- 2^-24 * (|err'| + omd * |err|) -- and is covered, with the float64 roundings of this function
    (2^-53 relative), by one further 2^-24 * |e'|:

        b <- decay_f * b + 2^-24 * (|e'| + omd * |p - e|) + 2^-24 * |e'|

    i.e. one rounding of the difference scaled by omd, one rounding of the fma, and one rounding for the carrier of the previous
    error, damped by the decay.  Derived from the two roundings of the kernel's expression, not measured.  A constant sequence
    p = e0 gives e = e0 exactly (p - e is 0) and b -> 2^-23 |e0| (1 - decay_f^k) / omd."""
    omd = float(np.float32(1.0 - float(decay)))
    decay_f = 1.0 - omd
    e = np.asarray(e0, dtype=np.float64).copy()
    b = np.zeros_like(e)
    for p in p_seq:
        p = np.asarray(p, dtype=np.float64)
        diff = p - e
        e = e + omd * diff
        b = decay_f * b + U * (np.abs(e) + omd * np.abs(diff)) + U * np.abs(e)
    return e, b


class OddShapes(torch.nn.Module):
    """Five parameter vectors of ODD_SIZES elements; only the optimizer ever looks at them."""

    def __init__(self):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n)) for n in ODD_SIZES])


def odd_module(dev):
    torch.manual_seed(5)
    return OddShapes().to(dev)


def modules(dev):
    """name -> a fresh copy of the two small modules."""
    import grad_guard_ref as G
    return {"odd": odd_module(dev), "small": G.small_module(dev)}


def gradients(total, steps, seed, scale=1.0):
    """`steps` seeded fp32 gradient vectors of `total` elements (CPU), magnitudes over four decades."""
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(total, generator=g) * 10.0 ** (torch.rand(total, generator=g) * 4.0 - 3.0)).float() for _ in range(steps)]
