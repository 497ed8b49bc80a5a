"""GPU: the register-chain set-conv kernels (csrc/setconv_chain.hip: CH_INFER, CH_POOL, CH_BWD3, CH_BWD2 and the batched inference
launch) operator by operator -- one PointLocalFeature(3 + 3 -> 32 -> 32 -> 64 | 64 -> 64 -> 64) in eval mode driven through
fused_blocks.set_conv -- against (a) the per-layer kernels sequenced from Python (FB.USE_BLOCK_CALLS = False: SetConvFn, which never
takes the chain) and (b) tests/setconv_ref.py in fp64 on the neighbour lists of the product's own ball query (bit-exact against the
oracle in test_gpu_ops.py).  Every case asserts through cmf_setconv_path which kernels its descriptor took.  Shapes and seeds:
tests/setconv_chain_case.py; their preconditions (no ReLU or argmax decided differently by fp32 and fp64) are asserted on the CPU by
tests/test_setconv_ref.py.

Bounds (nothing is derived from a kernel's output).  Forward against (a): equality, bit for bit.  Against fp64, per tensor:
    max |kernel - fp64|  <=  4 x max |plain fp32 torch evaluation of the same reference - fp64|  +  ulp32(largest |entry|),
the yardstick computed here on the CPU for the case's own inputs (setconv_chain_case.Yardstick): the kernels sum the same rounding
population in another order (k pairs per MFMA step, per-wave statistics rows, per-workgroup slabs).  The issue states the small
cases' metrics as "elementwise for the output, max-abs over the tensor's max-abs for gradients": both are the largest elementwise
error of the tensor (dividing both sides by the tensor's largest entry changes nothing).  The large case compares 2-norms,
||kernel - fp64|| <= 4 ||fp32 - fp64|| + ulp32(largest |entry|) sqrt(numel): at 35 M activations fp32 and fp64 do not agree on
every mask, so single elements differ by whole terms on either side.  Backward against (a): the sum of both sides' allowances
(the large case: in the 2-norm and, because both sides share their masks, element by element as well).

Every test prints, per case and tensor, the fp32 yardstick, the kernel's error and the allowance (pytest -s).  Worst figures measured
on an MI355X (also in DESIGN.md "Register-chain tests", with the mutations these tests were tried against):
    small cases   output     fp32 yardstick 1.97e-6 absolute, kernel 1.24e-6, <= 0.35 of the allowance
                  gradients  (of each tensor's largest entry) yardstick 7e-8 .. 5.8e-7, chain 4.8e-7, per-layer 4.8e-7, <= 0.42 of the
                             allowance; chain - per-layer 2.9e-7, <= 0.17 of its allowance
    large case    output     yardstick 1.42e-6, kernel 1.28e-6, 0.22 of the allowance
                  gradients  (norm-relative) yardstick 1.0e-7 .. 8.1e-5 (2e-5 and more below the ReLUs whose masks fp32 and fp64 decide
                             differently), chain 1.0e-7 .. 2.5e-7, per-layer 2.5e-7, <= 0.22 of the allowance; chain - per-layer 2.3e-7
                             (0.05), element by element 4.4e-7 of the largest entry (0.08)
"""
import ctypes

import pytest
import torch

from setconv_chain_case import (DEAD_CHANNELS, EDGE, INFER, LARGE, MLP, MLP2, PER_LAYER_UNDER_GRAD, TRAIN, Yardstick, block_grads,
                                block_params, init_block, make_inputs, walk)
from setconv_ref import max_err, ulp32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _path(desc):
    from cmflow_amd import _lib
    return _lib.lib().cmf_setconv_path(ctypes.addressof(desc))


@pytest.fixture
def paths(monkeypatch):
    """The cmf_setconv_path of every descriptor fused_blocks hands to cmf_setconv_forward while the test runs."""
    from cmflow_amd import fused_blocks as FB
    seen, real = [], FB._block_forward

    def tap(*a, **k):
        out, state = real(*a, **k)
        seen.append(_path(state["desc"]))
        return out, state
    monkeypatch.setattr(FB, "_block_forward", tap)
    return seen


def _run(case, dev, monkeypatch, block, grad):
    """One set_conv call (+ one backward) on the case's inputs -> (out, [dy, 18 parameter gradients] or None, ball-query indices)."""
    from cmflow_amd import fused_blocks as FB, pointnet2_utils as pointutils
    from cmflow_amd.radarflow_util import PointLocalFeature
    monkeypatch.setattr(FB, "USE_BLOCK_CALLS", block)
    mod, xyz, y, dout = make_inputs(case, PointLocalFeature)
    mod, xyz = mod.to(dev), xyz.to(dev)
    base = (y._base if case.sliced else y).to(dev).requires_grad_(grad)
    view = lambda t: t[:, :, 32:64] if case.sliced else t
    assert view(base).stride(1) == (128 if case.sliced else 32)
    with torch.set_grad_enabled(grad):
        out = FB.set_conv(mod, xyz, view(base))
    grads = None
    if grad:
        out.backward(dout.to(dev))
        grads = [view(base.grad)] + block_grads(mod)
    torch.cuda.synchronize()
    idx = pointutils.ball_query(case.radius, case.S, xyz, xyz)
    return out.detach(), grads, idx


_YARDS = {}


def _yard(case, idx, backward):
    """The case's references (computed once, shared by the tests that use the case)."""
    from cmflow_amd.radarflow_util import PointLocalFeature
    key = (case.name, backward)
    if key not in _YARDS:
        mod, xyz, y, dout = make_inputs(case, PointLocalFeature)
        params, buffers = block_params(mod)
        _YARDS[key] = Yardstick(case, xyz, y, idx.cpu(), dout, params, buffers, backward=backward)
    return _YARDS[key]


def _check_forward(case, yd, chain, layer):
    assert torch.equal(chain, layer), "%s: the chain's output is not bit-identical to the per-layer kernels' (%.3g)" % (
        case.name, float((chain - layer).abs().max()))
    err, allow = max_err(chain, yd.out), yd.out_allowance()
    print("%-16s out        fp32 yardstick %.3g  kernel %.3g  allowance %.3g  ratio %.2f" % (case.name, yd.out_yard, err, allow, err / allow))
    assert err <= allow, "%s: out %.3g > %.3g" % (case.name, err, allow)


def _check_backward(case, yd, chain, layer):
    bad = []
    for k, name in enumerate(yd.names):
        allow = yd.grad_allowance(k)
        top = float(yd.g64[k].abs().max())
        e64, epl = max_err(chain[k], yd.g64[k]), max_err(chain[k], layer[k])
        el64 = max_err(layer[k], yd.g64[k])
        print("%-16s %-3s max %.3g  fp32 yardstick %.3g  chain %.3g  per-layer %.3g  allowance %.3g  ratio %.2f | chain - per-layer %.3g ratio %.2f"
              % (case.name, name, top, yd.g_yard[k], e64, el64, allow, e64 / allow if allow else float(e64 > 0),
                 epl, epl / (2 * allow) if allow else float(epl > 0)))
        if not (e64 <= allow and epl <= 2 * allow):
            bad.append((name, e64, epl, allow))
    assert not bad, "%s: (gradient, error against fp64, against the per-layer kernels, allowance) %s" % (case.name, bad)


@pytest.mark.parametrize("case", INFER, ids=lambda c: c.name)
def test_inference_forward(dev, monkeypatch, paths, case):
    """CH_INFER (no_grad: path 1) -- prefetch tails of one, two and three blocks, idle waves, a sample boundary at every block, every S,
    more than one workgroup, and a y operand with row pitch 128."""
    chain, _, idx = _run(case, dev, monkeypatch, True, False)
    assert paths == [1]
    layer, _, _ = _run(case, dev, monkeypatch, False, False)
    assert paths == [1]                                     # (the comparator never reaches a block call)
    _check_forward(case, _yard(case, idx, False), chain, layer)


@pytest.mark.parametrize("case", TRAIN + EDGE, ids=lambda c: c.name)
def test_training_forward_and_backward(dev, monkeypatch, paths, case):
    """CH_POOL, CH_BWD3, CH_BWD2 (grad enabled, M a multiple of 128: path 2): the output, dy and the 18 parameter gradients of one
    backward call with a random dout -- dWx from the three dxyz sums, dW2 / dW3 from the per-workgroup slabs, the BN 0 / BN 1
    gradients from the per-wave statistics rows.  Edge inputs: radius 0.01 (every ball repeats its centre: all slots tied, offsets
    and dWx exactly zero), radius 50 (every ball full), BN 2 bias -100 on eight channels (pooled output exactly 0 there, nothing
    flows back).  Tied slots repeat one source point, so every observable is independent of the slot chosen."""
    chain, gchain, idx = _run(case, dev, monkeypatch, True, True)
    assert paths == [2]
    layer, glayer, _ = _run(case, dev, monkeypatch, False, True)
    assert paths == [2]
    yd = _yard(case, idx, True)
    _check_forward(case, yd, chain, layer)
    _check_backward(case, yd, gchain, glayer)
    if case.radius < 0.1:
        assert bool((idx.cpu() == torch.arange(case.N, dtype=idx.dtype).view(1, case.N, 1)).all())
        assert float(gchain[1].abs().max()) == 0.0          # dWx = sum dU1 (x) (xyz[src] - xyz[centre]) with every offset zero
    if case.dead:
        g = dict(zip(yd.names, gchain))
        assert float(g["w3"][DEAD_CHANNELS].abs().max()) == 0.0 and float(g["g3"][DEAD_CHANNELS].abs().max()) == 0.0 \
            and float(g["b3"][DEAD_CHANNELS].abs().max()) == 0.0
        assert float(g["w4"][:, DEAD_CHANNELS].abs().max()) == 0.0          # the pooled rows are exactly zero on those channels


def test_rows_not_a_multiple_of_128_take_the_per_layer_kernels_under_grad(dev, monkeypatch, paths):
    """160 rows with a backward call to follow: the chain's statistics rows want whole 128-row tiles, so the block call must say
    path 0 -- and still be right."""
    case = PER_LAYER_UNDER_GRAD
    block, gblock, idx = _run(case, dev, monkeypatch, True, True)
    assert paths == [0]
    layer, glayer, _ = _run(case, dev, monkeypatch, False, True)
    yd = _yard(case, idx, True)
    _check_forward(case, yd, block, layer)
    _check_backward(case, yd, gblock, glayer)


def test_backward_with_more_than_four_blocks_per_wave(dev, monkeypatch, paths):
    """(33, 256, 32): 8448 blocks -- from 8193 on the backward passes walk more than four blocks per wave (the benchmark's B = 64 does;
    nothing compared it with anything).  Here five, the last wave three, the last workgroup half idle.  Masks cannot be flip-free
    between fp32 and fp64 at 35 M activations, so elements are compared with the per-layer kernels (same masks: the forward is
    bit-identical) and with fp64 in the 2-norm."""
    case = LARGE
    blocks, bpw, waves, last, groups, last_waves = walk(case, True)
    assert blocks > 8192 and bpw == 5 and last == 3 and 0 < last_waves < 4
    chain, gchain, idx = _run(case, dev, monkeypatch, True, True)
    assert paths == [2]
    layer, glayer, _ = _run(case, dev, monkeypatch, False, True)
    yd = _yard(case, idx, True)
    _check_forward(case, yd, chain, layer)
    norm = lambda a, b: float((a.detach().cpu().double() - b.detach().cpu().double()).norm())
    bad = []
    for k, name in enumerate(yd.names):
        r = yd.g64[k]
        allow = 4.0 * norm(yd.g32[k], r) + ulp32(r.abs().max()) * r.numel() ** 0.5
        e64, epl, rn = norm(gchain[k], r), norm(gchain[k], glayer[k]), float(r.norm())
        # chain and per-layer kernels share their masks, so they are also compared element by element, as in the small cases
        eel, allow_el, top = max_err(gchain[k], glayer[k]), 2 * yd.grad_allowance(k), float(r.abs().max())
        print("%-16s %-3s |ref| %.3g  fp32 yardstick %.3g  chain %.3g  per-layer %.3g  ratio %.2f | chain - per-layer %.3g ratio %.2f  (norm-relative)"
              " | elementwise / max %.3g: fp32 yardstick %.3g  chain - per-layer %.3g ratio %.2f"
              % (case.name, name, rn, norm(yd.g32[k], r) / rn, e64 / rn, norm(glayer[k], r) / rn, e64 / allow, epl / rn, epl / (2 * allow),
                 top, yd.g_yard[k] / top, eel / top, eel / allow_el))
        if not (e64 <= allow and epl <= 2 * allow and eel <= allow_el):
            bad.append((name, e64 / rn, epl / rn, allow / rn, eel, allow_el))
    assert not bad, bad


def test_batched_inference_launch(dev, monkeypatch):
    """cmf_setconv_chain_infer_batch: the four scales of a MultiScaleEncoder (radii 2 / 4 / 8 / 16, S = 4 / 8 / 16 / 32: four grids of
    different sizes in one launch) through multi_scale_set_conv, and eight blocks -- the same encoder over two clouds -- through the
    dual-cloud plan.  Each scale's slice is bit-identical to set_conv on that scale alone.  (fused_blocks.dual_cloud_set_conv itself
    serves train-mode BatchNorm only and declines an eval-mode call, which is asserted; the eight-block launch is issued the way
    DualCloudBlockFn.forward issues its calls: EncoderPlan(clouds=2), bind_forward, _multi_call.)"""
    from cmflow_amd import _lib, fused_blocks as FB
    from cmflow_amd.radarflow_util import MultiScaleEncoder
    g = torch.Generator().manual_seed(11)
    B, N, ns = 5, 8, 4
    enc = MultiScaleEncoder((2.0, 4.0, 8.0, 16.0), (4, 8, 16, 32), in_channel=3, mlp=MLP, mlp2=MLP2)
    for m in enc.ms_ls:
        init_block(m, g)
    enc = enc.to(dev).eval()
    mods = list(enc.ms_ls)
    clouds = [((torch.rand(B, N, 3, generator=g) * torch.tensor([12.0, 12.0, 2.0])).to(dev).contiguous(),
               torch.randn(B, N, ns * 32, generator=g).to(dev)) for _ in range(2)]
    batched = lambda plan: _lib.lib().cmf_setconv_forward_bodies_batched(plan.n, ctypes.addressof(plan.descs))
    with torch.no_grad():
        singles = [[FB.set_conv(m, xyz, y_all[:, :, 32 * i:32 * i + 32]) for i, m in enumerate(mods)] for xyz, y_all in clouds]
        out = FB.multi_scale_set_conv(enc, mods, FB.scale_streams(ns), *clouds[0])
        plan = next(iter(enc._plans.values()))
        assert plan.n == 4 and [_path(d) for d in plan.descs] == [1] * 4 and batched(plan) == 1
        for i in range(ns):
            assert torch.equal(out[:, :, 64 * i:64 * i + 64], singles[0][i]), "scale %d" % i

        streams = FB.scale_streams(ns, 0) + FB.scale_streams(ns, 1)
        assert FB.dual_cloud_set_conv(enc, mods, streams, clouds[0][0], clouds[0][1], clouds[1][0], clouds[1][1]) is None
        plan2 = FB.EncoderPlan(mods, B, N, 32, False, dev, clouds=2)
        outs = [torch.empty(B * N, ns * 64, device=dev) for _ in range(2)]
        saved = torch.empty(plan2.off_saved[-1], device=dev)
        scratch = torch.empty(plan2.off_fwd[-1], device=dev)
        plan2.bind_forward(clouds, saved, scratch, outs, 1)
        FB._multi_call(False, plan2, streams, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert plan2.n == 8 and [_path(d) for d in plan2.descs] == [1] * 8 and batched(plan2) == 1
        for c in range(2):
            for i in range(ns):
                assert torch.equal(outs[c].view(B, N, -1)[:, :, 64 * i:64 * i + 64], singles[c][i]), "cloud %d scale %d" % (c, i)
