"""Test fixture: the cases of tests/test_gpu_setconv_chain.py (the first encoder's 6 -> 32 -> 32 -> 64 | 64 -> 64 -> 64 set-conv block
under eval-mode BatchNorm) and the one way their inputs are generated, shared with tests/test_setconv_ref.py, which checks on the
CPU that every small case's fixed seed keeps the fp32 and the fp64 evaluation of the reference on the same ReLU masks and argmax
sources.  Inputs are drawn on the CPU from a seeded generator, so both test modules see the same numbers.

A case is (B, N, S) + what differs from the plain set-up: radius (default 4 m in the 12 x 12 x 2 m box), `sliced` (y is the column
slice [:, :, 32:64] of a (B,N,128) tensor: row pitch 128, the way the model's stacked first conv hands it over) and `dead` (BN 2 bias
= -100 on 8 of the 64 channels).  Blocks of 32 rows = B N S / 32."""
import collections

import torch

from setconv_ref import max_err, set_conv_ref, ulp32

MLP, MLP2 = [32, 32, 64], [64, 64, 64]
DEAD_CHANNELS = [1, 6, 19, 31, 32, 40, 57, 63]                        # both halves of the 64 and both 4-channel lane halves
Case = collections.namedtuple("Case", "name B N S radius sliced dead seed")


def _c(B, N, S, seed, radius=4.0, sliced=False, dead=False, tag=""):
    return Case("%dx%dx%d%s" % (B, N, S, tag), B, N, S, radius, sliced, dead, seed)


# Seeds: the smallest of 0, 1, 2, ... for which the case meets the preconditions test_setconv_ref.py asserts with a factor 2 to spare
# (min |u| >= 2e-5).  No case was dropped or reshaped to get there.
# With N = 8 a ball holds at most eight different points and every slot from the ninth on repeats the first: the maximum over the
# first eight slots is then the maximum over all, and the group maximum's steps across 8 and 16 lanes decide nothing (dropping one
# went unnoticed by every N = 8 case).  These two have S different points in every ball, in both forward groups and backward.
FULL = [_c(2, 16, 16, 3, radius=50.0, tag="-full"), _c(1, 32, 32, 27, radius=50.0, tag="-full")]
INFER = [_c(1, 8, 4, 0),               # 32 rows: one block, three idle waves
         _c(5, 8, 4, 0),               # 160 rows: a sample boundary at every block, the second wave walks one block
         _c(3, 16, 4, 1),              # 192 rows: ... two blocks
         _c(7, 8, 4, 1),               # 224 rows: ... three blocks
         _c(3, 8, 8, 0), _c(3, 8, 16, 0), _c(3, 8, 32, 0),      # four, two, one point(s) per block
         _c(17, 8, 32, 2),             # 136 blocks: nine workgroups, the last one half idle
         _c(2, 16, 8, 0, sliced=True, tag="-ldy128")] + FULL
TRAIN = [_c(4, 8, 4, 0), _c(12, 8, 4, 0), _c(2, 16, 8, 0), _c(2, 8, 16, 0), _c(4, 8, 32, 0), _c(2, 16, 8, 0, sliced=True, tag="-ldy128")] + FULL
PER_LAYER_UNDER_GRAD = _c(5, 8, 4, 0, tag="-grad")                    # 160 rows: no multiple of 128 -> the per-layer kernels
EDGE = [_c(4, 8, 4, 0, radius=0.01, tag="-r0.01"),      # every ball repeats its centre: all slots tied
        _c(4, 8, 4, 0, radius=50.0, tag="-r50"),        # every ball full
        _c(4, 8, 4, 0, dead=True, tag="-dead"),         # BN 2 bias -100 on DEAD_CHANNELS
        _c(4, 8, 32, 0, radius=0.01, tag="-r0.01"),
        _c(4, 8, 32, 3, radius=50.0, tag="-r50"),
        _c(4, 8, 32, 0, dead=True, tag="-dead")]
SMALL = list({c.name: c for c in INFER + TRAIN + [PER_LAYER_UNDER_GRAD] + EDGE}.values())
LARGE = _c(33, 256, 32, 0, radius=2.0)                                # 8448 blocks: more than 4 per wave in the backward passes


def blocks_per_wave(blocks, backward):
    """csrc/setconv_chain.hip chain_blocks_per_wave, restated: the arithmetic the cases above are chosen by."""
    return max(4, min(32 if backward else 16, -(-blocks // (2048 if backward else 3072))))


def walk(case, backward):
    """-> (blocks, blocks per wave, waves with work, blocks of the last such wave, workgroups, working waves of the last workgroup)"""
    blocks = case.B * case.N * case.S // 32
    bpw = blocks_per_wave(blocks, backward)
    waves = -(-blocks // bpw)
    return blocks, bpw, waves, blocks - (waves - 1) * bpw, -(-waves // 4), waves - (-(-waves // 4) - 1) * 4


def init_block(mod, g):
    """Fill a PointLocalFeature (the product's or the oracle's: same members) from generator g: conv weights ~ N(0, 1/fan_in) (the
    coordinate columns of the first conv 0.3: offsets are metres), BN gamma in [0.5, 1.5], beta ~ 0.2 N, running mean ~ 0.3 N,
    running var in [0.5, 2]."""
    with torch.no_grad():
        for i, conv in enumerate(list(mod.mlp_convs) + list(mod.mlp2_convs)):
            w = torch.randn(conv.weight.shape, generator=g) / conv.weight.shape[1] ** 0.5
            if i == 0:
                w[:, :3] = torch.randn(w.shape[0], 3, 1, 1, generator=g) * 0.3
            conv.weight.copy_(w)
        for bn in list(mod.mlp_bns) + list(mod.mlp2_bns):
            c = bn.num_features
            bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
            bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
            bn.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)
    return mod.eval()


def make_inputs(case, cls):
    """-> (module of class `cls` in eval mode on the CPU, xyz (B,N,3), y (B,N,32) -- a view with row pitch 128 if case.sliced --,
    dout (B,N,64)), all fp32, drawn from the case's seed."""
    g = torch.Generator().manual_seed(1000 * case.seed + 7)
    mod = init_block(cls(case.radius, case.S, in_channel=3, mlp=MLP, mlp2=MLP2), g)
    if case.dead:
        with torch.no_grad():
            mod.mlp_bns[2].bias[DEAD_CHANNELS] = -100.0
    xyz = (torch.rand(case.B, case.N, 3, generator=g) * torch.tensor([12.0, 12.0, 2.0])).contiguous()
    y = torch.randn(case.B, case.N, 128 if case.sliced else 32, generator=g)
    dout = torch.randn(case.B, case.N, 64, generator=g)
    return mod, xyz, (y[:, :, 32:64] if case.sliced else y), dout


def block_params(mod):
    """The 18 parameters in the order of set_conv_ref (= fused_blocks.set_conv_params) and the six (mean, var, eps)."""
    w2d = lambda conv: conv.weight.view(conv.weight.shape[0], conv.weight.shape[1])
    convs, bns = list(mod.mlp_convs) + list(mod.mlp2_convs), list(mod.mlp_bns) + list(mod.mlp2_bns)
    params = []
    for l, (conv, bn) in enumerate(zip(convs, bns)):
        params += [w2d(conv)[:, :3] if l == 0 else w2d(conv), bn.weight, bn.bias]
    return params, [(bn.running_mean, bn.running_var, bn.eps) for bn in bns]


def block_grads(mod):
    """The gradients autograd left on the module, in the order of block_params (wx: the coordinate columns of the first conv's)."""
    params, _ = block_params(mod)
    out = []
    for l, p in enumerate(params):
        base = p._base if p._base is not None else p
        g = base.grad.view(base.shape[0], -1) if base.dim() == 4 else base.grad
        out.append(g[:, :3] if l == 0 else g)
    return out


PARAM_NAMES = ["wx", "g1", "b1", "w2", "g2", "b2", "w3", "g3", "b3", "w4", "g4", "b4", "w5", "g5", "b5", "w6", "g6", "b6"]


class Yardstick:
    """The reference in fp64 and in fp32 on one case's inputs, and the bounds that follow (DESIGN.md "Register-chain tests"): a
    quantity computed in fp32 may differ from the fp64 value by 4 x the error of the PLAIN fp32 torch evaluation of the same
    reference (the kernels sum the same rounding population in another order) + one fp32 ulp of the tensor's largest entry.
    Nothing here sees a kernel's output."""

    def __init__(self, case, xyz, y, idx, dout, params, buffers, backward=True):
        self.case = case
        self.r64 = set_conv_ref(xyz, y, idx, params, buffers, torch.float64)
        self.r32 = set_conv_ref(xyz, y, idx, params, buffers, torch.float32)
        self.out = self.r64.out.detach()
        self.out_yard = max_err(self.r32.out, self.out)
        self.names = ["dy"] + PARAM_NAMES
        if backward:
            self.g64 = [t.detach() for t in self.r64.grads(dout)]
            self.g32 = [t.detach() for t in self.r32.grads(dout)]
            self.g_yard = [max_err(a, r) for a, r in zip(self.g32, self.g64)]

    @staticmethod
    def allowance(yard, ref):
        return 4.0 * yard + ulp32(ref.abs().max())

    def out_allowance(self):
        return self.allowance(self.out_yard, self.out)

    def grad_allowance(self, k):
        return self.allowance(self.g_yard[k], self.g64[k])
