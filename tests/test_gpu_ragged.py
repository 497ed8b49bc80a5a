"""GPU: ragged batches -- B frame pairs of their own point counts in one call (CMFlow.forward_ragged and the counted kernels).

Yardsticks are never the ragged path itself: the parent's DENSE entry points at B = 1 on the truncated sample (bit-exact claims) and
the CPU oracle at B = 1 on the truncated sample (model level, bounds of tests/test_gpu_model.py::test_odd_shapes_match_oracle).
Every op-level case runs twice: padding filled with +-1e4 (large; squares and sums stay finite in fp32) and with copies of valid
points.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from cmflow_amd import synth
from oracle import cmflow_oracle as O

pytestmark = pytest.mark.gpu
_f32, _i32 = torch.float32, torch.int32
RADII, NSAMPLES = (2.0, 4.0, 8.0, 16.0), (4, 8, 16, 32)
# counts per sample: the maximum, 1 below a multiple of 64, a prime, the cost volume's minimum (8), a single point, and one more
COUNTS = (300, 255, 211, 8, 1, 97)
NMAX = 300
FILLS = ("big", "copies")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _pad_fill(t, counts, fill, seed=0):
    """t (B, Nmax, ...) with valid rows [0, counts[i]): overwrite the padded rows with +-1e4 or with copies of valid rows."""
    t = t.clone()
    g = torch.Generator().manual_seed(seed)
    for i, c in enumerate(counts):
        n = t.shape[1] - c
        if n == 0 or (c == 0 and fill == "copies"):                 # nothing to pad / no valid row to copy: the rows stay as drawn
            continue
        if fill == "big":
            sign = (torch.randint(0, 2, (n, *t.shape[2:]), generator=g) * 2 - 1).to(t.dtype)
            t[i, c:] = 1e4 * sign
        else:
            t[i, c:] = t[i, torch.randint(0, c, (n,), generator=g)]
    return t


def _cloud(B, N, seed):
    b = synth.make_batch(B, N, seed=seed)
    return b["pc1"].transpose(1, 2).contiguous(), b["pc2"].transpose(1, 2).contiguous()      # (B,N,3)


# padded sizes of the nested ball query: NMAX with COUNTS, and the edges of the kernel's chunk-count ladder (n <= 256: 1 chunk,
# <= 512: 2, else 4) with a full sample, one row short of it, a sample WITHOUT centres (a wave with no live centre skips the cloud),
# and odd counts: a wave serves G = 2 consecutive centres at these shapes, so an odd count ends inside a wave's group
BQ_CASES = ((NMAX, COUNTS),) + tuple((n, (n, n - 1, 211, 8, 1, 0, 97)) for n in (256, 257, 513))


@pytest.mark.parametrize("fill", FILLS)
def test_counted_nested_ball_query_is_bit_exact(dev, fill):
    """All four (radius, nsample) pairs, two clouds in one launch: every valid centre's list == cmf_ball_query on the truncated
    sample; padded centres write zero rows.  Every chunk-count instantiation of the kernel (BQ_CASES)."""
    from cmflow_amd import _lib
    for nmax, c1 in BQ_CASES:
        B = len(c1)
        x1, x2 = _cloud(B, nmax, 11)
        c2 = c1[::-1]
        x1, x2 = _pad_fill(x1, c1, fill).to(dev), _pad_fill(x2, c2, fill, 1).to(dev)
        n1, n2 = torch.tensor(c1, dtype=_i32, device=dev), torch.tensor(c2, dtype=_i32, device=dev)
        idx = [[torch.full((B, nmax, s), -7, dtype=_i32, device=dev) for s in NSAMPLES] for _ in range(2)]
        radii = (ctypes.c_float * 4)(*RADII)
        ns = (ctypes.c_int * 4)(*NSAMPLES)
        cl = (ctypes.c_void_p * 2)(x1.data_ptr(), x2.data_ptr())
        ip = (ctypes.c_void_p * 8)(*[t.data_ptr() for c in idx for t in c])
        cn = (ctypes.c_void_p * 2)(n1.data_ptr(), n2.data_ptr())
        _lib.check(_lib.lib().cmf_ball_query_multi_counted(B, nmax, nmax, 4, ctypes.addressof(radii), ctypes.addressof(ns), 2, ctypes.addressof(cl),
                                                           ctypes.addressof(cl), ctypes.addressof(ip), ctypes.addressof(cn), ctypes.addressof(cn),
                                                           _lib.stream_ptr()), "cmf_ball_query_multi_counted")
        for c, (x, counts) in enumerate(((x1, c1), (x2, c2))):
            for q, (r, s) in enumerate(zip(RADII, NSAMPLES)):
                for i, n in enumerate(counts):
                    assert not idx[c][q][i, n:].any(), (nmax, c, q, i, n)
                    if n == 0:
                        continue
                    xs = x[i:i + 1, :n].contiguous()
                    want = torch.zeros(1, n, s, dtype=_i32, device=dev)
                    _lib.check(_lib.lib().cmf_ball_query(1, n, n, r, s, xs.data_ptr(), xs.data_ptr(), want.data_ptr(), _lib.stream_ptr()), "cmf_ball_query")
                    assert torch.equal(idx[c][q][i, :n], want[0]), (nmax, c, q, i, n)
                    assert int(idx[c][q][i, :n].max()) < n


# the list-length ladder of the kNN launcher (K = 1, 4, 8, 16, 32) over one padded database of 1100 rows: past the kernel's LDS tile
# (1024 points), one row past it, exactly the tile, a single point (shorter than every list but the first) and an empty sample;
# 70 queries per sample: one full and one partial wave
KNN_NSAMPLES = (1, 4, 8, 16, 32)
KNN_NMAX, KNN_COUNTS, KNN_QUERIES = 1100, (1100, 1025, 1024, 1, 0), 70


@pytest.mark.parametrize("fill", FILLS)
def test_counted_knn_is_bit_exact(dev, fill):
    from cmflow_amd.radarflow_util import knn_point, knn_point_counted
    B = len(COUNTS)
    x1, x2 = _cloud(B, NMAX, 12)
    c1, c2 = COUNTS, (8, 300, 97, 255, 211, 9)                       # n2 >= 8: the cost volume's nsample
    x1, x2 = _pad_fill(x1, c1, fill).to(dev), _pad_fill(x2, c2, fill, 1).to(dev)
    n2 = torch.tensor(c2, dtype=_i32, device=dev)
    got, gd = knn_point_counted(8, x2, x1, n2, return_dist=True)
    for i, (a, b) in enumerate(zip(c1, c2)):
        want, wd = knn_point(8, x2[i:i + 1, :b].contiguous(), x1[i:i + 1, :a].contiguous(), return_dist=True, i32=True)
        assert torch.equal(got[i, :a], want[0]), i
        assert torch.equal(gd[i, :a].view(_i32), wd[0].view(_i32)), i
        assert int(got[i].max()) < b                                 # padded queries too: valid rows of their own sample
    # every rung of the ladder, the tile edge, and the counts below a list's length
    qs, db = _cloud(len(KNN_COUNTS), KNN_NMAX, 13)
    qs, db = qs[:, :KNN_QUERIES].contiguous().to(dev), _pad_fill(db, KNN_COUNTS, fill, 2).to(dev)
    cnt = torch.tensor(KNN_COUNTS, dtype=_i32, device=dev)
    for ns in KNN_NSAMPLES:
        got, gd = knn_point_counted(ns, db, qs, cnt, return_dist=True)
        assert got.dtype == _i32 and got.shape == gd.shape == (len(KNN_COUNTS), KNN_QUERIES, ns)
        for i, n in enumerate(KNN_COUNTS):
            if n == 0:                                               # as the dense kernel answers n = 0: index 0, distance 0
                assert not got[i].any() and not gd[i].view(_i32).any(), (ns, i)
                continue
            want, wd = knn_point(ns, db[i:i + 1, :n].contiguous(), qs[i:i + 1], return_dist=True, i32=True)
            assert torch.equal(got[i], want[0]), (ns, i, n)
            assert torch.equal(gd[i].view(_i32), wd[0].view(_i32)), (ns, i, n)


@pytest.mark.parametrize("fill", FILLS)
def test_counted_global_max_is_bit_exact(dev, fill):
    from cmflow_amd import fused_blocks as FB
    B, C = len(COUNTS), 256
    g = torch.Generator().manual_seed(5)
    f = torch.randn(B, NMAX, C, generator=g)
    f[:, :, 3] = 0.25                                                # a channel of ties: arg = the first row
    f = _pad_fill(f, COUNTS, fill).to(dev)
    cnt = torch.tensor(COUNTS, dtype=_i32, device=dev)
    out, arg = FB.global_max_cat_counted(f, cnt, want_arg=True)
    for i, n in enumerate(COUNTS):
        fi = f[i:i + 1, :n].contiguous()
        want = torch.empty(1, n, 2 * C, dtype=_f32, device=dev)
        warg = torch.empty(1, C, dtype=_i32, device=dev)
        FB._lib.check(FB.L().cmf_global_max_cat(1, n, C, fi.data_ptr(), C, want.data_ptr(), 2 * C, warg.data_ptr(), FB._lib.stream_ptr()), "gm")
        assert torch.equal(out[i, :n].view(_i32), want[0].view(_i32)), i
        assert torch.equal(arg[i], warg[0]), i
        assert torch.equal(out[i, n:, C:], out[i, :1, C:].expand(NMAX - n, C)) and torch.equal(out[i, n:, :C], f[i, n:])


@pytest.mark.parametrize("fill", FILLS)
def test_counted_ego_refine_is_bit_exact(dev, fill):
    """The reduction order over the points is the dense kernel's (lane-strided, then the wave fold), so the transform, the refined
    flow and the mask are asserted BIT-exact against the dense call per truncated sample (stronger than the issue's rtol 3e-5 /
    atol 2e-4 fall-back); padded slots are zeros."""
    from cmflow_amd.radarflow_util import ego_refine, ego_refine_counted
    B = len(COUNTS)
    b = synth.make_batch(B, NMAX, seed=21)
    g = torch.Generator().manual_seed(3)
    pc1 = b["pc1"].transpose(1, 2)
    flow = 0.3 * torch.randn(B, NMAX, 3, generator=g)
    score = torch.rand(B, NMAX, 1, generator=g)
    pc1, flow, score = (_pad_fill(t.contiguous(), COUNTS, fill, k) for k, t in enumerate((pc1, flow, score)))
    pc1, flow, score = pc1.transpose(1, 2).contiguous().to(dev), flow.transpose(1, 2).contiguous().to(dev), score[:, :, 0].contiguous().to(dev)
    cnt = torch.tensor(COUNTS, dtype=_i32, device=dev)
    for eps in (1e-4, 0.0):
        trans, sf, mask, stat = ego_refine_counted(flow, pc1, score, cnt, eps, 0.5)
        for i, n in enumerate(COUNTS):
            wt, wsf, wm = ego_refine(flow[i:i + 1, :, :n].contiguous(), pc1[i:i + 1, :, :n].contiguous(), score[i:i + 1, :n].contiguous(), eps, 0.5)
            assert torch.equal(mask[i, :n], wm[0]), i
            assert torch.equal(trans[i].view(_i32), wt[0].view(_i32)), (i, n, trans[i], wt[0])
            assert torch.equal(sf[i, :, :n].view(_i32), wsf[0].view(_i32)), i
            assert torch.equal(stat[i, :n], score[i, :n])
            assert not sf[i, :, n:].any() and not mask[i, n:].any() and not stat[i, n:].any()


def _metric_inputs(B, N, seed, all_moving=None):
    b = synth.make_batch(B, N, seed=seed, train_extras=True)
    g = torch.Generator().manual_seed(seed)
    labels = b["flow_label"]
    pred = labels + 0.08 * torch.randn(B, N, 3, generator=g)
    mask = (torch.rand(B, N, generator=g) < 0.7).float()
    mask[:, 0], mask[:, 1] = 1.0, 0.0                                # both classes in every sample (counts >= 2 here)
    if all_moving is not None:
        mask[all_moving] = 0.0
    pred_m = torch.where(torch.rand(B, N, generator=g) < 0.85, mask, 1.0 - mask)
    pred_t = b["gt_trans"].clone()
    pred_t[:, :3, 3] += 0.01 * torch.randn(B, 3, generator=g)
    return b["pc1"], pred, labels, mask, pred_m, b["gt_trans"], pred_t


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("all_moving", [None, 4])
def test_counted_metrics_equal_the_mean_of_per_sample_dense_calls(dev, fill, all_moving):
    """== mean over the samples of the dense kernel at B = 1 on the truncated sample, rtol 1e-12 (fp64 sums of the same terms; the
    order of the final B-term mean is the only difference).  all_moving: one sample without static points -- stat_rne is NaN there
    as in numpy, compared with equal_nan; the other case has both classes in every sample and allows no NaN."""
    from cmflow_amd import eval_util as E
    counts = (300, 255, 211, 8, 2, 97) if all_moving is None else (300, 255, 211, 8, 1, 97)      # n = 1 cannot hold both classes
    B = len(counts)
    pc, pred, labels, mask, pred_m, gt_t, pr_t = _metric_inputs(B, NMAX, 31, all_moving)
    pcr = _pad_fill(pc.transpose(1, 2).contiguous(), counts, fill).transpose(1, 2).contiguous()
    pred, labels = _pad_fill(pred, counts, fill, 1), _pad_fill(labels, counts, fill, 2)
    mask_p, pred_m_p = _pad_fill(mask.unsqueeze(2), counts, fill, 3)[:, :, 0], _pad_fill(pred_m.unsqueeze(2), counts, fill, 4)[:, :, 0]
    t = lambda x: x.contiguous().to(dev)
    cnt = torch.tensor(counts, dtype=_i32, device=dev)
    got = E.eval_batch_ragged(t(pcr), t(pred), t(labels), t(mask_p), t(pred_m_p), t(gt_t), t(pr_t), cnt)
    got = np.array([float(v) for d in got for v in d.values()])
    per = []
    for i, n in enumerate(counts):
        w = E.eval_batch(t(pcr[i:i + 1, :, :n]), t(pred[i:i + 1, :n]), t(labels[i:i + 1, :n]), t(mask_p[i:i + 1, :n]), t(pred_m_p[i:i + 1, :n]),
                         t(gt_t[i:i + 1]), t(pr_t[i:i + 1]))
        per.append([float(v) for d in w for v in d.values()])
    want = np.array(per).sum(axis=0) / B
    print("counted metrics", got, "per-sample mean", want)
    if all_moving is None:
        assert np.isfinite(got).all() and np.isfinite(want).all()
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    else:
        assert np.isnan(want[3]) and np.isnan(want[1])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)


# ---- model level -------------------------------------------------------------------------------------------------------------------
MODEL_COUNTS = ((256, 256), (211, 187), (97, 130), (300, 256), (64, 40), (33, 9))


def _weights(manifest, golden_dir, t=False):
    return synth.synth_state_dict(manifest, seed=1234, calib=os.path.join(golden_dir, "bn_calib_cmflow_t.npz" if t else "bn_calib_cmflow.npz"))


def _nets(manifest, golden_dir, args, dev, t=False):
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    sd = _weights(manifest, golden_dir, t)
    ref = (O.CMFlow_T if t else O.CMFlow)(args)
    ref.load_state_dict(sd)
    net = (CMFlow_T if t else CMFlow)(args)
    net.load_state_dict(sd)
    return ref.eval(), net.to(dev).eval()


def _ragged_batch(counts, nmax1, nmax2, fill, seed=7, dev=None):
    """synth.make_batch(B, 300, seed) with sample i truncated to its counts, then padded to (nmax1, nmax2) with `fill`."""
    B = len(counts)
    b = synth.make_batch(B, 300, seed=seed)
    out = {}
    for k, col, nm in (("pc1", 0, nmax1), ("ft1", 0, nmax1), ("pc2", 1, nmax2), ("ft2", 1, nmax2)):
        t = b[k].transpose(1, 2)                                      # (B,300,3)
        if nm > 300:
            t = torch.cat((t, torch.zeros(B, nm - 300, 3)), dim=1)
        t = _pad_fill(t[:, :nm].contiguous(), [c[col] for c in counts], fill, seed={'pc1': 1, 'ft1': 2, 'pc2': 3, 'ft2': 4}[k])
        out[k] = t.transpose(1, 2).contiguous()
    out["n1"] = torch.tensor([c[0] for c in counts], dtype=_i32)
    out["n2"] = torch.tensor([c[1] for c in counts], dtype=_i32)
    return {k: v.to(dev) for k, v in out.items()} if dev is not None else out


def _sample(rb, i):
    n1, n2 = int(rb["n1"][i]), int(rb["n2"][i])
    return (rb["pc1"][i:i + 1, :, :n1].contiguous(), rb["pc2"][i:i + 1, :, :n2].contiguous(),
            rb["ft1"][i:i + 1, :, :n1].contiguous(), rb["ft2"][i:i + 1, :, :n2].contiguous())


def _check_against(got, i, n1, want, what):
    """The bounds of test_odd_shapes_match_oracle on sample i's valid slice; returns the number of mask flips."""
    sf, sc, tr, mk = got[0][i:i + 1, :, :n1].cpu(), got[1][i:i + 1, :, :n1].cpu(), got[2][i:i + 1].cpu(), got[3][i:i + 1, :n1].cpu()
    wsf, wsc, wtr, wmk = (w.cpu() for w in want[:4])
    flips = mk != wmk
    assert flips.float().mean().item() <= 0.01, (what, i)
    ok = ~flips.unsqueeze(1).expand(-1, 3, -1)
    scale = max(1.0, float(wsf.abs().max()))
    e_sf, e_sc = (sf - wsf)[ok].abs().max().item(), (sc - wsc).abs().max().item()
    print("%s sample %d (n1=%d): flips %d, |flow err| %.3g (bound %.3g), |stat_cls err| %.3g" % (what, i, n1, int(flips.sum()), e_sf, 2e-4 * scale, e_sc))
    assert e_sf <= 2e-4 * scale, (what, i, e_sf)
    assert e_sc <= 2e-4, (what, i, e_sc)
    if not flips.any():
        np.testing.assert_allclose(tr.numpy(), wtr.numpy(), rtol=3e-5, atol=2e-4, err_msg="%s sample %d" % (what, i))
    return int(flips.sum())


def _assert_padding_defined(got, n1s):
    for i, n1 in enumerate(n1s):
        assert not got[0][i, :, n1:].any() and not got[1][i, :, n1:].any() and not got[3][i, n1:].any(), i


def test_forward_ragged_matches_oracle_per_sample(dev, manifest, golden_dir, args):
    """B = 6 ragged pairs (N1 != N2, n2 = 9 included) against the CPU oracle at B = 1 on each truncated pair.  The 1 % flip cap is a
    condition on the inputs: the oracle's smallest |stat_cls - 0.5| over all valid points was measured at 3.3e-3 (sample 1), 16 x the
    2e-4 score bound -- the margin is asserted (>= 10 x the bound) so a change of synth cannot silently erode it."""
    ref, net = _nets(manifest, golden_dir, args, dev)
    cpu = _ragged_batch(MODEL_COUNTS, 300, 256, "big")
    rb = {k: v.to(dev) for k, v in cpu.items()}
    with torch.no_grad():
        got = net.forward_ragged(rb["pc1"], rb["pc2"], rb["ft1"], rb["ft2"], rb["n1"], rb["n2"], validate=True)
        assert got[0].shape == (6, 3, 300) and got[1].shape == (6, 1, 300) and got[2].shape == (6, 4, 4) and got[3].shape == (6, 300)
        assert got[3].dtype == torch.bool
        margin, static = 1.0, []
        for i, (n1, _) in enumerate(MODEL_COUNTS):
            want = ref(*_sample(cpu, i), None, "test")
            margin = min(margin, float((want[1] - 0.5).abs().min()))
            static.append(float(want[3].float().mean()))
            _check_against(got, i, n1, want, "oracle")
    print("oracle margin |stat_cls - 0.5| min = %.3g; static share per sample %s" % (margin, static))
    assert margin >= 2e-3, margin
    _assert_padding_defined(got, [c[0] for c in MODEL_COUNTS])


def test_forward_ragged_matches_the_dense_forward_per_sample(dev, manifest, golden_dir, args):
    """Against the dense forward at B = 1 on each truncated pair: the neighbour indices of every set-conv block (both encoders, taken
    from fused_blocks.IDX_TAP) bit-exact on the valid rows, outputs within the oracle bounds.  Outputs are not required bit-exact:
    cmf_gemm picks its tiles by M."""
    from cmflow_amd import fused_blocks as FB
    _, net = _nets(manifest, golden_dir, args, dev)
    rb = _ragged_batch(MODEL_COUNTS, 300, 256, "copies", dev=dev)
    B = len(MODEL_COUNTS)
    with torch.no_grad():
        FB.IDX_TAP = []
        try:
            got = net.forward_ragged(rb["pc1"], rb["pc2"], rb["ft1"], rb["ft2"], rb["n1"], rb["n2"])
            tap_r = FB.IDX_TAP
            assert len(tap_r) == 8                                   # 4 scales of the shared first-encoder call (2B samples) + 4 of the second
            for i, (n1, n2) in enumerate(MODEL_COUNTS):
                FB.IDX_TAP = []
                want = net(*_sample(rb, i), None, "test")
                tap_d = FB.IDX_TAP                                   # N1 != N2: enc1(cloud 1) x4, enc1(cloud 2) x4, enc2 x4; else 4 + 4
                _check_against(got, i, n1, want, "dense B=1")
                for q in range(4):
                    r1, r2, e2 = tap_r[q][2][i, :n1], tap_r[q][2][B + i, :n2], tap_r[4 + q][2][i, :n1]
                    if len(tap_d) == 12:
                        d1, d2, de = tap_d[q][2][0], tap_d[4 + q][2][0], tap_d[8 + q][2][0]
                    else:
                        assert len(tap_d) == 8 and n1 == n2
                        d1, d2, de = tap_d[q][2][0], tap_d[q][2][1], tap_d[4 + q][2][0]
                    assert torch.equal(r1, d1) and torch.equal(r2, d2) and torch.equal(e2, de), (i, q)
        finally:
            FB.IDX_TAP = None


def test_padding_does_not_leak(dev, manifest, golden_dir, args):
    """Identical valid data, different padding contents AND different padded sizes (300 / 256 and 384 / 320): bit-identical valid slices."""
    _, net = _nets(manifest, golden_dir, args, dev)
    a = _ragged_batch(MODEL_COUNTS, 300, 256, "big", dev=dev)
    b = _ragged_batch(MODEL_COUNTS, 384, 320, "copies", dev=dev)
    with torch.no_grad():
        ga = net.forward_ragged(a["pc1"], a["pc2"], a["ft1"], a["ft2"], a["n1"], a["n2"])
        gb = net.forward_ragged(b["pc1"], b["pc2"], b["ft1"], b["ft2"], b["n1"], b["n2"])
    for i, (n1, _) in enumerate(MODEL_COUNTS):
        assert torch.equal(ga[3][i, :n1], gb[3][i, :n1]), i
        for k in (0, 1):
            d = (ga[k][i, :, :n1] - gb[k][i, :, :n1]).abs().max().item()
            assert torch.equal(ga[k][i, :, :n1].view(_i32), gb[k][i, :, :n1].view(_i32)), (i, k, d)
        assert torch.equal(ga[2][i].view(_i32), gb[2][i].view(_i32)), i
    _assert_padding_defined(gb, [c[0] for c in MODEL_COUNTS])


def test_batch_composition_does_not_leak(dev, manifest, golden_dir, args):
    """Sample i's valid slice is bit-identical whether it is batched with samples of other sizes or repeated B times (same padded
    sizes, so every GEMM sees the same M and picks the same tiles)."""
    _, net = _nets(manifest, golden_dir, args, dev)
    rb = _ragged_batch(MODEL_COUNTS, 300, 256, "big", dev=dev)
    B = len(MODEL_COUNTS)
    with torch.no_grad():
        got = net.forward_ragged(rb["pc1"], rb["pc2"], rb["ft1"], rb["ft2"], rb["n1"], rb["n2"])
        for i in (1, 4, 5):
            rep = {k: v[i:i + 1].expand(B, *v.shape[1:]).contiguous() for k, v in rb.items()}
            g2 = net.forward_ragged(rep["pc1"], rep["pc2"], rep["ft1"], rep["ft2"], rep["n1"], rep["n2"])
            n1 = MODEL_COUNTS[i][0]
            for j in (0, B - 1):
                for k in (0, 1):
                    assert torch.equal(got[k][i, :, :n1].view(_i32), g2[k][j, :, :n1].view(_i32)), (i, j, k)
                assert torch.equal(got[2][i].view(_i32), g2[2][j].view(_i32)) and torch.equal(got[3][i], g2[3][j]), (i, j)


def test_dense_degenerate_case_equals_forward(dev, manifest, golden_dir, args):
    """All counts = Nmax = 256: what forward returns, within the oracle bounds (and the same neighbour lists by the op tests)."""
    _, net = _nets(manifest, golden_dir, args, dev)
    b = {k: v.to(dev) for k, v in synth.make_batch(4, 256, seed=7).items()}
    n = torch.full((4,), 256, dtype=_i32, device=dev)
    with torch.no_grad():
        got = net.forward_ragged(b["pc1"], b["pc2"], b["ft1"], b["ft2"], n, n, validate=True)
        want = net(b["pc1"], b["pc2"], b["ft1"], b["ft2"], None, "test")
    for i in range(4):
        _check_against(got, i, 256, tuple(w[i:i + 1] for w in want), "dense forward")


def test_cmflow_t_forward_ragged_clip_matches_oracle(dev, manifest_t, golden_dir, args):
    """A 3-frame ragged clip with gfeat carried, against the oracle's CMFlow_T frame by frame at B = 1 (each side carries its own
    state), with the forward bounds of test_full_size_cmflow_t_clip_matches_oracle per sample: mask equal, stat_cls within 1e-4, the
    transform by that test's own _check_transform (rotation <= 2e-6 rad, R entries <= 1e-5, |dt| <= 1e-4 + |dR|_2 |cA|, bottom row
    exact; weights = the oracle's normalised stat_cls over the valid points -- CMFlow-T adds no eps, cmflow_t.py:119), flow EPE mean
    within 1e-4 and max within 1e-4 + 2e-6 * 100 + dt with dt bounded by that check, gfeat within 1e-4."""
    from test_gpu_model import _check_transform
    ref, net = _nets(manifest_t, golden_dir, args, dev, t=True)
    counts = ((256, 256), (211, 187), (97, 130), (300, 256))
    B = len(counts)
    g_net, g_ref = None, [None] * B
    for f in range(3):
        cpu = _ragged_batch(counts, 300, 256, FILLS[f % 2], seed=7 + 1000 * f)
        rb = {k: v.to(dev) for k, v in cpu.items()}
        with torch.no_grad():
            got = net.forward_ragged(rb["pc1"], rb["pc2"], rb["ft1"], rb["ft2"], rb["n1"], rb["n2"], g_net)
            assert len(got) == 5 and got[4].shape == (B, 256)
            for i, (n1, _) in enumerate(counts):
                smp = _sample(cpu, i)
                want = ref(*smp, None, "test", g_ref[i])
                assert torch.equal(got[3][i:i + 1, :n1].cpu(), want[3]), (f, i)
                assert float((got[1][i:i + 1, :, :n1].cpu() - want[1]).abs().max()) <= 1e-4, (f, i)
                score = want[1].squeeze(1)
                ang, dt = _check_transform(got[2][i:i + 1], want[2], smp[0], score / score.sum(dim=1, keepdim=True))
                epe = (got[0][i:i + 1, :, :n1].cpu() - want[0]).norm(dim=1)
                print("CMFlow-T ragged frame %d sample %d: EPE mean %.3g max %.3g, rot %.3g rad, dt %.3g m, static share %.2f"
                      % (f, i, float(epe.mean()), float(epe.max()), ang, dt, float(want[3].float().mean())))
                assert float(epe.mean()) <= 1e-4 and float(epe.max()) <= 1e-4 + 2e-6 * 100.0 + dt, (f, i)
                np.testing.assert_allclose(got[4][i:i + 1].cpu().numpy(), want[4].numpy(), rtol=0, atol=1e-4)
                g_ref[i] = want[4]
        g_net = got[4]


def test_forward_ragged_errors(dev, manifest, golden_dir, args):
    from cmflow_amd.raflow import RaFlow
    _, net = _nets(manifest, golden_dir, args, dev)
    rb = _ragged_batch(MODEL_COUNTS, 300, 256, "copies", dev=dev)
    call = lambda n1, n2, **kw: net.forward_ragged(rb["pc1"], rb["pc2"], rb["ft1"], rb["ft2"], n1, n2, **kw)
    with pytest.raises(RuntimeError):                                # autograd on
        call(rb["n1"], rb["n2"])
    with torch.no_grad():
        net.train()
        with pytest.raises(RuntimeError):
            call(rb["n1"], rb["n2"])
        net.eval()
        bad2 = rb["n2"].clone(); bad2[5] = 7
        with pytest.raises(ValueError):
            call(rb["n1"], bad2, validate=True)
        bad1 = rb["n1"].clone(); bad1[0] = 301
        with pytest.raises(ValueError):
            call(bad1, rb["n2"], validate=True)
        bad0 = rb["n1"].clone(); bad0[2] = 0
        with pytest.raises(ValueError):
            call(bad0, rb["n2"], validate=True)
        big = torch.zeros(1, 3, 1025, device=dev)
        n = torch.tensor([1025], dtype=_i32, device=dev)
        with pytest.raises(ValueError):
            net.forward_ragged(big, big, big, big, n, n)
        class A:
            num_points, stat_thres, rigid_thres = 256, 0.5, 0.15
        with pytest.raises(NotImplementedError):
            RaFlow(A()).to(dev).eval().forward_ragged(rb["pc1"], rb["pc2"], rb["ft1"], rb["ft2"], rb["n1"], rb["n2"])


def test_collated_split_runs_end_to_end(dev, manifest, golden_dir, args, tmp_path):
    """dataset.collate_ragged -> extract_data_info_ragged -> forward_ragged -> eval_batch_ragged on the ragged synthetic split, against
    the per-frame B = 1 loop the reference's test protocol runs (main.py:203).  Asserted on the end-point error: both sides average the
    per-sample mean of |pred - label|, and the flows differ by at most 2e-4 x max(1, |flow|max) per component on unflipped points (the
    bound of the forward tests), so the averages differ by at most sqrt(3) times that when no mask flips.  The segmentation metrics depend on
    the masks alone and are asserted equal (rtol 1e-12) given zero flips.  The remaining ones count points against thresholds (a point at
    a threshold moves them by 1 / n) or follow the transform (bounded in the clip test, conditioned on |cA|) and are printed."""
    from cmflow_amd import dataset as D, eval_util as E
    _, net = _nets(manifest, golden_dir, args, dev)
    D.write_synthetic_split(str(tmp_path))

    class DA:
        num_points, eval = 256, True
    items = []
    for part in ("train", "test"):
        d = D.vodDataset(DA(), str(tmp_path), part)
        items += [d[i] for i in range(len(d))]
    assert len(items) == 6
    info = D.extract_data_info_ragged(D.collate_ragged(items), device=dev)
    pc1, pc2, ft1, ft2, trans, gt, mask, _, _, _, _, n1, n2 = info
    acc, scale, flips = None, 1.0, 0
    with torch.no_grad():
        sf, cls, pt, mk = net.forward_ragged(pc1, pc2, ft1, ft2, n1, n2, validate=True)
        got = E.eval_batch_ragged(pc1, sf.transpose(1, 2).contiguous(), gt, mask, mk.float(), trans, pt, n1)
        for i in range(len(items)):
            a, b = int(n1[i]), int(n2[i])
            o = net(pc1[i:i + 1, :, :a].contiguous(), pc2[i:i + 1, :, :b].contiguous(), ft1[i:i + 1, :, :a].contiguous(),
                    ft2[i:i + 1, :, :b].contiguous(), None, "test")
            w = E.eval_batch(pc1[i:i + 1, :, :a].contiguous(), o[0].transpose(1, 2).contiguous(), gt[i:i + 1, :a].contiguous(),
                             mask[i:i + 1, :a].contiguous(), o[3].float(), trans[i:i + 1], o[2])
            v = np.array([float(x) for d in w for x in d.values()])
            acc = v if acc is None else acc + v
            scale = max(scale, float(o[0].abs().max()))
            flips += int((o[3] != mk[i:i + 1, :a]).sum())
    got = np.array([float(x) for d in got for x in d.values()])
    print("batched", got, "per-frame loop", acc / len(items), "mask flips", flips)
    assert flips == 0
    assert abs(got[6] - acc[6] / len(items)) <= 3 ** 0.5 * 2e-4 * scale
    # acc / miou / sen are functions of the masks alone: with no flip both sides average the same six numbers in the same order
    np.testing.assert_allclose(got[9:12], acc[9:12] / len(items), rtol=1e-12, atol=0)
