"""GPU: cmflow_amd/prepare.py (cmf_prepare_count / _pairs / _scans) against the float64 restatement of the reference's preprocess step
(tests/prepare_ref.py) on the synthetic scans, poses and tracks of tests/prepare_case.py.

Before anything is compared every case asserts, on the restatement alone, that no decision sits on a tie (Case.reference ->
prepare_ref.assert_margins): projected coordinates at least 1e-6 px from a half-integer; box faces, the 3 m gate and the 0.05 m rule
at least 1e-9 m from equality.  With coordinates below 100 m and pixels below 1e4 over about ten float64 operations the two sides
differ by about 1e-13 m / 1e-11 px, so inside those margins they decide alike and no case is excluded.
Then: counts, kept source rows, offsets, masks, u and v are exact; tab2 and the coordinate, feature and optical-flow columns of tab1
are bit-exact copies; labels and trans are within one float32 ulp of the restatement's value (both sides compute in float64 and round
once: only a rounding tie or the summation order of numpy's BLAS can differ) -- the number of elements that differ at all is printed."""
import numpy as np
import pytest
import torch

import prepare_case as PC
import prepare_ref as R
from cmflow_amd import dataset as D
from cmflow_amd import evaluate as EV
from cmflow_amd import prepare as P
from prepare_case import product_calib

pytestmark = pytest.mark.gpu
EDGES = [1, 63, 64, 65, 255, 256, 257, 1000]          # raw scan lengths around the wave (64) and the workgroup chunk (256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_one_ulp(got, want, what):
    """|got - want| <= the float32 spacing at |want|, element by element; prints how many elements differ at all."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = int((got != want).sum())
    print("%s: %d of %d elements differ" % (what, differ, want.size))
    ok = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)
    assert ok.all(), (what, got[~ok][:4], want[~ok][:4])


def build(case, dev, chunks=None, clip=None):
    """The case through SplitBuilder: one add, or one per (scan range, pair range) of ``chunks``"""
    b = P.SplitBuilder(product_calib(case), case.mode, dev)
    if chunks is None:
        b.add(case.packed_scans, case.scan_off, case.pairs, case.odom, case.packed_tracks, case.track_off, case.flows, clip)
    else:
        assert all(c is case.calib[0] for c in case.calib)
        for (s0, s1), (f0, f1) in chunks:
            b.add(np.concatenate(case.scans[s0:s1]), case.scan_off[s0:s1 + 1] - case.scan_off[s0], case.pairs[f0:f1] - s0, case.odom[s0:s1],
                  np.concatenate(case.tracks[s0:s1]), case.track_off[s0:s1 + 1] - case.track_off[s0],
                  None if case.flows is None else case.flows[f0:f1], None if clip is None else clip[f0:f1])
    return b


def check_filter(case, dev):
    """cmf_prepare_count against the restatement's filter, scan by scan: counts, the kept source rows in order, u and v"""
    keep, uv, count = (t.cpu().numpy() for t in P.count_scans(case.packed_scans, case.scan_off, product_calib(case), dev))
    assert keep.dtype == np.int32 and keep.shape == (case.scan_off[-1],) and uv.shape == (case.scan_off[-1], 2)
    for s, scan in enumerate(case.scans):
        idx, uvs, _ = R.filter_scan(scan, case.calib[s])
        k = keep[case.scan_off[s]:case.scan_off[s + 1]]
        assert count[s] == idx.size, (s, count[s], idx.size)
        assert np.array_equal(np.nonzero(k >= 0)[0], idx), s               # the same source rows ...
        assert np.array_equal(k[idx], np.arange(idx.size)), s              # ... in scan order
        assert np.array_equal(uv[case.scan_off[s]:case.scan_off[s + 1]][idx], uvs), s
    return count


def check_split(case, split, kept, what="", min_points=(1, 1)):
    """A built split against the restatement's items of the kept pairs"""
    ref = case.reference()
    n1 = np.array([r[1][0].shape[0] for r in ref])
    n2 = np.array([r[1][1].shape[0] for r in ref])
    want_kept = np.nonzero((n1 >= min_points[0]) & (n2 >= min_points[1]))[0]
    assert np.array_equal(kept, want_kept), (what, kept, want_kept)
    items = [ref[f][1] for f in kept]
    cat = lambda k: np.concatenate([np.asarray(it[k], dtype=np.float32).reshape(len(it[k]), -1) for it in items])
    assert split.off1.cpu().tolist() == np.concatenate([[0], np.cumsum(n1[kept])]).tolist(), what
    assert split.off2.cpu().tolist() == np.concatenate([[0], np.cumsum(n2[kept])]).tolist(), what
    assert len(split) == len(kept) and split.max_points == max(n1[kept].max(), n2[kept].max())
    tab1, tab2 = split.tab1.cpu().numpy(), split.tab2.cpu().numpy()
    assert tab1.shape == (n1[kept].sum(), 14) and tab2.shape == (n2[kept].sum(), 6)
    assert np.array_equal(bits(tab2), bits(np.concatenate([cat(1), cat(3)], axis=1))), what            # copies: bit for bit
    assert np.array_equal(bits(tab1[:, 0:6]), bits(np.concatenate([cat(0), cat(2)], axis=1))), what
    assert np.array_equal(bits(tab1[:, 12:14]), bits(cat(10))), what
    assert np.array_equal(tab1[:, 9:10], cat(6)), what                                                  # masks, u, v: exact
    assert np.array_equal(tab1[:, 10:11], cat(8)) and np.array_equal(tab1[:, 11:12], cat(9)), what
    assert_one_ulp(tab1[:, 6:9], cat(5), what + " labels")
    assert_one_ulp(split.trans.cpu().numpy(), np.stack([it[4].reshape(16) for it in items]), what + " trans")
    assert split.interval.cpu().tolist() == [np.float32(R.INTERVAL)] * len(kept)
    return items


def run_case(case, dev, what, **kw):
    check_filter(case, dev)
    split, kept = build(case, dev).finish(**kw)
    return split, check_split(case, split, kept, what, **kw)


# ---- raw scan lengths and the filter's edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [5, 7])
@pytest.mark.parametrize("mode", ["gt", "pseudo"])
def test_scan_lengths_around_the_wave_and_the_chunk(dev, cols, mode):
    """1 .. 1000 raw rows in one call, every scan frame 2 of one pair and frame 1 of the next; shared and per-scan calibration"""
    case = PC.chain(21 + cols, EDGES, mode, K=5, cols=cols, per_scan_calib=cols == 7)
    count = check_filter(case, dev)
    assert 0 < count[-1] < 1000
    split, kept = build(case, dev).finish()
    check_split(case, split, kept, "edges %d %s" % (cols, mode))
    fg = sum(int((r[1][6] != 1).sum()) for r in case.reference())
    assert fg > 0                                                          # the boxes do label points


def test_all_kept_none_kept_alternating(dev):
    inside = lambda i: (0.00917 * (i % 300) - 1.5, 0.3, 2.0)               # u = 968 + 50 x: inside the image, off every half pixel
    outside = lambda i: (0.00917 * (i % 300), 0.3, 5.0)                    # z = 5: above the height range
    for n in (1, 64, 257, 600):
        scans = [PC.rows([inside(i) for i in range(n)]), PC.rows([outside(i) for i in range(n)]),
                 PC.rows([inside(i) if i % 2 else outside(i) for i in range(n)]), PC.rows([inside(i) for i in range(n + 3)])]
        case = PC.simple_case(scans, "gt", pairs=[(0, 3), (0, 1), (2, 3), (1, 2), (3, 0)])
        count = check_filter(case, dev)
        assert count.tolist() == [n, 0, n // 2, n + 3]
        split, kept = build(case, dev).finish()
        assert kept.tolist() == ([0, 2, 4] if n > 1 else [0, 4])
        check_split(case, split, kept, "all / none / alternating, n = %d" % n)


def test_height_bounds_pixel_bounds_and_a_point_behind_the_camera(dev):
    up = float(np.nextafter(np.float32(3), np.float32(4)))
    pts = [(0, 0, 3.0), (0, 0, up), (0, 0, -3.0), (0, 0, -up),             # z = +-3 kept (-3: behind this camera), the next float32 dropped
           (-1, -1, -2.0),                                                 # behind the camera, projects to (1018, 658): kept, no depth test
           (-9.68, 0, 1), (-9.67, 0, 1), (9.68, 0, 1), (9.69, 0, 1),       # u = 0, 1, 1936, 1937
           (0, -6.08, 1), (0, -6.07, 1), (0, 6.08, 1), (0, 6.09, 1),       # v = 0, 1, 1216, 1217
           (1, 1, 0.0), (float("nan"), 0, 1), (0, 0, float("inf"))]        # w = 0, NaN, Inf: dropped
    want = [0, 2, 4, 6, 7, 10, 11]
    for cols in (5, 7):
        case = PC.simple_case([PC.rows(pts, cols), PC.rows(pts[::-1], cols)], "pseudo")
        count = check_filter(case, dev)
        assert count.tolist() == [len(want)] * 2
        assert R.filter_scan(case.scans[0], case.calib[0])[0].tolist() == want
        uvs = R.filter_scan(case.scans[0], case.calib[0])[1]
        assert uvs[[3, 4], 0].tolist() == [1, 1936] and uvs[[5, 6], 1].tolist() == [1, 1216] and uvs[2].tolist() == [1018, 658]
        split, items = run_case(case, dev, "bounds")
        assert split.tab1[:, 10].cpu().tolist() == uvs[:, 0].tolist()


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gt", "pseudo"])
@pytest.mark.parametrize("K", [0, 1, 8, 50])
def test_boxes_none_one_several_forty(dev, mode, K):
    """K own boxes per scan in the five kinds of prepare_case (3 m gate, id missing, id twice, overlapping, plus one without a point);
    K = 1: one box of the plain kind, which labels its points; K = 50: 41 matched records on one pair"""
    case = PC.chain(40 + K, [300, 280, 320], mode, K=K, kinds=K != 1)
    if K == 0:
        case.tracks = [np.zeros((0, 9)) for _ in case.scans]
        case.track_off = np.zeros(4, dtype=np.int64)
    split, items = run_case(case, dev, "K = %d %s" % (K, mode))
    ref = case.reference()
    fg = sum(int((it[6] != 1).sum()) for it in items)
    gates = np.concatenate([r[2]["margins"]["gate"] for r in ref])
    print("K = %d: %d foreground points, %d boxes with points, %d of them past the gate" % (K, fg, gates.size, (gates > 0).sum()))
    if K >= 8:
        assert fg > 0 and (gates > 0).any() and (gates < 0).any()
        boxes = [P.match_boxes(case.tracks[a], case.tracks[b], product_calib(case), product_calib(case)) for a, b in case.pairs]
        assert max(len(b) for b in boxes) >= (41 if K == 50 else 7)         # kind 1 has no match; the far box has
    else:
        assert (fg > 0 and (gates < 0).all()) if K == 1 else fg == 0


def test_later_box_wins_and_an_empty_frame_of_tracks(dev):
    """Two overlapping boxes in both orders (test_prepare_ref's hand case, on the GPU), and tracks in one frame only"""
    box = lambda x, y, z, id, score=0.75: [1.0, 1.0, 2.0, x, y, z, -np.pi / 2, score, id]
    pts = PC.rows([(0.5, 0, 2), (-0.5, 0, 2), (1.5, 0, 2), (3, 1, 2)])
    l1 = np.array([box(0, 0, 2, 1, 0.5), box(1, 0, 2, 2, 0.25)])
    l2 = np.array([box(0, 1, 2, 1), box(1, 0, 2.5, 2)])
    for first, labels, masks in ((l1, [[0, 0, 0.5], [0, 1, 0], [0, 0, 0.5], [0, 0, 0]], [0.75, 0.5, 0.75, 1]),
                                 (l1[::-1], [[0, 1, 0], [0, 1, 0], [0, 0, 0.5], [0, 0, 0]], [0.5, 0.5, 0.75, 1])):
        case = PC.simple_case([pts, pts, pts], "pseudo", tracks=[first, l2, np.zeros((0, 9))])
        case.odom[:] = np.eye(4)
        split, items = run_case(case, dev, "later box wins")
        tab1 = split.tab1.cpu().numpy()
        assert tab1[:4, 6:9].tolist() == labels and tab1[:4, 9].tolist() == masks
        assert not tab1[4:, 6:9].any() and (tab1[4:, 9] == 1).all()        # pair (1, 2): frame 2 has no rows, nothing is foreground


def test_both_sides_of_the_five_centimetre_rule(dev):
    """Boxes that move with the static world plus 0.04 m or 0.06 m under a turning, moving sensor ('gt'): foreground points that keep
    the box's label (moving) and foreground points that take the rigid flow and mask 1 (not moving), both present by construction"""
    case = PC.near_static_case()
    (_, item, extra), = case.reference()
    moving = extra["margins"]["moving"]
    assert (moving > 0).sum() >= 20 and (moving < 0).sum() >= 20, moving
    assert np.abs(moving).min() > 0.005                                    # |push| is 0.04 or 0.06: a centimetre from the threshold
    split, items = run_case(case, dev, "0.05 m rule")
    mask = split.tab1[:, 9].cpu().numpy()
    assert (mask != 1).sum() == (moving > 0).sum()                         # scores are below 1: a moving point's mask is 1 - score


def test_a_frame_of_the_largest_size(dev):
    """16384 kept points in frame 1 (every thread owns 64 of them: all 64 bits of its in-box and foreground masks) with boxes over the
    first, the middle and the last rows; one point more is refused (test_a_frame_above_the_cap_is_refused)"""
    case = PC.full_frame_case()
    (_, item, extra), = case.reference()
    assert len(item[0]) == D.DRAW_MAX_POINTS and (extra["margins"]["gate"] > 0).sum() == 1
    row = lambda r: r * 128
    assert item[5][[row(0), row(60), row(70), row(119), row(120), 16383]].tolist() == \
        [[0.5, 0, 0], [0, 0, np.float32(0.3)], [0, 0, np.float32(0.3)], [0.5, 0, 0], [0, np.float32(0.4), 0], [0, np.float32(0.4), 0]]
    split, items = run_case(case, dev, "full frame")
    assert split.max_points == D.DRAW_MAX_POINTS


def test_scans_without_any_row(dev):
    """Every scan empty: nothing is kept, nothing is read, and a split cannot be built from it"""
    case = PC.simple_case([np.zeros((0, 5), np.float32)] * 3)
    calib = product_calib(case)
    keep, uv, count = P.count_scans(case.packed_scans, case.scan_off, calib, dev)
    assert keep.shape == (0,) and uv.shape == (0, 2) and count.tolist() == [0, 0, 0]
    pc, ft, n = P.filter_scans(case.packed_scans, case.scan_off, calib, dev)
    assert pc.shape == (3, 3, 1) and not pc.any() and not ft.any() and n.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="min_points"):
        build(case, dev).finish()


# ---- modes, images, chunks ------------------------------------------------------------------------------------------------------------
def test_flow_images_are_read_per_pair(dev):
    case = PC.chain(71, [200, 257, 180, 150], "pseudo", K=4, flows=2)     # pairs 0, 1 with an image, pair 2 without
    split, items = run_case(case, dev, "flow images")
    n1 = [it[0].shape[0] for it in items]
    opt = split.tab1[:, 12:14].cpu().numpy()
    assert np.abs(opt[:n1[0] + n1[1]]).min() > 0 and not opt[n1[0] + n1[1]:].any()
    none = PC.chain(71, [200, 257, 180, 150], "pseudo", K=4)
    assert not run_case(none, dev, "no image")[0].tab1[:, 12:14].any()


@pytest.mark.parametrize("mode", ["gt", "pseudo"])
def test_two_adds_are_one_add_bit_for_bit(dev, mode):
    case = PC.chain(81, [150, 200, 170, 260, 140, 210], mode, K=4, pairs=[(0, 1), (1, 2), (3, 4), (4, 5), (3, 5)],
                    flows=1 if mode == "pseudo" else 0)
    clip = np.array([7, 7, 9, 9, 9])
    one, kept1 = build(case, dev, clip=clip).finish()
    two, kept2 = build(case, dev, chunks=[((0, 3), (0, 2)), ((3, 6), (2, 5))], clip=clip).finish()
    check_split(case, one, kept1, "one add")
    assert kept1.tolist() == kept2.tolist() == [0, 1, 2, 3, 4] and one.clips == two.clips == [(0, 2), (2, 5)]
    for k in ("tab1", "tab2", "off1", "off2", "trans", "interval"):
        a, b = getattr(one, k), getattr(two, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert one.max_points == two.max_points


def test_min_points_drops_pairs_and_clips_follow(dev):
    case = PC.chain(91, [400, 30, 380, 350, 20, 390], "gt", K=3)
    ref = case.reference()
    n1, n2 = [r[1][0].shape[0] for r in ref], [r[1][1].shape[0] for r in ref]
    cut = (max(n1[1], n1[4]) + 1, max(n2[0], n2[3]) + 1)
    split, kept = build(case, dev, clip=np.array([1, 1, 1, 2, 2])).finish(min_points=cut)
    assert kept.tolist() == [2] and split.clips == [(0, 1)]
    check_split(case, split, kept, "min_points", min_points=cut)
    split, kept = build(case, dev, clip=np.array([1, 1, 1, 2, 2])).finish(min_points=(1, cut[1]))
    assert kept.tolist() == [1, 2, 4] and split.clips == [(0, 2), (2, 3)]
    check_split(case, split, kept, "min_points", min_points=(1, cut[1]))
    split, kept = build(case, dev, clip=np.array([5, 5, 5, 5, 5])).finish(min_points=(1, cut[1]))
    assert kept.tolist() == [1, 2, 4] and split.clips == [(0, 2), (2, 3)]              # one tag: the clip is cut where pair 3 was dropped


def test_a_frame_above_the_cap_is_refused(dev):
    n = D.DRAW_MAX_POINTS + 1
    big = PC.rows([(0.0001 * (i % 10000) - 0.5, 0.2, 2.0) for i in range(n)])
    case = PC.simple_case([big, big[:10]])
    with pytest.raises(ValueError, match="more than"):
        build(case, dev)
    assert P.filter_scans(case.packed_scans, case.scan_off, product_calib(case), dev, nmax=16)[2].tolist() == [16, 10]      # truncated


# ---- the inference front end ----------------------------------------------------------------------------------------------------------
def test_filter_scans_pads_with_zeros_whatever_the_input_holds(dev):
    """Raw scans with NaN rows between and behind the valid ones and NaN in the extra columns: the kept rows in order, then zeros"""
    rng = np.random.default_rng(5)
    case = PC.chain(101, EDGES, "gt", K=0, cols=7)
    scans = []
    for s in case.scans:
        s = np.concatenate([s, np.full((7, 7), np.nan, np.float32)])
        s[rng.random(len(s)) < 0.2] = np.nan
        s[:, 5:] = np.nan
        scans.append(s)
    case = PC.Case(scans, case.calib, case.odom, case.tracks, case.pairs, "gt")
    calib = product_calib(case)
    pc, ft, n = P.filter_scans(case.packed_scans, case.scan_off, calib, dev)
    kept = [R.filter_scan(s, c)[0] for s, c in zip(case.scans, case.calib)]
    nmax = max(len(k) for k in kept)
    assert pc.shape == ft.shape == (len(scans), 3, nmax) and n.dtype == torch.int32 and n.tolist() == [len(k) for k in kept]
    for given in (None, nmax + 37):
        if given:
            pc, ft, n = P.filter_scans(case.packed_scans, case.scan_off, calib, dev, nmax=given)
            assert pc.shape == (len(scans), 3, given) and n.tolist() == [len(k) for k in kept]
        for s, k in enumerate(kept):
            rows = case.scans[s][k]
            assert np.array_equal(bits(pc[s, :, :len(k)].cpu().numpy()), bits(rows[:, 0:3].T)), s
            assert np.array_equal(bits(ft[s, :, :len(k)].cpu().numpy()), bits(rows[:, [4, 3, 3]].T)), s
            assert not bits(pc[s, :, len(k):].cpu().numpy()).any() and not bits(ft[s, :, len(k):].cpu().numpy()).any(), s    # +0.0 exactly


def _net(manifest, golden_dir, args, dev):
    import os
    from cmflow_amd import synth
    from cmflow_amd.cmflow import CMFlow
    net = CMFlow(args)
    net.load_state_dict(synth.synth_state_dict(manifest, seed=1234, calib=os.path.join(golden_dir, "bn_calib_cmflow.npz")))
    return net.to(dev).eval()


def test_raw_scans_into_forward_ragged(dev, manifest, golden_dir, args):
    """filter_scans -> pair_batch -> CMFlow.forward_ragged, bit-identical to the same call on a batch assembled from the restatement"""
    case = PC.chain(111, [300, 420, 256, 350], "gt", K=0)
    pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 0]])
    pc, ft, n = P.filter_scans(case.packed_scans, case.scan_off, product_calib(case), dev)
    batch = P.pair_batch(pc, ft, n, pairs)
    kept = [s[R.filter_scan(s, c)[0]] for s, c in zip(case.scans, case.calib)]
    nmax = max(len(k) for k in kept)
    assert min(len(k) for k in kept) >= 8

    def pad(rows):
        out = np.zeros((3, nmax), np.float32)
        out[:, :len(rows)] = rows.T
        return out

    mk = lambda cols, side: torch.from_numpy(np.stack([pad(kept[p[side]][:, cols]) for p in pairs])).to(dev)
    want = dict(pc1=mk([0, 1, 2], 0), pc2=mk([0, 1, 2], 1), ft1=mk([4, 3, 3], 0), ft2=mk([4, 3, 3], 1),
                n1=torch.tensor([len(kept[a]) for a, _ in pairs], dtype=torch.int32, device=dev),
                n2=torch.tensor([len(kept[b]) for _, b in pairs], dtype=torch.int32, device=dev))
    for k, w in want.items():
        assert batch[k].dtype == w.dtype and torch.equal(batch[k], w), k
    net = _net(manifest, golden_dir, args, dev)
    with torch.no_grad():
        got = net.forward_ragged(batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"], batch["n1"], batch["n2"], validate=True)
        ref = net.forward_ragged(want["pc1"], want["pc2"], want["ft1"], want["ft2"], want["n1"], want["n2"], validate=True)
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and torch.equal(g, r) and torch.isfinite(g.float()).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six(dev):
    """Six frames with moving (annotated: score 1) boxes in every one"""
    case = PC.chain(121, [420, 380, 450, 400, 390, 440, 410], "gt", K=6, score=1.0, kinds=False)
    split, kept = build(case, dev, clip=np.array([0, 0, 0, 1, 1, 1])).finish(min_points=(40, 40))
    return case, split, kept


def test_built_split_draws_sweeps_and_runs_an_epoch(six, dev):
    case, split, kept = six
    items = check_split(case, split, kept, "six", min_points=(40, 40))
    assert kept.tolist() == list(range(6)) and split.clips == [(0, 3), (3, 6)]
    assert all((it[6] == 0).sum() > 0 and (it[6] == 1).sum() > 0 for it in items)      # moving and static points in every frame
    host = D.DeviceSplit.from_items(items, dev)
    copies = ("pc1", "pc2", "ft1", "ft2", "fg_mask", "interval", "radar_u", "radar_v", "opt_flow", "n1", "n2")
    seen = []
    for a, b in zip(split.sweep(4), host.sweep(4)):
        seen += a["frames"].tolist()
        assert all(torch.equal(a[k], b[k]) for k in copies)
        assert_one_ulp(a["flow_label"].cpu().numpy(), b["flow_label"].cpu().numpy(), "sweep labels")
    assert seen == list(range(6))
    a, b = split.draw_frames([5, 0, 3]), host.draw_frames([5, 0, 3])
    assert all(torch.equal(a[k], b[k]) for k in copies)
    steps = list(split.epoch(2, 128, seed=3, epoch=1))
    assert len(steps) == 3
    for got, want in zip(steps, host.epoch(2, 128, seed=3, epoch=1)):
        assert got["pc1"].shape == (2, 3, 128) and torch.equal(got["idx1"], want["idx1"]) and torch.equal(got["pc2"], want["pc2"])
        assert torch.isfinite(got["flow_label"]).all()
    assert len(list(split.epoch_clips(1, 3, 64, seed=1, epoch=0))) == 2


def test_eval_split_on_a_built_split(six, dev, manifest, golden_dir, args):
    case, split, kept = six
    got = EV.eval_split(_net(manifest, golden_dir, args, dev), split, 4)
    numbers = np.array([float(v) for d in got[:3] for v in d.values()])
    print("eval_split on a built split:", numbers)
    assert numbers.shape == (14,) and np.isfinite(numbers).all()
    assert torch.equal(got[3].reshape(6, 16), split.trans) and torch.isfinite(got[4]).all()


def test_save_and_load_round_trip_a_built_split(six, dev, tmp_path):
    case, split, kept = six
    path = str(tmp_path / "built.pt")
    split.save(path)
    back = D.DeviceSplit.load(path, dev)
    for k in ("tab1", "tab2", "off1", "off2", "trans", "interval"):
        a, b = getattr(split, k), getattr(back, k)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert back.clips == split.clips and back.max_points == split.max_points and len(back) == 6
