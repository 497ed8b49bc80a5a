"""CPU: what cmflow_amd/instances.py means and what its host side does.  The numpy restatement (tests/instances_ref.py) is held against
a second, differently written implementation and against worlds whose answer is known without either; the special frames of the
GPU tests' case are checked to be what they are for; every refusal of ``cluster`` comes before any launch; ``instance_colors`` and
``agreement`` against loops; and the reference's own saved frames go through the restatement.  The device code is tied to the
restatement bit for bit in tests/test_gpu_instances.py."""
import inspect
import os

import numpy as np
import pytest
import torch

import instances_ref as ref
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import results as R
from cmflow_amd import vis

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32, f64 = np.float32, np.float64


def _same(a, b, what):
    assert a["count"] == b["count"], what
    for k in ("label", "kind", "size", "seed"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("centroid", "disp", "lo", "hi"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


@pytest.fixture(scope="module")
def case():
    return ref.build_case()


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pred", "gt"])
def test_restatement_agrees_with_the_breadth_first_search(case, which):
    off1, pos, flow, moving, T = ref.case_arrays(case, which)
    for f in range(len(case)):
        a, b = off1[f], off1[f + 1]
        for eps, min_points, weight in ((1.0, 1, 0.0), (1.0, 4, 2.5), (2.0, 2, 0.0), (1.0, 4, 0.0), (2.0, 4, 2.5)):
            if f == ref.F_CAP and (eps, min_points) != (1.0, 4):
                continue                                                     # the largest frame once per weight: the others cover the rest
            args = (pos[a:b], flow[a:b], moving[a:b], T[f], f64(eps * eps), f64(weight * weight), min_points)
            _same(ref.cluster_frame(*args), ref.cluster_frame_bfs(*args), (which, f, eps, min_points, weight))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_known_worlds_come_back_as_they_were_made(seed):
    """Objects further than 3 eps apart, each connected by steps of at most 0.6 eps: with min_points <= 2 the instances ARE the objects,
    numbered by their lowest point -- at any flow weight, since an object's points share one velocity."""
    eps = (0.8, 2.0)[seed % 2]
    pos, flow, moving, T, owner = ref.known_world(seed, eps)
    want = ref.known_labels(owner, moving)
    assert want.max() == 4 and (want[~moving] == -1).all()
    for fn in (ref.cluster_frame, ref.cluster_frame_bfs):
        for min_points, weight in ((1, 0.0), (2, 0.0), (2, 1.5)):
            got = fn(pos, flow, moving, T, f64(eps * eps), f64(weight * weight), min_points)
            assert np.array_equal(got["label"], want), (fn.__name__, min_points, weight)
            assert got["count"] == 5 and (got["kind"][moving] == ref.CORE).all() and (got["kind"][~moving] == ref.NONE).all()
            for c in range(5):
                mem = np.flatnonzero(want == c)
                assert got["size"][c] == len(mem) and got["seed"][c] == mem[0]
                assert np.abs(got["centroid"][c] - pos[mem].astype(f64).mean(0)) .max() < 1e-5
                assert np.abs(got["disp"][c] - flow[mem[0]]).max() < 1e-5      # identity ego-motion: d is the flow
                assert np.array_equal(got["lo"][c], pos[mem].min(0)) and np.array_equal(got["hi"][c], pos[mem].max(0))
            assert (got["size"][5:] == 0).all() and (got["seed"][5:] == -1).all() and not got["centroid"][5:].any()


def test_the_special_frames_are_what_they_are_for(case):
    run = lambda which, f, eps, mp, w: ref.cluster_frame(*[x[off1[f]:off1[f + 1]] for x in (pos, flow, moving)], T[f], f64(eps * eps), f64(w * w), mp)
    for which in ("pred", "gt"):
        off1, pos, flow, moving, T = ref.case_arrays(case, which)
        assert np.diff(off1).tolist() == list(ref.COUNTS)
        counts = [int(moving[off1[f]:off1[f + 1]].sum()) for f in range(len(case))]
        assert counts[ref.F_ONE] == 1 and counts[ref.F_STATIC] == 0 and counts[ref.F_ALL] == 65 and counts[ref.F_CAP] == 1024
        assert 0 < counts[ref.F_MIXED] < 97
        # one candidate: an instance of its own at min_points 1, noise above
        assert run(which, ref.F_ONE, 1.0, 1, 0.0)["count"] == 1 and run(which, ref.F_ONE, 1.0, 2, 0.0)["kind"].tolist() == [ref.NOISE]
        assert run(which, ref.F_STATIC, 2.0, 1, 0.0)["count"] == 0
        # the grid: distances exactly on eps -- a corner has 3 neighbours at eps 1 (<=), 1 under a strict compare
        idx = np.flatnonzero(moving[off1[ref.F_GRID]:off1[ref.F_GRID + 1]])
        p = pos[off1[ref.F_GRID]:off1[ref.F_GRID + 1]][idx]
        for w in ref.FLOW_WEIGHTS:
            d2 = ref.pair_d2(p, ref.displacement(p, flow[off1[ref.F_GRID]:off1[ref.F_GRID + 1]][idx], T[ref.F_GRID]), f64(w * w))
            assert (d2 == 1.0).sum() == 2 * 2 * 56 and (d2 == 4.0).sum() == 2 * 2 * 48, w
        g = run(which, ref.F_GRID, 1.0, 4, 0.0)                              # corners have 3 neighbours: borders; everything is one instance
        assert g["count"] == 1 and (g["kind"] == ref.BORDER).sum() == 4 and g["size"][0] == 64
        # the chain: one instance at eps 1, met end to end; every second neighbour only at eps 2
        c = run(which, ref.F_CHAIN, 1.0, 2, 2.5)
        assert c["count"] == 1 and c["size"][0] == 300 and c["seed"][0] == 0
        assert run(which, ref.F_CHAIN, 1.0, 4, 0.0)["count"] == 0            # three neighbours at most
        # the bridge: a border point that ties between two instances goes with the lower-indexed CORE, which is instance 1's
        b = run(which, ref.F_BRIDGE, 1.0, 4, 2.5)
        x = len(ref.BRIDGE_A) + len(ref.BRIDGE_B)
        assert b["count"] == 2 and b["kind"][x] == ref.BORDER and b["label"][x] == 1 and b["label"][x - 1] == 0 and b["label"][5] == 1
        assert b["seed"][:2].tolist() == [0, 5] and b["size"][:2].tolist() == [6, 7]
        assert run(which, ref.F_BRIDGE, 1.0, 2, 0.0)["size"][0] == 13         # the bridge point is a core point itself: one instance
        # twins: coincident points are neighbours at distance 0
        t = run(which, ref.F_TWINS, 1.0, 2, 0.0)
        assert (t["kind"] == ref.CORE).all()
        # overlap: one object by position, two once the displacement counts
        o0, o1 = run(which, ref.F_OVERLAP, 1.0, 4, 0.0), run(which, ref.F_OVERLAP, 1.0, 4, 2.5)
        assert o0["size"][0] >= 110 and set(o0["label"][:120].tolist()) <= {0, -1}
        lab0, lab1 = o1["label"][0:120:2], o1["label"][1:120:2]
        assert o1["count"] >= 2 and (lab0 >= 0).sum() >= 50 and (lab1 >= 0).sum() >= 50
        assert not (set(lab0[lab0 >= 0].tolist()) & set(lab1[lab1 >= 0].tolist()))


def test_full_restatement_packs_like_the_split(case):
    off1, pos, flow, moving, T = ref.case_arrays(case, "gt")
    ids = [ref.F_BRIDGE, ref.F_PAIR, ref.F_BRIDGE]
    out = ref.cluster(off1, pos, flow, moving, T, ids, 1.0, 2, 0.0)
    again = ref.cluster(off1, pos, flow, moving, T, ids, 1.0, 2, 0.0, frame_fn=ref.cluster_frame_bfs)
    for k in ref.KEYS + ("count",):
        assert np.array_equal(out[k], again[k]), k
    chosen = np.zeros(int(off1[-1]), bool)
    for f in ids:
        chosen[off1[f]:off1[f + 1]] = True
    assert (out["label"][~chosen] == -1).all() and not out["kind"][~chosen].any() and not out["seed"][~chosen].any()
    assert out["count"].nonzero()[0].tolist() == [ref.F_BRIDGE, ref.F_PAIR] and out["count"][ref.F_PAIR] == 1


# ---- host logic -------------------------------------------------------------------------------------------------------------------------
def _cpu_split(counts, seed=0):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s).astype(f32)
    items = [(r(n, 3), r(4, 3), r(n, 3), r(4, 3), np.eye(4, dtype=f32), r(n, 3), (rng.random(n) < 0.5).astype(f32), 0.1, r(n), r(n), r(n, 2))
             for n in counts]
    return D.DeviceSplit.from_items(items, "cpu")


def test_every_refusal_comes_before_any_launch():
    split = _cpu_split([5, 1, 9, 1025])
    store = R.SplitResults.empty(split)
    with pytest.raises(ValueError, match="which"):
        I.cluster(split, store, which="label")
    with pytest.raises(ValueError, match="store"):
        I.cluster(split, None, which="pred")
    with pytest.raises(ValueError, match="not the one"):
        I.cluster(_cpu_split([5, 1, 9, 1024]), store)                       # as many frames, another row count
    with pytest.raises(ValueError, match="not the one"):
        I.cluster(_cpu_split([5, 1, 1034]), store)                          # as many rows, another frame count
    for eps in (0.0, -1.0, float("nan"), float("inf"), None, "2"):
        with pytest.raises(ValueError, match="eps"):
            I.cluster(split, None, which="gt", eps=eps, frames=[0])
    for weight in (-0.5, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="flow_weight"):
            I.cluster(split, None, which="gt", flow_weight=weight, frames=[0])
    for min_points in (0, -3, 2.0, None, True):
        with pytest.raises(ValueError, match="min_points"):
            I.cluster(split, None, which="gt", min_points=min_points, frames=[0])
    for frames in ([4], [-1], torch.tensor([0, 7])):
        with pytest.raises(ValueError, match="outside"):
            I.cluster(split, None, which="gt", frames=frames)
    with pytest.raises(ValueError, match="int64"):
        I.cluster(split, None, which="gt", frames=torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError, match="1025 points"):
        I.cluster(split, None, which="gt")                                  # frames=None selects the large frame too
    with pytest.raises(ValueError, match="1025 points"):
        I.cluster(split, None, which="gt", frames=[1, 3])
    with pytest.raises(ValueError, match="no results"):
        I.cluster(split, store, frames=[0, 2])                              # nothing is done
    store.done[:2] = 1
    with pytest.raises(ValueError, match="no results"):
        I.cluster(split, store, frames=[1, 2])
    # everything in order: only the device is wrong -- and that is the LAST refusal
    with pytest.raises(RuntimeError, match="GPU"):
        I.cluster(split, store, frames=[1, 0])
    with pytest.raises(RuntimeError, match="GPU"):
        I.cluster(split, None, which="gt", frames=[0, 1, 2], eps=0.5, min_points=7, flow_weight=0.0)
    with pytest.raises(RuntimeError, match="GPU"):
        store.instances(split, frames=[0], flow_weight=3)
    assert list(inspect.signature(I.cluster).parameters) == ["split", "store", "which", "eps", "min_points", "flow_weight", "frames"]
    sig = inspect.signature(I.cluster).parameters
    assert (sig["which"].default, sig["eps"].default, sig["min_points"].default, sig["flow_weight"].default) == ("pred", 2.0, 2, 0.0)
    assert I.MAX_POINTS == ref.MAX_POINTS and (I.NONE, I.NOISE, I.BORDER, I.CORE) == (ref.NONE, ref.NOISE, ref.BORDER, ref.CORE)


def test_instance_colours_are_the_loops():
    rng = np.random.default_rng(3)
    label = np.concatenate((np.arange(-1, 30), rng.integers(-1, 1024, 200))).astype(np.int32)
    kind = rng.integers(0, 4, label.size).astype(np.uint8)
    got = vis.instance_colors(torch.from_numpy(label), torch.from_numpy(kind)).numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, ref.instance_colors(label, kind))
    assert vis.INSTANCE_PALETTE == ref.PALETTE and len(set(ref.PALETTE)) == 12
    assert vis.LAYERS == ("flow", "flow_gt", "seg", "seg_gt")
    one = vis.instance_colors(torch.tensor([13, 13, 13, -1], dtype=torch.int32), torch.tensor([3, 2, 1, 0], dtype=torch.uint8)).tolist()
    assert one == [list(ref.PALETTE[1]), list(ref.PALETTE[1]), [200, 200, 200], [120, 120, 120]]


def _as_result(off1, ids, out, which):
    """A FrameInstances on the CPU from the restatement's packed outputs."""
    t = torch.from_numpy
    tables = tuple(t(out[k]) for k in I.TABLES)
    return I.FrameInstances(t(off1.astype(np.int32)), t(np.asarray(ids, dtype=np.int64)), t(out["label"]), t(out["kind"]), t(out["count"]), tables,
                            torch.full((len(off1) - 1,), 0.1), which, 1.0, 2, 0.0, off1, np.asarray(ids, dtype=np.int64))


def test_agreement_is_the_loops(case):
    ids = [ref.F_MIXED, ref.F_STATIC, ref.F_OVERLAP, ref.F_BRIDGE, ref.F_ALL, ref.F_MIXED]
    sides = {}
    for which in ("pred", "gt"):
        off1, pos, flow, moving, T = ref.case_arrays(case, which)
        sides[which] = ref.cluster(off1, pos, flow, moving, T, ids, 2.0, 2, 0.0)
    pred, gt = _as_result(off1, ids, sides["pred"], "pred"), _as_result(off1, ids, sides["gt"], "gt")
    got = I.agreement(pred, gt)
    want = ref.agreement(off1, ids, sides["pred"]["label"], sides["pred"]["size"], sides["gt"]["label"], sides["gt"]["size"])
    assert got["iou"].dtype == torch.float64 and got["iou"].shape == (len(ids),)
    iou, held = got["iou"].numpy(), ~np.isnan(want)
    assert np.array_equal(np.isnan(iou), ~held) and np.array_equal(iou[held].view(np.uint64), want[held].view(np.uint64)), (iou, want)
    assert np.isnan(want[1]) and ((want > 0) & (want < 1)).sum() >= 2 and want[0] == want[5]
    assert got["count_pred"].tolist() == sides["pred"]["count"][ids].tolist() and got["count_gt"].tolist() == sides["gt"]["count"][ids].tolist()
    same = I.agreement(gt, gt)["iou"].numpy()
    assert np.array_equal(np.isnan(same), np.isnan(want)) and (same[~np.isnan(same)] == 1.0).all()
    with pytest.raises(ValueError):
        I.agreement(pred, _as_result(off1, ids[:-1], sides["gt"], "gt"))
    with pytest.raises(ValueError):
        I.agreement(pred, sides["gt"])
    # frame(): the first K rows of the tables, the frame's points; velocity(): disp over the interval
    fr = gt.frame(ref.F_BRIDGE)
    K = int(sides["gt"]["count"][ref.F_BRIDGE])
    assert K >= 1 and fr["size"].shape == (K,) and fr["centroid"].shape == (K, 3) and fr["label"].shape == (257,) and int(fr["count"]) == K
    assert torch.equal(gt.velocity(), gt.disp / torch.tensor(0.1)) and gt.velocity().shape == gt.disp.shape and gt.velocity().abs().max() > 0
    with pytest.raises(IndexError):
        gt.frame(len(case))


# ---- the reference's own saved frames ---------------------------------------------------------------------------------------------------
def test_saved_frames_go_through_the_restatement():
    g = np.load(os.path.join(GOLDEN, "saved_results_delft_12_w12.npz"))
    off, pc1, pred_f, pred_m, pred_t = g["off"], g["pc1"], g["pred_f"], g["pred_m"], g["pred_t"]
    assert off.shape == (13,) and int(g["first_frame"]) == 727
    out = ref.cluster(off, pc1, pred_f, pred_m == 0, pred_t, list(range(12)), 2.0, 2, 0.0)
    again = ref.cluster(off, pc1, pred_f, pred_m == 0, pred_t, list(range(12)), 2.0, 2, 0.0, frame_fn=ref.cluster_frame_bfs)
    for k in ref.KEYS + ("count",):
        assert np.array_equal(out[k], again[k]), k
    for f in range(12):
        a, b = off[f], off[f + 1]
        K = int(out["count"][f])
        assert out["size"][a:a + K].tolist() == ref.SAVED_SIZES[f], (f, out["size"][a:a + K].tolist())
        assert int((out["kind"][a:b] == ref.NOISE).sum()) == ref.SAVED_NOISE[f], f
        assert not (out["kind"][a:b] == ref.BORDER).any()
        assert int((out["kind"][a:b] != ref.NONE).sum()) == int((pred_m[a:b] == 0).sum()) == sum(ref.SAVED_SIZES[f]) + ref.SAVED_NOISE[f]
