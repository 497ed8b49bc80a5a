"""GPU: moving-object instances of a test run (cmflow_amd/instances.py) -- cmf_cluster_moving bit for bit against its numpy
restatement (tests/instances_ref.py) over eps, min_points, flow_weight and both sources, the C entry point on sentinel-filled
buffers, selections, the reference's own saved frames, the pictures, the agreement measure, and that none of it waits for the
device.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import instances_ref as ref
import vis_ref
from cmflow_amd import _lib
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import results as R
from cmflow_amd import vis

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
INT_KEYS, FLOAT_KEYS = ("label", "kind", "count", "size", "seed"), ("centroid", "disp", "lo", "hi")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _filled(frames, dev):
    split = D.DeviceSplit.from_items(ref.as_items(frames), dev)
    store = R.SplitResults.empty(split)
    store.flow.copy_(torch.from_numpy(np.concatenate([fr["flow"] for fr in frames])))
    store.mask.copy_(torch.from_numpy(np.concatenate([fr["mask"] for fr in frames])))
    store.pred_trans.copy_(torch.from_numpy(np.stack([fr["pred_t"] for fr in frames])))
    store.done.fill_(1)
    return split, store


@pytest.fixture(scope="module")
def case(dev):
    frames = ref.build_case()
    split, store = _filled(frames, dev)
    assert split.counts_host[0].tolist() == list(ref.COUNTS)
    return frames, split, store


_wants, _d2 = {}, {"pred": {}, "gt": {}}


def _want(frames, which, eps, min_points, weight):
    """The restatement of the whole case, computed once per combination (the pair distances once per source and weight)."""
    key = (which, eps, min_points, weight)
    if key not in _wants:
        _wants[key] = ref.cluster(*ref.case_arrays(frames, which), list(range(len(frames))), eps, min_points, weight, cache=_d2[which])
    return _wants[key]


def _host(inst):
    return {k: getattr(inst, k).cpu().numpy() for k in INT_KEYS + FLOAT_KEYS}


def _same(got, want, what, rows=slice(None)):
    assert got["label"].dtype == np.int32 and got["kind"].dtype == np.uint8 and got["count"].dtype == np.int32 and got["centroid"].dtype == f32
    for k in INT_KEYS:
        g, w = (got[k], want[k]) if k == "count" else (got[k][rows], want[k][rows])
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:4].tolist())
    for k in FLOAT_KEYS:
        bad = np.argwhere(got[k][rows].view(np.uint32) != want[k][rows].view(np.uint32))
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist(), got[k][rows][bad[:4, 0]].tolist(), want[k][rows][bad[:4, 0]].tolist())


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", ref.FLOW_WEIGHTS)
@pytest.mark.parametrize("which", ["pred", "gt"])
def test_cluster_is_the_restatement(case, which, weight):
    frames, split, store = case
    for eps in ref.EPS:
        for min_points in ref.MIN_POINTS:
            inst = I.cluster(split, store if which == "pred" else None, which=which, eps=eps, min_points=min_points, flow_weight=weight)
            assert inst.label.is_cuda and inst.frames.tolist() == list(range(len(frames))) and inst.off is split.off1
            _same(_host(inst), _want(frames, which, eps, min_points, weight), (which, eps, min_points, weight))
    # the case reaches what it is for: borders, noise, a frame with hundreds of instances, the chain as ONE instance, the tie
    want = _want(frames, which, 1.0, 4, weight)
    off = np.concatenate(([0], np.cumsum(ref.COUNTS)))
    assert (want["kind"] == ref.BORDER).sum() >= 9 and (want["kind"] == ref.NOISE).sum() > 20
    x = off[ref.F_BRIDGE] + len(ref.BRIDGE_A) + len(ref.BRIDGE_B)
    assert want["kind"][x] == ref.BORDER and want["label"][x] == 1
    chain = _want(frames, which, 1.0, 2, weight)
    assert chain["count"][ref.F_CHAIN] == 1 and chain["size"][off[ref.F_CHAIN]] == 300
    assert _want(frames, which, 1.0, 1, weight)["count"][ref.F_CAP] > 100
    if which == "pred":
        got = _host(store.instances(split, eps=2.0, min_points=4, flow_weight=weight))
        _same(got, _want(frames, "pred", 2.0, 4, weight), "store.instances")


# ---- 2. the C entry point on sentinel-filled buffers ------------------------------------------------------------------------------------
def _call(split, store, off, ids, nsel, rows, eps, min_points, weight, dev):
    """cmf_cluster_moving itself over the frames that ``off`` declares; outputs of ``rows`` rows (>= total) and a count of
    len(off) + 4 entries, pre-filled with sentinels -> host arrays."""
    i32, u8, f = torch.int32, torch.uint8, torch.float32
    off_d = torch.tensor(off, dtype=i32, device=dev)
    sel = None if ids is None else torch.tensor(ids, dtype=torch.int64, device=dev)
    out = {"label": torch.full((rows,), -99, dtype=i32, device=dev), "kind": torch.full((rows,), 77, dtype=u8, device=dev),
           "count": torch.full((len(off) + 4,), -5, dtype=i32, device=dev), "size": torch.full((rows,), -98, dtype=i32, device=dev),
           "seed": torch.full((rows,), -97, dtype=i32, device=dev)}
    for k in FLOAT_KEYS:
        out[k] = torch.full((rows, 3), -7.5, dtype=f, device=dev)
    p = _lib.dev_ptr
    _lib.check(_lib.lib().cmf_cluster_moving(
        nsel, len(off) - 1, p(sel, torch.int64), p(off_d, i32), split.tab1.shape[0], p(split.tab1, f), split.tab1.shape[1], p(store.flow, f),
        p(store.mask, u8), p(store.pred_trans.reshape(-1, 16), f), 0, float(eps) * float(eps), float(weight) * float(weight), min_points,
        p(out["label"], i32), p(out["kind"], u8), p(out["count"], i32), p(out["size"], i32), p(out["seed"], i32),
        *(p(out[k], f) for k in FLOAT_KEYS), _lib.stream_ptr()), "cmf_cluster_moving")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


SENTINEL = {"label": -99, "kind": 77, "size": -98, "seed": -97, "centroid": -7.5, "disp": -7.5, "lo": -7.5, "hi": -7.5}


def _untouched(got, rows_mask):
    return all((got[k][rows_mask] == v).all() for k, v in SENTINEL.items())


def test_entry_point_writes_its_frames_and_nothing_else(case, dev):
    frames, split, store = case
    F, total = len(frames), split.tab1.shape[0]
    off = np.concatenate(([0], np.cumsum(ref.COUNTS))).tolist()
    eps, mp, w = 1.0, 2, 2.5
    want = _want(frames, "pred", eps, mp, w)
    # ids outside the split are clamped (to frames 0 and 10), one id twice
    ids, clamped = [-5, 6, 99, 3, 3, 8], [0, 6, 10, 3, 3, 8]
    got = _call(split, store, off, ids, len(ids), total + 64, eps, mp, w, dev)
    chosen = np.zeros(total + 64, bool)
    for f in clamped:
        chosen[off[f]:off[f + 1]] = True
        rows = slice(off[f], off[f + 1])
        for k in INT_KEYS[:2] + INT_KEYS[3:] + FLOAT_KEYS:
            assert np.array_equal(got[k][rows], want[k][rows]) if k in INT_KEYS else \
                np.array_equal(got[k][rows].view(np.uint32), want[k][rows].view(np.uint32)), (f, k)
        K = int(want["count"][f])
        assert got["count"][f] == K
        a, b = off[f] + K, off[f + 1]                                        # behind K: empty table rows, as defined
        assert (got["size"][a:b] == 0).all() and (got["seed"][a:b] == -1).all() and not any(got[k][a:b].any() for k in FLOAT_KEYS)
    assert chosen.sum() == sum(ref.COUNTS[f] for f in set(clamped)) and _untouched(got, ~chosen)
    rest = np.ones(len(got["count"]), bool)
    rest[clamped] = False
    assert (got["count"][rest] == -5).all()
    # NULL frames: frames 0 .. nsel-1
    got = _call(split, store, off, None, 3, total + 64, eps, mp, w, dev)
    chosen[:] = False
    chosen[:off[3]] = True
    assert _untouched(got, ~chosen) and got["count"][:3].tolist() == want["count"][:3].tolist() and (got["count"][3:] == -5).all()
    assert np.array_equal(got["label"][:off[3]], want["label"][:off[3]]) and np.array_equal(got["kind"][:off[3]], want["kind"][:off[3]])
    # other frames over the same rows: one declared with 1025 points comes back empty, one whose rows end behind ``total`` owns none
    odd = [0, 1025, off[ref.F_CAP], total, total + 900]                      # 1025 | 88 | the 1024 of the cap frame | 900 behind the end
    eps, mp, w = 2.0, 2, 0.0
    got = _call(split, store, odd, None, 4, total + 64, eps, mp, w, dev)
    pos, flow, mask = (t.cpu().numpy() for t in (split.tab1[:, :3], store.flow, store.mask))
    T = store.pred_trans.cpu().numpy()
    mine = ref.cluster(np.array(odd[:4]), pos, flow, mask == 0, T, [0, 1, 2], eps, mp, w)
    assert got["count"][:4].tolist() == mine["count"].tolist() + [0] and mine["count"][0] == 0 and mine["count"][1] > 0 and mine["count"][2] > 0
    _same({k: (v[:total] if k != "count" else v[:3]) for k, v in got.items()}, mine, "declared frames")
    assert (got["label"][:1025] == -1).all() and not got["kind"][:1025].any() and (got["seed"][:1025] == -1).all() and not got["size"][:1025].any()
    assert _untouched(got, np.arange(total + 64) >= total) and (got["count"][4:] == -5).all()


# ---- 3. selections ----------------------------------------------------------------------------------------------------------------------
def test_a_selections_frames_are_rows_of_the_full_run(case, dev):
    frames, split, store = case
    off = np.concatenate(([0], np.cumsum(ref.COUNTS)))
    ids = [10, 3, 3, 0, 5, 6]
    want = _want(frames, "pred", 1.0, 4, 2.5)
    chosen = np.zeros(off[-1], bool)
    for f in ids:
        chosen[off[f]:off[f + 1]] = True
    for sel in (ids, torch.tensor(ids, dtype=torch.int64), torch.tensor(ids, dtype=torch.int64, device=dev)):
        inst = I.cluster(split, store, eps=1.0, min_points=4, flow_weight=2.5, frames=sel)
        got = _host(inst)
        assert inst.frames.tolist() == ids and len(inst) == len(ids)
        part = {k: (np.where(np.isin(np.arange(len(frames)), ids), v, 0) if k == "count" else v) for k, v in want.items()}
        _same(got, part, "selection", chosen)
        assert (got["label"][~chosen] == -1).all() and not any(got[k][~chosen].any() for k in ("kind", "size", "seed") + FLOAT_KEYS)
    view = inst.frame(5)
    K = int(want["count"][5])
    assert view["size"].tolist() == want["size"][off[5]:off[5] + K].tolist() and view["label"].shape == (257,) and int(view["count"]) == K
    vel = inst.velocity()                                                   # every frame of the case has the interval 0.1 s
    assert vel.shape == inst.disp.shape and torch.equal(vel, inst.disp / split.interval[0]) and float(vel.abs().max()) > 1.0
    empty = I.cluster(split, store, frames=[])
    assert len(empty) == 0 and (empty.label == -1).all() and not empty.count.any()
    store.done[4] = 0
    try:
        with pytest.raises(ValueError):
            I.cluster(split, store, frames=[5, 4])
        assert len(I.cluster(split, store, frames=[5, 3])) == 2
        assert len(I.cluster(split, None, which="gt", frames=[4])) == 1
    finally:
        store.done[4] = 1


# ---- 4. the reference's own saved frames ------------------------------------------------------------------------------------------------
def test_saved_frames_bit_for_bit(golden_dir, dev):
    g = np.load(os.path.join(golden_dir, "saved_results_delft_12_w12.npz"))
    off = g["off"]
    frames = [{"pos1": g["pc1"][a:b], "flow": g["pred_f"][a:b], "label": np.zeros((b - a, 3), f32), "mask": g["pred_m"][a:b],
               "gt_mask": np.ones(b - a, f32), "pred_t": g["pred_t"][k], "gt_t": np.eye(4, dtype=f32)}
              for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]
    split, store = _filled(frames, dev)
    for eps, mp, w in ((2.0, 2, 0.0), (1.0, 3, 1.0)):
        want = ref.cluster(off, g["pc1"], g["pred_f"], g["pred_m"] == 0, g["pred_t"], list(range(12)), eps, mp, w)
        got = _host(I.cluster(split, store, eps=eps, min_points=mp, flow_weight=w))
        _same(got, want, (eps, mp, w))
    got = _host(I.cluster(split, store))                                    # the defaults: eps 2, min_points 2, position alone
    for f in range(12):
        a, b = off[f], off[f + 1]
        assert got["size"][a:a + got["count"][f]].tolist() == ref.SAVED_SIZES[f]
        assert int((got["kind"][a:b] == ref.NOISE).sum()) == ref.SAVED_NOISE[f] and not (got["kind"][a:b] == ref.BORDER).any()


# ---- 5. pictures ------------------------------------------------------------------------------------------------------------------------
def test_render_instances_is_the_rasterisers_restatement(case):
    frames, split, store = case
    inst = I.cluster(split, store, eps=1.0, min_points=4, flow_weight=0.0)
    want = _want(frames, "pred", 1.0, 4, 0.0)
    colors = ref.instance_colors(want["label"], want["kind"])
    assert np.array_equal(vis.instance_colors(inst.label, inst.kind).cpu().numpy(), colors)
    off = np.concatenate(([0], np.cumsum(ref.COUNTS)))
    pos = np.concatenate([fr["pos1"] for fr in frames])
    some = [ref.F_OVERLAP, ref.F_ONE, ref.F_BRIDGE, ref.F_MIXED]
    for w, h, xr, yr in vis_ref.VIEWS:
        view = vis.BevView(w, h, xr, yr, radius_px=1.5, guides=True)
        p = view.kernel_params()
        for sel, ids in ((None, list(range(len(frames)))), (some, some)):
            got = vis.render_instances(inst, split, sel, view)
            assert got.shape == (len(ids), h, w, 3) and got.dtype == torch.uint8 and got.is_cuda
            got = got.cpu().numpy()
            for s, f in enumerate(ids):
                a, b = off[f], off[f + 1]
                pic = vis_ref.render_frame(pos[a:b], colors[a:b], np.ones(b - a, np.uint8), w, h, p, True)
                bad = np.argwhere((got[s] != pic).any(-1))
                assert bad.size == 0, (w, f, len(bad), bad[:6].tolist())
    shown = [{tuple(c) for c in got[s].reshape(-1, 3).tolist()} for s in (0, 3)]      # the overlap frame's object; noise and static points
    assert ref.PALETTE[0] in shown[0] and ref.DIM_GREY in shown[1] and ref.LIGHT_GREY in shown[1]
    part = I.cluster(split, store, eps=1.0, min_points=4, flow_weight=0.0, frames=some)
    assert torch.equal(vis.render_instances(part, split, None, view), vis.render_instances(inst, split, some, view))


# ---- 6. agreement -----------------------------------------------------------------------------------------------------------------------
def test_agreement_is_the_loops(case):
    frames, split, store = case
    off = np.concatenate(([0], np.cumsum(ref.COUNTS)))
    for ids in (None, [8, 4, 8, 1]):
        pred = I.cluster(split, store, eps=2.0, min_points=2, flow_weight=0.0, frames=ids)
        gt = I.cluster(split, None, which="gt", eps=2.0, min_points=2, flow_weight=0.0, frames=ids)
        got = I.agreement(pred, gt)
        assert all(v.is_cuda for v in got.values()) and got["iou"].dtype == torch.float64
        p, q = _want(frames, "pred", 2.0, 2, 0.0), _want(frames, "gt", 2.0, 2, 0.0)
        sel = list(range(len(frames))) if ids is None else ids
        want = ref.agreement(off, sel, p["label"], p["size"], q["label"], q["size"])
        iou, held = got["iou"].cpu().numpy(), ~np.isnan(want)
        assert np.array_equal(np.isnan(iou), ~held) and np.array_equal(iou[held].view(np.uint64), want[held].view(np.uint64)), (iou, want)
        assert got["count_pred"].tolist() == p["count"][sel].tolist() and got["count_gt"].tolist() == q["count"][sel].tolist()
        same = I.agreement(gt, gt)["iou"].cpu().numpy()
        assert np.array_equal(np.isnan(same), ~held) and (same[held] == 1.0).all()
    assert np.isnan(want[3]) and ((want > 0) & (want < 1)).any()


# ---- 7. nothing waits for the device ----------------------------------------------------------------------------------------------------
def test_no_call_waits_for_the_device(case):
    frames, split, store = case
    view = vis.BevView(*vis_ref.VIEWS[0][:2], vis_ref.VIEWS[0][2], vis_ref.VIEWS[0][3], radius_px=1.5)
    warm = I.cluster(split, None, which="gt", eps=1.0, min_points=2, flow_weight=2.5)      # warm: library, counts_host
    vis.render_instances(warm, split, None, view)
    I.agreement(warm, warm)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gt = I.cluster(split, None, which="gt", eps=1.0, min_points=2, flow_weight=2.5)
        some = I.cluster(split, None, which="gt", eps=2.0, min_points=4, frames=[9, 2])
        pics = [vis.render_instances(gt, split, None, view), vis.render_instances(some, split, None, view)]
        same = I.agreement(gt, warm)
        speed = gt.velocity()
        with pytest.raises(RuntimeError):
            split.off1.cpu()                                               # the control: a read-back IS caught in this mode
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _same(_host(gt), _want(frames, "gt", 1.0, 2, 2.5), "no wait")
    assert some.count.tolist() == np.where(np.isin(np.arange(len(frames)), [9, 2]), _want(frames, "gt", 2.0, 4, 0.0)["count"], 0).tolist()
    assert pics[0].shape == (len(frames), view.height, view.width, 3) and pics[1].shape[0] == 2 and speed.shape == gt.disp.shape
    assert bool((same["iou"][~torch.isnan(same["iou"])] == 1).all())
