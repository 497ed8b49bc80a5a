"""GPU: a test run's clouds accumulated over a window of frames (cmflow_amd/accumulate.py) -- cmf_accumulate bit for bit against its
numpy restatement (tests/accumulate_ref.py) in every mode, the C entry point on sentinel-filled buffers, selections, the reference's
own saved frames, the error measures, the pictures, and that none of it waits for the device."""
import os

import numpy as np
import pytest
import torch

import accumulate_ref as ref
import vis_ref
from cmflow_amd import _lib
from cmflow_amd import accumulate as A
from cmflow_amd import dataset as D
from cmflow_amd import results as R
from cmflow_amd import vis

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _filled(frames, dev, clips):
    split = D.DeviceSplit.from_items(ref.as_items(frames), dev, clips)
    store = R.SplitResults.empty(split)
    store.flow.copy_(torch.from_numpy(np.concatenate([fr["flow"] for fr in frames])))
    store.mask.copy_(torch.from_numpy(np.concatenate([fr["mask"] for fr in frames])))
    store.pred_trans.copy_(torch.from_numpy(np.stack([fr["pred_t"] for fr in frames])))
    store.done.fill_(1)
    return split, store


@pytest.fixture(scope="module")
def case(dev):
    frames = ref.build_case()
    split, store = _filled(frames, dev, [tuple(c) for c in ref.CLIPS])
    assert split.counts_host[0].tolist() == list(ref.COUNTS)
    return frames, split, store


_wants = {}


def _want(frames, which, window, dynamic):
    """The restatement of the whole case, computed once per combination."""
    key = (which, window, dynamic)
    if key not in _wants:
        _wants[key] = ref.accumulate(*ref.case_arrays(frames, which), ref.CLIPS, list(range(len(frames))), window, dynamic)
    return _wants[key]


def _host(acc):
    return {"off": acc.off.cpu().numpy(), "xyz": acc.xyz.cpu().numpy(), "src": acc.src.cpu().numpy(), "age": acc.age.cpu().numpy(),
            "count": acc.count.cpu().numpy()}


def _same(got, want, what):
    assert got["off"].tolist() == want["off"].tolist(), what
    assert got["xyz"].dtype == f32 and got["src"].dtype == np.int32 and got["age"].dtype == np.uint8 and got["count"].dtype == np.int32
    for k in ("count", "src", "age"):
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())
    bad = np.argwhere(got["xyz"].view(np.uint32) != want["xyz"].view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got["xyz"][bad[:4, 0]].tolist(), want["xyz"][bad[:4, 0]].tolist())


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pred", "gt"])
def test_accumulate_is_the_restatement(case, which):
    frames, split, store = case
    for window in ref.WINDOWS:
        for dynamic in ref.MODES:
            acc = A.accumulate(split, store if which == "pred" else None, window=window, which=which, dynamic=dynamic)
            assert acc.xyz.is_cuda and acc.window == window and acc.frames.tolist() == list(range(len(frames)))
            _same(_host(acc), _want(frames, which, window, dynamic), (which, window, dynamic))
    want = _want(frames, which, 8, "drop")
    assert (want["count"] < np.diff(want["off"])).any() and want["age"][want["src"] >= 0].max() == 6     # the case reaches what it is for
    moved = np.abs(_want(frames, which, 8, "propagate")["xyz"] - _want(frames, which, 8, "keep")["xyz"]).max(-1)
    assert (moved > 0.1).sum() > 100
    assert _host(store.accumulate(split, window=2, which=which))["xyz"].tobytes() == _want(frames, which, 2, "keep")["xyz"].tobytes()


# ---- 2. the C entry point on sentinel-filled buffers ------------------------------------------------------------------------------------
def _call(split, store, ids, first, cap_off, cap_total, rows, window, mode, dev):
    """cmf_accumulate itself; outputs of ``rows`` rows (>= cap_total) pre-filled with sentinels -> host arrays."""
    i32, u8 = torch.int32, torch.uint8
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    sel, first_d, cap_d = t(ids, torch.int64), t(first, i32), t(cap_off, i32)
    xyz = torch.full((rows, 3), -7.5, dtype=torch.float32, device=dev)
    src = torch.full((rows,), -99, dtype=i32, device=dev)
    age = torch.full((rows,), 77, dtype=u8, device=dev)
    count = torch.full((len(ids),), -5, dtype=i32, device=dev)
    p = _lib.dev_ptr
    _lib.check(_lib.lib().cmf_accumulate(
        len(ids), len(split), p(sel, torch.int64), p(first_d, i32), p(split.off1, i32), split.tab1.shape[0], p(split.tab1, torch.float32),
        split.tab1.shape[1], p(store.flow, torch.float32), p(store.mask, u8), p(store.pred_trans.reshape(-1, 16), torch.float32), window,
        A.DYNAMIC.index(mode), 0, p(cap_d, i32), cap_total, p(xyz, torch.float32), p(src, i32), p(age, u8), p(count, i32), _lib.stream_ptr()),
        "cmf_accumulate")
    torch.cuda.synchronize()
    return xyz.cpu().numpy(), src.cpu().numpy(), age.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("mode", ["drop", "propagate"])
def test_entry_point_writes_its_capacity_and_nothing_else(case, dev, mode):
    frames, split, store = case
    F, window = len(frames), 5
    want = _want(frames, "pred", window, mode)
    # ids outside the split are clamped (to frames 0 and 10), a first frame outside [0, j] likewise; capacities 3 rows larger than the
    # sources need -- but 5 rows SMALLER for frame 6 -- behind 7 rows that belong to nobody and before 9 more
    ids, clamped = [-5, 6, 99, 3, 3, 9], [0, 6, 10, 3, 3, 9]
    starts = ref.clip_starts(F, ref.CLIPS)
    first = [int(starts[j]) for j in clamped]
    first[0], first[3] = 4, -3                                              # -> 0 and 0
    need = np.diff(want["off"])[clamped]
    cap = need + 3
    cap[1] = need[1] - 5
    cap_off = 7 + np.concatenate(([0], np.cumsum(cap)))
    cap_total, rows = int(cap_off[-1]) + 9, int(cap_off[-1]) + 9 + 64
    xyz, src, age, count = _call(split, store, ids, first, cap_off.tolist(), cap_total, rows, window, mode, dev)
    outside = np.ones(rows, bool)
    for s, j in enumerate(clamped):
        a, b = int(cap_off[s]), int(cap_off[s + 1])
        outside[a:b] = False
        w0 = int(want["off"][j])
        n = min(int(want["count"][j]), b - a)
        assert count[s] == n, (s, count[s], n)
        assert np.array_equal(xyz[a:a + n].view(np.uint32), want["xyz"][w0:w0 + n].view(np.uint32)), s
        assert np.array_equal(src[a:a + n], want["src"][w0:w0 + n]) and np.array_equal(age[a:a + n], want["age"][w0:w0 + n]), s
        assert not xyz[a + n:b].any() and (src[a + n:b] == -1).all() and (age[a + n:b] == 255).all(), s      # the padding, as defined
    assert mode == "drop" or count[1] == cap[1] < want["count"][6]          # the points that do not fit are left out
    assert outside.sum() == 7 + 9 + 64
    assert (xyz[outside] == -7.5).all() and (src[outside] == -99).all() and (age[outside] == 77).all()
    # offsets that do not describe the outputs: the target whose capacity ends behind cap_total writes nothing but its count
    c2 = int(np.diff(want["off"])[2])
    xyz, src, age, count = _call(split, store, [2, 4], [0, 0], [0, c2, c2 + 1000], c2 + 10, c2 + 1100, window, mode, dev)
    assert count.tolist() == [int(want["count"][2]), 0]
    assert np.array_equal(src[:c2], want["src"][want["off"][2]:want["off"][3]])
    assert (src[c2:] == -99).all() and (age[c2:] == 77).all() and (xyz[c2:] == -7.5).all()


# ---- 3. selections ----------------------------------------------------------------------------------------------------------------------
def test_a_selections_targets_are_rows_of_the_full_run(case, dev):
    frames, split, store = case
    ids = [10, 3, 3, 0, 7, 6]
    for dynamic in ("propagate", "drop"):
        want = _want(frames, "pred", 5, dynamic)
        for sel in (ids, torch.tensor(ids, dtype=torch.int64), torch.tensor(ids, dtype=torch.int64, device=dev)):
            acc = A.accumulate(split, store, window=5, dynamic=dynamic, frames=sel)
            got = _host(acc)
            assert acc.frames.tolist() == ids and len(acc) == len(ids)
            assert np.diff(got["off"]).tolist() == np.diff(want["off"])[ids].tolist()
            for s, j in enumerate(ids):
                a, b, w0, w1 = got["off"][s], got["off"][s + 1], want["off"][j], want["off"][j + 1]
                assert got["count"][s] == want["count"][j]
                assert np.array_equal(got["xyz"][a:b].view(np.uint32), want["xyz"][w0:w1].view(np.uint32)), (dynamic, s)
                assert np.array_equal(got["src"][a:b], want["src"][w0:w1]) and np.array_equal(got["age"][a:b], want["age"][w0:w1])
    empty = A.accumulate(split, store, window=5, frames=[])
    assert len(empty) == 0 and empty.xyz.shape == (0, 3) and empty.off.tolist() == [0]
    store.done[4] = 0
    try:
        with pytest.raises(ValueError):
            A.accumulate(split, store, window=2, frames=[5])
        assert len(A.accumulate(split, store, window=2, frames=[6, 3])) == 2   # frame 4 is no source of these
        assert len(A.accumulate(split, None, window=2, which="gt", frames=[5])) == 1
    finally:
        store.done[4] = 1


# ---- 4. the reference's own saved frames ------------------------------------------------------------------------------------------------
def test_saved_frames_bit_for_bit(golden_dir, dev):
    g = np.load(os.path.join(golden_dir, "saved_results_delft_12_w12.npz"))
    off = g["off"]
    frames = [{"pos1": g["pc1"][a:b], "flow": g["pred_f"][a:b], "label": np.zeros((b - a, 3), f32), "mask": g["pred_m"][a:b],
               "gt_mask": np.ones(b - a, f32), "pred_t": g["pred_t"][k], "gt_t": np.eye(4, dtype=f32)}
              for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]
    split, store = _filled(frames, dev, None)
    for dynamic in ref.MODES:
        want = ref.accumulate(off, g["pc1"], g["pred_f"], g["pred_m"] == 0, g["pred_t"], None, list(range(12)), 8, dynamic)
        _same(_host(A.accumulate(split, store, window=8, dynamic=dynamic)), want, dynamic)
    assert want["age"][want["src"] >= 0].max() == 7 and (want["count"][1:] < np.diff(want["off"])[1:]).all()


# ---- 5. the error measures --------------------------------------------------------------------------------------------------------------
def test_accumulation_error_is_numpys(case, dev):
    frames, split, store = case
    for window, dynamic in ((8, "propagate"), (5, "keep"), (1, "keep")):
        pred = A.accumulate(split, store, window=window, dynamic=dynamic)
        gt = A.accumulate(split, None, window=window, which="gt", dynamic=dynamic)
        got = A.accumulation_error(pred, gt)
        assert all(v.is_cuda and v.dtype == torch.float64 for v in got.values())
        p, q = _want(frames, "pred", window, dynamic), _want(frames, "gt", window, dynamic)
        want = dict(zip(("mean", "max", "per_age"), ref.accumulation_error(p["xyz"], q["xyz"], p["off"], p["age"], window)))
        for k in want:
            g, w = got[k].cpu().numpy(), want[k]
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (window, k)
            ok = ~np.isnan(w)
            assert (np.abs(g[ok] - w[ok]) <= 1e-12 * np.abs(w[ok])).all(), (window, k, g, w)
        assert np.isnan(want["mean"][[0, 7]]).all() and (window == 1 or want["mean"][1] > 0.01) and want["per_age"][0] == 0
        again = A.accumulation_error(pred, gt)
        assert all(torch.equal(got[k].view(torch.int64), again[k].view(torch.int64)) for k in got)      # deterministic
    # a store that holds the labels: the two accumulations are the same numbers, the error exactly 0
    mirror = R.SplitResults.empty(split)
    mirror.flow.copy_(split.tab1[:, 6:9])
    mirror.mask.copy_((split.tab1[:, 9] != 0).to(torch.uint8))
    mirror.pred_trans.copy_(split.trans.reshape(-1, 4, 4))
    mirror.done.fill_(1)
    pred, gt = A.accumulate(split, mirror, window=8, dynamic="propagate"), A.accumulate(split, None, window=8, which="gt", dynamic="propagate")
    assert torch.equal(pred.xyz.view(torch.int32), gt.xyz.view(torch.int32))
    zero = A.accumulation_error(pred, gt)
    for k, v in zero.items():
        v = v.cpu().numpy()
        assert (v[~np.isnan(v)] == 0).all() and (~np.isnan(v)).sum() >= 7, k


# ---- 6. pictures ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer,dynamic", [("seg", "drop"), ("age", "keep")])
def test_render_accumulated_is_the_rasterisers_restatement(case, layer, dynamic):
    frames, split, store = case
    window = 5
    acc = A.accumulate(split, store, window=window, dynamic=dynamic)
    want = _want(frames, "pred", window, dynamic)
    if layer == "age":
        colors, drawn = ref.age_colors(want["age"], window), (want["src"] >= 0).astype(np.uint8)
    else:
        per_frame = [vis_ref.frame_colors(layer, fr["flow"], fr["label"], fr["mask"], fr["gt_mask"]) for fr in frames]
        all_c, all_d = np.concatenate([c for c, _ in per_frame]), np.concatenate([d for _, d in per_frame])
        held = want["src"] >= 0
        colors, drawn = all_c[np.maximum(want["src"], 0)], all_d[np.maximum(want["src"], 0)] * held
    for w, h, xr, yr in vis_ref.VIEWS:
        view = vis.BevView(w, h, xr, yr, radius_px=1.5, guides=True)
        got = vis.render_accumulated(acc, None if layer == "age" else store, split, layer, view)
        assert got.shape == (len(frames), h, w, 3) and got.dtype == torch.uint8 and got.is_cuda
        got = got.cpu().numpy()
        p = view.kernel_params()
        for s in range(len(frames)):
            a, b = int(want["off"][s]), int(want["off"][s + 1])
            pic = vis_ref.render_frame(want["xyz"][a:b], colors[a:b], drawn[a:b], w, h, p, True)
            bad = np.argwhere((got[s] != pic).any(-1))
            assert bad.size == 0, (layer, w, s, len(bad), bad[:6].tolist())
    newest = np.array(vis_ref.ROYAL_BLUE if layer == "age" else vis_ref.TOMATO, dtype=np.uint8)
    assert (got[6] == newest).all(-1).any() and len(np.unique(got[6].reshape(-1, 3), axis=0)) >= 4


# ---- 7. nothing waits for the device ----------------------------------------------------------------------------------------------------
def test_no_call_waits_for_the_device(case):
    frames, split, store = case
    view = vis.BevView(*vis_ref.VIEWS[0][:2], vis_ref.VIEWS[0][2], vis_ref.VIEWS[0][3], radius_px=1.5)
    pred = A.accumulate(split, store, window=5, dynamic="propagate")        # warm: library, pinned pool, counts_host; 'pred' copies ``done``
    A.accumulation_error(pred, A.accumulate(split, None, window=5, which="gt", dynamic="propagate"))
    vis.render_accumulated(pred, store, split, "seg", view)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        kept = A.accumulate(split, None, window=5, which="gt", dynamic="keep")
        gt = A.accumulate(split, None, window=5, which="gt", dynamic="propagate")
        some = A.accumulate(split, None, window=5, which="gt", dynamic="drop", frames=[9, 2])
        err = A.accumulation_error(pred, gt)
        pics = [vis.render_accumulated(pred, store, split, "seg", view), vis.render_accumulated(kept, None, split, "age", view)]
        with pytest.raises(RuntimeError):
            split.off1.cpu()                                               # the control: a read-back IS caught in this mode
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert _host(gt)["xyz"].tobytes() == _want(frames, "gt", 5, "propagate")["xyz"].tobytes()
    assert _host(kept)["xyz"].tobytes() == _want(frames, "gt", 5, "keep")["xyz"].tobytes()
    assert some.count.tolist() == _want(frames, "gt", 5, "drop")["count"][[9, 2]].tolist()
    assert bool(torch.isfinite(err["per_age"]).all()) and pics[0].shape == pics[1].shape == (len(frames), view.height, view.width, 3)
