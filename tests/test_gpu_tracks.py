"""GPU: moving-object instances tracked across a clip's frames (cmflow_amd/tracks.py) -- cmf_track_instances bit for bit against its
numpy restatement (tests/tracks_ref.py) on a clustered world for both sources, the C entry point on hand-made tables (ladder, ties,
gate, NaN, overflow) with sentinel-filled buffers and arguments that have to be clamped, the reference's own saved frames, the
pictures, ``SplitResults.tracks``, and that none of it waits for the device.  Every comparison is exact: integers equal, ``pred`` as
uint32."""
import os

import numpy as np
import pytest
import torch

import instances_ref as iref
import tracks_ref as ref
import vis_ref
from cmflow_amd import _lib
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import results as R
from cmflow_amd import tracks as K
from cmflow_amd import vis

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ARRAYS = ref.PER_INSTANCE + ref.PER_TRACK + ref.PER_CLIP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _filled(frames, dev, clips=None):
    split = D.DeviceSplit.from_items(iref.as_items(frames), dev, clips)
    store = R.SplitResults.empty(split)
    store.flow.copy_(torch.from_numpy(np.concatenate([fr["flow"] for fr in frames])))
    store.mask.copy_(torch.from_numpy(np.concatenate([fr["mask"] for fr in frames])))
    store.pred_trans.copy_(torch.from_numpy(np.stack([fr["pred_t"] for fr in frames])))
    store.done.fill_(1)
    return split, store


@pytest.fixture(scope="module")
def world(dev):
    frames, owners = ref.build_world()
    split, store = _filled(frames, dev, [tuple(c) for c in ref.WORLD_CLIPS])
    return frames, split, store


def _host(tr):
    return {k: getattr(tr, k).cpu().numpy() for k in ARRAYS}


def _restated(inst, T, clips, gate, max_gap):
    """The restatement on the tables the device clustered (read back): the same inputs as the kernel's."""
    off1 = inst.off.cpu().numpy()
    return ref.track(off1, int(off1[-1]), inst.count.cpu().numpy(), inst.label.cpu().numpy(), inst.centroid.cpu().numpy(), inst.disp.cpu().numpy(),
                     T.reshape(-1, 16).cpu().numpy(), clips, gate, max_gap)


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap", [0, 2])
@pytest.mark.parametrize("which", ["pred", "gt"])
def test_track_is_the_restatement(world, dev, which, max_gap):
    frames, split, store = world
    inst = I.cluster(split, store if which == "pred" else None, which=which)
    tr = K.track(inst, split, store if which == "pred" else None, gate=ref.GATE, max_gap=max_gap)
    assert tr.track.is_cuda and tr.clips_host.tolist() == [list(c) for c in ref.WORLD_CLIPS] and tr.clips.tolist() == tr.clips_host.tolist()
    T = store.pred_trans if which == "pred" else split.trans
    want = _restated(inst, T, ref.WORLD_CLIPS, ref.GATE, max_gap)
    ref.same(_host(tr), want, (which, max_gap))
    # the world is what it is for: objects kept through an absence of two frames at max_gap 2, lost at 0
    assert want["ntracks"].tolist() == [ref.WORLD_OBJECTS + (1 if max_gap else 2), ref.WORLD_OBJECTS] and (want["age"] > 1).sum() > 60
    assert ((want["gap"] == 3).any()) == (max_gap == 2)
    assert np.array_equal(tr.lengths().cpu().numpy(), np.where(want["hits"] > 0, want["last"] - want["birth"] + 1, 0))
    if max_gap == 2:
        # other clip ranges over the same instances: frames outside the one range are clips of their own; a selection leaves frames
        # without instances, which everything coasts through
        other, _ = _filled(frames, dev, [(2, 9)])
        part = I.cluster(other, store if which == "pred" else None, which=which, frames=[f for f in range(len(frames)) if f not in (4, 12)])
        got = K.track(part, other, store if which == "pred" else None, gate=ref.GATE, max_gap=max_gap)
        clips = ref.plan_clips(len(frames), [(2, 9)])
        assert got.clips_host.tolist() == clips.tolist() and len(got) == 12
        ref.same(_host(got), _restated(part, T, clips, ref.GATE, max_gap), (which, "one range"))
        view = got.frame(5)
        a = int(part.offsets_host[5])
        assert view["track"].shape == (ref.WORLD_OBJECTS - 1,) and torch.equal(view["gap"], got.gap[a:a + len(view["gap"])])
        assert (view["gap"] >= 2).any()                                      # frame 4 was not selected


# ---- 2. the C entry point on sentinel-filled buffers ------------------------------------------------------------------------------------
SENTINEL = {"track": -99, "prev_row": -98, "gap": -97, "age": -96, "pred": -7.5, "point_track": -95, "birth": -94, "last": -93, "hits": -92,
            "ntracks": -91, "overflow": -90}


def _call(t, dev, clips, total, count, rows, gate, max_gap):
    """cmf_track_instances itself on the tables ``t``; outputs of ``rows`` rows and len(clips) + 3 clip entries, sentinel-filled."""
    i32, f = torch.int32, torch.float32
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    clips_d = up(np.asarray(clips, dtype=np.int32).reshape(-1, 2), i32)
    ins = [up(t["off1"], i32), up(count, i32), up(t["label"], i32), up(t["centroid"], f), up(t["disp"], f), up(t["T"], f)]
    out = {k: torch.full((rows, 3) if k == "pred" else (rows,) if k not in ref.PER_CLIP else (len(clips) + 3,), SENTINEL[k],
                         dtype=f if k == "pred" else i32, device=dev) for k in ARRAYS}
    p = _lib.dev_ptr
    _lib.check(_lib.lib().cmf_track_instances(
        len(clips), len(count), p(clips_d, i32), p(ins[0], i32), total, p(ins[1], i32), p(ins[2], i32), p(ins[3], f), p(ins[4], f), p(ins[5], f),
        float(gate) * float(gate), max_gap, *(p(out[k], f if k == "pred" else i32) for k in ARRAYS), _lib.stream_ptr()), "cmf_track_instances")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _want(t, clips, total, count, rows, gate, max_gap):
    return ref.track(t["off1"], total, count, t["label"], t["centroid"], t["disp"], t["T"], clips, gate, max_gap,
                     out=ref.outputs(rows, len(clips) + 3, SENTINEL))


def test_entry_point_on_hand_made_tables(dev):
    t = ref.build_tables()
    F, total = len(t["count"]), t["total"]
    rows = total + 64
    for max_gap in (2, 0, 16):
        got = _call(t, dev, t["clips"], total, t["count"], rows, 2.0, max_gap)
        want = _want(t, t["clips"], total, t["count"], rows, 2.0, max_gap)
        ref.same(got, want, ("tables", max_gap))
        assert all((got[k][total:] == SENTINEL[k]).all() for k in ref.PER_INSTANCE + ref.PER_TRACK)
        assert all((got[k][len(t["clips"]):] == SENTINEL[k]).all() for k in ref.PER_CLIP)
        assert all((got[k][:total] != SENTINEL[k]).all() for k in ref.PER_INSTANCE + ref.PER_TRACK)      # the clips cover every frame
    # (tests/test_tracks_host.py asserts, on the restatement, that these tables reach the ladder's 200 rounds, the ties, the gate, the NaN
    # and the overflow; here: the restatement's answer at max_gap 2 is the device's)
    want = _want(t, t["clips"], total, t["count"], rows, 2.0, 2)
    a = int(t["off1"][int(t["clips"][ref.C_LADDER][0]) + 1])
    assert want["track"][a:a + ref.LADDER].tolist() == list(range(ref.LADDER))[::-1] and want["overflow"][ref.C_OVERFLOW] == 1
    # arguments that have to be clamped: a clip range reaching behind F, one starting before 0, a count above the frame's rows, a frame
    # whose rows end behind ``total``; the frames between the two clips belong to none
    first = int(t["clips"][ref.C_RANDOM][0])
    count = t["count"].copy()
    count[first + 1] = 5000
    short = int(t["off1"][F - 1]) + 2
    clips = [(first, F + 9), (-3, 2)]
    got = _call(t, dev, clips, short, count, rows, 2.0, 2)
    want = _want(t, clips, short, count, rows, 2.0, 2)
    ref.same(got, want, "clamped")
    untouched = np.ones(rows, bool)
    untouched[:int(t["off1"][2])] = False
    untouched[int(t["off1"][first]):int(t["off1"][F - 1])] = False
    assert all((got[k][untouched] == SENTINEL[k]).all() and (got[k][~untouched] != SENTINEL[k]).all() for k in ref.PER_INSTANCE + ref.PER_TRACK)
    a, b = int(t["off1"][first + 1]), int(t["off1"][first + 2])
    assert (got["track"][a:b] >= 0).all() and got["ntracks"][:2].tolist() == want["ntracks"][:2].tolist() and got["ntracks"][1] == 3
    # refusals of the entry point itself: nothing is launched
    for gate2, max_gap in ((float("nan"), 2), (4.0, -1), (4.0, 17)):
        z = torch.zeros(8, dtype=torch.int32, device=dev)
        zf = torch.zeros(8, 3, dtype=torch.float32, device=dev)
        p = _lib.dev_ptr
        assert _lib.lib().cmf_track_instances(1, 1, p(z, torch.int32), p(z, torch.int32), 0, p(z, torch.int32), p(z, torch.int32), p(zf, torch.float32),
                                              p(zf, torch.float32), p(zf, torch.float32), gate2, max_gap, *([p(z, torch.int32)] * 4), p(zf, torch.float32),
                                              *([p(z, torch.int32)] * 6), _lib.stream_ptr()) != 0


# ---- 3. the reference's own saved frames ------------------------------------------------------------------------------------------------
def test_saved_frames(golden_dir, dev):
    g = np.load(os.path.join(golden_dir, "saved_results_delft_12_w12.npz"))
    off = g["off"]
    frames = [{"pos1": g["pc1"][a:b], "flow": g["pred_f"][a:b], "label": np.zeros((b - a, 3), f32), "mask": g["pred_m"][a:b],
               "gt_mask": np.ones(b - a, f32), "pred_t": g["pred_t"][k], "gt_t": np.eye(4, dtype=f32)}
              for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]
    split, store = _filled(frames, dev)
    inst = I.cluster(split, store)                                          # the defaults: eps 2, min_points 2, position alone
    tr = K.track(inst, split, store, gate=2.0, max_gap=2)
    got = _host(tr)
    ref.same(got, _restated(inst, store.pred_trans, [(0, 12)], 2.0, 2), "saved frames")
    count = inst.count.cpu().numpy()
    assert [got["track"][off[f]:off[f] + count[f]].tolist() for f in range(12)] == [[0], [0, 1]] + [[0]] * 10
    assert got["ntracks"].tolist() == [2] and got["hits"][:3].tolist() == [12, 1, 0] and got["overflow"].tolist() == [0]


# ---- 4. pictures ------------------------------------------------------------------------------------------------------------------------
def test_render_tracks_is_the_rasterisers_restatement(world):
    frames, split, store = world
    inst = I.cluster(split, store)
    tr = K.track(inst, split, store, gate=ref.GATE, max_gap=2)
    want = _restated(inst, store.pred_trans, ref.WORLD_CLIPS, ref.GATE, 2)
    kind = inst.kind.cpu().numpy()
    colors = iref.instance_colors(want["point_track"], kind)
    off = inst.offsets_host
    pos = np.concatenate([fr["pos1"] for fr in frames])
    some = [9, 0, 5, 12]
    w, h, xr, yr = vis_ref.VIEWS[0]
    view = vis.BevView(w, h, xr, yr, radius_px=1.5, guides=True)
    p = view.kernel_params()
    for sel, ids in ((None, list(range(len(frames)))), (some, some)):
        got = vis.render_tracks(tr, inst, split, sel, view)
        assert got.shape == (len(ids), h, w, 3) and got.dtype == torch.uint8 and got.is_cuda
        got = got.cpu().numpy()
        for s, f in enumerate(ids):
            a, b = off[f], off[f + 1]
            pic = vis_ref.render_frame(pos[a:b], colors[a:b], np.ones(b - a, np.uint8), w, h, p, True)
            bad = np.argwhere((got[s] != pic).any(-1))
            assert bad.size == 0, (f, len(bad), bad[:6].tolist())
    # an object keeps its colour where its instance number changes: the tracks' picture differs from the instances' somewhere
    assert (want["point_track"] != inst.label.cpu().numpy()).any()
    assert not torch.equal(vis.render_tracks(tr, inst, split, None, view), vis.render_instances(inst, split, None, view))


# ---- 5. the store's shorthand -----------------------------------------------------------------------------------------------------------
def test_store_tracks_is_cluster_then_track(world):
    frames, split, store = world
    inst = I.cluster(split, store, eps=1.5, min_points=3, flow_weight=0.5)
    want = _host(K.track(inst, split, store, gate=1.5, max_gap=1))
    got = store.tracks(split, gate=1.5, max_gap=1, eps=1.5, min_points=3, flow_weight=0.5)
    ref.same(_host(got), want, "store.tracks")
    assert torch.equal(got.inst.label, inst.label) and (got.gate, got.max_gap) == (1.5, 1)
    ref.same(_host(store.tracks(split, inst=inst, gate=1.5, max_gap=1)), want, "store.tracks(inst)")
    gt = I.cluster(split, None, which="gt")
    ref.same(_host(store.tracks(split, inst=gt)), _host(K.track(gt, split)), "store.tracks(gt)")


# ---- 6. nothing waits for the device ----------------------------------------------------------------------------------------------------
def test_no_call_waits_for_the_device(world):
    frames, split, store = world
    w, h, xr, yr = vis_ref.VIEWS[0]
    view = vis.BevView(w, h, xr, yr, radius_px=1.5)
    inst = I.cluster(split, None, which="gt")                                # warm: library, counts_host
    pred = I.cluster(split, store)
    warm = K.track(inst, split)
    vis.render_tracks(warm, inst, split, None, view)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gt = K.track(inst, split, gate=ref.GATE, max_gap=2)
        pr = K.track(pred, split, store, gate=ref.GATE, max_gap=0)
        pics = vis.render_tracks(gt, inst, split, [3, 11], view)
        spans = gt.lengths()
        with pytest.raises(RuntimeError):
            split.off1.cpu()                                               # the control: a read-back IS caught in this mode
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    ref.same(_host(gt), _restated(inst, split.trans, ref.WORLD_CLIPS, ref.GATE, 2), "no wait, gt")
    ref.same(_host(pr), _restated(pred, store.pred_trans, ref.WORLD_CLIPS, ref.GATE, 0), "no wait, pred")
    assert pics.shape == (2, h, w, 3) and int(spans.max()) == 10
