"""GPU: per-track object states of a test run (cmflow_amd/objects.py) -- cmf_track_states bit for bit against its numpy restatement
(tests/objects_ref.py) on a clustered and tracked world for both sources, the C entry point on corrupted tables (garbage and cyclic
links, gaps that must be clamped, a NaN centroid, a count beyond a frame's rows, an empty clip, a one-frame clip, a frame outside
the tables) with sentinel-filled and oversized buffers, the pose of a clip's first frame and across a clip boundary, the store's
shorthand and the views, and that none of it waits for the device.  Every comparison is exact: integers equal, float32 arrays as
uint32, float64 arrays as uint64 (a NaN for a NaN)."""
import numpy as np
import pytest
import torch

import instances_ref as iref
import objects_ref as ref
import results_ref as rref
from cmflow_amd import _lib
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import objects as O
from cmflow_amd import results as R
from cmflow_amd import tracks as K

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TORCH = {np.int32: torch.int32, f32: torch.float32, f64: torch.float64}


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
    frames, owners, truth = ref.build_world(flow_noise=0.01)
    split, store = _filled(frames, dev, [tuple(c) for c in ref.WORLD_CLIPS])
    return frames, split, store


def _host(obj):
    return {k: getattr(obj, k).cpu().numpy() for k in ref.KEYS}


def _restated(trk, split, T, poses, params=ref.PARAMS):
    """The restatement on the tables the device clustered and tracked and the poses it chained (read back): the kernel's inputs."""
    inst = trk.inst
    off1 = inst.off.cpu().numpy()
    return ref.states(off1, int(off1[-1]), inst.count.cpu().numpy(), inst.label.cpu().numpy(), inst.centroid.cpu().numpy(), inst.disp.cpu().numpy(),
                      trk.track.cpu().numpy(), trk.prev_row.cpu().numpy(), trk.gap.cpu().numpy(), split.tab1.cpu().numpy(), poses.cpu().numpy(),
                      trk.clips_host, *params)


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pred", "gt"])
def test_estimate_is_the_restatement(world, dev, which):
    frames, split, store = world
    st = store if which == "pred" else None
    inst = I.cluster(split, st, which=which)
    trk = K.track(inst, split, st, gate=ref.GATE, max_gap=2)
    obj = O.estimate(trk, split, st)
    assert obj.state.is_cuda and obj.state.dtype == torch.float64 and obj.pos.dtype == torch.float32 and len(obj) == 2
    T = store.pred_trans if which == "pred" else split.trans
    # the poses are cmf_pose_chain's on the tracker's clips
    poses = rref.pose_chain(T.cpu().numpy().reshape(-1, 4, 4), ref.WORLD_CLIPS)
    assert np.array_equal(obj.poses.cpu().numpy().view(np.uint64), poses.reshape(-1, 16).view(np.uint64))
    got, want = _host(obj), _restated(trk, split, T, obj.poses)
    ref.same(got, want, which)
    # the world is what it is for: a gap of 3, a single hit, both heading sources, chains of at least 3
    held = want["row_frame"] >= 0
    assert sorted(len(c) for c in ref.chains(want, len(held))) == [1, 7, 7, 7, 7, 7, 9, 11, 11, 11, 11]
    assert (trk.gap.cpu().numpy() == 3).any() and np.bincount(want["heading_src"][held]).tolist() == [18, 71]
    # other parameters: no process noise, every moving instance a heading
    other = (0.3, 0.1, 0.0, 0.0)
    ref.same(_host(O.estimate(trk, split, st, *other)), _restated(trk, split, T, obj.poses, other), (which, other))


# ---- 2. the C entry point on corrupted tables and sentinel-filled buffers ---------------------------------------------------------------
SENTINEL = {"row_frame": -99, "next_row": -98, "heading_src": -97, "filt": -7.5, "fcov": -6.5, "state": -5.5, "scov": -4.5, "pos": -3.5, "vel": -2.5,
            "heading": -1.5, "box_center": -0.5, "box_size": -8.5}


def _call(t, dev, clips, total, rows, params=ref.PARAMS):
    """cmf_track_states itself on the tables ``t``; outputs of ``rows`` rows, sentinel-filled."""
    i32, f = torch.int32, torch.float32
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    clips_d = up(np.asarray(clips, dtype=np.int32).reshape(-1, 2), i32)
    ints = [up(t[k], i32) for k in ("off1", "count", "label", "track", "prev_row", "gap")]
    cen, disp, tab1, poses = up(t["centroid"], f), up(t["disp"], f), up(t["tab1"], f), up(t["poses"], torch.float64)
    out = {k: torch.full((rows, ref.WIDTH[k]) if ref.WIDTH[k] else (rows,), SENTINEL[k], dtype=TORCH[ref.dtype_of(k)], device=dev) for k in ref.KEYS}
    p = _lib.dev_ptr
    sp, sd, sa, md = (float(v) for v in params)
    _lib.check(_lib.lib().cmf_track_states(
        len(clips), len(t["count"]), p(clips_d, i32), p(ints[0], i32), total, p(ints[1], i32), p(ints[2], i32), p(cen, f), p(disp, f),
        p(ints[3], i32), p(ints[4], i32), p(ints[5], i32), p(tab1, f), t["tab1"].shape[1], poses.data_ptr(), sp * sp, sd * sd, sa * sa, md * md,
        *(p(out[k], out[k].dtype) for k in ref.KEYS), _lib.stream_ptr()), "cmf_track_states")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_entry_point_bounds_itself_on_corrupted_tables(dev):
    """Nothing here can fault: the kernel follows a link only to a row its own search found, caps every walk and clamps every gap
    (include/cmflow_hip.h), and tests/test_objects_host.py takes the same tables through the restatement on the CPU."""
    frames, owners, truth = ref.build_world()
    clean = ref.world_tables(frames, "gt")
    t, clips, total = ref.corrupt_tables(clean)
    t["poses"] = rref.pose_chain(t["T"], clips).reshape(-1, 16)
    F, rows = len(t["count"]), clean["total"] + 64
    got = _call(t, dev, clips, total, rows)
    want = ref.run(t, out=ref.outputs(rows, SENTINEL), clips=clips, total=total)
    ref.same(got, want, "corrupted")
    owned = np.zeros(rows, bool)
    owned[:int(t["off1"][F - 1])] = True                                    # the clips cover frames 0 .. F-2; the last frame ends behind ``total``
    for k in ref.KEYS:
        assert (got[k][~owned] == SENTINEL[k]).all(), k                     # sentinels outside owned rows stay intact
    for k in ref.INT_KEYS:
        assert (got[k][owned] != SENTINEL[k]).all(), k
    a, b = int(t["off1"][5]), int(t["off1"][6])
    assert (got["row_frame"][a:b] == 5).all()                               # K beyond the frame's rows: clamped to them
    # the clean tables through the same call, sentinel-filled: the world's own clips, every frame owned
    got = _call(clean, dev, ref.WORLD_CLIPS, clean["total"], rows)
    ref.same(got, ref.run(clean, out=ref.outputs(rows, SENTINEL)), "clean")
    assert all((got[k][clean["total"]:] == SENTINEL[k]).all() and (got[k][:clean["total"]] != SENTINEL[k]).all() for k in ref.KEYS)
    # refusals of the entry point itself: nothing is launched
    z = torch.zeros(8, dtype=torch.int32, device=dev)
    zf = torch.zeros(8, 3, dtype=torch.float32, device=dev)
    zd = torch.zeros(8, 16, dtype=torch.float64, device=dev)
    p = _lib.dev_ptr
    for rp, rd, q, m2, ld in ((float("nan"), 1.0, 0.0, 0.0, 3), (0.0, 1.0, 0.0, 0.0, 3), (1.0, -1.0, 0.0, 0.0, 3), (1.0, 1.0, -1.0, 0.0, 3),
                              (1.0, 1.0, 0.0, float("nan"), 3), (1.0, 1.0, 0.0, 0.0, 2)):
        i, fl = p(z, torch.int32), p(zf, torch.float32)
        assert _lib.lib().cmf_track_states(1, 1, i, i, 0, i, i, fl, fl, i, i, i, fl, ld, zd.data_ptr(), rp, rd, q, m2, i, i, zd.data_ptr(), zd.data_ptr(),
                                           zd.data_ptr(), zd.data_ptr(), fl, fl, fl, i, fl, fl, _lib.stream_ptr()) != 0


# ---- 3. the pose of a clip's first frame and across a clip boundary ---------------------------------------------------------------------
def test_first_frame_and_clip_boundary_poses(world, dev):
    """poses[f-1] is the pose of scan 1 of frame f -- except at a clip's first frame, where it belongs to the clip before and the
    identity is taken: poisoning it must change nothing of the second clip; and with the same frames as ONE clip the second part is measured through
    the chain that runs on across the boundary, which changes every state behind it."""
    frames, split, store = world
    clean = ref.world_tables(frames, "gt")
    rows, total = clean["total"], clean["total"]
    base = _call(clean, dev, ref.WORLD_CLIPS, total, rows)
    poisoned = dict(clean, poses=clean["poses"].copy())
    boundary = ref.WORLD_CLIPS[1][0]
    poisoned["poses"][boundary - 1] = np.nan                                 # the last pose of the first clip: scan 2 of ITS last frame, nothing of the second clip
    got = _call(poisoned, dev, ref.WORLD_CLIPS, total, rows)
    a = int(clean["off1"][boundary])
    for k in ref.KEYS:
        assert np.array_equal(got[k][a:], base[k][a:]), k
    assert np.isfinite(got["state"][a:]).all() and np.isnan(got["state"][:a]).any()      # the first clip's last frame did read it (as A_f)
    first_rows = np.flatnonzero(base["row_frame"] == boundary)
    assert len(first_rows) == 5 and first_rows[0] == a
    zp = base["filt"][first_rows][:, :3]
    heads = clean["prev_row"][first_rows] < 0
    assert heads.all() and np.array_equal(zp, clean["centroid"][first_rows].astype(f64))     # the identity: a head's filtered position IS its centroid
    # one clip over everything: the restatement agrees, and the rows behind the boundary differ from the two-clip result
    one = dict(clean, poses=rref.pose_chain(clean["T"], [(0, len(frames))]).reshape(-1, 16))
    got = _call(one, dev, [(0, len(frames))], total, rows)
    ref.same(got, ref.run(one, out=ref.outputs(rows, SENTINEL), clips=[(0, len(frames))]), "one clip")
    assert np.array_equal(got["state"][:a], base["state"][:a]) and not np.array_equal(got["state"][first_rows], base["state"][first_rows])


# ---- 4. the store's shorthand and the views -----------------------------------------------------------------------------------------------
def test_store_objects_views_velocity_and_track_size(world):
    frames, split, store = world
    inst = I.cluster(split, store, eps=1.5, min_points=3, flow_weight=0.5)
    trk = K.track(inst, split, store, gate=1.5, max_gap=1)
    want = _host(O.estimate(trk, split, store, sigma_pos=0.4, min_disp=0.1))
    got = store.objects(split, sigma_pos=0.4, min_disp=0.1, gate=1.5, max_gap=1, eps=1.5, min_points=3, flow_weight=0.5)
    ref.same(_host(got), want, "store.objects")
    assert (got.sigma_pos, got.sigma_disp, got.sigma_acc, got.min_disp) == (0.4, 0.25, 0.25, 0.1) and (got.trk.gate, got.trk.max_gap) == (1.5, 1)
    obj = store.objects(split, trk=trk, sigma_pos=0.4, min_disp=0.1)
    ref.same(_host(obj), want, "store.objects(trk)")
    gt = K.track(I.cluster(split, None, which="gt"), split)
    ref.same(_host(store.objects(split, trk=gt)), _host(O.estimate(gt, split)), "store.objects(gt)")
    # the views and the derived arrays against numpy
    off, count = inst.offsets_host, inst.count.cpu().numpy()
    view = obj.frame(6)
    a = int(off[6])
    assert view["state"].shape == (int(count[6]), 6) and all(torch.equal(view[k], getattr(obj, k)[a:a + int(count[6])]) for k in ref.KEYS)
    per_row = np.repeat(split.interval.cpu().numpy(), np.diff(off))
    assert np.array_equal(obj.velocity().cpu().numpy().view(np.uint32), (want["vel"] / per_row[:, None]).astype(f32).view(np.uint32))
    yaw = np.arctan2(want["heading"][:, 1].astype(f64), want["heading"][:, 0].astype(f64))
    assert np.abs(obj.yaw().cpu().numpy() - yaw).max() <= 4 * 2.0 ** -22
    track = trk.track.cpu().numpy()
    size = np.zeros((len(track), 3), f32)
    for r in np.flatnonzero(want["row_frame"] >= 0):
        first = [c0 for c0, c1 in ref.WORLD_CLIPS if c0 <= want["row_frame"][r] < c1][0]
        size[int(off[first]) + track[r]] = np.maximum(size[int(off[first]) + track[r]], want["box_size"][r])
    got = obj.track_size()
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), size) and (size > 0).any(axis=1).sum() == int(trk.ntracks.sum())


# ---- 5. nothing waits for the device ----------------------------------------------------------------------------------------------------
def test_no_call_waits_for_the_device(world):
    frames, split, store = world
    inst, pred = I.cluster(split, None, which="gt"), I.cluster(split, store)
    gt_trk, pr_trk = K.track(inst, split, gate=ref.GATE, max_gap=2), K.track(pred, split, store, gate=ref.GATE, max_gap=2)
    O.estimate(gt_trk, split).track_size()                                  # warm: library, allocator
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gt = O.estimate(gt_trk, split)
        pr = O.estimate(pr_trk, split, store, sigma_acc=0.1)
        sizes, speed, yaw = gt.track_size(), pr.velocity(), pr.yaw()
        with pytest.raises(RuntimeError):
            split.off1.cpu()                                               # the control: a read-back IS caught in this mode
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    ref.same(_host(gt), _restated(gt_trk, split, split.trans, gt.poses), "no wait, gt")
    ref.same(_host(pr), _restated(pr_trk, split, store.pred_trans, pr.poses, (0.5, 0.25, 0.1, 0.05)), "no wait, pred")
    assert sizes.shape == (split.tab1.shape[0], 3) and speed.shape == sizes.shape and yaw.shape == (sizes.shape[0],)
