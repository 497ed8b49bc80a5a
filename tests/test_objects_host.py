"""CPU: what cmflow_amd/objects.py means and what its host side does.  The numpy restatement (tests/objects_ref.py: the filter and the
Rauch-Tung-Striebel recursion of include/cmflow_hip.h) is held against a second, differently written smoother (the MAP estimate by
least squares) and against a world whose answer is known without either; the headings and the boxes are checked to be what they are
for; with noise on the centroids the smoothed positions must beat the raw ones; the corrupted tables of the entry point's test go
through the restatement; every refusal of ``estimate`` comes before any launch; the header's prototype and the ctypes signature
agree; and the reference's own saved frames go through the restatement.  The device code is tied to the restatement bit for bit in
tests/test_gpu_objects.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import instances_ref as iref
import objects_ref as ref
import results_ref as rref
import tracks_ref as tref
from cmflow_amd import _lib
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import objects as O
from cmflow_amd import results as R
from cmflow_amd import tracks as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
f32, f64 = np.float32, np.float64
# The largest difference between the restatement's smoothed states and the least-squares solution, over both worlds, both clips and
# all three axes at the default parameters, as measured when this test was written: 5.4e-14 m (positions of up to 60 m in float64).
# The tolerance is 100 times that and, as required, never more than 1e-6 m.
LSTSQ_MEASURED = 5.4e-14
TOL = min(100 * LSTSQ_MEASURED, 1e-6)


@pytest.fixture(scope="module")
def worlds():
    """{exact: (frames, owners, truth, tables of the labels' side, the restatement's outputs)}"""
    made = {}
    for exact in (True, False):
        frames, owners, truth = ref.build_world(exact=exact)
        t = ref.world_tables(frames, "gt")
        made[exact] = (frames, owners, truth, t, ref.run(t))
    return made


def _first_of(f):
    return [a for a, b in ref.WORLD_CLIPS if a <= f < b][0]


def _measured(t, rows, out):
    """(len(rows),3) zp and zd of the rows, in the clip's axes."""
    poses = t["poses"].reshape(-1, 4, 4)
    z = [ref.measure(poses, _first_of(int(out["row_frame"][k])), int(out["row_frame"][k]), t["centroid"][k], t["disp"][k]) for k in rows]
    return np.array([a for a, _ in z]), np.array([b for _, b in z])


# ---- the world is what it is for ---------------------------------------------------------------------------------------------------------
def test_the_world_has_what_the_kernel_can_get_wrong(worlds):
    for exact, (frames, owners, truth, t, out) in worlds.items():
        assert len(frames) <= 20 and max(len(fr["pos1"]) for fr in frames) <= 40 and ref.WORLD_OBJECTS <= 6
        lengths = sorted(len(c) for c in ref.chains(out, t["total"]))
        assert lengths == [1, 7, 7, 7, 7, 7, 9, 11, 11, 11, 11]              # a single hit, an absence (9 of 11), chains of at least 3
        held = out["row_frame"] >= 0
        assert sorted(set(t["gap"][held].tolist())) == [0, 1, 3]             # the absence of two frames: a gap of 3
        who = ref.row_owner(t, owners)
        assert (out["heading_src"][held & (who == ref.SLOW)] == 0).all() and (out["heading_src"][held & (who != ref.SLOW)] == 1).all()
        assert (who[held] == ref.SLOW).sum() == 18 and (who[held] == ref.ONCE).sum() == 1
        assert tref_rotates(t["T"]) and int(held.sum()) == int(t["count"].sum()) == 89
        # the links are the inverse of the tracker's prev_row, and row_frame is the frame
        for r in np.flatnonzero(held):
            assert out["next_row"][r] < 0 or t["prev_row"][out["next_row"][r]] == r
            assert t["prev_row"][r] < 0 or out["next_row"][t["prev_row"][r]] == r
            assert t["off1"][out["row_frame"][r]] <= r < t["off1"][out["row_frame"][r] + 1]
        rest = ~held
        assert (out["row_frame"][rest] == -1).all() and (out["heading_src"][rest] == -1).all() and not out["state"][rest].any() and not out["box_size"][rest].any()


def tref_rotates(T):
    return bool((np.abs(T[:, 0, 1]) > 0.02).all())


# ---- the restatement against least squares ------------------------------------------------------------------------------------------------
def test_restatement_is_the_map_estimate(worlds):
    worst = worst_cov = 0.0
    for exact, (frames, owners, truth, t, out) in worlds.items():
        assert ref.PARAMS[2] > 0
        for chain in ref.chains(out, t["total"]):
            zp, zd = _measured(t, chain, out)
            gaps = [min(max(int(t["gap"][k]), 1), ref.MAX_GAP + 1) for k in chain[1:]]
            for r in range(3):
                x, cov = ref.smooth_lstsq(zp[:, r], zd[:, r], gaps, *ref.PARAMS[:3])
                worst = max(worst, float(np.abs(x - out["state"][chain][:, [r, 3 + r]]).max()))
                worst_cov = max(worst_cov, float(np.abs(cov - out["scov"][chain]).max()))
    print("restatement against lstsq: largest difference %.3g m (tolerance %.3g), covariance %.3g m^2" % (worst, TOL, worst_cov))
    assert worst <= TOL and TOL <= 1e-6
    assert worst_cov <= 1e-12                                                # measured 1.3e-16 on entries of at most 0.25 m^2: the inverse of the normal matrix


def test_smoothed_state_is_the_truth_on_the_noise_free_world(worlds):
    """exact world: every position, flow and transform is a dyadic rational float32 holds, so the measurements are the truth and the
    smoother must return it.  (In the other world the float32 positions are rounded by up to 2e-6 m -- 3e-6 m in the states, more than
    the tolerance allows -- which is why the exact world exists.)"""
    frames, owners, truth, t, out = worlds[True]
    want = ref.row_truth(t, owners, truth)
    held = out["row_frame"] >= 0
    zp, zd = _measured(t, np.flatnonzero(held), out)
    assert np.array_equal(zp, want[held][:, :3]) and np.array_equal(zd, want[held][:, 3:])
    for k in ("state", "filt"):
        err = float(np.abs(out[k][held] - want[held]).max())
        print("%s against the truth: %.3g (tolerance %.3g)" % (k, err, TOL))
        assert err <= TOL
    assert (out["scov"][held][:, 0] <= out["fcov"][held][:, 0] * (1 + 1e-12)).all() and (out["scov"][held][:, 0] > 0).all()
    rounded = worlds[False]
    held = rounded[4]["row_frame"] >= 0
    err = float(np.abs(rounded[4]["state"][held] - ref.row_truth(rounded[3], rounded[1], rounded[2])[held]).max())
    assert 1e-7 < err < 1e-5                                                 # float32 coordinates at 40 m: what the other world cannot show


def _frame_axes(t, f, v):
    """A vector of the clip's axes in the scan-1 axes of frame f, by numpy.linalg."""
    first = _first_of(f)
    W = np.eye(4) if f == first else t["poses"].reshape(-1, 4, 4)[f - 1]
    return np.linalg.inv(W[:3, :3]) @ v


def test_headings_point_along_the_true_velocity(worlds):
    for exact, (frames, owners, truth, t, out) in worlds.items():
        who = ref.row_owner(t, owners)
        checked = 0
        for r in np.flatnonzero(out["row_frame"] >= 0):
            f = int(out["row_frame"][r])
            if who[r] == ref.SLOW:
                assert out["heading"][r].tolist() == [1.0, 0.0]
                continue
            vel = truth[0 if f < ref.WORLD_CLIPS[0][1] else 1][1][who[r]]
            v = _frame_axes(t, f, vel)
            want = v[:2] / np.linalg.norm(v[:2])
            # a unit vector's coordinates rounded to float32: 2^-24 each; the exact world's states are the truth to TOL, the other
            # world's to the 3e-6 m of its float32 coordinates on displacements of at least 0.25 m a frame
            bound = 2.0 ** -24 + (TOL if exact else 3e-6 / 0.25) / np.linalg.norm(v[:2])
            assert np.abs(out["heading"][r].astype(f64) - want).max() <= bound, (exact, r, out["heading"][r], want)
            assert abs(np.linalg.norm(out["heading"][r].astype(f64)) - 1.0) <= 2.0 ** -23
            checked += 1
        assert checked == 71


def test_boxes_enclose_their_points_and_no_smaller_box_does(worlds):
    for exact, (frames, owners, truth, t, out) in worlds.items():
        for r in np.flatnonzero(out["row_frame"] >= 0):
            f = int(out["row_frame"][r])
            a, b = int(t["off1"][f]), int(t["off1"][f + 1])
            pts = t["tab1"][a:b][t["label"][a:b] == r - a].astype(f64)
            assert len(pts) >= 2
            h = out["heading"][r].astype(f64)
            n = np.array([-h[1], h[0]])
            centre, size = out["box_center"][r].astype(f64), out["box_size"][r].astype(f64)
            rel = pts - centre
            along = np.stack([rel[:, :2] @ h, rel[:, :2] @ n, rel[:, 2]], axis=1)
            # the box is formed in float64 and every output rounded once to float32: a face lies within half a float32 ulp of the
            # centre's coordinates (|h . e| <= |ex| + |ey|) and a quarter ulp of the size, plus the tolerance
            ulp = lambda v: float(np.spacing(np.abs(v).astype(f32)).astype(f64).sum())
            bound = np.array([0.5 * ulp(out["box_center"][r, :2]), 0.5 * ulp(out["box_center"][r, :2]), 0.5 * ulp(out["box_center"][r, 2:])]) \
                + 0.25 * np.spacing(out["box_size"][r]).astype(f64) + TOL
            assert (np.abs(along.max(axis=0) - size / 2) <= bound).all(), (exact, r, along.max(axis=0), size / 2, bound)   # every face touches a point
            assert (np.abs(along.min(axis=0) + size / 2) <= bound).all(), (exact, r, along.min(axis=0), size / 2, bound)
            if out["heading_src"][r] == 0:                                   # the axis-aligned box the instance already has
                lo, hi = pts.min(axis=0), pts.max(axis=0)
                assert np.abs(size - (hi - lo)).max() <= 2 * bound.max() and np.abs(centre - (lo + hi) / 2).max() <= 2 * bound.max()


def test_smoothing_beats_the_raw_centroids_under_noise(worlds):
    """Gaussian noise of 0.3 m (seed 0) on the centroids of the rounded world, the tracks those of the clean world, the default
    parameters.  Measured: raw RMS position error 0.544 m, smoothed 0.237 m (seeds 1-3: 0.509/0.202, 0.522/0.234, 0.479/0.201)."""
    frames, owners, truth, clean, _ = worlds[False]
    t = ref.world_tables(frames, "gt", sigma=0.3, seed=0)
    out = ref.run(t)
    want = ref.row_truth(clean, owners, truth)
    held = out["row_frame"] >= 0
    raw, _ = _measured(t, np.flatnonzero(held), out)
    rms = lambda e: float(np.sqrt((e ** 2).sum(axis=1).mean()))
    raw_rms, smooth_rms = rms(raw - want[held][:, :3]), rms(out["state"][held][:, :3] - want[held][:, :3])
    print("noise 0.3 m: raw RMS %.3f m, smoothed RMS %.3f m" % (raw_rms, smooth_rms))
    assert 0.4 < raw_rms < 0.7                                               # the noise is there: sqrt(3) * 0.3 = 0.52
    assert smooth_rms < raw_rms


# ---- what the GPU test asks of the entry point, here of the restatement ------------------------------------------------------------------
def test_corrupted_tables_go_through_the_restatement(worlds):
    t = worlds[False][3]
    bad, clips, total = ref.corrupt_tables(t)
    F, rows = len(bad["count"]), t["total"] + 8
    bad["poses"] = rref.pose_chain(bad["T"], clips).reshape(-1, 16)
    fill = {k: -77 for k in ref.KEYS}
    out = ref.run(bad, out=ref.outputs(rows, fill), clips=clips, total=total)
    owned = np.zeros(rows, bool)
    owned[:int(t["off1"][F - 1])] = True                                    # the five clips cover frames 0 .. F-2; the last frame ends behind total
    for k in ref.KEYS:
        assert (out[k][~owned] == -77).all(), k
    for k in ref.INT_KEYS:
        assert (out[k][owned] != -77).all(), k
    a, b = int(t["off1"][5]), int(t["off1"][6])
    assert (out["row_frame"][a:b] == 5).all()                               # count 5000: clamped to the frame's rows, every row an instance
    held = out["row_frame"][:total] >= 0
    nxt = out["next_row"][:total][held]
    assert ((nxt < 0) | (out["row_frame"][np.maximum(nxt, 0)] > out["row_frame"][:total][held])).all()   # a successor lies in a strictly later frame
    assert max(len(c) for c in ref.chains(out, total)) <= 10                # no chain is longer than its clip: (4, 14) is the longest
    assert np.isnan(out["state"][:total][held]).any()                       # the NaN centroid went through the arithmetic


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def _cpu_split(counts, clips=None):
    rng = np.random.default_rng(0)
    z = lambda *s: np.zeros(s, dtype=f32)
    items = [(rng.standard_normal((n, 3)).astype(f32), z(4, 3) + 1, z(n, 3), z(4, 3), np.eye(4, dtype=f32), z(n, 3), z(n), 0.1, z(n), z(n), z(n, 2))
             for n in counts]
    return D.DeviceSplit.from_items(items, "cpu", clips)


def _cpu_tracks(split, which="gt"):
    total, F = split.tab1.shape[0], len(split)
    t = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    tables = (t(total), t(total), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32))
    off = np.concatenate(([0], np.cumsum(split.counts_host[0])))
    inst = I.FrameInstances(split.off1, torch.arange(F), t(total) - 1, t(total, dt=torch.uint8), t(F), tables, split.interval, which, 2.0, 2, 0.0,
                            off, np.arange(F))
    arrays = (t(total) - 1, t(total) - 1, t(total), t(total), t(total, 3, dt=torch.float32), t(total) - 1, t(total) - 1, t(total) - 1, t(total))
    clips = K.plan_clips(F, split.clips)
    return K.InstanceTracks(inst, arrays, t(len(clips)), t(len(clips)), torch.from_numpy(clips), clips, 2.0, 2)


def test_every_refusal_comes_before_any_launch():
    split = _cpu_split([5, 1, 9, 4])
    store = R.SplitResults.empty(split)
    trk, pred = _cpu_tracks(split), _cpu_tracks(split, "pred")
    with pytest.raises(ValueError, match="track"):
        O.estimate(trk.inst, split)
    with pytest.raises(ValueError, match="store"):
        O.estimate(pred, split)
    with pytest.raises(ValueError, match="not the one"):
        O.estimate(trk, _cpu_split([5, 1, 9, 5]))
    with pytest.raises(ValueError, match="not the one"):
        O.estimate(trk, _cpu_split([5, 1, 13]))
    with pytest.raises(ValueError, match="not the one"):
        O.estimate(pred, split, R.SplitResults.empty(_cpu_split([5, 1, 9, 3, 1])))
    for name in ("sigma_pos", "sigma_disp"):
        for v in (0.0, -1.0, float("nan"), float("inf"), None, "2", True):
            with pytest.raises(ValueError, match=name):
                O.estimate(trk, split, **{name: v})
    for name in ("sigma_acc", "min_disp"):
        for v in (-1e-9, float("nan"), float("inf"), None, "0", False):
            with pytest.raises(ValueError, match=name):
                O.estimate(trk, split, **{name: v})
    with pytest.raises(ValueError, match="belong to the tracks"):
        store.objects(split, trk=pred, gate=3.0)
    # everything in order: only the device is wrong -- and that is the LAST refusal
    with pytest.raises(RuntimeError, match="GPU"):
        O.estimate(trk, split, sigma_acc=0.0, min_disp=0.0)
    with pytest.raises(RuntimeError, match="GPU"):
        O.estimate(pred, split, store, sigma_pos=1, sigma_disp=2)
    with pytest.raises(RuntimeError, match="GPU"):
        store.objects(split, trk=pred, sigma_pos=0.3)
    with pytest.raises(RuntimeError, match="GPU"):
        store.objects(split, which="gt", gate=1.5, min_disp=0.1)            # forms instances first: their refusal, on the same ground
    sig = inspect.signature(O.estimate).parameters
    assert list(sig) == ["trk", "split", "store", "sigma_pos", "sigma_disp", "sigma_acc", "min_disp"]
    assert tuple(sig[k].default for k in list(sig)[2:]) == (None,) + ref.PARAMS == (None, 0.5, 0.25, 0.25, 0.05)
    assert list(inspect.signature(R.SplitResults.objects).parameters)[:3] == ["self", "split", "trk"]
    assert O.PER_INSTANCE == ref.KEYS


def test_views_velocity_and_track_size_on_the_host(worlds):
    frames, owners, truth, t, out = worlds[False]
    F, total = len(t["count"]), t["total"]
    z3 = torch.zeros(total, 3)
    interval = torch.tensor([0.1 + 0.01 * (f % 3) for f in range(F)])
    off = torch.from_numpy(t["off1"].astype(np.int32))
    inst = I.FrameInstances(off, torch.arange(F), torch.from_numpy(t["label"]), torch.ones(total, dtype=torch.uint8), torch.from_numpy(t["count"]),
                            (torch.zeros(total, dtype=torch.int32), torch.zeros(total, dtype=torch.int32), torch.from_numpy(t["centroid"]),
                             torch.from_numpy(t["disp"]), z3, z3), interval, "gt", 2.0, 2, 0.0, t["off1"].astype(np.int64), np.arange(F))
    tr = tref.track(t["off1"], total, t["count"], t["label"], t["centroid"], t["disp"], t["T"].reshape(-1, 16), ref.WORLD_CLIPS, ref.GATE, 2)
    trk = K.InstanceTracks(inst, tuple(torch.from_numpy(tr[k]) for k in tref.PER_INSTANCE + tref.PER_TRACK), torch.from_numpy(tr["ntracks"]),
                           torch.from_numpy(tr["overflow"]), torch.from_numpy(t["clips"]), t["clips"], ref.GATE, 2)
    base = np.zeros(F, np.int64)
    for a, b in ref.WORLD_CLIPS:
        base[a:b] = t["off1"][a]
    obj = O.TrackObjects(trk, tuple(torch.from_numpy(out[k]) for k in ref.KEYS), torch.from_numpy(t["poses"]), torch.from_numpy(base), interval, *ref.PARAMS)
    assert len(obj) == 2 and (obj.sigma_pos, obj.sigma_disp, obj.sigma_acc, obj.min_disp, obj.which) == ref.PARAMS + ("gt",)
    view = obj.frame(6)
    a = int(t["off1"][6])
    assert view["state"].shape == (6, 6) and view["heading"].shape == (6, 2) and torch.equal(view["box_size"], obj.box_size[a:a + 6])
    per_row = np.repeat(interval.numpy(), np.diff(t["off1"]))
    assert np.array_equal(obj.velocity().numpy(), out["vel"] / per_row[:, None])
    yaw = np.arctan2(out["heading"][:, 1].astype(f64), out["heading"][:, 0].astype(f64))
    assert np.abs(obj.yaw().numpy() - yaw).max() <= 4 * 2.0 ** -22          # a convenience, not bit-exact: four float32 ulps at pi
    want = np.zeros((total, 3), f32)
    for r in np.flatnonzero(out["row_frame"] >= 0):
        row = base[out["row_frame"][r]] + tr["track"][r]
        want[row] = np.maximum(want[row], out["box_size"][r])
    got = obj.track_size().numpy()
    assert got.dtype == f32 and np.array_equal(got, want) and (want > 0).any(axis=1).sum() == int(tr["ntracks"].sum()) == 11


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_prototype_and_ctypes_signature_agree():
    text = open(os.path.join(REPO, "include", "cmflow_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+cmf_track_states\s*\(([^)]*)\)\s*;", text)
    assert m
    kinds = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double}
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else kinds[arg.rsplit(" ", 1)[0]])
    assert want == _lib.SIGNATURES["cmf_track_states"] and len(want) == 32
    # the outputs follow the inputs in the order ``estimate`` passes them
    names = [" ".join(a.split()).rsplit(" ", 1)[1].lstrip("*") for a in m.group(1).split(",")]
    assert tuple(names[19:31]) == ref.KEYS and names[31] == "stream"
    src = open(os.path.join(REPO, "cmflow_amd", "csrc", "Makefile")).read()
    assert re.search(r"objects\.o: FLAGS \+= -ffp-contract=off", src)


# ---- the reference's own saved frames -----------------------------------------------------------------------------------------------------
def test_saved_frames_go_through_the_restatement():
    g = np.load(os.path.join(GOLDEN, "saved_results_delft_12_w12.npz"))
    off, pc1, pred_f, pred_m, pred_t = g["off"], g["pc1"], g["pred_f"], g["pred_m"], g["pred_t"]
    inst = iref.cluster(off, pc1, pred_f, pred_m == 0, pred_t, list(range(12)), 2.0, 2, 0.0)
    T = pred_t.reshape(12, 16).astype(f32)
    trk = tref.track(off, int(off[-1]), inst["count"], inst["label"], inst["centroid"], inst["disp"], T, [(0, 12)], 2.0, 2)
    poses = rref.pose_chain(T.reshape(12, 4, 4), [(0, 12)]).reshape(12, 16)
    out = ref.states(off, int(off[-1]), inst["count"], inst["label"], inst["centroid"], inst["disp"], trk["track"], trk["prev_row"], trk["gap"],
                     np.ascontiguousarray(pc1[:, :3]).astype(f32), poses, [(0, 12)], *ref.PARAMS)
    found = sorted(ref.chains(out, int(off[-1])), key=len)
    assert [len(c) for c in found] == [1, 12]
    rows = found[1]
    assert rows == [int(off[f]) for f in range(12)] and out["row_frame"][rows].tolist() == list(range(12))
    for k in ref.KEYS:
        assert np.isfinite(out[k][rows]).all(), k
    assert (out["heading_src"][rows] == 1).all() and (out["box_size"][rows] > 0).all()
    assert np.abs(np.linalg.norm(out["heading"][rows].astype(f64), axis=1) - 1.0).max() < 1e-6
    # the smoothed positions stay near the measured ones (0.61 m is the tracker's largest prediction error on these frames)
    assert np.abs(out["pos"][rows] - inst["centroid"][rows]).max() < 0.62
