"""CPU: what cmflow_amd/accumulate.py means and what its host side does.  The numpy restatement (tests/accumulate_ref.py) is held
against worlds whose answer is known without it -- static points seen from moving sensors, an object at constant velocity -- and
against the pose chain of results_ref; the product's host arithmetic (capacities, refusals) against the restatement's; the
reference's own saved frames go through it.  The device code is tied to the restatement bit for bit in tests/test_gpu_accumulate.py."""
import inspect
import os

import numpy as np
import pytest
import torch

import accumulate_ref as ref
import results_ref
from cmflow_amd import accumulate as A
from cmflow_amd import dataset as D
from cmflow_amd import results as R
from cmflow_amd import vis

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32, f64 = np.float32, np.float64

# The restatement on float32-rounded inputs (what a split holds) against the same restatement on the unrounded float64 inputs, window 8,
# ranges up to 60 m, 16 seeds of each world below (test_the_bound_is_four_times_the_measured_rounding prints and re-measures it):
MEASURED_ROUNDING_STATIC = 9.54e-6                          # metres, largest coordinate deviation seen
MEASURED_ROUNDING_MOVING = 3.85e-6
BOUND_STATIC = 4 * MEASURED_ROUNDING_STATIC
BOUND_MOVING = 4 * MEASURED_ROUNDING_MOVING
WINDOW = 8


def _rigid(rng, yaw_max=0.1, step=1.5):
    yaw, pitch, roll = rng.uniform(-yaw_max, yaw_max), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)
    c, s = np.cos, np.sin
    Rz = np.array([[c(yaw), -s(yaw), 0], [s(yaw), c(yaw), 0], [0, 0, 1.0]])
    Ry = np.array([[c(pitch), 0, s(pitch)], [0, 1, 0], [-s(pitch), 0, c(pitch)]])
    Rx = np.array([[1.0, 0, 0], [0, c(roll), -s(roll)], [0, s(roll), c(roll)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = (rng.uniform(0.5, step), rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05))
    return T


def _apply(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


def static_world(seed, L=12, K=300):
    """K fixed world points, L+1 sensor poses (sensor -> world, each a rigid step from the last), scan k = a random subset of the world
    in sensor k's coordinates, up to 60 m away.  Frame k = (scan k, scan k+1), T_k = inv(P_k+1) P_k.  All float64.
    -> off1, pos, T (L,4,4), which world point every row is, poses, world."""
    rng = np.random.default_rng(seed)
    poses = [np.eye(4)]
    for _ in range(L):
        poses.append(poses[-1] @ _rigid(rng))
    world = np.stack([rng.uniform(5.0, 60.0, K), rng.uniform(-25.0, 25.0, K), rng.uniform(-2.0, 4.0, K)], axis=1)
    pos, who, off1 = [], [], [0]
    for k in range(L):
        pick = np.sort(rng.choice(K, rng.integers(K // 3, K), replace=False))
        pos.append(_apply(np.linalg.inv(poses[k]), world[pick]))
        who.append(pick)
        off1.append(off1[-1] + pick.size)
    T = np.stack([np.linalg.inv(poses[k + 1]) @ poses[k] for k in range(L)])
    return np.array(off1), np.concatenate(pos), T, np.concatenate(who), poses, world


def moving_world(seed, L=12, K=120, B=40):
    """Translation-only ego-motion (sensor k at c_k), K static world points and a rigid object of B points at constant world velocity
    v; every scan sees a random subset of both.  The flow of a point is its own displacement from scan k to scan k+1 in sensor
    coordinates.  -> off1, pos, flow, moving, T, (static?, index) per row, c, world, body, v."""
    rng = np.random.default_rng(seed)
    c = np.concatenate((np.zeros((1, 3)), np.cumsum(np.stack([rng.uniform(0.5, 1.5, L), rng.uniform(-0.2, 0.2, L), rng.uniform(-0.05, 0.05, L)], axis=1), axis=0)))
    world = np.stack([rng.uniform(5.0, 60.0, K), rng.uniform(-25.0, 25.0, K), rng.uniform(-2.0, 4.0, K)], axis=1)
    body = np.array([30.0, -5.0, 0.5]) + rng.uniform(-2.0, 2.0, (B, 3))
    v = np.array([-1.1, 0.6, 0.02])                                         # metres per frame
    pos, flow, moving, who, off1 = [], [], [], [], [0]
    for k in range(L):
        ps, pb = np.sort(rng.choice(K, rng.integers(K // 2, K), replace=False)), np.sort(rng.choice(B, rng.integers(B // 2, B), replace=False))
        step = c[k + 1] - c[k]
        pos += [world[ps] - c[k], body[pb] + k * v - c[k]]
        flow += [np.broadcast_to(-step, (ps.size, 3)), np.broadcast_to(v - step, (pb.size, 3))]
        moving += [np.zeros(ps.size, bool), np.ones(pb.size, bool)]
        who += [np.stack((np.ones(ps.size, np.int64), ps), 1), np.stack((np.zeros(pb.size, np.int64), pb), 1)]
        off1.append(off1[-1] + ps.size + pb.size)
    T = np.tile(np.eye(4), (L, 1, 1))
    T[:, :3, 3] = -(c[1:] - c[:-1])
    return np.array(off1), np.concatenate(pos), np.concatenate(flow), np.concatenate(moving), T, np.concatenate(who), c, world, body, v


def _rounded(*arrays):
    return [np.asarray(a).astype(f32) for a in arrays]


def _run_static(seed):
    off1, pos, T, who, poses, world = static_world(seed)
    ids = list(range(len(T)))
    p32, T32 = _rounded(pos, T)
    zeros, still = np.zeros_like(pos), np.zeros(len(pos), bool)
    got = ref.accumulate(off1, p32, zeros.astype(f32), still, T32, None, ids, WINDOW, "keep")
    ideal = ref.accumulate(off1, pos, zeros, still, T, None, ids, WINDOW, "keep", rounded=False)
    target = np.repeat(np.arange(len(ids)), np.diff(got["off"]))
    truth = np.stack([_apply(np.linalg.inv(poses[j]), world[who[r]]) for j, r in zip(target, got["src"])])
    return got, ideal, truth


def _run_moving(seed, dynamic):
    off1, pos, flow, moving, T, who, c, world, body, v = moving_world(seed)
    ids = list(range(len(T)))
    p32, f32_, T32 = _rounded(pos, flow, T)
    got = ref.accumulate(off1, p32, f32_, moving, T32, None, ids, WINDOW, dynamic)
    ideal = ref.accumulate(off1, pos, flow, moving, T, None, ids, WINDOW, dynamic, rounded=False)
    target = np.repeat(np.arange(len(ids)), np.diff(got["off"]))
    truth = np.stack([world[m] - c[j] if st else body[m] + j * v - c[j] for j, (st, m) in zip(target, who[got["src"]])])
    return got, ideal, truth, moving[got["src"]]


# ---- meaning ----------------------------------------------------------------------------------------------------------------------------
def test_the_bound_is_four_times_the_measured_rounding():
    """The two constants above, measured again: float32-rounded inputs against unrounded ones through the same restatement."""
    dev_s = max(np.abs(g["xyz"].astype(f64) - i["xyz"]).max() for g, i, _ in (_run_static(s) for s in range(16)))
    dev_m = max(np.abs(g["xyz"].astype(f64) - i["xyz"]).max() for g, i, _, _ in (_run_moving(s, "propagate") for s in range(16)))
    print("rounding of the inputs, window %d: static world %.3g m, moving world %.3g m" % (WINDOW, dev_s, dev_m))
    assert dev_s <= MEASURED_ROUNDING_STATIC * 1.0001 and dev_m <= MEASURED_ROUNDING_MOVING * 1.0001
    assert dev_s >= MEASURED_ROUNDING_STATIC / 2 and dev_m >= MEASURED_ROUNDING_MOVING / 2      # the constants are not stale


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_static_points_land_on_the_world_as_seen_from_the_target(seed):
    """Every source point of every age must lie where ITS world point is in the target's sensor frame: an inverted transform, a
    reversed product or a wrong source frame errs by metres."""
    got, ideal, truth = _run_static(seed)
    assert got["age"].max() == WINDOW - 1 and (got["count"] == np.diff(got["off"])).all()
    err = np.abs(got["xyz"].astype(f64) - truth).max()
    print("static world %d: %d rows, max error %.3g m (bound %.3g), unrounded %.3g" % (seed, len(truth), err, BOUND_STATIC, np.abs(ideal["xyz"] - truth).max()))
    assert np.abs(ideal["xyz"] - truth).max() < 1e-11
    assert err <= BOUND_STATIC


@pytest.mark.parametrize("seed", [100, 101])
def test_a_moving_object_is_carried_to_its_current_position(seed):
    got, ideal, truth, moving = _run_moving(seed, "propagate")
    err = np.abs(got["xyz"].astype(f64) - truth).max()
    print("moving world %d: propagate max error %.3g m (bound %.3g), %d moving rows" % (seed, err, BOUND_MOVING, int(moving.sum())))
    assert np.abs(ideal["xyz"] - truth).max() < 1e-11 and err <= BOUND_MOVING
    kept, _, _, _ = _run_moving(seed, "keep")
    e = np.abs(kept["xyz"].astype(f64) - truth).max(-1)
    older = moving & (kept["age"] >= 1)
    assert older.sum() > 50 and e[~older].max() <= BOUND_MOVING            # static points and the current scan are right either way
    assert e[older].min() > 1.0                                             # a trail: at least one step of 1.1 m behind
    dropped, _, _, _ = _run_moving(seed, "drop")
    held = dropped["src"] >= 0
    assert (dropped["count"] == [int(h.sum()) for h in np.split(held, dropped["off"][1:-1])]).all()
    assert held.sum() == len(truth) - older.sum() and not held.all()
    back = {(int(t), int(s)): x for t, s, x in zip(np.repeat(np.arange(len(kept["count"])), np.diff(kept["off"])), kept["src"], kept["xyz"])}
    tg = np.repeat(np.arange(len(dropped["count"])), np.diff(dropped["off"]))
    assert all(np.array_equal(back[(int(t), int(s))], x) for t, s, x in zip(tg[held], dropped["src"][held], dropped["xyz"][held]))


def test_chain_is_the_relative_pose_of_the_pose_chain():
    """For exactly rigid transforms M_g = inv(P_j-1) P_j-g-1 with P = results_ref.pose_chain (P_k: the pose at scan 2 of frame k, the
    identity before the clip's first frame)."""
    rng = np.random.default_rng(4)
    L = 14
    T = np.stack([ref.small_transform(rng, exact=True) for _ in range(L)])
    clips = [(0, 9), (9, L)]
    P = results_ref.pose_chain(T, clips)
    worst = 0.0
    for a, b in clips:
        pose = lambda k: np.eye(4) if k < a else P[k]
        for j in range(a, b):
            M = ref.chain(T, j, min(12, j - a + 1))
            for g, Mg in enumerate(M):
                want = np.linalg.inv(pose(j - 1)) @ pose(j - g - 1)
                worst = max(worst, np.abs(Mg - want[:3]).max())
    print("chain against the pose chain: %.3g" % worst)
    assert worst <= 1e-12


# ---- host logic -------------------------------------------------------------------------------------------------------------------------
def _cpu_split(counts, clips=None, seed=0):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s).astype(f32)
    items = [(r(n, 3), r(4, 3), r(n, 3), r(4, 3), np.eye(4, dtype=f32), r(n, 3), (rng.random(n) < 0.5).astype(f32), 0.1, r(n), r(n), r(n, 2))
             for n in counts]
    return D.DeviceSplit.from_items(items, "cpu", clips)


def test_plan_is_the_restatements_capacity_rule():
    counts = [5, 1, 9, 4, 7, 3, 6, 2, 8]
    for clips in (None, [(0, 1), (1, 2), (2, 9)], [(0, 4), (4, 9)], [(1, 5)]):  # clips of one frame; frames outside every clip
        for window in (1, 2, 3, 8, 64):                                     # longer than any clip
            for ids in (list(range(9)), [8, 2, 2, 0], []):
                first, ages, cap_off = A.plan(counts, clips, ids, window)
                G, want = ref.capacities(counts, clips, ids, window)
                assert ages.tolist() == G.tolist() and cap_off.tolist() == want.tolist(), (clips, window, ids)
                assert first.tolist() == ref.clip_starts(9, clips)[ids].tolist()
                assert first.dtype == np.int32 and cap_off.dtype == np.int64
    first, ages, cap_off = A.plan(counts, [(0, 1), (1, 2), (2, 9)], range(9), 64)
    assert ages.tolist() == [1, 1, 1, 2, 3, 4, 5, 6, 7] and cap_off[1:3].tolist() == [5, 6]
    with pytest.raises(ValueError):
        A.plan(counts, None, [9], 2)
    with pytest.raises(ValueError):
        A.plan(counts, None, [-1], 2)


def test_drop_counts_and_padding_of_the_restatement():
    frames = ref.build_case()
    for which in ("pred", "gt"):
        off1, pos, flow, moving, T = ref.case_arrays(frames, which)
        out = ref.accumulate(off1, pos, flow, moving, T, ref.CLIPS, list(range(len(frames))), 5, "drop")
        start = ref.clip_starts(len(frames), ref.CLIPS)
        for j in range(len(frames)):
            want = ref.COUNTS[j] + sum(int((~moving[off1[i]:off1[i + 1]]).sum()) for i in range(max(start[j], j - 4), j))
            assert out["count"][j] == want
            a, b = out["off"][j] + want, out["off"][j + 1]
            assert (out["src"][a:b] == -1).all() and (out["age"][a:b] == 255).all() and not out["xyz"][a:b].any()
            assert (out["src"][out["off"][j]:a] >= 0).all()
        j = ref.F_ALL_MOVING + 1                                            # its predecessor contributes nothing
        assert ref.F_ALL_MOVING not in set(np.searchsorted(off1, out["src"][out["off"][j]:out["off"][j + 1]][:out["count"][j]], side="right") - 1)


def test_every_refusal_comes_before_any_launch():
    split = _cpu_split([5, 1, 9, 4], [(0, 3), (3, 4)])
    store = R.SplitResults.empty(split)
    for window in (0, 65, -1, 2.5, None):
        with pytest.raises(ValueError, match="window"):
            A.accumulate(split, store, window=window, which="gt")
    with pytest.raises(ValueError, match="which"):
        A.accumulate(split, store, window=2, which="label")
    with pytest.raises(ValueError, match="dynamic"):
        A.accumulate(split, store, window=2, which="gt", dynamic="trail")
    with pytest.raises(ValueError, match="store"):
        A.accumulate(split, None, window=2, which="pred")
    with pytest.raises(ValueError, match="not the one"):
        A.accumulate(_cpu_split([5, 1, 9, 5]), store, window=2)             # as many frames, another row count
    with pytest.raises(ValueError, match="not the one"):
        A.accumulate(_cpu_split([5, 1, 13]), store, window=2)               # as many rows, another frame count
    with pytest.raises(ValueError, match="no results"):
        A.accumulate(split, store, window=2)                                # nothing is done
    store.done[2:] = 1
    with pytest.raises(ValueError, match="no results"):
        A.accumulate(split, store, window=2, frames=[2])                    # frame 1 is a source of target 2
    with pytest.raises(ValueError, match="outside"):
        A.accumulate(split, store, window=2, frames=[4])
    with pytest.raises(ValueError, match="int64"):
        A.accumulate(split, store, window=2, frames=torch.tensor([1], dtype=torch.int32))
    # everything in order: only the device is wrong -- and that is the LAST refusal
    with pytest.raises(RuntimeError, match="GPU"):
        A.accumulate(split, store, window=1, frames=[2, 3])
    with pytest.raises(RuntimeError, match="GPU"):
        A.accumulate(split, store, window=2, frames=[3])                    # frame 3 starts a clip: frame 2 is no source... and is done anyway
    with pytest.raises(RuntimeError, match="GPU"):
        A.accumulate(split, None, window=64, which="gt", dynamic="propagate")
    with pytest.raises(RuntimeError, match="GPU"):
        store.accumulate(split, window=1, frames=[2])
    assert list(inspect.signature(R.SplitResults.accumulate).parameters) == ["self", "split", "window", "which", "dynamic", "frames"]
    assert list(inspect.signature(A.accumulate).parameters) == ["split", "store", "window", "which", "dynamic", "frames"]


def test_two_to_the_31_rows_are_refused():
    F, n = 64, 2 ** 24
    off = torch.arange(F + 1, dtype=torch.int64).mul(n).to(torch.int32)     # 2^30 rows: a split may be that large
    split = D.DeviceSplit(torch.zeros((0, 14)), torch.zeros((0, 6)), off, off, torch.zeros((F, 16)), torch.zeros(F), n)
    with pytest.raises(ValueError, match="2\\^31"):
        A.accumulate(split, None, window=64, which="gt")                    # 2^24 * 2080 rows
    with pytest.raises(ValueError, match="2\\^31"):
        A.accumulate(split, None, window=3, which="gt")                     # 2^24 * 189
    with pytest.raises(RuntimeError, match="GPU"):
        A.accumulate(split, None, window=2, which="gt")                     # 2^24 * 127 = 2^31 - 2^24 rows pass the count


def test_error_and_rendering_refusals_and_the_age_colours():
    cap = np.array([0, 3, 5], dtype=np.int64)
    mk = lambda dynamic, window=4, off=cap: A.AccumulatedClouds(torch.from_numpy(off).to(torch.int32), torch.tensor([3, 2], dtype=torch.int32),
                                                                torch.zeros((5, 3)), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8),
                                                                torch.arange(2), window, "gt", dynamic, off, np.arange(2))
    with pytest.raises(ValueError):
        A.accumulation_error(mk("drop"), mk("keep"))
    with pytest.raises(ValueError):
        A.accumulation_error(mk("keep"), mk("keep", window=5))
    with pytest.raises(ValueError):
        A.accumulation_error(mk("keep"), mk("propagate", off=np.array([0, 2, 5], dtype=np.int64)))
    split = _cpu_split([3, 2])
    with pytest.raises(ValueError):
        vis.render_accumulated(mk("keep"), R.SplitResults.empty(split), split, "depth")
    with pytest.raises(RuntimeError):
        vis.render_accumulated(mk("keep"), None, split, "age")
    for window in (1, 2, 5, 8, 64):
        age = np.concatenate((np.arange(window), [255, 64])).astype(np.uint8)
        got = vis.age_colors(torch.from_numpy(age), window).numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, ref.age_colors(age, window))
        assert got[0].tolist() == [65, 105, 225] and got[-1].tolist() == [80, 80, 80]
        assert window == 1 or got[window - 1].tolist() != [80, 80, 80]


# ---- the reference's own saved frames ---------------------------------------------------------------------------------------------------
def test_saved_frames_go_through_the_restatement():
    g = np.load(os.path.join(GOLDEN, "saved_results_delft_12_w12.npz"))
    off, pc1, pred_f, pred_m, pred_t = g["off"], g["pc1"], g["pred_f"], g["pred_m"], g["pred_t"]
    assert off.shape == (13,) and pc1.shape == (off[-1], 3) and pc1.dtype == f32 and pred_t.shape == (12, 4, 4) and int(g["first_frame"]) == 727
    moving = pred_m == 0
    assert 100 < moving.sum() < 400
    ids = list(range(12))
    for dynamic in ref.MODES:
        out = ref.accumulate(off, pc1, pred_f, moving, pred_t, None, ids, 8, dynamic)
        held = out["src"] >= 0
        assert np.isfinite(out["xyz"]).all() and (held == (out["age"] != 255)).all()
        now = out["age"] == 0
        assert np.array_equal(out["xyz"][now].view(np.uint32), pc1[out["src"][now]].view(np.uint32))
        assert np.abs(out["xyz"][held] - pc1[out["src"][held]]).max() < 15.0   # eight frames of driving, not a flight
    out = ref.accumulate(off, pc1, pred_f, moving, pred_t, None, ids, 8, "propagate")
    rows = (out["age"] == 1) & moving[out["src"]]
    want = (pc1[out["src"][rows]].astype(f64) + pred_f[out["src"][rows]].astype(f64)).astype(f32)
    assert rows.sum() > 100 and (np.abs(out["xyz"][rows] - want) <= np.spacing(np.abs(want))).all()
