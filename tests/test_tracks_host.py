"""CPU: what cmflow_amd/tracks.py means and what its host side does.  The numpy restatement (tests/tracks_ref.py: the literal sorted
greedy) is held against a second, differently written association (the mutual-best rounds the kernel runs) and against a world
whose answer is known without either; the special clips of the entry point's tables are checked to be what they are for; every
refusal of ``track`` comes before any launch; and the reference's own saved frames go through the restatement.  The device code is
tied to the restatement bit for bit in tests/test_gpu_tracks.py."""
import inspect
import os

import numpy as np
import pytest
import torch

import instances_ref as iref
import tracks_ref as ref
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import results as R
from cmflow_amd import tracks as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def tables():
    return ref.build_tables()


@pytest.fixture(scope="module")
def tracked(tables):
    t = tables
    stats = {}
    args = (t["off1"], t["total"], t["count"], t["label"], t["centroid"], t["disp"], t["T"], t["clips"], 2.0, 2)
    out = ref.track(*args)
    again = ref.track(*args, associate=ref.associate_rounds, stats=stats)
    return out, again, stats


def _clip_rows(t, clip, frame):
    """(first row, K) of frame ``frame`` of clip ``clip`` of the tables."""
    f = int(t["clips"][clip][0]) + frame
    return int(t["off1"][f]), int(t["count"][f])


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_restatement_agrees_with_the_rounds_on_tie_heavy_tables(seed):
    rng = np.random.default_rng(seed)
    edges = 0
    for _ in range(25):
        args = ref.random_tables(rng)
        F = len(args[0]) - 1
        for gate, max_gap in ((1.0, 0), (1.5, 1), (2.0, 3)):
            a = ref.track(*args, [(0, F)], gate, max_gap)
            b = ref.track(*args, [(0, F)], gate, max_gap, associate=ref.associate_rounds)
            ref.same(a, b, (seed, gate, max_gap))
            edges += int((a["age"] > 1).sum())
    assert edges > 100
    # one frame at a time: cost matrices with ties and NaNs, both associations
    for _ in range(100):
        L, Kk = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        P = rng.integers(0, 3, (L, 3)).astype(f64)
        c = rng.integers(0, 3, (Kk, 3)).astype(f32)
        P[rng.random(L) < 0.1, 0] = np.nan
        c[rng.random(Kk) < 0.1, 1] = np.nan
        ids = np.sort(rng.choice(100, L, replace=False))
        for gate2 in (1.0, 2.0, 5.0):
            assert np.array_equal(ref.associate_greedy(P, ids, c, f64(gate2))[0], ref.associate_rounds(P, ids, c, f64(gate2))[0])


def test_the_tables_agree_between_both_associations(tracked):
    out, again, stats = tracked
    ref.same(out, again, "tables")


# ---- a known world ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    frames, owners = ref.build_world()
    return frames, owners, {which: ref.world_tables(frames, which) for which in ("pred", "gt")}


def _object_tracks(frames, owners, tabs, out):
    """per object, the list over the frames of the track its instance got (None where the object has no instance)."""
    off1, label = tabs[0], tabs[3]
    seen = [[] for _ in range(ref.WORLD_OBJECTS)]
    for f in range(len(frames)):
        a = int(off1[f])
        for k in range(ref.WORLD_OBJECTS):
            labels = set(label[a:int(off1[f + 1])][owners[f] == k].tolist())
            assert len(labels) == 1                                          # an object is one instance or none
            lab = labels.pop()
            seen[k].append(None if lab < 0 else int(out["track"][a + lab]))
    return seen


@pytest.mark.parametrize("which", ["pred", "gt"])
def test_known_world_keeps_its_identities(world, which):
    frames, owners, tabs = world
    tab = tabs[which]
    F = len(frames)
    assert [int(c) for c in tab[2]].count(ref.WORLD_OBJECTS) >= 10 and T_has_rotation(tab[6])
    out = ref.track(*tab, ref.WORLD_CLIPS, ref.GATE, 2)
    ref.same(out, ref.track(*tab, ref.WORLD_CLIPS, ref.GATE, 2, associate=ref.associate_rounds), which)
    seen = _object_tracks(frames, owners, tab, out)
    lost = ref.WORLD_LOST[which]
    for first, end in ref.WORLD_CLIPS:
        ids = []
        for k in range(ref.WORLD_OBJECTS):
            held = [t for t in seen[k][first:end] if t is not None]
            absent = ref.WORLD_ABSENT[which].get(k, ()) if first == 0 else ()
            assert len(held) == end - first - len(absent)
            if k == lost and first == 0:                                     # absent for max_gap + 1 frames: a new id, the clip's next
                before = end - first - len(absent) - sum(1 for t in seen[k][first + max(absent) + 1:end])
                assert set(held[:before]) == {held[0]} and set(held[before:]) == {ref.WORLD_OBJECTS} and held[0] < ref.WORLD_OBJECTS
            else:                                                            # one id for the whole clip, absent for max_gap frames or not
                assert len(set(held)) == 1, (which, k, held)
            ids.append(held[0])
        assert sorted(ids) == list(range(ref.WORLD_OBJECTS))                 # ids restart with every clip
    assert out["ntracks"].tolist() == [ref.WORLD_OBJECTS + 1, ref.WORLD_OBJECTS] and not out["overflow"].any()
    # the tables: every track of the second clip lives through all of it; the matched predictions are close, the gaps are what was made
    a = int(tab[0][ref.WORLD_CLIPS[1][0]])
    assert out["birth"][a:a + 5].tolist() == [10] * 5 and out["last"][a:a + 5].tolist() == [F - 1] * 5 and out["hits"][a:a + 5].tolist() == [8] * 5
    assert out["hits"][a + 5] == 0 and out["birth"][a + 5] == -1
    matched = out["age"] > 1
    err = np.linalg.norm(out["pred"][matched].astype(f64) - tab[4][matched].astype(f64), axis=1)
    assert matched.sum() > 60 and err.max() < (0.1 if which == "pred" else 1e-3), err.max()
    assert sorted(set(out["gap"][matched].tolist())) == [1, 3]
    # at max_gap 0 every absence ends the track
    none = ref.track(*tab, ref.WORLD_CLIPS, ref.GATE, 0)
    assert none["ntracks"].tolist() == [ref.WORLD_OBJECTS + 2, ref.WORLD_OBJECTS] and set(none["gap"][none["age"] > 1].tolist()) == {1}
    # every member point carries its instance's track
    lab = tab[3]
    base = np.repeat(tab[0][:-1], np.diff(tab[0]))
    want = np.where(lab >= 0, out["track"][base + np.maximum(lab, 0)], -1)
    assert np.array_equal(out["point_track"], want)


def T_has_rotation(T):
    return bool((np.abs(T.reshape(-1, 4, 4)[:, 0, 1]) > 0.02).all())


# ---- the special clips ------------------------------------------------------------------------------------------------------------------
def test_the_special_clips_are_what_they_are_for(tables, tracked):
    t, (out, again, stats) = tables, tracked
    tr = lambda clip, frame: out["track"][_clip_rows(t, clip, frame)[0]:sum(_clip_rows(t, clip, frame))].tolist()
    # on the gate: G2 = 4 = gate2 exactly, matched; 2.25 away: a new track
    a, _ = _clip_rows(t, ref.C_GATE, 1)
    assert tr(ref.C_GATE, 0) == [0, 1] and tr(ref.C_GATE, 1) == [0, 2]
    assert ref.cost(t["centroid"][a - 5:a - 4].astype(f64), t["centroid"][a:a + 1])[0, 0] == 4.0 and out["pred"][a].tolist() == [0, 0, 0]
    assert (out["gap"][a], out["age"][a], out["prev_row"][a]) == (1, 2, a - 5) and (out["gap"][a + 1], out["age"][a + 1], out["prev_row"][a + 1]) == (0, 1, -1)
    assert ref.track(t["off1"], t["total"], t["count"], t["label"], t["centroid"], t["disp"], t["T"], t["clips"][:1], 1.9999999, 2)["track"][a] == 2
    # two tracks equally far: the lower id; the other coasts and takes the instance of the next frame
    assert tr(ref.C_TIE_TRACKS, 1) == [0] and tr(ref.C_TIE_TRACKS, 2) == [1]
    a, _ = _clip_rows(t, ref.C_TIE_TRACKS, 2)
    assert out["gap"][a] == 2 and out["age"][a] == 2
    # two instances equally far: the lower j; the other opens a track
    assert tr(ref.C_TIE_INSTANCES, 1) == [0, 1]
    # the crossing: nearest first
    assert tr(ref.C_CROSSING, 1) == [1, 0]
    # a NaN centroid: a new track each time, and its track never matches
    assert tr(ref.C_NAN, 1) == [0, 2, 1] and tr(ref.C_NAN, 2) == [0, 1, 3]
    base = int(t["off1"][t["clips"][ref.C_NAN][0]])
    assert out["ntracks"][ref.C_NAN] == 4 and out["hits"][base:base + 5].tolist() == [3, 3, 1, 1, 0]
    # the ladder: (T_k, I_k) for every k, one pair per round -- a loop cut short cannot pass
    assert tr(ref.C_LADDER, 1) == list(range(ref.LADDER))[::-1] and stats["rounds"] >= ref.LADDER >= 200
    # over capacity: the 1024 coasting tracks die at once; the second set goes on
    assert out["overflow"].tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert tr(ref.C_OVERFLOW, 1) == list(range(1024, 2048)) and tr(ref.C_OVERFLOW, 2) == [1029, 1030, 1031, 1032]
    base = int(t["off1"][t["clips"][ref.C_OVERFLOW][0]])
    first = int(t["clips"][ref.C_OVERFLOW][0])
    assert (out["last"][base:base + 1024] == first).all() and (out["hits"][base:base + 1024] == 1).all() and out["ntracks"][ref.C_OVERFLOW] == 2048
    calm = ref.track(t["off1"], t["total"], t["count"], t["label"], t["centroid"], t["disp"], t["T"], t["clips"], 2.0, 0)
    assert not calm["overflow"].any()                                        # max_gap 0: nothing coasts, nothing overflows
    # the random clip: ties decided, a frame without instances coasted through
    a, k = _clip_rows(t, ref.C_RANDOM, 4)
    assert (out["gap"][a:a + k] == 2).any() and (out["age"][_clip_rows(t, ref.C_RANDOM, 5)[0]:][:20] > 2).any()
    # labels outside 0 .. K-1 give no track
    lab = t["label"]
    a, k = _clip_rows(t, ref.C_RANDOM, 1)
    rows = slice(a, int(t["off1"][int(t["clips"][ref.C_RANDOM][0]) + 2]))
    assert (lab[rows] >= k).any() and (out["point_track"][rows][(lab[rows] < 0) | (lab[rows] >= k)] == -1).all()
    assert (out["point_track"][rows][(lab[rows] >= 0) & (lab[rows] < k)] >= 0).all()


def test_clamps_of_the_entry_point_in_the_restatement(tables):
    """What the GPU test asks of cmf_track_instances, here of the restatement: a clip that reaches behind F, a count above the frame's
    rows, a frame whose rows end behind ``total`` -- and sentinels stay wherever no owned frame is."""
    t = tables
    F = len(t["count"])
    first = int(t["clips"][ref.C_RANDOM][0])
    count = t["count"].copy()
    count[first + 1] = 5000
    total = int(t["off1"][F - 1]) + 2                                        # the last frame ends behind it
    fill = {k: -77 for k in ref.KEYS}
    out = ref.track(t["off1"], total, count, t["label"], t["centroid"], t["disp"], t["T"], [(first, F + 9), (-3, 2)], 2.0, 2,
                    out=ref.outputs(t["total"] + 8, 2, fill))
    n1 = int(t["off1"][first + 2] - t["off1"][first + 1])
    a = int(t["off1"][first + 1])
    assert (out["track"][a:a + n1] >= 0).all()                               # clamped to the frame's rows: every row an instance
    last = slice(int(t["off1"][F - 1]), None)
    assert all((out[k][last] == -77).all() for k in ref.PER_INSTANCE + ref.PER_TRACK)
    between = slice(int(t["off1"][2]), int(t["off1"][first]))
    assert all((out[k][between] == -77).all() for k in ref.PER_INSTANCE + ref.PER_TRACK)
    assert out["ntracks"][1] == 3 and out["ntracks"][0] > 40 and (out["track"][:int(t["off1"][2])] != -77).all()


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def _cpu_split(counts, clips=None):
    rng = np.random.default_rng(0)
    z = lambda *s: np.zeros(s, dtype=f32)
    items = [(rng.standard_normal((n, 3)).astype(f32), z(4, 3) + 1, z(n, 3), z(4, 3), np.eye(4, dtype=f32), z(n, 3), z(n), 0.1, z(n), z(n), z(n, 2))
             for n in counts]
    return D.DeviceSplit.from_items(items, "cpu", clips)


def _cpu_instances(split, which="gt"):
    total, F = split.tab1.shape[0], len(split)
    t = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    tables = (t(total), t(total), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32))
    off = np.concatenate(([0], np.cumsum(split.counts_host[0])))
    return I.FrameInstances(split.off1, torch.arange(F), t(total) - 1, t(total, dt=torch.uint8), t(F), tables, split.interval, which, 2.0, 2, 0.0,
                            off, np.arange(F))


def test_every_refusal_comes_before_any_launch():
    split = _cpu_split([5, 1, 9, 4])
    store = R.SplitResults.empty(split)
    inst, pred = _cpu_instances(split), _cpu_instances(split, "pred")
    with pytest.raises(ValueError, match="cluster"):
        K.track({"label": None}, split)
    with pytest.raises(ValueError, match="store"):
        K.track(pred, split)
    with pytest.raises(ValueError, match="not the one"):
        K.track(inst, _cpu_split([5, 1, 9, 5]))
    with pytest.raises(ValueError, match="not the one"):
        K.track(inst, _cpu_split([5, 1, 13]))
    with pytest.raises(ValueError, match="not the one"):
        K.track(pred, split, R.SplitResults.empty(_cpu_split([5, 1, 9, 3, 1])))
    for gate in (0.0, -1.0, float("nan"), float("inf"), None, "2", True):
        with pytest.raises(ValueError, match="gate"):
            K.track(inst, split, gate=gate)
    for max_gap in (-1, 17, 2.0, None, True, "1"):
        with pytest.raises(ValueError, match="max_gap"):
            K.track(inst, split, max_gap=max_gap)
    for clips, word in (([(0, 3), (2, 4)], "overlaps"), ([(3, 1)], "descends"), ([(-5, 2), (1, 2)], "overlaps")):
        with pytest.raises(ValueError, match=word):
            K.track(inst, _cpu_split([5, 1, 9, 4], clips))
    # everything in order: only the device is wrong -- and that is the LAST refusal
    with pytest.raises(RuntimeError, match="GPU"):
        K.track(inst, split, gate=1.5, max_gap=0)
    with pytest.raises(RuntimeError, match="GPU"):
        K.track(pred, split, store, max_gap=16)
    with pytest.raises(RuntimeError, match="GPU"):
        store.tracks(split, inst=pred, gate=3)
    assert list(inspect.signature(K.track).parameters) == ["inst", "split", "store", "gate", "max_gap"]
    sig = inspect.signature(K.track).parameters
    assert (sig["store"].default, sig["gate"].default, sig["max_gap"].default) == (None, 2.0, 2)
    assert (K.MAX_LIVE, K.MAX_GAP) == (ref.MAX_LIVE, ref.MAX_GAP) == (1024, 16)
    sig = inspect.signature(R.SplitResults.tracks).parameters
    assert list(sig)[:5] == ["self", "split", "inst", "gate", "max_gap"] and (sig["gate"].default, sig["max_gap"].default) == (2.0, 2)


def test_clip_plan_is_the_loop():
    for F, clips in ((7, None), (7, [(0, 3), (3, 7)]), (9, [(5, 8), (1, 3)]), (6, [(-4, 2), (4, 99)]), (5, [(2, 2), (0, 1)]), (4, []), (0, None)):
        got = K.plan_clips(F, clips)
        assert got.dtype == np.int32 and got.shape[1] == 2 and np.array_equal(got, ref.plan_clips(F, clips)), (F, clips, got.tolist())
    assert K.plan_clips(9, [(5, 8), (1, 3)]).tolist() == [[0, 1], [1, 3], [3, 4], [4, 5], [5, 8], [8, 9]]


def test_lengths_and_views_on_the_host(tables, tracked):
    t, (out, _, _) = tables, tracked
    F, total = len(t["count"]), t["total"]
    z3 = torch.zeros(total, 3)
    inst = I.FrameInstances(torch.from_numpy(t["off1"]), torch.arange(F), torch.from_numpy(t["label"]), torch.ones(total, dtype=torch.uint8),
                            torch.from_numpy(t["count"]), (torch.zeros(total, dtype=torch.int32), torch.zeros(total, dtype=torch.int32),
                                                           torch.from_numpy(t["centroid"]), torch.from_numpy(t["disp"]), z3, z3),
                            torch.full((F,), 0.1), "gt", 2.0, 2, 0.0, t["off1"].astype(np.int64), np.arange(F))
    arrays = tuple(torch.from_numpy(out[k]) for k in ref.PER_INSTANCE + ref.PER_TRACK)
    res = K.InstanceTracks(inst, arrays, torch.from_numpy(out["ntracks"]), torch.from_numpy(out["overflow"]), torch.from_numpy(t["clips"]),
                           t["clips"], 2.0, 2)
    want = np.where(out["hits"] > 0, out["last"] - out["birth"] + 1, 0)
    assert res.lengths().dtype == torch.int32 and np.array_equal(res.lengths().numpy(), want) and want.max() == 6 and len(res) == 8
    f = int(t["clips"][ref.C_NAN][0]) + 1
    view = res.frame(f)
    assert view["track"].tolist() == [0, 2, 1] and view["pred"].shape == (3, 3) and view["point_track"].shape == (6,)
    assert (res.gate, res.max_gap, res.which) == (2.0, 2, "gt")


# ---- the reference's own saved frames ---------------------------------------------------------------------------------------------------
def test_saved_frames_go_through_the_restatement():
    g = np.load(os.path.join(GOLDEN, "saved_results_delft_12_w12.npz"))
    off, pc1, pred_f, pred_m, pred_t = g["off"], g["pc1"], g["pred_f"], g["pred_m"], g["pred_t"]
    inst = iref.cluster(off, pc1, pred_f, pred_m == 0, pred_t, list(range(12)), 2.0, 2, 0.0)
    args = (off, int(off[-1]), inst["count"], inst["label"], inst["centroid"], inst["disp"], pred_t.reshape(12, 16).astype(f32), [(0, 12)], 2.0, 2)
    out = ref.track(*args)
    ref.same(out, ref.track(*args, associate=ref.associate_rounds), "saved frames")
    tracks = [out["track"][off[f]:off[f] + inst["count"][f]].tolist() for f in range(12)]
    assert tracks == [[0], [0, 1]] + [[0]] * 10
    assert out["ntracks"].tolist() == [2] and out["hits"][:3].tolist() == [12, 1, 0] and out["overflow"].tolist() == [0]
    assert out["birth"][:2].tolist() == [0, 1] and out["last"][:2].tolist() == [11, 1]
    matched = out["age"] > 1
    err = np.linalg.norm(out["pred"][matched].astype(f64) - inst["centroid"][matched].astype(f64), axis=1)
    assert matched.sum() == 11 and 0.3 < err.max() < 0.62                    # the largest matched prediction error: 0.61 m
