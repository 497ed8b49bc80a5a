"""CPU: what cmflow_amd/score.py means and what its host side does.  The numpy restatement (tests/score_ref.py: the definition of
include/cmflow_hip.h as loops over frames, instances and points) is held against a second, differently written score (Python sets
per instance, an exhaustive search for the matching, a track's history kept as a list) on the worlds and on a few hundred
small tables full of overlaps of exactly one half; no instance ever passes the threshold with two partners; a side scored against
itself is perfect; on the tracking world the counts, the id switches and the fragmentations are those the world's owners imply;
a hand-built clip holds every case once; corrupted tables go through the restatement without an index error and without a write
outside owned rows; every refusal of ``score`` comes before any launch; the header's prototype and the ctypes signature agree;
``summary`` and ``state_errors`` agree with numpy; and the reference's own saved frames go through.  The device code is tied to the
restatement bit for bit in tests/test_gpu_score.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import instances_ref as iref
import objects_ref as oref
import score_ref as ref
import tracks_ref as tref
from cmflow_amd import _lib
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import objects as O
from cmflow_amd import results as R
from cmflow_amd import score as S
from cmflow_amd import tracks as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
f32, f64 = np.float32, np.float64
IOUS = (0.5, 0.6, 0.75)


@pytest.fixture(scope="module")
def tracking():
    return ref.tracking_world()


@pytest.fixture(scope="module")
def small_tables():
    rng = np.random.default_rng(11)
    return [ref.random_tables(rng) for _ in range(300)]


def _score(sides, a, b, iou=0.5, clips=tref.WORLD_CLIPS):
    return ref.score(sides[a]["off1"], sides[a]["total"], clips, iou, ref.side(sides[b]), ref.side(sides[a]))


# ---- the restatement against a second implementation ------------------------------------------------------------------------------------
def test_restatement_is_the_set_based_score_on_the_worlds(tracking):
    frames, owners, sides = tracking
    _, osides = ref.objects_world()
    for name, s, clips in (("tracking", sides, tref.WORLD_CLIPS), ("objects", osides, oref.WORLD_CLIPS)):
        for pred, gt in (("pred", "gt"), ("gt", "gt"), ("gt", "pred")):
            for iou in IOUS:
                out = _score(s, pred, gt, iou, clips)
                res = ref.score_sets(s[pred]["off1"], s[pred]["total"], clips, iou, ref.side(s[gt]), ref.side(s[pred]))
                ref.agree(out, res, clips, (name, pred, gt, iou))


def test_restatement_is_the_set_based_score_on_small_tables(small_tables):
    halves = matched = switches = frags = 0
    for off1, total, gt, pred in small_tables:
        clips = [(0, len(off1) - 1)]
        for iou in IOUS:
            out = ref.score(off1, total, clips, iou, gt, pred)
            ref.agree(out, ref.score_sets(off1, total, clips, iou, gt, pred), clips, iou)
        out = ref.score(off1, total, clips, 0.5, gt, pred)
        matched, switches, frags = matched + int(out["tp"][0]), switches + int(out["ids"][0]), frags + int(out["frags"][0])
        for f in range(len(off1) - 1):
            a, b = int(off1[f]), int(off1[f + 1])
            G, P = ref.frame_sets(gt["label"][a:b], int(gt["count"][f])), ref.frame_sets(pred["label"][a:b], int(pred["count"][f]))
            halves += sum(2 * len(A & B) == len(A | B) for A in G for B in P if A & B)
    assert halves > 500 and matched > 500 and switches > 100 and frags > 20, (halves, matched, switches, frags)   # the tables hold what they are for


def test_no_instance_passes_with_two_partners(small_tables):
    for off1, total, gt, pred in small_tables:
        for f in range(len(off1) - 1):
            a, b = int(off1[f]), int(off1[f + 1])
            G, P = ref.frame_sets(gt["label"][a:b], int(gt["count"][f])), ref.frame_sets(pred["label"][a:b], int(pred["count"][f]))
            for iou in IOUS:
                pairs = ref.passing_pairs(G, P, iou)
                assert len(set(g for g, _ in pairs)) == len(pairs) == len(set(p for _, p in pairs)), (f, iou, pairs)
                # exactly one half never passes, at any of the thresholds
                assert all(2 * len(G[g] & P[p]) > len(G[g] | P[p]) for g, p in pairs)


# ---- known answers ------------------------------------------------------------------------------------------------------------------------
def test_a_side_against_itself_is_perfect(tracking):
    frames, owners, sides = tracking
    for which in ("pred", "gt"):
        for iou in IOUS + (0.999,):
            out = _score(sides, which, which, iou)
            assert not out["fp"].any() and not out["fn"].any() and not out["ids"].any() and not out["frags"].any()
            assert (out["tp"] == out["gt_total"]).all() and out["tp"].sum() == sides[which]["count"].sum() > 80
            assert (out["iou_units"] == out["tp"].astype(np.int64) * ref.IOU_UNIT).all()
            assert np.array_equal(out["match"], out["match_gt"]) and (out["covered"] == out["seen"]).all()
            held = out["match"] >= 0
            assert (out["match"][held] == np.flatnonzero(held)).all() and (out["iou"][held] == 1.0).all() and not out["iou"][~held].any()
            motsa = (out["tp"].astype(f64) - out["fp"] - out["ids"]) / out["gt_total"]
            assert (motsa == 1.0).all()


def _implied(owners, max_gap=2):
    """What the world's owners and WORLD_ABSENT imply at ``max_gap``, without the restatement: an object a source calls moving is one
    instance of that source; it keeps its id through an absence of at most ``max_gap`` frames and gets a new one after a longer
    one.  -> (per frame (tp, fp, fn), per clip (ids, frags))."""
    frame, clip = [], []
    for ci, (first, end) in enumerate(tref.WORLD_CLIPS):
        seen = {w: {k: [(ci == 0 and f - first in tref.WORLD_ABSENT[w].get(k, ())) is False and k in owners[f] for f in range(first, end)]
                    for k in range(tref.WORLD_OBJECTS)} for w in ("pred", "gt")}
        ident = {}
        for w in ("pred", "gt"):                                            # the id of object k at frame g: (k, epoch)
            for k in range(tref.WORLD_OBJECTS):
                epoch, missed, ids = 0, 0, []
                for g, there in enumerate(seen[w][k]):
                    if there:
                        epoch, missed = epoch + (missed > max_gap), 0
                    else:
                        missed += 1
                    ids.append((k, epoch) if there else None)
                ident[w, k] = ids
        for g in range(end - first):
            both = sum(seen["pred"][k][g] and seen["gt"][k][g] for k in range(tref.WORLD_OBJECTS))
            frame.append((both, sum(seen["pred"][k][g] for k in range(tref.WORLD_OBJECTS)) - both, sum(seen["gt"][k][g] for k in range(tref.WORLD_OBJECTS)) - both))
        ids = frags = 0
        for k in range(tref.WORLD_OBJECTS):
            history = {}                                                    # gt id -> [partner id or None], in frame order
            for g in range(end - first):
                t = ident["gt", k][g]
                if t is None:
                    continue
                partner = ident["pred", k][g]
                earlier = [u for u in history.get(t, []) if u is not None]
                if partner is not None and earlier:
                    ids += earlier[-1] != partner
                    frags += history[t][-1] is None
                history.setdefault(t, []).append(partner)
        clip.append((ids, frags))
    return frame, clip


def test_tracking_world_costs_what_its_owners_imply(tracking):
    frames, owners, sides = tracking
    out = _score(sides, "pred", "gt")
    frame, clip = _implied(owners)
    assert [tuple(int(out[k][f]) for k in ref.PER_FRAME) for f in range(len(frames))] == frame
    assert [(int(out["ids"][c]), int(out["frags"][c])) for c in range(2)] == clip == [(1, 2), (0, 0)]
    # the object of WORLD_LOST['pred'] comes back under a new id: exactly one switch, at its first frame back; the absences of the
    # pred side are the two fragmentations; the gt side's absences are false positives and cost no identity
    assert out["fp"].tolist() == [5, 0] and out["fn"].tolist() == [5, 0] and out["tp"].tolist() == [40, 40]
    back = max(tref.WORLD_ABSENT["pred"][tref.WORLD_LOST["pred"]]) + 1
    a, b = int(sides["gt"]["off1"][back]), int(sides["gt"]["off1"][back + 1])
    assert np.flatnonzero(out["switch"]).tolist() == [r for r in range(a, b) if out["switch"][r]] and out["switch"][a:b].sum() == 1
    held = out["match"] >= 0
    assert (out["iou"][held] == 1.0).all()                                  # both sources cluster the same points of an object
    # a new gt id (the object of WORLD_LOST['gt']) is a new track, not a switch: 5 objects + 1 in the first clip, 5 in the second
    assert int((out["seen"] > 0).sum()) == 11


def test_hand_built_clip():
    off1, total, gt, pred, want = ref.hand_clip()
    F = len(off1) - 1
    assert F == 9 and max(np.diff(off1)) < 10 and 0 in np.diff(off1) and 1 in np.diff(off1)
    out = ref.score(off1, total, [(0, F)], 0.5, gt, pred)
    assert [tuple(int(out[k][f]) for k in ref.PER_FRAME) for f in range(F)] == want["frame"]
    assert np.flatnonzero(out["switch"]).tolist() == want["switch"] and np.flatnonzero(out["frag"]).tolist() == want["frag"]
    assert {k: int(out[k][0]) for k in want["clip"]} == want["clip"] and int(out["iou_units"][0]) == want["units"]
    assert {u: int(out["seen"][u]) for u in want["seen"]} == want["seen"] and int(out["seen"].sum()) == sum(want["seen"].values())
    assert {u: int(out["covered"][u]) for u in want["covered"]} == want["covered"] and int(out["covered"].sum()) == sum(want["covered"].values())
    assert out["last_partner"][:4].tolist() == [5, 1, -1, 1]
    # the overlap of exactly one half is unmatched, the one of 2/3 matched at 0.5 and not at 0.7
    a = int(off1[1])
    assert out["match"][a:a + 2].tolist() == [a, -1] and out["match_gt"][a:a + 3].tolist() == [a, -1, -1]
    assert out["iou"][a] == f64(2) / f64(3) and out["iou"][a + 1] == 0.0
    other = ref.score(off1, total, [(0, F)], 0.7, gt, pred)
    assert tuple(int(other[k][1]) for k in ref.PER_FRAME) == want["iou_07"] and other["match"][a] == -1
    # the instance without identity is matched and counted, and no track's row knows of it
    r = want["no_identity"]
    assert out["match_gt"][r] == r and out["frame_tp"][5] == 1 and gt["track"][r] == -7
    ref.agree(out, ref.score_sets(off1, total, [(0, F)], 0.5, gt, pred), [(0, F)], "hand")
    ref.agree(other, ref.score_sets(off1, total, [(0, F)], 0.7, gt, pred), [(0, F)], "hand 0.7")


def test_edge_tables_are_what_they_are_for():
    off1, total, clips, gt, pred = ref.edge_tables()
    assert np.diff(off1).tolist() == [0, 1, 63, 64, 65, 1024, 1024, 5]
    out = ref.score(off1, total, clips, 0.5, gt, pred)
    assert (gt["count"][5], pred["count"][5]) == (1, 512) and tuple(out[k][5] for k in ref.PER_FRAME) == (0, 512, 1)
    assert (gt["count"][6], pred["count"][6]) == (341, 341) and tuple(out[k][6] for k in ref.PER_FRAME) == (0, 341, 341)   # one half everywhere
    assert tuple(out[k][1] for k in ref.PER_FRAME) == (1, 0, 0) and out["frame_tp"][2] == 21 and out["frame_tp"][3] == 1 and out["frame_tp"][4] == 22
    assert out["tp"].tolist() == [45, 0, 2] and out["gt_total"].tolist() == [1 + 21 + 22 + 22 + 1 + 341, 0, 2]


# ---- what the GPU test asks of the entry point, here of the restatement ------------------------------------------------------------------
def test_corrupted_tables_go_through_the_restatement(tracking):
    frames, owners, sides = tracking
    off1, total, clips, gt, pred = ref.corrupt_tables(sides)
    F, rows = len(off1) - 1, sides["gt"]["total"] + 8
    fill = {k: -77 for k in ref.KEYS}
    out = ref.score(off1, total, clips, 0.5, gt, pred, out=ref.outputs(rows, F, len(clips), fill))
    owned = ref.owned_rows(off1, total, clips, rows)
    assert 0 < owned.sum() < total and not owned[total:].any()
    for k in ref.PER_ROW:
        assert (out[k][~owned] == -77).all() and (out[k][owned] != -77).all(), k
    for k in ref.PER_FRAME + ref.PER_CLIP:
        assert (out[k] != -77).all(), k                                     # the clips cover every frame
    a, b = int(off1[5]), int(off1[6])
    assert out["frame_fp"][5] + out["frame_tp"][5] == b - a                 # count 5000: clamped to the frame's rows
    assert out["frame_tp"][6] == out["frame_fp"][6] == out["frame_fn"][6] == 0          # count -4: no instances
    for f in (7, 8, 12, 13, 15, 16, 17):
        assert tuple(out[k][f] for k in ref.PER_FRAME) == (0, 0, 0), f      # frames that own no rows
    assert owned[int(off1[9]):int(off1[10])].all() and not owned[int(off1[7]):int(off1[9])].any()      # the gap behind the solid rows
    assert out["tp"].sum() > 20 and (out["seen"][owned] >= 0).all() and out["seen"].max() <= 10


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def _cpu_split(counts, clips=None):
    rng = np.random.default_rng(0)
    z = lambda *s: np.zeros(s, dtype=f32)
    items = [(rng.standard_normal((n, 3)).astype(f32), z(4, 3) + 1, z(n, 3), z(4, 3), np.eye(4, dtype=f32), z(n, 3), z(n), 0.1, z(n), z(n), z(n, 2))
             for n in counts]
    return D.DeviceSplit.from_items(items, "cpu", clips)


def _cpu_objects(split, which="gt"):
    total, F = split.tab1.shape[0], len(split)
    t = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    fl = torch.float32
    off = np.concatenate(([0], np.cumsum(split.counts_host[0])))
    inst = I.FrameInstances(split.off1, torch.arange(F), t(total) - 1, t(total, dt=torch.uint8), t(F),
                            (t(total), t(total), t(total, 3, dt=fl), t(total, 3, dt=fl), t(total, 3, dt=fl), t(total, 3, dt=fl)), split.interval, which,
                            2.0, 2, 0.0, off, np.arange(F))
    arrays = (t(total) - 1, t(total) - 1, t(total), t(total), t(total, 3, dt=fl), t(total) - 1, t(total) - 1, t(total) - 1, t(total))
    clips = K.plan_clips(F, split.clips)
    trk = K.InstanceTracks(inst, arrays, t(len(clips)), t(len(clips)), torch.from_numpy(clips), clips, 2.0, 2)
    f8 = torch.float64
    states = (t(total) - 1, t(total) - 1, t(total, 6, dt=f8), t(total, 3, dt=f8), t(total, 6, dt=f8), t(total, 3, dt=f8), t(total, 3, dt=fl), t(total, 3, dt=fl),
              t(total, 2, dt=fl), t(total) - 1, t(total, 3, dt=fl), t(total, 3, dt=fl))
    return O.TrackObjects(trk, states, t(F, 16, dt=f8), t(F, dt=torch.int64), split.interval, *oref.PARAMS)


def test_every_refusal_comes_before_any_launch():
    split = _cpu_split([5, 1, 9, 4])
    store = R.SplitResults.empty(split)
    pred, gt = _cpu_objects(split, "pred"), _cpu_objects(split)
    for bad in (pred.trk, pred.inst, None, "pred"):
        with pytest.raises(ValueError, match="estimate"):
            S.score(bad, gt, split)
        with pytest.raises(ValueError, match="estimate"):
            S.score(pred, bad, split)
    with pytest.raises(ValueError, match="not the one"):
        S.score(pred, gt, _cpu_split([5, 1, 9, 5]))
    with pytest.raises(ValueError, match="not the one"):
        S.score(pred, gt, _cpu_split([5, 1, 13]))
    with pytest.raises(ValueError, match="offsets"):
        S.score(pred, _cpu_objects(_cpu_split([5, 2, 8, 4])), split)
    with pytest.raises(ValueError, match="clips"):
        S.score(pred, _cpu_objects(_cpu_split([5, 1, 9, 4], [(0, 2), (2, 4)])), split)
    for v in (0.49999, 0.0, 1.0, 1.5, -0.5, float("nan"), float("inf"), None, "0.5", True):
        with pytest.raises(ValueError, match="iou"):
            S.score(pred, gt, split, iou=v)
        with pytest.raises(ValueError, match="iou"):
            store.score_tracks(split, iou=v, pred=pred, gt=gt)
        with pytest.raises(ValueError, match="iou"):
            store.score_tracks(split, iou=v, which="gt")                    # the threshold is refused before the chains are formed
    with pytest.raises(ValueError, match="belong to the object states"):
        store.score_tracks(split, pred=pred, gt=gt, gate=3.0)
    with pytest.raises(ValueError, match="which"):
        store.score_tracks(split, which="gt")
    # everything in order: only the device is wrong -- and that is the LAST refusal
    for iou in (0.5, 0.75, np.float32(0.5), 0.9999999):
        with pytest.raises(RuntimeError, match="GPU"):
            S.score(pred, gt, split, iou=iou)
    with pytest.raises(RuntimeError, match="GPU"):
        store.score_tracks(split, pred=pred, gt=gt)
    with pytest.raises(ValueError, match="no results"):
        store.score_tracks(split, gt=gt, gate=1.5)                          # forms the pred side first: the store is not filled
    store.done.fill_(1)
    with pytest.raises(RuntimeError, match="GPU"):
        store.score_tracks(split, gt=gt, gate=1.5, min_disp=0.1)                   # forms the pred side first: its refusal, on the same ground
    sig = inspect.signature(S.score).parameters
    assert list(sig) == ["pred", "gt", "split", "iou"] and sig["iou"].default == 0.5
    assert list(inspect.signature(R.SplitResults.score_tracks).parameters)[:5] == ["self", "split", "iou", "pred", "gt"]
    assert S.KEYS == ref.KEYS and S.IOU_UNIT == ref.IOU_UNIT == I.IOU_UNIT


def test_prototype_and_ctypes_signature_agree():
    text = open(os.path.join(REPO, "include", "cmflow_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+cmf_score_tracks\s*\(([^)]*)\)\s*;", text)
    assert m
    kinds = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double}
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else kinds[arg.rsplit(" ", 1)[0]])
    assert want == _lib.SIGNATURES["cmf_score_tracks"] and len(want) == 32
    # the outputs follow the inputs in the order ``score`` passes them (``switch`` is a keyword of C: the header says ``switches``)
    names = [" ".join(a.split()).rsplit(" ", 1)[1].lstrip("*") for a in m.group(1).split(",")]
    assert tuple("switch" if n == "switches" else n for n in names[13:31]) == ref.KEYS and names[31] == "stream"
    src = open(os.path.join(REPO, "cmflow_amd", "csrc", "Makefile")).read()
    assert re.search(r"score\.o: FLAGS \+= -ffp-contract=off -Rpass-analysis=kernel-resource-usage", src)


# ---- the derived numbers ------------------------------------------------------------------------------------------------------------------
def _cpu_side(t, which, clips):
    """A TrackObjects on the CPU from a dict of tables as objects_ref.world_tables returns it, the states by the restatement."""
    F, total = len(t["count"]), t["total"]
    z3 = torch.zeros(total, 3)
    interval = torch.full((F,), 0.1)
    off = torch.from_numpy(t["off1"].astype(np.int32))
    inst = I.FrameInstances(off, torch.arange(F), torch.from_numpy(t["label"]), torch.ones(total, dtype=torch.uint8), torch.from_numpy(t["count"]),
                            (torch.zeros(total, dtype=torch.int32), torch.zeros(total, dtype=torch.int32), torch.from_numpy(t["centroid"]),
                             torch.from_numpy(t["disp"]), z3, z3), interval, which, 2.0, 2, 0.0, t["off1"].astype(np.int64), np.arange(F))
    tr = tref.track(t["off1"], total, t["count"], t["label"], t["centroid"], t["disp"], t["T"].reshape(-1, 16), clips, oref.GATE, 2)
    carr = np.asarray(clips, dtype=np.int32)
    trk = K.InstanceTracks(inst, tuple(torch.from_numpy(tr[k]) for k in tref.PER_INSTANCE + tref.PER_TRACK), torch.from_numpy(tr["ntracks"]),
                           torch.from_numpy(tr["overflow"]), torch.from_numpy(carr), carr, oref.GATE, 2)
    out = oref.run(t)
    base = np.zeros(F, np.int64)
    for a, b in clips:
        base[a:b] = t["off1"][a]
    return O.TrackObjects(trk, tuple(torch.from_numpy(out[k]) for k in oref.KEYS), torch.from_numpy(t["poses"]), torch.from_numpy(base), interval, *oref.PARAMS)


@pytest.fixture(scope="module")
def cpu_score():
    """The objects world scored on the CPU: the TrackScore built from the restatement's outputs."""
    frames, sides = ref.objects_world(flow_noise=0.05)
    clips = oref.WORLD_CLIPS
    pred, gt = _cpu_side(sides["pred"], "pred", clips), _cpu_side(sides["gt"], "gt", clips)
    total = sides["gt"]["total"]
    out = ref.score(sides["gt"]["off1"], total, clips, 0.5, ref.side(sides["gt"]), ref.side(sides["pred"]))
    rows = torch.from_numpy(S.clip_of_rows(sides["gt"]["off1"], np.asarray(clips), total))
    return S.TrackScore(pred, gt, 0.5, tuple(torch.from_numpy(out[k]) for k in ref.KEYS), rows), out, sides


def test_summary_and_state_errors_agree_with_numpy(cpu_score):
    score, out, sides = cpu_score
    C = len(score)
    clip_of_row = score.clip_of_row.numpy()
    got, want = score.summary(), ref.summary_numpy(out, clip_of_row)
    for k, v in want.items():
        if k != "all":
            assert got[k].dtype == torch.float64 and np.array_equal(got[k].numpy(), v, equal_nan=True), k     # ratios of whole numbers: exact
    for k, v in want["all"].items():
        assert np.array_equal(got["all"][k].numpy(), v, equal_nan=True), k
    assert want["tracks"].tolist() == [6, 5] and 0 < want["MOTSA"][0] <= 1 and want["recall"][0] <= 1
    pred, gt = ({k: getattr(s, k).numpy() for k in oref.KEYS} for s in (score.pred, score.gt))
    errs = score.state_errors()
    got = {k: {m: errs[k][m].numpy() for m in ("mean", "max")} for k in S.STATE_KEYS + ("heading",)}
    want = ref.errors_numpy(out, pred, gt, clip_of_row, C)
    ref.check_errors(got, want, C)
    assert errs["count"].tolist() == [len(v) for v in want["pos"]] == out["tp"].tolist()
    assert errs["heading_count"].tolist() == [len(v) for v in want["heading"]] and 0 < errs["heading_count"].sum() < errs["count"].sum()
    assert 0 < got["pos"]["max"].max() < 0.5 and got["vel"]["mean"].min() > 0          # the flow noise shows, and stays small
    # a clip without a match: NaN, and zero denominators are NaN
    empty = S.TrackScore(score.pred, score.gt, 0.5, tuple(torch.zeros_like(getattr(score, k)) - int(k in ("match", "match_gt", "last_partner")) for k in ref.KEYS),
                         score.clip_of_row)
    assert all(torch.isnan(empty.summary()[k]).all() for k in ("MOTSA", "sMOTSA", "MOTSP", "recall", "precision"))
    assert torch.isnan(empty.state_errors()["pos"]["mean"]).all() and torch.isnan(empty.state_errors()["heading"]["max"]).all()


def test_views_and_worst_on_the_host(cpu_score):
    score, out, sides = cpu_score
    off = sides["gt"]["off1"]
    for f in (0, 4, 12):
        a, Kp, Kg = int(off[f]), int(sides["pred"]["count"][f]), int(sides["gt"]["count"][f])
        view = score.frame(f)
        assert view["match"].shape == (Kp,) and view["match_gt"].shape == (Kg,) and torch.equal(view["iou"], score.iou[a:a + Kp])
        assert torch.equal(view["frag"], score.frag[a:a + Kg]) and (int(view["tp"]), int(view["fp"]), int(view["fn"])) == tuple(int(out[k][f]) for k in ref.PER_FRAME)
    missed = out["frame_fp"].astype(np.int64) + out["frame_fn"]
    order = sorted(range(len(missed)), key=lambda f: (-missed[f], f))
    for k in (0, 1, 5, len(missed), len(missed) + 7):
        frames, values = score.worst(k)
        assert frames.tolist() == order[:k] and values.tolist() == [int(missed[f]) for f in order[:k]]
    with pytest.raises(ValueError, match="k"):
        score.worst(-1)


# ---- the reference's own saved frames -----------------------------------------------------------------------------------------------------
def test_saved_frames_go_through_the_restatement():
    """The reference's saved results hold its predictions only -- no labels -- so the fixture has no ``'gt'`` side of its own.  The two
    sides scored here are the chain on the saved predictions at two settings of ``eps`` (2.0, the default, as the ``pred`` side; 1.0
    in the place of the labels' side): what ``score`` allows, and what the fixture can honestly give."""
    g = np.load(os.path.join(GOLDEN, "saved_results_delft_12_w12.npz"))
    off, pc1, pred_f, pred_m, pred_t = g["off"], g["pc1"], g["pred_f"], g["pred_m"], g["pred_t"]
    assert int(g["first_frame"]) == 727 and off.shape == (13,)
    T = pred_t.reshape(12, 16).astype(f32)
    total, clips = int(off[-1]), [(0, 12)]
    sides = {}
    for name, eps in (("pred", 2.0), ("gt", 1.0)):
        inst = iref.cluster(off, pc1, pred_f, pred_m == 0, pred_t, list(range(12)), eps, 2, 0.0)
        trk = tref.track(off, total, inst["count"], inst["label"], inst["centroid"], inst["disp"], T, clips, 2.0, 2)
        sides[name] = {"count": inst["count"], "label": inst["label"], "track": trk["track"], "prev_row": trk["prev_row"]}
    assert sides["pred"]["count"].sum() == 13 and sides["gt"]["count"].sum() > 13
    for iou in IOUS:
        out = ref.score(off, total, clips, iou, sides["gt"], sides["pred"])
        ref.agree(out, ref.score_sets(off, total, clips, iou, sides["gt"], sides["pred"]), clips, iou)
        assert np.isfinite(out["iou"]).all() and ((out["iou"] == 0) | (out["iou"] > iou)).all() and (out["iou"] <= 1).all()
        assert out["tp"][0] + out["fp"][0] == 13 and out["tp"][0] + out["fn"][0] == out["gt_total"][0] == sides["gt"]["count"].sum()
    out = ref.score(off, total, clips, 0.5, sides["pred"], sides["pred"])
    assert out["tp"][0] == 13 and not out["fp"][0] and not out["ids"][0] and out["iou_units"][0] == 13 * ref.IOU_UNIT
