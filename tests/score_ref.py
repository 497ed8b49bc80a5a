"""numpy restatement of cmflow_amd/csrc/score.hip (tests/test_score_host.py, tests/test_gpu_score.py): the definition of
include/cmflow_hip.h written plainly as loops over frames, instances and points -- the labels that count, the sizes and the overlaps
counted from them, the one float64 division and its strict compare, the identity walk over a gt track's matches; a second,
differently written score (Python sets per instance, an exhaustive search for the matching, a track's history kept as a list) that
must agree with it; the hand-built clip that holds every case once; the frames at the kernel's edges; and the corrupted tables the
entry point is called with.  The worlds are those of tracks_ref / objects_ref.  Nothing here imports cmflow_amd."""
import numpy as np

import objects_ref as oref
import tracks_ref as tref

f64 = np.float64
MAX_POINTS = 1024                                           # CMF_INST_MAX_POINTS: a frame of more rows has no instances
MAX_LIVE = tref.MAX_LIVE
IOU_UNIT = 2 ** 30
PER_PRED = ("match", "iou")
PER_GT = ("match_gt", "switch", "frag")
PER_FRAME = ("frame_tp", "frame_fp", "frame_fn")
PER_TRACK = ("seen", "covered", "last_partner")
PER_CLIP = ("tp", "fp", "fn", "ids", "frags", "gt_total", "iou_units")
KEYS = ("match", "match_gt", "iou", "switch", "frag") + PER_FRAME + PER_TRACK + PER_CLIP      # the entry point's order
PER_ROW = PER_PRED + PER_GT + PER_TRACK
FILL = {"match": -1, "match_gt": -1, "last_partner": -1}    # what ``score`` fills its outputs with; every other array: 0
STATE_KEYS = ("pos", "vel", "box_size")                    # what ``state_errors`` compares, and the heading
GT_TABLES = ("count", "label", "track", "prev_row")         # what the call reads of the gt side; of the pred side: all but prev_row


def dtype_of(k):
    return f64 if k == "iou" else np.int64 if k == "iou_units" else np.int32


def outputs(rows, frames, nclips, fill=FILL):
    """The outputs of cmf_score_tracks -- ``rows`` rows, ``frames`` frames, ``nclips`` clips -- filled: -> dict."""
    size = lambda k: rows if k in PER_ROW else frames if k in PER_FRAME else nclips
    return {k: np.full(size(k), fill.get(k, 0), dtype_of(k)) for k in KEYS}


def _counted(label, K):
    """A frame's labels as the definition counts them: 0 .. K-1, anything else -1."""
    lab = np.asarray(label).astype(np.int64)
    return np.where((lab >= 0) & (lab < K), lab, -1)


def score(off1, total, clips, iou, gt, pred, out=None):
    """cmf_score_tracks -> dict of the outputs (``out``: arrays to write into, e.g. sentinel-filled ones; default: ``outputs`` with the
    fills of cmflow_amd.score.score).  ``gt``: dict of count, label, track, prev_row; ``pred``: of count, label, track."""
    off1 = np.asarray(off1, dtype=np.int64)
    F, total, iou = len(off1) - 1, int(total), f64(iou)
    clips = np.asarray(clips, dtype=np.int64).reshape(-1, 2)
    out = outputs(total, F, len(clips)) if out is None else out
    for ci, (first, end) in enumerate(clips):
        first = min(max(int(first), 0), F)
        end = min(max(int(end), first), F)
        base = int(off1[first])
        clip_ok = 0 <= base <= total
        top = solid = base                                  # solid: the end of the clip's owned rows that follow base without a gap
        sums = dict.fromkeys(PER_CLIP, 0)
        for f in range(first, end):
            s, e = int(off1[f]), int(off1[f + 1])
            owns = clip_ok and s >= top and e >= s and e <= total
            n = e - s if owns else 0
            if owns:
                top = e
                if s == solid:
                    solid = e
            row0 = s if owns else 0
            small = n <= MAX_POINTS
            Kg = min(max(int(gt["count"][f]), 0), n, MAX_LIVE) if owns and small else 0
            Kp = min(max(int(pred["count"][f]), 0), n, MAX_LIVE) if owns and small else 0
            # ---- the fills of the frame's rows: the per-track tables start empty, the rows behind K hold no instance
            for k in PER_TRACK:
                out[k][row0:row0 + n] = FILL.get(k, 0)
            out["match"][row0 + Kp:row0 + n], out["iou"][row0 + Kp:row0 + n] = -1, 0.0
            for k in PER_GT:
                out[k][row0 + Kg:row0 + n] = FILL.get(k, 0)
            # ---- labels, sizes, overlaps: counted point by point
            g, p = _counted(gt["label"][row0:row0 + n], Kg), _counted(pred["label"][row0:row0 + n], Kp)
            size_g, size_p, c = np.zeros(Kg, np.int64), np.zeros(Kp, np.int64), np.zeros((Kg, Kp), np.int64)
            for i in range(n):
                if g[i] >= 0:
                    size_g[g[i]] += 1
                if p[i] >= 0:
                    size_p[p[i]] += 1
                if g[i] >= 0 and p[i] >= 0:
                    c[g[i], p[i]] += 1
            # ---- the matching: one division, one strict compare
            mg, mp, q_of = np.full(Kg, -1, np.int64), np.full(Kp, -1, np.int64), np.zeros(Kp, f64)
            for a in range(Kg):
                for b in range(Kp):
                    if c[a, b] > 0:
                        q = f64(c[a, b]) / f64(size_g[a] + size_p[b] - c[a, b])
                        if q > iou:
                            assert mg[a] < 0 and mp[b] < 0  # at most one partner: the argument of the header
                            mg[a], mp[b], q_of[b] = b, a, q
            for b in range(Kp):
                out["match"][row0 + b] = row0 + mp[b] if mp[b] >= 0 else -1
                out["iou"][row0 + b] = q_of[b]
                if mp[b] >= 0:
                    sums["iou_units"] += int(np.floor(q_of[b] * f64(IOU_UNIT)))
            tp = int((mg >= 0).sum())
            out["frame_tp"][f], out["frame_fp"][f], out["frame_fn"][f] = tp, Kp - tp, Kg - tp
            sums["tp"], sums["fp"], sums["fn"], sums["gt_total"] = sums["tp"] + tp, sums["fp"] + Kp - tp, sums["fn"] + Kg - tp, sums["gt_total"] + Kg
            # ---- identity: the gt instances in ascending number; a track counts once per frame, for its lowest instance
            tracks_here = []
            for a in range(Kg):
                row = row0 + a
                t = int(gt["track"][row])
                t = t if t >= 0 and base + t < solid else -1
                ident = t >= 0 and t not in tracks_here
                tracks_here.append(t)
                out["match_gt"][row] = row0 + mg[a] if mg[a] >= 0 else -1
                sw = fr = 0
                if ident:
                    tr = base + t
                    out["seen"][tr] += 1
                    if mg[a] >= 0:
                        u = int(pred["track"][row0 + mg[a]])
                        u = u if u >= 0 and base + u < solid else -1
                        if out["covered"][tr] > 0:           # m' exists
                            sw = int(out["last_partner"][tr] != u)
                            before = int(gt["prev_row"][row])
                            fr = int(not (base <= before < row0 and before < solid and out["match_gt"][before] >= 0))
                        out["covered"][tr] += 1
                        out["last_partner"][tr] = u
                out["switch"][row], out["frag"][row] = sw, fr
                sums["ids"], sums["frags"] = sums["ids"] + sw, sums["frags"] + fr
        for k in PER_CLIP:
            out[k][ci] = sums[k]
    return out


def owned_rows(off1, total, clips, rows):
    """(rows) bool: the rows of the frames that own theirs, by the walk of ``score``."""
    off1 = np.asarray(off1, dtype=np.int64)
    F, owned = len(off1) - 1, np.zeros(rows, bool)
    for first, end in np.asarray(clips, dtype=np.int64).reshape(-1, 2):
        first = min(max(int(first), 0), F)
        end = min(max(int(end), first), F)
        top = int(off1[first])
        if not 0 <= top <= total:
            continue
        for f in range(first, end):
            s, e = int(off1[f]), int(off1[f + 1])
            if top <= s <= e <= total:
                owned[s:e], top = True, e
    return owned


def same(got, want, what=""):
    """Exact: integers equal, ``iou`` as uint64."""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype == dtype_of(k), (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if k == "iou":
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist(), np.asarray(got[k])[tuple(bad[0])], np.asarray(want[k])[tuple(bad[0])])


# ---- the score a second time: sets, an exhaustive search, histories -------------------------------------------------------------------------
def frame_sets(label, K):
    """The instances of a frame as sets of point indices, from the labels that count."""
    return [set(np.flatnonzero(np.asarray(label) == k).tolist()) for k in range(K)]


def passing_pairs(G, P, iou):
    """Every (g, p) whose sets overlap by more than ``iou``: Python's own true division of the two whole numbers (correctly rounded,
    as the definition's float64 division is -- 3 of 5 is NOT above a threshold of 0.6, whose float64 lies a hair below the rational)
    and a strict compare.  An exhaustive search, no assumption that a partner is unique."""
    iou = float(iou)
    return [(a, b) for a, A in enumerate(G) for b, B in enumerate(P) if A & B and len(A & B) / len(A | B) > iou]


def score_sets(off1, total, clips, iou, gt, pred):
    """The definition over well-formed tables (offsets that ascend inside ``total``, frames of at most 1024 points), written with sets:
    per frame the pairs that pass, searched exhaustively, and per gt track its history [(row, partner's track or None)] -> dict of the
    per-frame and per-clip counts, ``match`` and the rows with a switch or a fragmentation."""
    off1 = np.asarray(off1, dtype=np.int64)
    F = len(off1) - 1
    res = {"match": np.full(total, -1, np.int64), "frame": np.zeros((F, 3), np.int64), "clip": [], "switch": set(), "frag": set(), "units": [],
           "seen": {}, "covered": {}}
    for ci, (first, end) in enumerate(clips):
        base = int(off1[first])
        history = {}
        tp = fp = fn = units = 0
        for f in range(first, end):
            a, b = int(off1[f]), int(off1[f + 1])
            Kg, Kp = min(max(int(gt["count"][f]), 0), b - a), min(max(int(pred["count"][f]), 0), b - a)
            rows = b - base                                                 # a track's id lies below the clip's rows so far
            G, P = frame_sets(gt["label"][a:b], Kg), frame_sets(pred["label"][a:b], Kp)
            pairs = passing_pairs(G, P, iou)
            assert len(set(x for x, _ in pairs)) == len(pairs) == len(set(y for _, y in pairs))
            partner = dict(pairs)
            for x, y in pairs:
                res["match"][a + y] = a + x
                units += int(np.floor(f64(len(G[x] & P[y])) / f64(len(G[x] | P[y])) * f64(IOU_UNIT)))
            res["frame"][f] = len(pairs), Kp - len(pairs), Kg - len(pairs)
            tp, fp, fn = tp + len(pairs), fp + Kp - len(pairs), fn + Kg - len(pairs)
            for x in range(Kg):
                t = int(gt["track"][a + x])
                if not 0 <= t < rows or any(int(gt["track"][a + y]) == t for y in range(x)):
                    continue
                u = None
                if x in partner:
                    u = int(pred["track"][a + partner[x]])
                    u = u if 0 <= u < rows else -1
                    earlier = [e for e in history.get(t, []) if e[1] is not None]
                    if earlier:
                        if earlier[-1][1] != u:
                            res["switch"].add(a + x)
                        if history[t][-1][1] is None or history[t][-1][0] != int(gt["prev_row"][a + x]):
                            res["frag"].add(a + x)
                history.setdefault(t, []).append((a + x, u))
        for t, h in history.items():
            res["seen"][base + t], res["covered"][base + t] = len(h), sum(e[1] is not None for e in h)
        res["clip"].append((tp, fp, fn))
        res["units"].append(units)
    return res


def agree(out, res, clips, what=""):
    """The restatement's outputs against ``score_sets``'s."""
    assert np.array_equal(out["match"], res["match"]), what
    assert np.array_equal(np.stack([out[k] for k in PER_FRAME], axis=1), res["frame"]), what
    assert [tuple(int(out[k][c]) for k in ("tp", "fp", "fn")) for c in range(len(clips))] == res["clip"], what
    assert out["iou_units"].tolist() == res["units"], what
    assert set(np.flatnonzero(out["switch"]).tolist()) == res["switch"] and set(np.flatnonzero(out["frag"]).tolist()) == res["frag"], what
    assert {int(r): int(out["seen"][r]) for r in np.flatnonzero(out["seen"])} == res["seen"], what
    assert {r: int(out["covered"][r]) for r in res["covered"]} == res["covered"] and int(out["covered"].sum()) == sum(res["covered"].values()), what
    assert out["ids"].sum() == len(res["switch"]) and out["frags"].sum() == len(res["frag"]), what


# ---- the derived numbers, in numpy ---------------------------------------------------------------------------------------------------------
def summary_numpy(out, clip_of_row):
    """``TrackScore.summary`` in numpy -> dict of (C) float64 arrays and "all"."""
    C = len(out["tp"])
    c = {k: out[k].astype(f64) for k in ("tp", "fp", "fn", "ids", "frags", "gt_total")}
    c["iou_sum"] = out["iou_units"].astype(f64) / f64(IOU_UNIT)
    seen, cov = out["seen"].astype(np.int64), out["covered"].astype(np.int64)
    for name, flag in (("tracks", seen > 0), ("mostly_tracked", (seen > 0) & (5 * cov >= 4 * seen)), ("mostly_lost", (seen > 0) & (5 * cov < seen))):
        c[name] = np.bincount(clip_of_row[flag], minlength=C).astype(f64)

    def derive(c):
        with np.errstate(all="ignore"):
            return dict(c, MOTSA=(c["tp"] - c["fp"] - c["ids"]) / c["gt_total"], sMOTSA=(c["iou_sum"] - c["fp"] - c["ids"]) / c["gt_total"],
                        MOTSP=c["iou_sum"] / c["tp"], recall=c["tp"] / (c["tp"] + c["fn"]), precision=c["tp"] / (c["tp"] + c["fp"]))

    res = derive(c)
    res["all"] = derive({k: np.asarray(v.sum()) for k, v in c.items()})
    return res


def errors_numpy(out, pred, gt, clip_of_row, C):
    """``TrackScore.state_errors`` in numpy -> {key: (count (C), values per clip: list of arrays)}."""
    held = np.flatnonzero(out["match"] >= 0)
    g = out["match"][held]
    res = {}
    for k in STATE_KEYS:
        d = pred[k][held].astype(f64) - gt[k][g].astype(f64)
        res[k] = (held, np.sqrt((d * d).sum(axis=1)))
    both = (pred["heading_src"][held] == 1) & (gt["heading_src"][g] == 1)
    hp, hg = pred["heading"][held][both].astype(f64), gt["heading"][g][both].astype(f64)
    res["heading"] = (held[both], np.arctan2(np.abs(hp[:, 0] * hg[:, 1] - hp[:, 1] * hg[:, 0]), hp[:, 0] * hg[:, 0] + hp[:, 1] * hg[:, 1]))
    return {k: [v[clip_of_row[rows] == c] for c in range(C)] for k, (rows, v) in res.items()}


def check_errors(got, want, C):
    """mean and max per clip against numpy.  The terms are the same numbers up to the rounding of three products, two sums and a root
    (or an atan2): within 4 * 2^-52 relative each.  A float64 sum of n terms in any order lies within (n - 1) 2^-53 times the sum of
    magnitudes of the exact sum, two orders within n 2^-52 of each other; the quotient by n adds one rounding."""
    for k, per_clip in want.items():
        for c in range(C):
            v = per_clip[c]
            n = len(v)
            if n == 0:
                assert np.isnan(got[k]["mean"][c]) and np.isnan(got[k]["max"][c])
                continue
            bound = ((n + 4) * 2.0 ** -52 * np.abs(v).sum()) / n + 2.0 ** -52 * abs(v.mean())
            assert abs(got[k]["mean"][c] - v.mean()) <= bound, (k, c, got[k]["mean"][c], v.mean(), bound)
            assert abs(got[k]["max"][c] - v.max()) <= 4 * 2.0 ** -52 * v.max(), (k, c)


# ---- the worlds --------------------------------------------------------------------------------------------------------------------------
def side(t):
    """What the call reads of one side, from a dict of tables."""
    return {k: t[k] for k in GT_TABLES}


def tracking_world(max_gap=2):
    """The world of tracks_ref clustered and tracked by the restatements, both sources -> (frames, owners, {which: tables})."""
    frames, owners = tref.build_world()
    sides = {}
    for which in ("pred", "gt"):
        off1, total, count, label, centroid, disp, T = tref.world_tables(frames, which)
        trk = tref.track(off1, total, count, label, centroid, disp, T, tref.WORLD_CLIPS, tref.GATE, max_gap)
        sides[which] = {"off1": np.asarray(off1), "total": total, "count": count, "label": label, "track": trk["track"], "prev_row": trk["prev_row"]}
    return frames, owners, sides


def objects_world(flow_noise=0.01):
    """The world of objects_ref, both sources -> (frames, {which: tables as objects_ref.world_tables returns them})."""
    frames, owners, truth = oref.build_world(flow_noise=flow_noise)
    return frames, {which: oref.world_tables(frames, which) for which in ("pred", "gt")}


def random_tables(rng, frames=4, nmax=9):
    """A clip of small frames whose instances are runs of two or four points, the other side's the same runs shifted by one or two
    points -- overlaps of exactly one half everywhere (2 of 4, 1 of 2 against 2 of 2 ...) -- with points dropped at random; tracks
    drawn from a handful of ids, prev_row the track's row before (or -1) -> (off1, total, gt, pred)."""
    counts = rng.integers(0, nmax + 1, frames)
    off1 = np.concatenate(([0], np.cumsum(counts)))
    total = int(off1[-1])
    sides = []
    for s in range(2):
        count, label = np.zeros(frames, np.int32), np.full(total, -1, np.int32)
        track, prev_row = np.full(total, -1, np.int32), np.full(total, -1, np.int32)
        last = {}
        for f in range(frames):
            n, a = int(counts[f]), int(off1[f])
            run, shift = int(rng.choice([1, 2, 2, 4])), int(rng.integers(0, 3)) if s else 0
            lab = (np.arange(n) + shift) // run
            lab = np.unique(lab, return_inverse=True)[1].reshape(-1) if n else lab
            lab = np.where(rng.random(n) < 0.15, -1, lab)
            kept = np.unique(lab[lab >= 0])
            lab = np.where(lab >= 0, np.searchsorted(kept, lab), -1)
            K = len(kept)
            count[f], label[a:a + n] = K, lab
            ids = rng.permutation(max(K, min(6, int(off1[f + 1]))))[:K]      # below the clip's rows so far, as a tracker numbers
            for k in range(K):
                track[a + k], prev_row[a + k] = ids[k], last.get(int(ids[k]), -1)
                last[int(ids[k])] = a + k
        sides.append({"count": count, "label": label, "track": track, "prev_row": prev_row})
    return off1, total, sides[0], sides[1]


# ---- the hand-built clip: every case once -------------------------------------------------------------------------------------------------
def hand_clip():
    """Nine frames of at most nine points, one clip -> (off1, total, gt, pred, want): the labels per point, the tracks per instance and
    what must come out at iou 0.5, worked out by hand.
      0  gt {0..3} (track 0) and {4, 5} (track 1); pred the same sets (tracks 0, 1): two matches at IoU 1
      1  gt {0, 1, 2} (track 0) against pred {0, 1} (track 0): 2 of 3, matched at 0.5 and not at 0.7; gt {3..6} (track 1) against pred
         {5..8}: 2 of 6; gt {7, 8} (track 2) against the same pred {5..8}: 2 of 4, EXACTLY one half, unmatched
      2  gt track 0 matched by pred track 5: an id switch; its instance directly before (frame 1) was matched: no fragmentation
      3  gt track 0 unmatched (the pred side has nothing)
      4  gt track 0 matched by pred track 5 again: a fragmentation without a switch; gt track 2 unmatched
      5  a gt instance whose track is -7, matched: no identity -- it counts in tp and nowhere else
      6  a frame the pred side did not select (count 0, labels -1): two misses
      7  an empty frame
      8  a one-point frame: one instance on both sides, gt track 3 seen for the first time"""
    g_lab, p_lab, g_trk, p_trk = [], [], [], []
    #  frame 0
    g_lab.append([0, 0, 0, 0, 1, 1, -1]);           p_lab.append([0, 0, 0, 0, 1, 1, -1]);           g_trk.append([0, 1]);     p_trk.append([0, 1])
    #  frame 1: gt 0 = {0,1,2} against pred 0 = {0,1}: 2 of 3 (matched at 0.5 only); gt 1 = {3,4,5,6} against pred 1 = {5,6,7,8}: 2 of 6;
    #           gt 2 = {7,8} against pred 1: 2 of 4 = exactly one half (unmatched)
    g_lab.append([0, 0, 0, 1, 1, 1, 1, 2, 2]);      p_lab.append([0, 0, -1, -1, -1, 1, 1, 1, 1]);   g_trk.append([0, 1, 2]);  p_trk.append([0, 2])
    #  frame 2
    g_lab.append([0, 0, 0, -1]);                    p_lab.append([0, 0, 0, -1]);                    g_trk.append([0]);        p_trk.append([5])
    #  frame 3
    g_lab.append([-1, 0, 0]);                       p_lab.append([-1, -1, -1]);                     g_trk.append([0]);        p_trk.append([])
    #  frame 4
    g_lab.append([0, 0, 1, 1, 1]);                  p_lab.append([0, 0, -1, -1, -1]);               g_trk.append([0, 2]);     p_trk.append([5])
    #  frame 5
    g_lab.append([0, 0, 0]);                        p_lab.append([0, 0, 0]);                        g_trk.append([-7]);       p_trk.append([3])
    #  frame 6: pred did not select it; frame 7: empty
    g_lab.append([0, 0, 1, 1]);                     p_lab.append([-1, -1, -1, -1]);                 g_trk.append([0, 2]);     p_trk.append([])
    g_lab.append([]);                               p_lab.append([]);                               g_trk.append([]);         p_trk.append([])
    #  frame 8
    g_lab.append([0]);                              p_lab.append([0]);                              g_trk.append([3]);        p_trk.append([1])
    counts = [len(x) for x in g_lab]
    off1 = np.concatenate(([0], np.cumsum(counts)))
    total, F = int(off1[-1]), len(counts)

    def tables(labels, tracks):
        t = {"count": np.array([len(k) for k in tracks], np.int32), "label": np.full(total, -1, np.int32), "track": np.full(total, -1, np.int32),
             "prev_row": np.full(total, -1, np.int32)}
        last = {}
        for f in range(F):
            a = int(off1[f])
            t["label"][a:a + counts[f]] = labels[f]
            for k, u in enumerate(tracks[f]):
                t["track"][a + k], t["prev_row"][a + k] = u, last.get(u, -1)
                last[u] = a + k
        return t

    gt, pred = tables(g_lab, g_trk), tables(p_lab, p_trk)
    o = [int(v) for v in off1]
    want = {"frame": [(2, 0, 0), (1, 1, 2), (1, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0), (0, 0, 2), (0, 0, 0), (1, 0, 0)],
            "switch": [o[2]], "frag": [o[4]], "iou_07": (0, 2, 3), "units": 6 * IOU_UNIT + int(np.floor(f64(2) / f64(3) * f64(IOU_UNIT))),
            "no_identity": o[5], "seen": {0: 6, 1: 2, 2: 3, 3: 1}, "covered": {0: 4, 1: 1, 2: 0, 3: 1},
            "clip": {"tp": 7, "fp": 1, "fn": 6, "ids": 1, "frags": 1, "gt_total": 13}}
    return off1, total, gt, pred, want


# ---- frames at the kernel's edges ----------------------------------------------------------------------------------------------------------
def edge_tables():
    """One clip with frames of 0, 1, 63, 64, 65, 1024 and 1024 points, an empty clip and a one-frame clip -> (off1, total, clips, gt,
    pred).  The small frames: runs of three points against the same runs shifted by one.  The first 1024-point frame: the gt side one
    instance of everything, the pred side 512 instances of two points.  The second: both sides 1024/3 triples, the pred side's shifted
    by one point -- every overlap is 2 of 4, one half, so nothing matches (the last point of either side is left over: -1)."""
    sizes = [0, 1, 63, 64, 65, 1024, 1024, 5]
    off1 = np.concatenate(([0], np.cumsum(sizes)))
    total, F = int(off1[-1]), len(sizes)
    gt = {"count": np.zeros(F, np.int32), "label": np.full(total, -1, np.int32), "track": np.full(total, -1, np.int32), "prev_row": np.full(total, -1, np.int32)}
    pred = {k: v.copy() for k, v in gt.items()}
    for f, n in enumerate(sizes):
        a = int(off1[f])
        i = np.arange(n)
        if f == 5:
            g, p = np.zeros(n, np.int64), i // 2
        elif f == 6:
            g, p = np.where(i < 1023, i // 3, -1), np.where(i >= 1, (i - 1) // 3, -1)
        else:
            g, p = i // 3, (i + (f % 2)) // 3
        for t, lab in ((gt, g), (pred, p)):
            K = int(lab.max()) + 1 if n else 0
            t["count"][f], t["label"][a:a + n] = K, lab
            t["track"][a:a + K] = np.arange(K)                              # instance k is track k in every frame
            if f > 0:
                before = int(off1[f - 1])
                Kb = int(t["count"][f - 1])
                t["prev_row"][a:a + K] = np.where(np.arange(K) < Kb, before + np.arange(K), -1)
    clips = np.array([(0, 7), (3, 3), (7, 8)], dtype=np.int32)
    return off1, total, clips, gt, pred


# ---- corrupted tables for the entry point -------------------------------------------------------------------------------------------------
def corrupt_tables(sides, seed=4):
    """The tracking world's tables with everything the entry point has to bound itself against -> (off1, total, clips, gt, pred): labels
    at and beyond K and hugely negative, a ``count`` far beyond a frame's rows and a negative one, track ids beyond the clip's rows,
    negative, and one id twice in a frame, ``prev_row`` far outside the tables, behind the row itself and in a two-cycle, offsets that
    descend (a frame that owns no rows, the frames behind it cut off), ``total`` cut inside the last frame; the clips: one reaching
    behind F, an empty one, a one-frame one, one that starts at the frame whose offset lies outside the tables.  No two clips overlap."""
    rng = np.random.default_rng(seed)
    gt, pred = ({k: np.array(s[k], copy=True) for k in GT_TABLES} for s in (sides["gt"], sides["pred"]))
    off1 = np.array(sides["gt"]["off1"], dtype=np.int64)
    F, total = len(off1) - 1, int(off1[-1])
    for t in (gt, pred):
        rows = rng.choice(total, 40, replace=False)
        t["label"][rows[:10]] = [2 ** 31 - 1, -2 ** 31, -2, 1024, 1025, 7, 8, 9, 100000, -100000]
        t["label"][rows[10:20]] = t["count"][np.searchsorted(off1, rows[10:20], side="right") - 1]      # exactly K
        held = np.flatnonzero(t["track"] >= 0)
        bad = rng.choice(held, 12, replace=False)
        t["track"][bad[:6]] = [2 ** 31 - 1, -2 ** 31, total, total + 5, -3, int(off1[10]) + 1]
        t["prev_row"][bad[6:12]] = [2 ** 31 - 1, -2 ** 31, total + 3, int(bad[6]), int(bad[7]) + 40, -9]
        late = held[t["prev_row"][held] >= 0]
        a, b = int(late[4]), int(late[-4])
        t["prev_row"][a], t["prev_row"][b] = b, a                           # a two-cycle
        t["count"][5], t["count"][6] = 5000, -4
    dup = int(off1[2])
    gt["track"][dup + 1] = gt["track"][dup]                                 # one id twice in a frame
    off1[8] = total + 9                                                     # frames 7 and 8 own no rows, frame 9 does: a gap behind the clip's solid rows
    off1[13] = off1[12] - 7                                                 # descending: frame 12 owns no rows, frame 13 starts below top
    off1[16] = total + 50                                                   # outside the tables: the clip that starts there owns nothing
    clips = np.array([(14, 16), (4, 4), (3, 4), (4, 14), (-3, 3), (16, F + 9)], dtype=np.int32)
    return off1.astype(np.int32), int(off1[F - 1]) + 2, clips, gt, pred
