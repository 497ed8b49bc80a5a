"""numpy restatement of cmflow_amd/csrc/tracks.hip (tests/test_tracks_host.py, tests/test_gpu_tracks.py): the cost, the coasting
displacement and the prediction in float64 with the operation order of include/cmflow_hip.h written out, so that every product and
sum is one rounded float64 operation (numpy's elementwise ``*`` and ``+`` never fuse); the association as the definition has it, the
literal sorted greedy over the edges; a second, differently written association (mutual-best rounds over masked arg-mins, what
the kernel does) that must agree with it; a world whose answer is known without either; and the hand-made instance tables the
entry point is called with.  Nothing here imports cmflow_amd."""
import numpy as np

import instances_ref as iref

f32, f64 = np.float32, np.float64
MAX_LIVE, MAX_GAP = 1024, 16
PER_INSTANCE = ("track", "prev_row", "gap", "age", "pred", "point_track")
PER_TRACK = ("birth", "last", "hits")
PER_CLIP = ("ntracks", "overflow")
KEYS = PER_INSTANCE + PER_TRACK + PER_CLIP
FILL = {"track": -1, "prev_row": -1, "gap": 0, "age": 0, "pred": 0.0, "point_track": -1, "birth": -1, "last": -1, "hits": 0, "ntracks": 0,
        "overflow": 0}                                      # what ``track`` of cmflow_amd/tracks.py fills its outputs with


def outputs(rows, nclips, fill=FILL):
    """The outputs of cmf_track_instances, ``rows`` rows and ``nclips`` clips, filled: -> dict."""
    out = {k: np.full(rows, fill[k], np.int32) for k in ("track", "prev_row", "gap", "age", "point_track") + PER_TRACK}
    out["pred"] = np.full((rows, 3), fill["pred"], f32)
    out.update({k: np.full(nclips, fill[k], np.int32) for k in PER_CLIP})
    return out


# ---- the association of one frame, twice --------------------------------------------------------------------------------------------------
def cost(P, c):
    """(L,K) float64: G2 = (e0*e0 + e1*e1) + e2*e2, e_r = P_r - (double)c_r.  P (L,3) float64, c (K,3) float32."""
    with np.errstate(all="ignore"):
        e = P[:, None, :] - c.astype(f64)[None, :, :]
        sq = e * e
        return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def associate_greedy(P, ids, c, gate2):
    """The definition: the edges (G2 <= gate2) in ascending (G2, track id, j); an edge matches iff neither end is matched.
    -> (match (K) int64: the position in the live list of the track instance j matched, or -1; 1)."""
    G2 = cost(P, c)
    with np.errstate(all="ignore"):
        edges = sorted((float(G2[u, j]), int(ids[u]), int(j), int(u)) for u, j in np.argwhere(G2 <= gate2))
    match, taken = np.full(len(c), -1, np.int64), set()
    for _, _, j, u in edges:
        if match[j] < 0 and u not in taken:
            match[j] = u
            taken.add(u)
    return match, 1


def associate_rounds(P, ids, c, gate2):
    """The same matching, written differently: the cost coordinate by coordinate, then rounds in which every unmatched track picks its
    best unmatched instance (the first of equal minima: the lowest j), every unmatched instance its best unmatched track (the live
    list ascends in track id, so the first of equal minima is the lowest id), and the pairs that picked each other match -- until a
    round matches nothing.  -> (match, the rounds that matched something)."""
    L, K = len(P), len(c)
    assert list(ids) == sorted(ids)
    G2 = np.zeros((L, K), dtype=f64)
    with np.errstate(all="ignore"):
        for r in range(3):
            e = np.subtract.outer(P[:, r], c[:, r].astype(f64))
            G2 = G2 + e * e if r else e * e
        edge = G2 <= gate2
    free_t, free_i = np.ones(L, bool), np.ones(K, bool)
    match, rounds = np.full(K, -1, np.int64), 0
    while True:
        usable = edge & free_t[:, None] & free_i[None, :]
        if not usable.any():
            break
        key = np.where(usable, G2, np.inf)                                   # gate2 is finite: an edge never costs inf
        t_pick = np.where(usable.any(axis=1), key.argmin(axis=1), -1)
        i_pick = np.where(usable.any(axis=0), key.argmin(axis=0), -1)
        pairs = [(u, j) for u, j in enumerate(t_pick) if j >= 0 and i_pick[j] == u]
        assert pairs                                                         # the smallest usable edge is always mutual
        for u, j in pairs:
            match[j], free_t[u], free_i[j] = u, False, False
        rounds += 1
    return match, rounds


# ---- the clip walk ------------------------------------------------------------------------------------------------------------------------
def track(off1, total, count, label, centroid, disp, T, clips, gate, max_gap, out=None, associate=associate_greedy, stats=None):
    """cmf_track_instances -> dict of the outputs (``out``: arrays to write into, e.g. sentinel-filled ones; default: ``outputs`` with
    the fills of cmflow_amd.tracks.track).  gate2 is formed as the host forms it.  ``stats``: a dict that receives ``rounds``, the
    largest number ``associate`` reported for a frame."""
    off1 = np.asarray(off1, dtype=np.int64)
    F, total = len(off1) - 1, int(total)
    assert centroid.dtype == f32 and disp.dtype == f32 and T.dtype == f32 and 0 <= max_gap <= MAX_GAP
    T = T.reshape(F, 4, 4).astype(f64)
    gate2 = f64(float(gate) * float(gate))
    clips = np.asarray(clips, dtype=np.int64).reshape(-1, 2)
    out = outputs(total, len(clips)) if out is None else out
    most = 0
    for ci, (first, end) in enumerate(clips):
        first = min(max(int(first), 0), F)
        end = min(max(int(end), first), F)
        base = int(off1[first])
        clip_ok = 0 <= base <= total
        top, owned = base, []
        live, next_id, overflow = [], 0, 0                                   # live: dicts in ascending track id
        finished = []

        for f in range(first, end):
            s, e = int(off1[f]), int(off1[f + 1])
            owns = clip_ok and s >= top and e >= s and e <= total
            n = e - s if owns else 0
            if owns:
                top = e
                owned.append((s, e))
            K = min(max(int(count[f]), 0), n, MAX_LIVE) if owns else 0
            row0 = s if owns else 0
            c, Tf = centroid[row0:row0 + K], T[f]
            P = np.array([t["P"] for t in live], dtype=f64).reshape(-1, 3)
            match, rounds = associate(P, [t["id"] for t in live], c, gate2) if K and live else (np.full(K, -1, np.int64), 0)
            most = max(most, rounds)
            births, itrack = [], np.full(K, -1, np.int64)
            for t in live:
                t["matched"] = False
            for j in range(K):
                row = row0 + j
                fresh = {"P": c[j].astype(f64), "D": disp[row].astype(f64), "miss": 0, "last_row": row, "last": f, "matched": True}
                if match[j] >= 0:
                    t = live[match[j]]
                    t["hits"] += 1
                    out["track"][row], out["prev_row"][row], out["gap"][row], out["age"][row] = t["id"], t["last_row"], f - t["last"], t["hits"]
                    out["pred"][row] = t["P"].astype(f32)
                    t.update(fresh)
                else:
                    t = dict(fresh, id=next_id + len(births), hits=1, birth=f)
                    out["track"][row], out["prev_row"][row], out["gap"][row], out["age"][row] = t["id"], -1, 0, 1
                    out["pred"][row] = c[j]
                    births.append(t)
                itrack[j] = t["id"]
            survivors, coasting = [], 0
            for t in live:
                if not t["matched"]:
                    t["miss"] += 1
                    t["dead"] = t["miss"] > max_gap
                    coasting += not t["dead"]
                else:
                    t["dead"] = False
            if K + coasting > MAX_LIVE:
                overflow += 1
                for t in live:
                    t["dead"] = t["dead"] or not t["matched"]
            for t in live:
                if t["dead"]:
                    finished.append(t)
                    continue
                if not t["matched"]:
                    D = t["D"]
                    with np.errstate(all="ignore"):
                        t["D"] = np.array([(Tf[r, 0] * D[0] + Tf[r, 1] * D[1]) + Tf[r, 2] * D[2] for r in range(3)], dtype=f64)
                survivors.append(t)
            live = survivors + births
            next_id += len(births)
            for t in live:
                p, D = t["P"], t["D"]
                with np.errstate(all="ignore"):
                    t["P"] = np.array([(((Tf[r, 0] * p[0] + Tf[r, 1] * p[1]) + Tf[r, 2] * p[2]) + Tf[r, 3]) + D[r] for r in range(3)], dtype=f64)
            for k in ("track", "prev_row"):
                out[k][row0 + K:row0 + n] = -1
            for k in ("gap", "age", "pred"):
                out[k][row0 + K:row0 + n] = 0
            lab = label[row0:row0 + n].astype(np.int64)
            held = (lab >= 0) & (lab < K)
            out["point_track"][row0:row0 + n] = np.where(held, itrack[np.where(held, lab, 0)] if K else -1, -1)

        for t in finished + live:
            row = base + t["id"]
            out["birth"][row], out["last"][row], out["hits"][row] = t["birth"], t["last"], t["hits"]
        out["ntracks"][ci], out["overflow"][ci] = next_id, overflow
        for s, e in owned:
            lo = max(s, base + next_id)
            if lo < e:
                out["birth"][lo:e], out["last"][lo:e], out["hits"][lo:e] = -1, -1, 0
    if stats is not None:
        stats["rounds"] = most
    return out


def same(got, want, what=""):
    """Exact: integers equal, ``pred`` as uint32."""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if k == "pred":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist(), np.asarray(got[k])[tuple(bad[0])], np.asarray(want[k])[tuple(bad[0])])


def plan_clips(F, clips):
    """The clips of cmflow_amd.tracks.plan_clips, by a loop over the frames: the given ranges clamped, a frame outside every range a
    clip of its own, in frame order."""
    cover = np.full(F, -1)
    for k, (a, b) in enumerate([(0, F)] if clips is None else clips):
        cover[max(int(a), 0):min(int(b), F)] = k
    out, f = [], 0
    while f < F:
        g = f + 1
        while cover[f] >= 0 and g < F and cover[g] == cover[f]:
            g += 1
        out.append((f, g))
        f = g
    return np.array(out, dtype=np.int32).reshape(-1, 2)


# ---- a world whose answer is known without an association --------------------------------------------------------------------------------
WORLD_CLIPS = ((0, 10), (10, 18))
WORLD_OBJECTS = 5
GATE, EPS = 2.0, 2.0
# the frames of the FIRST clip in which an object's points are called static, per source: absent for 2 frames (kept at max_gap 2), for 3 (lost)
WORLD_ABSENT = {"pred": {1: (3, 4), 2: (3, 4, 5)}, "gt": {3: (4, 5), 0: (2, 3, 4)}}
WORLD_LOST = {"pred": 2, "gt": 0}                           # the object that comes back under a new id at max_gap 2


def _pose(f):
    yaw = 0.03 * f
    R = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    return R, np.array([1.0 * f, 0.1 * f, 0.0])


def build_world(seed=5):
    """Rigid objects at constant velocity seen from a sensor that drives and turns, two clips -> (frames, owners): ``frames`` in the
    format of instances_ref.build_case (pos1, flow, label, mask, gt_mask, pred_t, gt_t), ``owners`` per frame the generating object of
    every point (-1: clutter).  Every object is a blob of 6 .. 12 points within 0.5 m of its centre in every coordinate (one
    instance at eps 2), the objects keep more than 3 gates (and 3 eps) apart; the point order is shuffled anew in every frame, so an
    object's instance number changes from frame to frame.  The prediction's flow carries 1 cm of noise, the labels none; in the
    frames of WORLD_ABSENT an object's points are called static by that source.  The transforms are the true ego-motion in float32."""
    rng = np.random.default_rng(seed)
    frames, owners = [], []
    for first, end in WORLD_CLIPS:
        shape = [rng.uniform(-0.5, 0.5, (int(rng.integers(6, 13)), 3)) for _ in range(WORLD_OBJECTS)]
        start = [np.array([12.0 + 3.0 * k, -24.0 + 12.0 * k, 0.3 * k]) for k in range(WORLD_OBJECTS)]
        vel = [np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.2, 0.2), 0.0]) for _ in range(WORLD_OBJECTS)]
        clutter = np.stack([rng.uniform(0, 40, 30), rng.uniform(-30, 30, 30), rng.uniform(-1, 1, 30)], axis=1)
        for g in range(end - first):
            (R0, t0), (R1, t1) = _pose(g), _pose(g + 1)
            world0 = [start[k] + g * vel[k] + shape[k] for k in range(WORLD_OBJECTS)] + [clutter]
            world1 = [start[k] + (g + 1) * vel[k] + shape[k] for k in range(WORLD_OBJECTS)] + [clutter]
            p0 = np.concatenate([(w - t0) @ R0 for w in world0])             # rows: R^T (w - t)
            p1 = np.concatenate([(w - t1) @ R1 for w in world1])
            own = np.concatenate([np.full(len(w), k if k < WORLD_OBJECTS else -1) for k, w in enumerate(world0)])
            order = rng.permutation(len(p0))
            p0, p1, own = p0[order], p1[order], own[order]
            Tm = np.eye(4)
            Tm[:3, :3], Tm[:3, 3] = R1.T @ R0, R1.T @ (t0 - t1)
            pos1 = p0.astype(f32)
            label = (p1 - p0).astype(f32)
            flow = (p1 - p0 + 0.01 * rng.standard_normal(p0.shape)).astype(f32)
            mask, gt_mask = (own < 0).astype(np.uint8), (own < 0).astype(f32)
            for k, gone in WORLD_ABSENT["pred"].items():
                if first == 0 and g in gone:
                    mask[own == k] = 1
            for k, gone in WORLD_ABSENT["gt"].items():
                if first == 0 and g in gone:
                    gt_mask[own == k] = 1.0
            frames.append({"pos1": pos1, "flow": flow, "label": label, "mask": mask, "gt_mask": gt_mask, "pred_t": Tm.astype(f32), "gt_t": Tm.astype(f32)})
            owners.append(own)
    return frames, owners


def world_tables(frames, which, eps=EPS, min_points=2, flow_weight=0.0):
    """The world clustered by the restatement of cmf_cluster_moving -> (off1, total, count, label, centroid, disp, T)."""
    off1, pos, flow, moving, T = iref.case_arrays(frames, which)
    inst = iref.cluster(off1, pos, flow, moving, T, list(range(len(frames))), eps, min_points, flow_weight)
    return off1, int(off1[-1]), inst["count"], inst["label"], inst["centroid"], inst["disp"], T.reshape(-1, 16)


# ---- hand-made instance tables for the entry point ---------------------------------------------------------------------------------------
C_GATE, C_TIE_TRACKS, C_TIE_INSTANCES, C_CROSSING, C_NAN, C_LADDER, C_OVERFLOW, C_RANDOM = range(8)
LADDER = 200


def _frame(centroids, disp=None, extra=3):
    c = np.asarray(centroids, dtype=f32).reshape(-1, 3)
    d = np.zeros_like(c) if disp is None else np.asarray(disp, dtype=f32).reshape(-1, 3)
    return {"c": c, "d": d, "n": len(c) + extra, "T": np.eye(4, dtype=f32)}


def ladder_positions(m=LADDER):
    """m tracks and m instances interleaved on a line, T0 I0 T1 I1 .. with strictly decreasing gaps (multiples of 1/256 below the gate
    of 2): every instance but the last is nearer to the track on its right, every track to the instance on its right, so a
    mutual-best round matches ONE pair, the last, and frees the next: (T_k, I_k) for every k, after m rounds."""
    gaps = (2.0 - 1.0 / 256) - np.arange(2 * m - 1) / 256.0
    x = np.concatenate(([0.0], np.cumsum(gaps)))
    assert gaps.min() > 0 and np.array_equal(x.astype(f32).astype(f64), x)
    return x[0::2], x[1::2]


def build_tables(seed=3):
    """-> dict: off1 (F+1), total, count (F), label (total), centroid, disp (total,3), T (F,16), clips (C,2): one clip per special
    case (C_*), identity transforms and zero displacements unless said otherwise, whole-number or dyadic coordinates, gate 2.
      GATE            a track at the origin, instances exactly 2 m away (on the gate: matched) and at (10, 0, 2.25) from a track at (10, 0, 0)
      TIE_TRACKS      tracks at x = -1 and x = 1, one instance at 0: the lower id wins; the other track coasts
      TIE_INSTANCES   a track at 0, instances at x = 1 (j 0) and x = -1 (j 1): the lower j wins, the other opens a track
      CROSSING        tracks at 0 and 2, instances at 1.25 and -1.75: nearest first gives (1, 1.25) and then (0, -1.75); track by track
                      would give track 0 the instance at 1.25 and leave the other without a track inside the gate
      NAN             a NaN centroid: no edge, a new track that nothing ever matches
      LADDER          ``ladder_positions``; the instances in descending x
      OVERFLOW        1024 instances, then 1024 distant ones (the first 1024 would coast: over capacity, they die), then four of
                      the second set (1020 coast, no birth: that fits)
      RANDOM          six frames of up to 40 instances on a small whole-number grid (ties everywhere), transforms that turn and shift
                      by whole numbers, random whole-number displacements, a frame with count 0 in the middle
    Every frame has a few rows more than instances; labels are random in -1 .. K+1 (K and K+1: no instance)."""
    rng = np.random.default_rng(seed)
    clips = []
    clips.append([_frame([(0, 0, 0), (10, 0, 0)]), _frame([(0, 2, 0), (10, 0, 2.25)])])
    clips.append([_frame([(-1, 0, 0), (1, 0, 0)]), _frame([(0, 0, 0)]), _frame([(1, 0, 0)])])
    clips.append([_frame([(0, 0, 0)]), _frame([(1, 0, 0), (-1, 0, 0)])])
    clips.append([_frame([(0, 0, 0), (2, 0, 0)]), _frame([(1.25, 0, 0), (-1.75, 0, 0)])])
    clips.append([_frame([(0, 0, 0), (5, 5, 0)]), _frame([(0, 1, 0), (np.nan, 5, 0), (5, 5, 1)]), _frame([(0, 1, 1), (5, 5, 0), (np.nan, 5, 0)])])
    tx, ix = ladder_positions()
    line = lambda x: np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)
    clips.append([_frame(line(tx)), _frame(line(ix[::-1]))])
    grid = np.stack([np.arange(1024) % 32 * 8.0, np.arange(1024) // 32 * 8.0, np.zeros(1024)], axis=1)
    far = grid + np.array([0.0, 0.0, 64.0])
    clips.append([_frame(grid, extra=0), _frame(far, extra=1), _frame(far[5:9])])
    rand = []
    for g in range(6):
        K = 0 if g == 3 else int(rng.integers(20, 41))
        fr = _frame(rng.integers(-4, 5, (K, 3)), rng.integers(-1, 2, (K, 3)))
        quarter = [np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]]), np.array([[-1, 0, 0], [0, -1, 0], [0, 0, 1]])][g % 3]
        fr["T"][:3, :3], fr["T"][:3, 3] = quarter, rng.integers(-1, 2, 3)
        rand.append(fr)
    clips.append(rand)
    frames = [fr for clip in clips for fr in clip]
    off1 = np.concatenate(([0], np.cumsum([fr["n"] for fr in frames])))
    total, F = int(off1[-1]), len(frames)
    centroid, disp = np.zeros((total, 3), f32), np.zeros((total, 3), f32)
    count, label = np.zeros(F, np.int32), np.full(total, -1, np.int32)
    for f, fr in enumerate(frames):
        K = len(fr["c"])
        centroid[off1[f]:off1[f] + K], disp[off1[f]:off1[f] + K], count[f] = fr["c"], fr["d"], K
        label[off1[f]:off1[f + 1]] = rng.integers(-1, K + 2, fr["n"])
    edges = np.concatenate(([0], np.cumsum([len(clip) for clip in clips])))
    return {"off1": off1.astype(np.int32), "total": total, "count": count, "label": label, "centroid": centroid, "disp": disp,
            "T": np.stack([fr["T"] for fr in frames]).reshape(F, 16), "clips": np.stack([edges[:-1], edges[1:]], axis=1).astype(np.int32)}


def random_tables(rng, frames=5, grid=3, kmax=12):
    """A clip of tie-heavy frames: centroids on a grid of ``grid``^3 whole numbers, NaNs here and there, whole-number transforms."""
    fr = []
    for _ in range(frames):
        K = int(rng.integers(0, kmax + 1))
        c = rng.integers(0, grid, (K, 3)).astype(f64)
        c[rng.random(K) < 0.08, int(rng.integers(0, 3))] = np.nan
        one = _frame(c, rng.integers(-1, 2, (K, 3)), extra=int(rng.integers(0, 3)))
        one["T"][:3, 3] = rng.integers(-1, 2, 3)
        fr.append(one)
    off1 = np.concatenate(([0], np.cumsum([f["n"] for f in fr])))
    total = int(off1[-1])
    centroid, disp, count = np.zeros((total, 3), f32), np.zeros((total, 3), f32), np.zeros(frames, np.int32)
    for f, one in enumerate(fr):
        K = len(one["c"])
        centroid[off1[f]:off1[f] + K], disp[off1[f]:off1[f] + K], count[f] = one["c"], one["d"], K
    label = rng.integers(-1, kmax, total).astype(np.int32)
    return off1, total, count, label, centroid, disp, np.stack([f["T"] for f in fr]).reshape(frames, 16)
