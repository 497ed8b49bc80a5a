"""numpy restatement of cmflow_amd/csrc/instances.hip (tests/test_instances_host.py, tests/test_gpu_instances.py): the own-motion
displacement, the pair distance and the sums in float64 with the operation order of include/cmflow_hip.h written out, so that every
product and sum is one rounded float64 operation (numpy's elementwise ``*`` and ``+`` never fuse); the clustering rules point by
point (the instances as a union-find forest over the neighbouring core points); a second, differently written implementation (an explicit adjacency matrix and a
breadth-first search) that must agree with it; worlds whose answer is known without either; and the builder of the case the GPU
tests share.  Nothing here imports cmflow_amd."""
from collections import deque

import numpy as np

f32, f64 = np.float32, np.float64
MAX_POINTS = 1024
NONE, NOISE, BORDER, CORE = 0, 1, 2, 3
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
           (70, 240, 240), (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (170, 110, 40))
LIGHT_GREY, DIM_GREY = (200, 200, 200), (120, 120, 120)
IOU_UNIT = 2 ** 30
# tests/golden/saved_results_delft_12_w12.npz, frames 727 .. 738 at eps 2, min_points 2, flow_weight 0 (an independent brute force):
# the sizes of every frame's instances, its noise points; there are no border points
SAVED_SIZES = ([16], [19, 2], [22], [18], [11], [15], [11], [14], [16], [12], [17], [21])
SAVED_NOISE = (0, 2, 1, 0, 2, 0, 0, 1, 0, 0, 2, 0)


def displacement(p, flow, T):
    """d_r = ((double)p_r + (double)f_r) - tp_r, tp_r = ((T[r][0] px + T[r][1] py) + T[r][2] pz) + T[r][3]: (n,3) float64 from float32."""
    assert p.dtype == f32 and flow.dtype == f32 and T.dtype == f32
    p, fl, T = p.astype(f64), flow.astype(f64), T.astype(f64)
    with np.errstate(all="ignore"):
        tp = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)
        return (p + fl) - tp


def pair_d2(p, d, w2):
    """(m,m) float64: D2(i,j) = ((dx*dx + dy*dy) + dz*dz) + w2 * ((ex*ex + ey*ey) + ez*ez), one row per point."""
    p = p.astype(f64)
    out = np.empty((len(p), len(p)), dtype=f64)
    with np.errstate(all="ignore"):
        for i in range(len(p)):
            dx, dy, dz = p[i, 0] - p[:, 0], p[i, 1] - p[:, 1], p[i, 2] - p[:, 2]
            ex, ey, ez = d[i, 0] - d[:, 0], d[i, 1] - d[:, 1], d[i, 2] - d[:, 2]
            out[i] = ((dx * dx + dy * dy) + dz * dz) + w2 * ((ex * ex + ey * ey) + ez * ez)
    return out


def _empty(n):
    z3 = lambda: np.zeros((n, 3), dtype=f32)
    return {"label": np.full(n, -1, np.int32), "kind": np.zeros(n, np.uint8), "count": 0, "size": np.zeros(n, np.int32),
            "seed": np.full(n, -1, np.int32), "centroid": z3(), "disp": z3(), "lo": z3(), "hi": z3()}


def _statistics(out, label, idx, p, d, seeds):
    """The instance tables of one frame from the candidates' labels, member by member in ascending point order."""
    for c, seed in enumerate(seeds):
        members = np.flatnonzero(label == c).tolist()                       # ascending
        S, E = np.zeros(3, dtype=f64), np.zeros(3, dtype=f64)
        lo, hi = p[members[0]].copy(), p[members[0]].copy()
        for i in members:
            S = S + p[i].astype(f64)
            E = E + d[i]
            for r in range(3):
                if p[i, r] < lo[r]:
                    lo[r] = p[i, r]
                if p[i, r] > hi[r]:
                    hi[r] = p[i, r]
        size = len(members)
        out["size"][c], out["seed"][c] = size, idx[seed]
        with np.errstate(all="ignore"):
            out["centroid"][c], out["disp"][c] = (S / f64(size)).astype(f32), (E / f64(size)).astype(f32)
        out["lo"][c], out["hi"][c] = lo, hi


def cluster_frame(pos, flow, cand, T, eps2, w2, min_points, d2=None):
    """One frame of cmf_cluster_moving.  pos, flow (n,3) float32; cand (n) bool; T (4,4) float32; eps2, w2 float64.
    -> dict label (n) int32, kind (n) uint8, count, size, seed (n) int32, centroid, disp, lo, hi (n,3) float32.
    ``d2``: the (m,m) result of ``pair_d2`` for these candidates, where the caller has it already."""
    n = len(pos)
    out = _empty(n)
    if n > MAX_POINTS:
        return out
    idx = np.flatnonzero(cand)
    m = len(idx)
    p, d = pos[idx], displacement(pos[idx], flow[idx], T)
    D2 = pair_d2(p, d, f64(w2)) if d2 is None else d2
    with np.errstate(all="ignore"):
        near = D2 <= f64(eps2)
    core = np.array([int(near[i].sum()) >= min_points for i in range(m)], dtype=bool)
    # instances: the classes of the core points under "is a neighbour of", as a union-find forest whose roots are the lowest indices
    parent = list(range(m))

    def root(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in range(m):
        if core[i]:
            for j in np.flatnonzero(near[i, i + 1:] & core[i + 1:]) + i + 1:
                a, b = root(i), root(int(j))
                parent[max(a, b)] = min(a, b)
    seeds = [i for i in range(m) if core[i] and root(i) == i]               # ascending: the numbering
    number = {s: k for k, s in enumerate(seeds)}
    label = np.array([number[root(i)] if core[i] else -1 for i in range(m)], dtype=np.int64).reshape(m)
    kind = np.where(core, CORE, NOISE).astype(np.uint8)
    for i in range(m):
        if core[i]:
            continue
        best = -1
        for j in np.flatnonzero(near[i] & core):                            # ascending, a strict compare: the lowest index among equals
            if best < 0 or D2[i, j] < D2[i, best]:
                best = int(j)
        if best >= 0:
            label[i], kind[i] = label[best], BORDER
    out["label"][idx], out["kind"][idx], out["count"] = label, kind, len(seeds)
    _statistics(out, label, idx, p, d, seeds)
    return out


def cluster_frame_bfs(pos, flow, cand, T, eps2, w2, min_points):
    """The same answer, written differently: every pair distance at once by broadcasting, an explicit adjacency matrix of the core
    points, a breadth-first search from every core point not yet reached, borders by a masked arg-min over the matrix rows, sums
    by sequential cumulative sums."""
    n = len(pos)
    out = _empty(n)
    if n > MAX_POINTS:
        return out
    idx = np.flatnonzero(cand)
    m = len(idx)
    p = pos[idx]
    d = displacement(p, flow[idx], T)
    with np.errstate(all="ignore"):
        a, b = p.astype(f64)[:, None, :] - p.astype(f64)[None, :, :], d[:, None, :] - d[None, :, :]
        sq, fq = a * a, b * b
        D2 = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + f64(w2) * ((fq[..., 0] + fq[..., 1]) + fq[..., 2])
        near = D2 <= f64(eps2)
    core = near.sum(axis=1) >= min_points
    adjacent = near & core[:, None] & core[None, :]
    component = np.full(m, -1, dtype=np.int64)
    seeds = []
    for start in np.flatnonzero(core):
        if component[start] >= 0:
            continue
        queue = deque([start])
        component[start] = len(seeds)
        while queue:
            at = queue.popleft()
            fresh = np.flatnonzero(adjacent[at] & (component < 0))
            component[fresh] = len(seeds)
            queue.extend(fresh.tolist())
        seeds.append(int(start))
    kind = np.where(core, CORE, NOISE).astype(np.uint8)
    reach = np.where(near & core[None, :] & ~core[:, None], D2, np.inf)    # row i: the distances of a non-core point to its core neighbours
    has = (near & core[None, :] & ~core[:, None]).any(axis=1)
    nearest = np.argmin(reach, axis=1) if m else np.zeros(0, dtype=np.int64)   # the first of equal minima: the lowest index
    component[has] = component[nearest[has]]
    kind[has] = BORDER
    out["label"][idx], out["kind"][idx], out["count"] = component, kind, len(seeds)
    for c, seed in enumerate(seeds):
        mem = np.flatnonzero(component == c)
        out["size"][c], out["seed"][c] = len(mem), idx[seed]
        with np.errstate(all="ignore"):
            out["centroid"][c] = (np.cumsum(p[mem].astype(f64), axis=0)[-1] / f64(len(mem))).astype(f32)
            out["disp"][c] = (np.cumsum(d[mem], axis=0)[-1] / f64(len(mem))).astype(f32)
        out["lo"][c], out["hi"][c] = p[mem].min(axis=0), p[mem].max(axis=0)
    return out


KEYS = ("label", "kind", "size", "seed", "centroid", "disp", "lo", "hi")


def cluster(off1, pos, flow, moving, T, ids, eps, min_points, flow_weight, frame_fn=cluster_frame, cache=None):
    """cmf_cluster_moving over the frames ``ids`` of a packed split -> dict of the packed outputs: label, kind, size, seed, centroid,
    disp, lo, hi over all rows (frames not selected: label -1, the rest 0) and count (F).  eps2 and w2 are formed as the host forms
    them.  ``cache``: a dict that keeps the pair distances of (frame, flow_weight) between calls."""
    off1 = np.asarray(off1, dtype=np.int64)
    total, F = int(off1[-1]), len(off1) - 1
    eps2, w2 = f64(float(eps) * float(eps)), f64(float(flow_weight) * float(flow_weight))
    out = _empty(total)
    out["seed"][:] = 0
    out["count"] = np.zeros(F, dtype=np.int32)
    for fr in ids:
        a, b = int(off1[fr]), int(off1[fr + 1])
        kw = {}
        if cache is not None and frame_fn is cluster_frame and b - a <= MAX_POINTS:
            key = (int(fr), float(flow_weight))
            if key not in cache:
                idx = np.flatnonzero(moving[a:b])
                cache[key] = pair_d2(pos[a:b][idx], displacement(pos[a:b][idx], flow[a:b][idx], T[fr]), w2)
            kw["d2"] = cache[key]
        one = frame_fn(pos[a:b], flow[a:b], moving[a:b], T[fr], eps2, w2, min_points, **kw)
        for k in KEYS:
            out[k][a:b] = one[k]
        out["count"][fr] = one["count"]
    return out


def instance_colors(label, kind):
    """vis.instance_colors in whole numbers: (n,3) uint8."""
    out = np.empty((len(label), 3), dtype=np.uint8)
    for i, (l, k) in enumerate(zip(label, kind)):
        out[i] = PALETTE[int(l) % 12] if k >= BORDER else LIGHT_GREY if k == NOISE else DIM_GREY
    return out


def agreement(off1, ids, label_pred, size_pred, label_gt, size_gt):
    """instances.agreement as loops over the points: -> (nsel) float64."""
    out = []
    for fr in ids:
        a, b = int(off1[fr]), int(off1[fr + 1])
        units, points = 0, 0
        for i in range(a, b):
            g, p = int(label_gt[i]), int(label_pred[i])
            if g < 0:
                continue
            points += 1
            if p < 0:
                continue
            c = sum(1 for k in range(a, b) if label_gt[k] == g and label_pred[k] == p)
            iou = f64(c) / f64(int(size_gt[a + g]) + int(size_pred[a + p]) - c)
            units += int(np.floor(iou * f64(IOU_UNIT)))
        out.append(f64(units) / (f64(points) * f64(IOU_UNIT)) if points else np.nan)
    return np.array(out, dtype=f64)


# ---- worlds whose answer is known without a clustering ----------------------------------------------------------------------------------
def known_world(seed, eps, K=5, per=(6, 30), step=0.6):
    """K rigid objects, each a random walk of points with steps of at most ``step * eps`` (so every point has a neighbour and the
    object is connected), the objects' boxes more than 3 eps apart, every object with a velocity of its own; static points scattered
    over everything; the points of all objects and the static ones shuffled together.  Identity ego-motion.
    -> pos, flow (n,3) float32, moving (n) bool, T (4,4) float32, owner (n) int64: the generating object, -1 for a static point."""
    rng = np.random.default_rng(seed)
    pos, flow, owner = [], [], []
    for k in range(K):
        cnt = int(rng.integers(per[0], per[1]))
        steps = rng.uniform(-1.0, 1.0, (cnt, 3))
        steps *= (step * eps * rng.uniform(0.2, 1.0, (cnt, 1))) / np.linalg.norm(steps, axis=1, keepdims=True)
        walk = np.cumsum(steps, axis=0)
        walk = np.clip(walk - walk[0], -4.0 * eps, 4.0 * eps)               # clipping moves a point TOWARDS its predecessor's box: still within a step
        pos.append(walk + np.array([k * (8.0 * eps + 3.5 * eps), 0.0, 0.0]))  # boxes 8 eps wide, gaps of 3.5 eps
        flow.append(np.broadcast_to(rng.uniform(-1.0, 1.0, 3), (cnt, 3)))
        owner.append(np.full(cnt, k))
    S = int(rng.integers(20, 60))
    pos.append(np.stack([rng.uniform(-4 * eps, K * 11.5 * eps, S), rng.uniform(-4 * eps, 4 * eps, S), rng.uniform(-4 * eps, 4 * eps, S)], axis=1))
    flow.append(np.zeros((S, 3)))
    owner.append(np.full(S, -1))
    pos, flow, owner = np.concatenate(pos), np.concatenate(flow), np.concatenate(owner)
    order = rng.permutation(len(pos))
    pos, flow, owner = pos[order].astype(f32), flow[order].astype(f32), owner[order]
    return pos, flow, owner >= 0, np.eye(4, dtype=f32), owner


def known_labels(owner, moving):
    """The labels the numbering rule gives the generating objects: 0, 1, .. in the order of each object's lowest point index
    (with min_points <= 2 every point of a connected object is a core point)."""
    order = []
    for i in np.flatnonzero(moving):
        if owner[i] not in order:
            order.append(owner[i])
    return np.array([order.index(o) if mv else -1 for o, mv in zip(owner, moving)], dtype=np.int32)


# ---- the case of the GPU tests ----------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 256, 257, 300, 8, 97, 2, 1024)     # the edges of a 64-lane wave and of a 256-thread chunk, tiny frames, the cap
F_ONE, F_STATIC, F_GRID, F_ALL, F_OVERLAP, F_BRIDGE, F_CHAIN, F_TWINS, F_MIXED, F_PAIR, F_CAP = range(11)
EPS = (1.0, 2.0)                                            # 1.0: the grid's and the bridge's distances are exactly eps, the chain is a chain
MIN_POINTS = (1, 2, 4)
FLOW_WEIGHTS = (0.0, 2.5)
CONST_FLOW = (0.5, -0.25, 0.125)                            # with the identity as transform and dyadic positions: d is exactly this, everywhere
# the bridge frame, on whole-number positions (their order in the frame: build_case)
BRIDGE_A = ((2, 0), (1, 0), (2, 1), (2, -1), (1, 1), (1, -1))             # (2, 0) is one unit from the bridge point (3, 0)
BRIDGE_B = ((4, 0), (5, 0), (4, 1), (4, -1), (5, 1), (5, -1))             # (4, 0) likewise
BRIDGE_X = (3, 0)


def small_transform(rng):
    """A scan-to-scan transform of a driving sensor in float32: a yaw of a few degrees, a metre or so forward, not exactly orthonormal."""
    yaw = rng.uniform(-0.08, 0.08)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = (-rng.uniform(0.5, 1.5), rng.uniform(-0.1, 0.1), rng.uniform(-0.02, 0.02))
    return (T + 1e-4 * rng.standard_normal((4, 4)) * (np.arange(4)[:, None] < 3)).astype(f32)


def build_case(seed=9):
    """-> list of per-frame dicts: pos1 (n,3), flow, label (n,3) float32, mask (n) uint8 (predicted; 0 = moving), gt_mask (n) float32 in
    {0, 1, 0.4} (0 = moving), pred_t, gt_t (4,4) float32.  The frames (F_*):
      ONE      one point, moving                            STATIC   no moving point
      GRID     an 8 x 8 grid of whole numbers, all moving, d constant: D2 is exactly 1, 2, 4, .. -- pairs lie ON eps = 1 and eps = 2
      ALL      every point moving, a dense random cloud     OVERLAP  two objects in one box, their d 1.5 m apart; static points around
      BRIDGE   two groups of six and one point exactly 1 m from a core of each (min_points 4, eps 1: a border, and a tie), d constant
      CHAIN    300 points 0.75 m apart in index order, d constant: at eps 1 each is a neighbour of the next only
      TWINS    four positions, each twice                   MIXED    moving and static points mixed, random flows
      PAIR     two moving points 0.9 m apart                CAP      1024 points, all moving
    Where d must be constant the transform is the identity and the flow CONST_FLOW on both sides (prediction and labels)."""
    rng = np.random.default_rng(seed)
    eye = np.eye(4, dtype=f32)
    frames = []
    for f, n in enumerate(COUNTS):
        box = (40.0, 20.0, 2.0) if f == F_CAP else (12.0, 6.0, 1.0)
        pos1 = np.stack([rng.uniform(0.0, box[0], n), rng.uniform(-box[1] / 2, box[1] / 2, n), rng.uniform(-box[2] / 2, box[2] / 2, n)], axis=1).astype(f32)
        flow, label = (0.3 * rng.standard_normal((n, 3))).astype(f32), (0.3 * rng.standard_normal((n, 3))).astype(f32)
        mask = (rng.random(n) < 0.6).astype(np.uint8)
        gt_mask = rng.choice(np.array([0.0, 0.0, 1.0, 1.0, 0.4], dtype=f32), n)
        pred_t, gt_t = small_transform(rng), small_transform(rng)
        const = f in (F_GRID, F_BRIDGE, F_CHAIN)
        if f in (F_ONE, F_GRID, F_ALL, F_CHAIN, F_TWINS, F_PAIR, F_CAP):
            mask[:], gt_mask[:] = 0, 0.0
        if f == F_STATIC:
            mask[:], gt_mask[:] = 1, rng.choice(np.array([1.0, 0.4], dtype=f32), n)
        if f == F_GRID:
            pos1 = np.stack([np.arange(64) % 8, np.arange(64) // 8, np.zeros(64)], axis=1).astype(f32)
        if f == F_OVERLAP:
            k = 120
            pos1[:k] = np.stack([rng.uniform(4.0, 7.0, k), rng.uniform(-1.5, 1.5, k), rng.uniform(-0.5, 0.5, k)], axis=1)
            pos1[k:, 0] += 14.0                                             # the others: away from the box
            mask[:k], gt_mask[:k] = 0, 0.0
            pred_t, gt_t = eye, eye
            for side in (flow, label):
                side[:k] = (0.02 * rng.standard_normal((k, 3))).astype(f32)
                side[:k:2, 0] += f32(1.5)                                   # every other point of the box belongs to the faster object
        if f == F_BRIDGE:
            # index order: A's far points, then B's core (4, 0), B's far points, then A's core (2, 0), then the bridge point: A is met
            # first (instance 0), but the core that ties with the lower INDEX belongs to B (instance 1)
            special = list(BRIDGE_A[1:]) + [BRIDGE_B[0]] + list(BRIDGE_B[1:]) + [BRIDGE_A[0], BRIDGE_X]
            k = len(special)
            pos1[:, 0] += 20.0
            pos1[:k] = [(x, y, 0.0) for x, y in special]
            mask[:k], gt_mask[:k] = 0, 0.0
            mask[k:], gt_mask[k:] = 1, 1.0
            mask[k:k + 3], gt_mask[k:k + 3] = 0, 0.0                        # three stray moving points among the static ones
        if f == F_CHAIN:
            pos1 = np.stack([0.75 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1).astype(f32)
        if f == F_TWINS:
            pos1[4:] = pos1[:4]
            pos1[1] = pos1[0] + np.array([0.5, 0.0, 0.0], dtype=f32)
            pos1[5] = pos1[1]
        if f == F_PAIR:
            pos1[1] = pos1[0] + np.array([0.0, 0.9, 0.0], dtype=f32)
        if const:
            pred_t, gt_t = eye, eye
            flow[:], label[:] = CONST_FLOW, CONST_FLOW
        frames.append({"pos1": pos1, "flow": flow, "label": label, "mask": mask, "gt_mask": gt_mask, "pred_t": pred_t, "gt_t": gt_t})
    return frames


def as_items(frames, n2=8):
    """The case as the whole-frame 11-tuples of DeviceSplit.from_items (cloud 2 and the unused columns: zeros)."""
    items = []
    for fr in frames:
        n = fr["pos1"].shape[0]
        z = lambda *s: np.zeros(s, dtype=f32)
        items.append((fr["pos1"], z(n2, 3) + 1, z(n, 3), z(n2, 3), fr["gt_t"], fr["label"], fr["gt_mask"], 0.1, z(n), z(n), z(n, 2)))
    return items


def case_arrays(frames, which):
    """(off1, pos, flow, moving, T) of a case for ``cluster``: the store's side (``pred``) or the split's (``gt``)."""
    off1 = np.concatenate(([0], np.cumsum([fr["pos1"].shape[0] for fr in frames])))
    pos = np.concatenate([fr["pos1"] for fr in frames])
    if which == "pred":
        return off1, pos, np.concatenate([fr["flow"] for fr in frames]), np.concatenate([fr["mask"] for fr in frames]) == 0, \
            np.stack([fr["pred_t"] for fr in frames])
    return off1, pos, np.concatenate([fr["label"] for fr in frames]), np.concatenate([fr["gt_mask"] for fr in frames]) == 0, \
        np.stack([fr["gt_t"] for fr in frames])
