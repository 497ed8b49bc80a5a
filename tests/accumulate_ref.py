"""numpy restatement of cmflow_amd/csrc/accumulate.hip (tests/test_accumulate_host.py, tests/test_gpu_accumulate.py): the chain and
the point arithmetic in float64 with the operation order of include/cmflow_hip.h written out, so that every product and sum is one
rounded float64 operation (numpy's elementwise ``*`` and ``+`` never fuse), the capacity and offset rule, the compaction of ``drop``
and the padding behind the count -- plus the builder of the case the GPU tests share.  Nothing here imports cmflow_amd."""
import numpy as np

f32, f64 = np.float32, np.float64
MAX_WINDOW = 64
MODES = ("keep", "propagate", "drop")


def clip_starts(F, clips):
    """The first frame of every frame's clip (F,) int64; a frame outside every clip is a clip of its own."""
    start = np.arange(F, dtype=np.int64)
    for a, b in ([(0, F)] if not clips else clips):
        a, b = max(int(a), 0), min(int(b), F)
        if b > a:
            start[a:b] = a
    return start


def capacities(counts, clips, ids, window):
    """-> (ages G (nsel), cap_off (nsel+1) int64): G = min(window, id - first + 1), a target's capacity is the point count of its G
    sources, frame by frame."""
    assert 1 <= window <= MAX_WINDOW
    start = clip_starts(len(counts), clips)
    G = [min(window, int(j) - int(start[j]) + 1) for j in ids]
    cap = [sum(int(counts[j - g]) for g in range(Gj)) for j, Gj in zip(ids, G)]
    return np.array(G, dtype=np.int64), np.concatenate(([0], np.cumsum(cap))).astype(np.int64)


def chain(T, j, G):
    """[M_0 .. M_G-1], each (3,4) float64: M_0 = I, M_g = M_g-1 . T[j-g] as affine maps, entry by entry in the header's order."""
    M = np.concatenate((np.eye(3), np.zeros((3, 1))), axis=1)
    out = [M]
    for g in range(1, G):
        t = np.asarray(T[j - g]).astype(f64)
        Q = np.empty((3, 4), dtype=f64)
        for c in range(3):
            Q[:, c] = (M[:, 0] * t[0, c] + M[:, 1] * t[1, c]) + M[:, 2] * t[2, c]
        Q[:, 3] = ((M[:, 0] * t[0, 3] + M[:, 1] * t[1, 3]) + M[:, 2] * t[2, 3]) + M[:, 3]
        M = Q
        out.append(M)
    return out


def _affine(A, p):
    """(n,3): ((A[r][0] px + A[r][1] py) + A[r][2] pz) + A[r][3] for every row r, float64."""
    return np.stack([((A[r, 0] * p[:, 0] + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]) + A[r, 3] for r in range(3)], axis=1)


def accumulate(off1, pos, flow, moving, T, clips, ids, window, dynamic, rounded=True):
    """cmf_accumulate.  off1 (F+1); pos, flow (total,3); moving (total) bool; T (F,4,4); clips or None; ids: the targets.
    ``rounded``: inputs are float32 and the output is rounded to float32 (the kernel); False: inputs are used as the float64 they
    are and nothing is rounded at the end (the host test's ideal).
    -> dict off (nsel+1) int64, count (nsel) int32, xyz (R,3), src (R) int32, age (R) uint8."""
    assert dynamic in MODES
    off1 = np.asarray(off1, dtype=np.int64)
    counts = np.diff(off1)
    G, cap_off = capacities(counts, clips, ids, window)
    R = int(cap_off[-1])
    xyz = np.zeros((R, 3), dtype=f32 if rounded else f64)
    src = np.full(R, -1, dtype=np.int32)
    age = np.full(R, 255, dtype=np.uint8)
    count = np.zeros(len(ids), dtype=np.int32)
    pos = np.asarray(pos)
    if rounded:
        assert pos.dtype == f32 and np.asarray(flow).dtype == f32 and np.asarray(T).dtype == f32
    with np.errstate(all="ignore"):
        for s, j in enumerate(ids):
            j = int(j)
            M = chain(T, j, int(G[s]))
            at = int(cap_off[s])
            for g in range(int(G[s]) - 1, -1, -1):                          # oldest age first
                i = j - g
                rows = np.arange(off1[i], off1[i + 1])
                mv = np.asarray(moving[rows], dtype=bool)
                if dynamic == "drop" and g > 0:
                    rows, mv = rows[~mv], mv[~mv]                           # in the frame's own order
                p = pos[rows]
                if g == 0:
                    q = p                                                   # bit for bit
                else:
                    p = p.astype(f64)
                    q = _affine(M[g], p)
                    if dynamic == "propagate" and mv.any():
                        f = np.asarray(flow[rows]).astype(f64)
                        d = (p + f) - _affine(np.asarray(T[i]).astype(f64), p)
                        N = M[g - 1]
                        e = np.stack([(N[r, 0] * d[:, 0] + N[r, 1] * d[:, 1]) + N[r, 2] * d[:, 2] for r in range(3)], axis=1)
                        q = np.where(mv[:, None], q + f64(g) * e, q)
                n = rows.size
                xyz[at:at + n] = q
                src[at:at + n] = rows
                age[at:at + n] = g
                at += n
            count[s] = at - int(cap_off[s])
    return {"off": cap_off, "count": count, "xyz": xyz, "src": src, "age": age}


def accumulation_error(x_pred, x_gt, off, age, window):
    """accumulate.accumulation_error in numpy, straight sums: -> (mean (nsel), max (nsel), per_age (window))."""
    e = np.sqrt(((x_pred.astype(f64) - x_gt.astype(f64)) ** 2).sum(-1))
    mean, top = [], []
    for s in range(len(off) - 1):
        v = e[off[s]:off[s + 1]][age[off[s]:off[s + 1]] >= 1]
        mean.append(v.mean() if v.size else np.nan)
        top.append(v.max() if v.size else np.nan)
    per_age = [e[age == g].mean() if (age == g).any() else np.nan for g in range(window)]
    return np.array(mean), np.array(top), np.array(per_age)


def age_colors(age, window):
    """vis.age_colors in whole numbers: (n,3) uint8."""
    g = np.minimum(np.asarray(age).astype(np.int64), window)[:, None]
    blue, back = np.array([(65, 105, 225)], dtype=np.int64), np.array([(80, 80, 80)], dtype=np.int64)
    return ((blue * (window - g) + back * g) // window).astype(np.uint8)


# ---- the case of the GPU tests ----------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 256, 257, 300, 8, 97, 2, 130)      # the edges of a 64-lane wave and of a 256-thread chunk, two chunks, tiny frames
CLIPS = ((0, 7), (7, 11))
F_ALL_MOVING = 5                                            # every point of this frame is moving, in the prediction and in the labels
WINDOWS = (1, 2, 5, 8)


def small_transform(rng, exact=False):
    """A scan-to-scan transform of a driving sensor: a yaw of a few degrees, a metre or so forward; not exactly orthonormal in
    float32 unless asked (then float64, exactly rigid up to rounding)."""
    yaw, pitch = rng.uniform(-0.08, 0.08), rng.uniform(-0.01, 0.01)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = (-rng.uniform(0.5, 1.5), rng.uniform(-0.1, 0.1), rng.uniform(-0.02, 0.02))
    return T if exact else (T + 1e-4 * rng.standard_normal((4, 4)) * (np.arange(4)[:, None] < 3)).astype(f32)


def build_case(seed=5):
    """-> list of per-frame dicts: pos1 (n,3), flow, label (n,3) float32, mask (n) uint8 (predicted; 0 = moving), gt_mask (n) float32 in
    {0, 1, 0.4} (0 = moving, 0.4: neither label -- static here), pred_t, gt_t (4,4) float32."""
    rng = np.random.default_rng(seed)
    frames = []
    for f, n in enumerate(COUNTS):
        pos1 = np.stack([rng.uniform(0.0, 16.0, n), rng.uniform(-4.0, 4.0, n), rng.uniform(-1.0, 1.0, n)], axis=1).astype(f32)
        mask = (rng.random(n) < 0.7).astype(np.uint8)
        gt_mask = rng.choice(np.array([0.0, 1.0, 1.0, 0.4], dtype=f32), n)
        if f == F_ALL_MOVING:
            mask[:], gt_mask[:] = 0, 0.0
        frames.append({"pos1": pos1, "flow": (0.3 * rng.standard_normal((n, 3))).astype(f32), "label": (0.3 * rng.standard_normal((n, 3))).astype(f32),
                       "mask": mask, "gt_mask": gt_mask, "pred_t": small_transform(rng), "gt_t": small_transform(rng)})
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
    """(off1, pos, flow, moving, T) of a case for ``accumulate``: the store's side (``pred``) or the split's (``gt``)."""
    off1 = np.concatenate(([0], np.cumsum([fr["pos1"].shape[0] for fr in frames])))
    pos = np.concatenate([fr["pos1"] for fr in frames])
    if which == "pred":
        return off1, pos, np.concatenate([fr["flow"] for fr in frames]), np.concatenate([fr["mask"] for fr in frames]) == 0, \
            np.stack([fr["pred_t"] for fr in frames])
    return off1, pos, np.concatenate([fr["label"] for fr in frames]), np.concatenate([fr["gt_mask"] for fr in frames]) == 0, \
        np.stack([fr["gt_t"] for fr in frames])
