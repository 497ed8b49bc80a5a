"""numpy restatement of cmflow_amd/csrc/objects.hip (tests/test_objects_host.py, tests/test_gpu_objects.py): the links, the filter,
the smoother, the change of axes, the heading and the box in float64 with the operation order of include/cmflow_hip.h written out,
so that every product, sum, quotient and root is one rounded float64 operation (numpy's elementwise ``*`` ``+`` ``/`` never fuse); a
second, differently written smoother (the MAP estimate by least squares over the stacked whitened residuals of a track) that must
agree with it; a small world of its own whose answer is known without either; and the corrupted tables the entry point is called
with.  Nothing here imports cmflow_amd."""
import numpy as np

import results_ref as rref
import tracks_ref as tref

f32, f64 = np.float32, np.float64
MAX_LIVE, MAX_GAP = tref.MAX_LIVE, tref.MAX_GAP
INT_KEYS = ("row_frame", "next_row", "heading_src")
F64_KEYS = ("filt", "fcov", "state", "scov")
F32_KEYS = ("pos", "vel", "heading", "box_center", "box_size")
KEYS = ("row_frame", "next_row", "filt", "fcov", "state", "scov", "pos", "vel", "heading", "heading_src", "box_center", "box_size")   # the entry point's order
WIDTH = {"row_frame": 0, "next_row": 0, "heading_src": 0, "filt": 6, "state": 6, "fcov": 3, "scov": 3, "pos": 3, "vel": 3, "heading": 2,
         "box_center": 3, "box_size": 3}
FILL = {"row_frame": -1, "next_row": -1, "heading_src": -1}     # what ``estimate`` fills its outputs with; every other array: 0
PARAMS = (0.5, 0.25, 0.25, 0.05)                                 # sigma_pos, sigma_disp, sigma_acc, min_disp: the defaults of ``estimate``


def dtype_of(k):
    return np.int32 if k in INT_KEYS else f64 if k in F64_KEYS else f32


def outputs(rows, fill=FILL):
    """The outputs of cmf_track_states, ``rows`` rows, filled: -> dict."""
    return {k: np.full((rows, WIDTH[k]) if WIDTH[k] else rows, fill.get(k, 0), dtype_of(k)) for k in KEYS}


def _scan1_pose(poses, f, first):
    """W_f: the upper three rows of poses[f-1]; the identity as numbers at the clip's first frame."""
    return np.eye(4, dtype=f64)[:3] if f == first else poses[f - 1, :3]


def _gap(g):
    return f64(min(max(int(g), 1), MAX_GAP + 1))


def _predict(g, q, p, v, a, b, c):
    pm = p + g * v
    am = (a + g * ((f64(2.0) * b) + g * c)) + (q * ((g * g) * g)) / f64(3.0)
    bm = (b + g * c) + (q * (g * g)) / f64(2.0)
    cm = c + q * g
    return pm, am, bm, cm


def measure(poses, first, f, c, d):
    """zp, zd of the header: the float32 centroid and displacement of a row of frame f in the clip's axes."""
    W, A = _scan1_pose(poses, f, first), poses[f, :3]
    c, d = c.astype(f64), d.astype(f64)
    zp = ((W[:, 0] * c[0] + W[:, 1] * c[1]) + W[:, 2] * c[2]) + W[:, 3]
    zd = (A[:, 0] * d[0] + A[:, 1] * d[1]) + A[:, 2] * d[2]
    return zp, zd


def clip_rows(off1, total, count, first, end):
    """The frames of a clamped clip as cmf_track_instances walks them -> (base, [(f, start, n, K)]); a frame that owns no rows: n = K = 0."""
    base = int(off1[first])
    clip_ok = 0 <= base <= total
    top, rows = base, []
    for f in range(first, end):
        s, e = int(off1[f]), int(off1[f + 1])
        owns = clip_ok and s >= top and e >= s and e <= total
        n = e - s if owns else 0
        if owns:
            top = e
        K = min(max(int(count[f]), 0), n, MAX_LIVE) if owns else 0
        rows.append((f, s if owns else 0, n, K))
    return base, rows


def states(off1, total, count, label, centroid, disp, track, prev_row, gap, tab1, poses, clips, sigma_pos, sigma_disp, sigma_acc, min_disp, out=None):
    """cmf_track_states -> dict of the outputs (``out``: arrays to write into, e.g. sentinel-filled ones; default: ``outputs`` with the
    fills of cmflow_amd.objects.estimate).  rp, rd, q, min_disp2 are formed as the host forms them."""
    off1 = np.asarray(off1, dtype=np.int64)
    F, total = len(off1) - 1, int(total)
    assert centroid.dtype == f32 and disp.dtype == f32 and tab1.dtype == f32 and poses.dtype == f64
    poses = poses.reshape(F, 4, 4)
    rp, rd = f64(float(sigma_pos) * float(sigma_pos)), f64(float(sigma_disp) * float(sigma_disp))
    q, min_disp2 = f64(float(sigma_acc) * float(sigma_acc)), f64(float(min_disp) * float(min_disp))
    out = outputs(total) if out is None else out
    with np.errstate(all="ignore"):
        for first, end in np.asarray(clips, dtype=np.int64).reshape(-1, 2):
            first = min(max(int(first), 0), F)
            end = min(max(int(end), first), F)
            N = end - first
            base, rows = clip_rows(off1, total, count, first, end)
            # ---- 1. links and fills
            for at, (f, start, n, K) in enumerate(rows):
                for j in range(K):
                    row, nxt = start + j, -1
                    for f2, start2, n2, K2 in rows[at + 1:at + 2 + MAX_GAP]:
                        hit = np.flatnonzero((prev_row[start2:start2 + K2] == row) & (track[start2:start2 + K2] == track[row]))   # ascending
                        if hit.size:
                            nxt = start2 + int(hit[0])
                            break
                    out["row_frame"][row], out["next_row"][row] = f, nxt
                for k in KEYS:
                    out[k][start + K:start + n] = FILL.get(k, 0)
            # ---- 2. chains
            for f, start, n, K in rows:
                for j in range(K):
                    head = start + j
                    before = int(prev_row[head])
                    if base <= before < start and out["next_row"][before] == head:
                        continue
                    k, steps = head, 0
                    while True:
                        fk = f if steps == 0 else min(max(int(out["row_frame"][k]), first), end - 1)
                        zp, zd = measure(poses, first, fk, centroid[k], disp[k])
                        if steps == 0:
                            p, v, a, b, c = zp, zd, rp, f64(0.0), rd
                        else:
                            g = _gap(gap[k])
                            pm, am, bm, cm = _predict(g, q, p, v, a, b, c)
                            s11, s12, s22 = am + rp, bm, cm + rd
                            det = s11 * s22 - s12 * s12
                            k11, k12 = (am * s22 - bm * s12) / det, (bm * s11 - am * s12) / det
                            k21, k22 = (bm * s22 - cm * s12) / det, (cm * s11 - bm * s12) / det
                            ep, ev = zp - pm, zd - v
                            p, v = pm + (k11 * ep + k12 * ev), v + (k21 * ep + k22 * ev)
                            a, b, c = am - (k11 * am + k12 * bm), bm - (k11 * bm + k12 * cm), cm - (k21 * bm + k22 * cm)
                        out["filt"][k, :3], out["filt"][k, 3:], out["fcov"][k] = p, v, (a, b, c)
                        steps += 1
                        nk = int(out["next_row"][k])
                        if nk <= k or nk >= total or steps >= N:
                            break
                        k = nk
                    out["state"][k, :3], out["state"][k, 3:], out["scov"][k] = p, v, (a, b, c)
                    for _ in range(steps - 1):
                        jrow = int(prev_row[k])
                        if jrow < base or jrow >= k:
                            break
                        g = _gap(gap[k])
                        fp, fv = out["filt"][jrow, :3].copy(), out["filt"][jrow, 3:].copy()
                        fa, fb, fc = out["fcov"][jrow]
                        pm, am, bm, cm = _predict(g, q, fp, fv, fa, fb, fc)
                        m11, m12, m21, m22 = fa + g * fb, fb, fb + g * fc, fc
                        dm = am * cm - bm * bm
                        c11, c12 = (m11 * cm - m12 * bm) / dm, (m12 * am - m11 * bm) / dm
                        c21, c22 = (m21 * cm - m22 * bm) / dm, (m22 * am - m21 * bm) / dm
                        dp, dv = p - pm, v - fv
                        p, v = fp + (c11 * dp + c12 * dv), fv + (c21 * dp + c22 * dv)
                        da, db, dc = a - am, b - bm, c - cm
                        e11, e12, e21, e22 = c11 * da + c12 * db, c11 * db + c12 * dc, c21 * da + c22 * db, c21 * db + c22 * dc
                        a, b, c = fa + (e11 * c11 + e12 * c12), fb + (e11 * c21 + e12 * c22), fc + (e21 * c21 + e22 * c22)
                        k = jrow
                        out["state"][k, :3], out["state"][k, 3:], out["scov"][k] = p, v, (a, b, c)
            # ---- 3. the frame's axes, the heading, the box
            for f, start, n, K in rows:
                W = _scan1_pose(poses, f, first)
                for j in range(K):
                    row = start + j
                    x, v = out["state"][row, :3].copy(), out["state"][row, 3:].copy()
                    ti = -((W[0, :3] * W[0, 3] + W[1, :3] * W[1, 3]) + W[2, :3] * W[2, 3])
                    P = ((W[0, :3] * x[0] + W[1, :3] * x[1]) + W[2, :3] * x[2]) + ti
                    V = (W[0, :3] * v[0] + W[1, :3] * v[1]) + W[2, :3] * v[2]
                    out["pos"][row], out["vel"][row] = P.astype(f32), V.astype(f32)
                    s2 = V[0] * V[0] + V[1] * V[1]
                    if s2 >= min_disp2 and s2 > 0.0:
                        s = np.sqrt(s2)
                        out["heading"][row], out["heading_src"][row] = (f32(V[0] / s), f32(V[1] / s)), 1
                    else:
                        out["heading"][row], out["heading_src"][row] = (f32(1.0), f32(0.0)), 0
                    hx, hy = f64(out["heading"][row, 0]), f64(out["heading"][row, 1])
                    cen = centroid[row]
                    c0, c1 = f64(cen[0]), f64(cen[1])
                    first_member = True
                    for i in np.flatnonzero(label[start:start + n] == j):       # the members, ascending
                        pt = tab1[start + i]
                        dx, dy = f64(pt[0]) - c0, f64(pt[1]) - c1
                        ai, bi, z = hx * dx + hy * dy, (-hy) * dx + hx * dy, pt[2]
                        if first_member:
                            first_member, amin, amax, bmin, bmax, lo, hi = False, ai, ai, bi, bi, z, z
                            continue
                        amin, amax = (ai if ai < amin else amin), (ai if ai > amax else amax)
                        bmin, bmax = (bi if bi < bmin else bmin), (bi if bi > bmax else bmax)
                        lo, hi = (z if z < lo else lo), (z if z > hi else hi)
                    if first_member:
                        out["box_size"][row], out["box_center"][row] = 0.0, cen
                    else:
                        ma, mb = (amin + amax) / f64(2.0), (bmin + bmax) / f64(2.0)
                        out["box_size"][row] = (f32(amax - amin), f32(bmax - bmin), f32(f64(hi) - f64(lo)))
                        out["box_center"][row] = (f32(c0 + (ma * hx - mb * hy)), f32(c1 + (ma * hy + mb * hx)), f32((f64(lo) + f64(hi)) / f64(2.0)))
    return out


def same(got, want, what=""):
    """Exact: integers equal, float32 arrays as uint32, float64 arrays as uint64; a NaN equals a NaN whatever its sign and payload."""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype == dtype_of(k), (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if k in INT_KEYS:
            differ = g != w
        else:
            bits = np.uint32 if k in F32_KEYS else np.uint64
            differ = (g.view(bits) != w.view(bits)) & ~(np.isnan(g) & np.isnan(w))
        bad = np.argwhere(differ)
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def chains(out, total):
    """The chains the links of ``out`` describe: lists of rows in frame order, one per row that is nobody's next_row."""
    held = np.flatnonzero(out["row_frame"][:total] >= 0)
    nxt = out["next_row"]
    followers = set(int(nxt[r]) for r in held if nxt[r] >= 0)
    found = []
    for r in held:
        if int(r) in followers:
            continue
        chain = [int(r)]
        while nxt[chain[-1]] >= 0:
            chain.append(int(nxt[chain[-1]]))
        found.append(chain)
    return found


# ---- the smoother a second time: the MAP estimate by least squares ------------------------------------------------------------------------
def smooth_lstsq(zp, zd, gaps, sigma_pos, sigma_disp, sigma_acc):
    """One axis of one track: zp, zd (m) the measured positions and displacements of its matches, gaps (m-1) the frames between
    them.  The smoothed (p_k, v_k) maximise the posterior, i.e. minimise the stacked whitened residuals
        (zp_k - p_k) / sigma_pos,   (zd_k - v_k) / sigma_disp,   L_k^-1 ((p_k+1, v_k+1) - F_k (p_k, v_k)),   L_k L_k^T = Q(g_k)
    with F = [[1, g], [0, 1]] and Q = sigma_acc^2 [[g^3/3, g^2/2], [g^2/2, g]] -- solved with numpy.linalg.lstsq in float64.
    -> (x (m,2), cov (m,3): the smoothed P_pp, P_pv, P_vv from the inverse of the normal matrix)."""
    m = len(zp)
    rows, rhs = [], []
    for k in range(m):
        for col, z, s in ((0, zp[k], sigma_pos), (1, zd[k], sigma_disp)):
            r = np.zeros(2 * m)
            r[2 * k + col] = 1.0 / s
            rows.append(r)
            rhs.append(z / s)
    for k in range(m - 1):
        g = float(gaps[k])
        Q = sigma_acc ** 2 * np.array([[g ** 3 / 3.0, g ** 2 / 2.0], [g ** 2 / 2.0, g]])
        Li = np.linalg.inv(np.linalg.cholesky(Q))
        block = np.zeros((2, 2 * m))
        block[:, 2 * k:2 * k + 2] = -Li @ np.array([[1.0, g], [0.0, 1.0]])
        block[:, 2 * k + 2:2 * k + 4] = Li
        rows.extend(block)
        rhs.extend([0.0, 0.0])
    A, y = np.array(rows), np.array(rhs)
    x = np.linalg.lstsq(A, y, rcond=None)[0].reshape(m, 2)
    cov = np.linalg.inv(A.T @ A)
    return x, np.array([[cov[2 * k, 2 * k], cov[2 * k, 2 * k + 1], cov[2 * k + 1, 2 * k + 1]] for k in range(m)])


# ---- a world whose answer is known without a filter ---------------------------------------------------------------------------------------
WORLD_CLIPS = ((0, 11), (11, 18))
WORLD_OBJECTS = 6
SLOW, ONCE, ABSENT = 4, 5, 1                                # the slow object, the one seen once, the one absent for two frames
ABSENT_FRAMES, ONCE_FRAME = (3, 4), 6                       # of the first clip (the second clip: ONCE is never seen, nobody is absent)
GATE, EPS = 2.0, 2.0
QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _pose(g, exact):
    """The sensor's pose at scan g of a clip.  exact: a quarter turn per frame and dyadic steps -- every coordinate of the world is
    then a dyadic rational that float32 holds exactly; otherwise 0.03 rad per frame."""
    if exact:
        return np.linalg.matrix_power(QUARTER, g % 4).round(), np.array([1.0 * g, 0.125 * g, 0.0])
    yaw = 0.03 * g
    return np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]), np.array([1.0 * g, 0.1 * g, 0.0])


def build_world(seed=7, exact=False, flow_noise=0.0):
    """Six rigid objects at constant velocity in the clip's axes seen from a sensor that drives and turns, two clips of 11 and 7
    frames, at most 40 points a frame -> (frames, owners, truth): ``frames`` in the format of instances_ref.build_case, ``owners`` per
    frame the generating object of every point (-1: clutter), ``truth`` per clip (centre (K,3) at the clip's first scan, velocity
    (K,3) per frame), both in the clip's axes -- an object's instance has the centroid centre + g * velocity at frame g.
    Every object is a blob of 4 .. 6 points (4 when exact) within 0.5 m of its centre, the objects keep more than 3 gates apart; the
    point order is shuffled anew in every frame.  Object SLOW moves 1/64 m a frame, below min_disp; ONCE is called moving in one frame
    of the first clip only; ABSENT is called static for two frames of the first clip (a gap of 3).  Both sources (prediction and
    labels) see the same; the prediction's flow carries ``flow_noise`` metres of noise.  The transforms are the true ego-motion.
    exact: every position, flow and transform is a dyadic rational exactly held in float32, so centroids, displacements and poses
    carry no rounding at all and the measurements ARE the truth."""
    rng = np.random.default_rng(seed)
    frames, owners, truth = [], [], []
    for first, end in WORLD_CLIPS:
        if exact:
            shape = [rng.integers(-8, 9, (4, 3)) / 16.0 for _ in range(WORLD_OBJECTS)]
            vel = [np.array([rng.choice([-1, 1]) * rng.integers(4, 17) / 16.0, rng.integers(-3, 4) / 16.0, 0.0]) for _ in range(WORLD_OBJECTS)]
        else:
            shape = [rng.uniform(-0.5, 0.5, (int(rng.integers(4, 7)), 3)) for _ in range(WORLD_OBJECTS)]
            vel = [np.array([rng.choice([-1, 1]) * rng.uniform(0.25, 1.0), rng.uniform(-0.2, 0.2), 0.0]) for _ in range(WORLD_OBJECTS)]
        vel[SLOW] = np.array([1.0 / 64, 0.0, 0.0])
        start = [np.array([12.0 + 3.0 * k, -24.0 + 12.0 * k, 0.25 * k]) for k in range(WORLD_OBJECTS)]
        clutter = np.stack([rng.integers(0, 40, 4), rng.integers(-30, 30, 4), rng.integers(-1, 2, 4)], axis=1).astype(f64)
        truth.append((np.stack([start[k] + shape[k].mean(axis=0) for k in range(WORLD_OBJECTS)]), np.stack(vel)))
        for g in range(end - first):
            (R0, t0), (R1, t1) = _pose(g, exact), _pose(g + 1, exact)
            world0 = [start[k] + g * vel[k] + shape[k] for k in range(WORLD_OBJECTS)] + [clutter]
            world1 = [start[k] + (g + 1) * vel[k] + shape[k] for k in range(WORLD_OBJECTS)] + [clutter]
            p0 = np.concatenate([(w - t0) @ R0 for w in world0])             # rows: R^T (w - t)
            p1 = np.concatenate([(w - t1) @ R1 for w in world1])
            own = np.concatenate([np.full(len(w), k if k < WORLD_OBJECTS else -1) for k, w in enumerate(world0)])
            order = rng.permutation(len(p0))
            p0, p1, own = p0[order], p1[order], own[order]
            Tm = np.eye(4)
            Tm[:3, :3], Tm[:3, 3] = R1.T @ R0, R1.T @ (t0 - t1)
            pos1, label = p0.astype(f32), (p1 - p0).astype(f32)
            flow = (p1 - p0 + flow_noise * rng.standard_normal(p0.shape)).astype(f32)
            static = own < 0
            if first == 0:
                static |= (own == ABSENT) & (g in ABSENT_FRAMES)
                static |= (own == ONCE) & (g != ONCE_FRAME)
            else:
                static |= own == ONCE
            frames.append({"pos1": pos1, "flow": flow, "label": label, "mask": static.astype(np.uint8), "gt_mask": static.astype(f32),
                           "pred_t": Tm.astype(f32), "gt_t": Tm.astype(f32)})
            owners.append(own)
            if exact:
                assert np.array_equal(pos1.astype(f64), p0) and np.array_equal(label.astype(f64), p1 - p0) and np.array_equal(Tm.astype(f32).astype(f64), Tm)
    return frames, owners, truth


def world_tables(frames, which, sigma=0.0, seed=0, gate=GATE, max_gap=2):
    """The world clustered and tracked by the restatements of cmf_cluster_moving and cmf_track_instances, the poses by the one of
    cmf_pose_chain -> dict of the arguments of ``states`` (tab1: the positions alone, ld 3).  ``sigma``: seeded Gaussian noise of
    that many metres added to the centroids AFTER tracking, so the tracks are those of the clean world."""
    off1, total, count, label, centroid, disp, T = tref.world_tables(frames, which, EPS)
    trk = tref.track(off1, total, count, label, centroid, disp, T, WORLD_CLIPS, gate, max_gap)
    if sigma:
        centroid = (centroid.astype(f64) + sigma * np.random.default_rng(seed).standard_normal(centroid.shape)).astype(f32)
    poses = rref.pose_chain(T.reshape(-1, 4, 4), WORLD_CLIPS).reshape(-1, 16)
    return {"off1": np.asarray(off1), "total": total, "count": count, "label": label, "centroid": centroid, "disp": disp, "track": trk["track"],
            "prev_row": trk["prev_row"], "gap": trk["gap"], "tab1": np.concatenate([fr["pos1"] for fr in frames]), "poses": poses,
            "clips": np.array(WORLD_CLIPS, dtype=np.int32), "T": T.reshape(-1, 4, 4)}


def run(t, params=PARAMS, out=None, **change):
    """``states`` on a dict of tables as ``world_tables`` returns it; ``change`` replaces entries (total, count, clips, ...)."""
    t = dict(t, **change)
    return states(t["off1"], t["total"], t["count"], t["label"], t["centroid"], t["disp"], t["track"], t["prev_row"], t["gap"], t["tab1"], t["poses"],
                  t["clips"], *params, out=out)


def row_owner(t, owners):
    """(total) int: the generating object of every instance row (-1 where the row holds no instance): the owner of its member points."""
    off1, total = t["off1"], t["total"]
    who = np.full(total, -1)
    for f, own in enumerate(owners):
        a = int(off1[f])
        for c in range(int(t["count"][f])):
            ids = set(own[t["label"][a:int(off1[f + 1])] == c].tolist())
            assert len(ids) == 1                                             # an instance is one object
            who[a + c] = ids.pop()
    return who


def row_truth(t, owners, truth):
    """(total,6) float64: the true (position, velocity) in the clip's axes of every instance row, NaN elsewhere."""
    who = row_owner(t, owners)
    want = np.full((t["total"], 6), np.nan)
    for (first, end), (centre, vel) in zip(WORLD_CLIPS, truth):
        for f in range(first, end):
            a = int(t["off1"][f])
            for c in range(int(t["count"][f])):
                k = who[a + c]
                want[a + c] = np.concatenate([centre[k] + (f - first) * vel[k], vel[k]])
    return want


# ---- corrupted tables for the entry point -----------------------------------------------------------------------------------------------
def corrupt_tables(t, seed=2):
    """The world's tables with everything the entry point has to bound itself against -> (tables, clips, total): ``prev_row`` garbage
    (far outside the tables on either side, rows behind a frame's K, later rows) and a two-cycle, ``gap`` 0 and 99, a NaN centroid,
    a count far beyond a frame's rows; the clips: one reaching behind F, an empty one, a one-frame one; ``total`` cut inside the
    last frame, which therefore owns no rows."""
    rng = np.random.default_rng(seed)
    t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}
    off1, F = t["off1"], len(t["count"])
    held = np.flatnonzero(t["track"] >= 0)
    late = held[t["prev_row"][held] >= 0]
    bad = rng.choice(late, 12, replace=False)
    t["prev_row"][bad[:8]] = [2 ** 31 - 1, -2 ** 31, -5, t["total"] + 3, int(off1[3]) - 1, int(off1[F]) - 1, int(bad[0]), int(off1[2]) + 30]
    a, b = int(late[5]), int(late[-5])                                      # a two-cycle: each the other's predecessor
    t["prev_row"][a], t["prev_row"][b] = b, a
    t["gap"][bad[8]], t["gap"][bad[9]], t["gap"][bad[10]] = 0, 99, -7
    t["centroid"][bad[11], 1] = np.nan
    t["centroid"][held[3], 0] = np.inf
    t["count"][5] = 5000
    clips = np.array([(14, F + 9), (4, 4), (3, 4), (4, 14), (-3, 3)], dtype=np.int32)
    return t, clips, int(off1[F - 1]) + 2
