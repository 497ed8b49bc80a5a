"""numpy restatements of cmflow_amd/results.py's device code (tests/test_results_host.py, tests/test_gpu_results.py): packing by
plain indexing, the pose chain with the operation order of include/cmflow_hip.h written out elementwise in float64, and the
odometry metrics with np.linalg."""
import numpy as np


def pack(store, off1, frames, n1, sf, stat_cls, mask, pre_trans, gt_trans):
    """cmf_pack_results by indexing: ``store`` is a dict of numpy arrays flow (T,3), score (T), mask (T), pred_trans, gt_trans (F,4,4),
    done (F), updated in place, slot by slot; frame ids clamped to [0, F-1]."""
    F, N = len(off1) - 1, sf.shape[2]
    for s, f in enumerate(frames):
        f = min(max(int(f), 0), F - 1)
        a = int(off1[f])
        n = min(int(n1[s]), int(off1[f + 1]) - a, N)
        store["flow"][a:a + n] = sf[s, :, :n].T
        if stat_cls is not None:
            store["score"][a:a + n] = stat_cls[s, :n]
        store["mask"][a:a + n] = mask[s, :n]
        store["pred_trans"][f] = pre_trans[s]
        store["gt_trans"][f] = gt_trans[s]
        store["done"][f] = 1
    return store


def pose_chain(T, clips):
    """cmf_pose_chain: T (F,4,4) float32, clips [first, last) -> (F,4,4) float64, NaN outside every clip.  Every entry of T becomes a
    Python float (a double) and every product and sum below is one rounded float64 operation, in the header's order."""
    F = T.shape[0]
    poses = np.full((F, 4, 4), np.nan, dtype=np.float64)
    for first, last in clips:
        P = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(3)]
        for k in range(max(int(first), 0), min(int(last), F)):
            q = [[float(T[k, r, c]) for c in range(4)] for r in range(4)]
            M = [[q[0][r], q[1][r], q[2][r], -((q[0][r] * q[0][3] + q[1][r] * q[1][3]) + q[2][r] * q[2][3])] for r in range(3)]
            M.append([0.0, 0.0, 0.0, 1.0])
            P = [[((P[r][0] * M[0][c] + P[r][1] * M[1][c]) + P[r][2] * M[2][c]) + P[r][3] * M[3][c] for c in range(4)] for r in range(3)]
            poses[k, :3] = P
            poses[k, 3] = (0.0, 0.0, 0.0, 1.0)
    return poses


def rigid_inverse(T):
    """odometry_util.se3_inverse in float64: (R^T, -R^T t)."""
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def pose_chain_linalg(T, clips, inverse=rigid_inverse):
    """The same chain with ``@`` and a matrix inverse: the straightforward statement the elementwise one is checked against."""
    F = T.shape[0]
    poses = np.full((F, 4, 4), np.nan, dtype=np.float64)
    for first, last in clips:
        P = np.eye(4)
        for k in range(max(int(first), 0), min(int(last), F)):
            P = P @ inverse(T[k].astype(np.float64))
            poses[k] = P
    return poses


def odometry_metrics(P, G, clips, deltas=(1, 10)):
    """SplitResults.odometry_metrics from the two chains (F,4,4) float64 with np.linalg: per clip lists and the overall numbers, plus
    "angle_range": the smallest and largest rotation angle (degrees) of any pair, for the caller to keep its cases away from 0 and 180."""
    keys = ["end_error", "ate_rmse", "path_length"] + [k % d for d in deltas for k in ("rpe_trans_%d", "rpe_rot_%d")]
    per = {k: [] for k in keys}
    sq_all, path_all, ends = [], 0.0, []
    rpe_all = {d: ([], []) for d in deltas}
    for a, b in clips:
        a, b = max(int(a), 0), min(int(b), len(P))
        tp, tg = P[a:b, :3, 3], G[a:b, :3, 3]
        if b > a:
            sq = ((tp - tg) ** 2).sum(-1)
            per["end_error"].append(np.sqrt(sq[-1]))
            per["ate_rmse"].append(np.sqrt(sq.mean()))
            path = np.linalg.norm(np.concatenate((tg[:1], np.diff(tg, axis=0))), axis=-1).sum()
            per["path_length"].append(path)
            sq_all += sq.tolist()
            path_all += path
            ends.append(np.sqrt(sq[-1]))
        else:
            per["end_error"].append(np.nan)
            per["ate_rmse"].append(np.nan)
            per["path_length"].append(0.0)
        for d in deltas:
            tr, rot = [], []
            for k in range(a, b - d):
                E = np.linalg.inv(np.linalg.inv(G[k]) @ G[k + d]) @ (np.linalg.inv(P[k]) @ P[k + d])
                tr.append(np.linalg.norm(E[:3, 3]))
                ax = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
                rot.append(abs(np.arctan2(np.linalg.norm(ax), np.trace(E[:3, :3]) - 1.0)) * 180.0 / np.pi)
            per["rpe_trans_%d" % d].append(np.mean(tr) if tr else np.nan)
            per["rpe_rot_%d" % d].append(np.mean(rot) if rot else np.nan)
            rpe_all[d][0].extend(tr)
            rpe_all[d][1].extend(rot)
    mean = lambda v: float(np.mean(v)) if len(v) else np.nan
    overall = {"end_error": mean(ends), "ate_rmse": np.sqrt(mean(sq_all)), "path_length": path_all}
    for d in deltas:
        overall["rpe_trans_%d" % d], overall["rpe_rot_%d" % d] = mean(rpe_all[d][0]), mean(rpe_all[d][1])
    angles = [x for d in deltas for x in rpe_all[d][1]]
    return {"clips": {k: np.array(v) for k, v in per.items()}, "overall": overall, "angle_range": (min(angles), max(angles)) if angles else None}
