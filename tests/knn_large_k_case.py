"""Inputs shared by tests/test_gpu_knn_large_k.py and tests/test_knn_large_k_host.py: the tie-heavy grid cloud, the fp32
direct-form distance of the extension's kNN (lib/src/interpolate_gpu.cu:9-57) in numpy, and the same cloud in three orders."""
import numpy as np
import torch


def grid_cloud(N, M, seed):
    """Queries (1, N, 3) and known points (1, M, 3) on the integer grid {0, 1, 2, 3}^3: 64 distinct positions, so M = 300 known
    points are full of exact duplicates and every query sees dozens of exactly equal distances."""
    g = torch.Generator().manual_seed(seed)
    unknown = torch.randint(0, 4, (1, N, 3), generator=g).float()
    known = torch.randint(0, 4, (1, M, 3), generator=g).float()
    return unknown.contiguous(), known.contiguous()


def direct_dist2(u, p):
    """(n, 3), (m, 3) fp32 -> (n, m) fp32: dx*dx, dy*dy, dz*dz, then (xx + yy) + zz, every operation rounded on its own."""
    u, p = np.asarray(u, np.float32), np.asarray(p, np.float32)
    d = u[:, None, :] - p[None, :, :]
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def stable_knn(u, p, k):
    """The first-seen rule spelled out: a stable sort of the distances keeps the lower index ahead on ties."""
    d = direct_dist2(u, p)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, order, axis=1), order.astype(np.int32)


def ordered_clouds(M, seed):
    """One random cloud of M points as {name: (1, M, 3)} in ascending, descending and shuffled distance to the origin."""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(M, 3, generator=g) * 20.0 - 10.0)
    d = torch.from_numpy(direct_dist2(np.zeros((1, 3), np.float32), pts.numpy())[0])
    asc = pts[torch.argsort(d, stable=True)]
    return {"ascending": asc[None].contiguous(), "descending": asc.flip(0)[None].contiguous(),
            "shuffled": asc[torch.randperm(M, generator=g)][None].contiguous()}
