"""The extension kNN (cmf_knn_points, behind knn_wrapper / pointnet2_utils.knn) past k = 64 -- the wave-per-query kernel
knn_wave_kernel of csrc/neighbor.hip -- in milliseconds per call at (b, n, m) = (8, 4096, 4096), k = 65 / 128 / 200, beside

  (a) the register-list kernel knn_kernel<64, true> at k = 64 on the same input (the largest list the older form takes);
  (b) torch.cdist + torch.topk(largest=False) on the same device at the same k (matmul-form distances and no first-seen tie
      rule: not a replacement, a reader's yardstick for the speed only).

Every variant is warmed up, a timed region is `calls` back-to-back calls ending in a device synchronise, the regions of the variants
alternate inside each repeat, and the table gives the median and the spread (min - max) over the repeats.  Before timing, the
lists of the wave kernel are checked against a stable sort of cdist-free fp32 direct-form distances on a slice of the input.

    python tools/knn_large_k_probe.py [calls=10] [repeats=7] > profiles/knn_large_k_probe.txt
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmflow_amd import synth
from cmflow_amd.pointnet2_utils import knn_wrapper

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
B, N, M = 8, 4096, 4096
dev = torch.device("cuda:0")
batch = synth.make_batch(B, N=max(N, M), seed=7)
unknown = batch["pc1"].permute(0, 2, 1)[:, :N].contiguous().to(dev)
known = batch["pc2"].permute(0, 2, 1)[:, :M].contiguous().to(dev)


def ours(k):
    d2 = torch.empty(B, N, k, device=dev)
    idx = torch.empty(B, N, k, dtype=torch.int32, device=dev)
    return lambda: knn_wrapper(B, N, M, k, unknown, known, d2, idx) and (d2, idx)


def torch_pair(k):
    return lambda: torch.topk(torch.cdist(unknown, known), k, dim=2, largest=False)


# the lists being timed are the right ones: first 64 queries of sample 0 against a stable sort of the direct-form distances
for k in (65, 128, 200):
    d2, idx = ours(k)()
    u, p = unknown[0, :64], known[0]
    diff = u[:, None, :] - p[None, :, :]
    sq = diff * diff
    dd = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    order = torch.sort(dd, dim=1, stable=True).indices[:, :k]
    assert torch.equal(idx[0, :64].long(), order), "k = %d: lists differ from a stable sort" % k
    assert torch.equal(d2[0, :64], torch.gather(dd, 1, order)), "k = %d: distances differ" % k

variants = [("knn_kernel<64> (registers), k = 64", ours(64))]
for k in (65, 128, 200):
    variants.append(("knn_wave_kernel, k = %d" % k, ours(k)))
for k in (64, 65, 128, 200):
    variants.append(("cdist + topk, k = %d" % k, torch_pair(k)))

times = {name: [] for name, _ in variants}
with torch.no_grad():
    for name, fn in variants:                       # warm-up
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _c in range(calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls)

print("extension kNN probe: (b, n, m) = (%d, %d, %d); %d calls per region, %d repeats, variants alternating; %s"
      % (B, N, M, calls, repeats, torch.cuda.get_device_name(0)))
print("%-38s %12s %24s %10s" % ("variant", "ms per call", "spread (min - max)", "vs k = 64"))
base = None
for name, _ in variants:
    ms = sorted(1e3 * t for t in times[name])
    med = statistics.median(ms)
    base = base or med
    print("%-38s %12.3f %11.3f - %-10.3f %9.2fx" % (name, med, ms[0], ms[-1], med / base))
