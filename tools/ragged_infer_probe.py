"""Inference on whole frames of their own sizes -- the reference's test protocol (main.py:203: batch_size = 1; dataset/vod.py:92-111
resamples for training only) -- two ways, in frames per second:

  (a) one CMFlow.forward per frame pair at B = 1 on the truncated clouds (N1 != N2): what the dense interface allows;
  (b) CMFlow.forward_ragged over B = 8 / 16 / 64 pairs padded to the batch's largest clouds, with per-sample counts.

Frames are synthetic, with the sizes dataset.write_synthetic_split uses (180-400 points in cloud 1, cloud 2 a few points off).  Every
variant is warmed up on all the shapes it will see, every timed region ends in a device synchronise, the regions of the variants
alternate inside each repeat, and the table gives the median and the spread (min - max) over the repeats.

    python tools/ragged_infer_probe.py [frames=64] [repeats=7] > profiles/ragged_infer_probe.txt
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from cmflow_amd import synth
from cmflow_amd.cmflow import CMFlow

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 64
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
net = CMFlow(bench.Args())
net.load_state_dict(bench.load_weights("cmflow"))
net = net.to(dev).eval()

g = torch.Generator().manual_seed(0)
n1 = torch.randint(180, 401, (frames,), generator=g)
n2 = (n1 + torch.randint(-33, 38, (frames,), generator=g)).clamp(min=8)
nmax = int(max(n1.max(), n2.max()))
pool = synth.make_batch(frames, nmax, seed=4)
KEYS = ("pc1", "pc2", "ft1", "ft2")
singles = []
for i in range(frames):
    a, b = int(n1[i]), int(n2[i])
    singles.append(tuple(pool[k][i:i + 1, :, :(a if k.endswith("1") else b)].contiguous().to(dev) for k in KEYS))


def batches(B):
    out = []
    for s in range(0, frames, B):
        sl = slice(s, min(frames, s + B))
        m1, m2 = int(n1[sl].max()), int(n2[sl].max())
        t = [pool[k][sl, :, :(m1 if k.endswith("1") else m2)].contiguous().to(dev) for k in KEYS]
        out.append((*t, n1[sl].to(dev, torch.int32), n2[sl].to(dev, torch.int32)))
    return out


def run_single():
    for s in singles:
        net(*s, None, "test")


def run_ragged(bs):
    for b in bs:
        net.forward_ragged(*b)


variants = [("forward, B = 1 per frame", run_single)]
for B in (8, 16, 64):
    if B <= frames:
        variants.append(("forward_ragged, B = %d" % B, (lambda bs: (lambda: run_ragged(bs)))(batches(B))))

times = {name: [] for name, _ in variants}
with torch.no_grad():
    for name, fn in variants:                       # warm-up: every shape of every variant, twice
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)

print("ragged inference probe: %d frame pairs, %d-%d points in cloud 1, %d-%d in cloud 2; %d repeats, variants alternating; %s"
      % (frames, int(n1.min()), int(n1.max()), int(n2.min()), int(n2.max()), repeats, torch.cuda.get_device_name(0)))
print("%-28s %12s %22s %14s" % ("variant", "frames/s", "spread (min - max)", "ms per frame"))
base = None
for name, _ in variants:
    fps = sorted(frames / t for t in times[name])
    med = statistics.median(fps)
    base = base or med
    print("%-28s %12.0f %10.0f - %-9.0f %14.3f   x%.2f" % (name, med, fps[0], fps[-1], 1e3 / med, med / base))
