"""Training on whole frames of their own sizes under eval-mode BatchNorm (the reference's regime after its first epoch) two ways, in
frames per second:

  (a) one step per frame at B = 1 on the cropped clouds (N1 != N2) through the dense model: make_labels -> forward(..., 'train') ->
      the loss -> backward -> Adam, what the dense interface allows (the dense loss kernel takes one N for both clouds, so the loss of
      such a frame goes through the counted kernel at B = 1);
  (b) TrainStep.step_ragged over B = 8 / 16 / 64 frames padded to the batch's largest clouds, with per-sample counts.

Every variant owns a copy of the network and its optimizer (a step changes the weights), is warmed up on all the shapes it will see,
every timed region ends in a device synchronise, the regions of the variants alternate inside each repeat, and the table gives the
median and the spread (min - max) over the repeats.  The variants do different arithmetic (B steps of one frame against one step on the
mean over B frames): the figure is frames consumed per second, not a like-for-like kernel comparison.

    python tools/ragged_train_probe.py [frames=64] [repeats=7] > profiles/ragged_train_probe.txt
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
from cmflow_amd.fused_blocks import join_side_streams
from cmflow_amd.losses import make_labels
from cmflow_amd.train import TrainStep

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 64
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
weights = bench.load_weights("cmflow")


def new_step():
    net = CMFlow(bench.Args())
    net.load_state_dict(weights)
    return TrainStep(net.to(dev).eval(), vr_thres=0.3)


g = torch.Generator().manual_seed(0)
n1 = torch.randint(180, 401, (frames,), generator=g)
n2 = (n1 + torch.randint(-33, 38, (frames,), generator=g)).clamp(min=9)
nmax = int(max(n1.max(), n2.max()))
pool = synth.make_batch(frames, nmax, seed=4, train_extras=True)
C1, C2 = ("pc1", "ft1"), ("pc2", "ft2")
ROWS = ("flow_label", "fg_mask", "radar_u", "radar_v", "opt_flow")


def crop(sl, m1, m2):
    out = {}
    for k, v in pool.items():
        v = v[sl]
        if k in C1:
            v = v[:, :, :m1]
        elif k in C2:
            v = v[:, :, :m2]
        elif k in ROWS:
            v = v[:, :m1]
        out[k] = v.contiguous().to(dev)
    return out


singles = [(crop(slice(i, i + 1), int(n1[i]), int(n2[i])), n1[i:i + 1].to(dev, torch.int32), n2[i:i + 1].to(dev, torch.int32))
           for i in range(frames)]


def batches(B):
    out = []
    for s in range(0, frames, B):
        sl = slice(s, min(frames, s + B))
        b = crop(sl, int(n1[sl].max()), int(n2[sl].max()))
        b["n1"], b["n2"] = n1[sl].to(dev, torch.int32), n2[sl].to(dev, torch.int32)
        out.append(b)
    return out


def run_single(step):
    for b, c1, c2 in singles:
        dyn, mseg = make_labels(b, step.vr_thres)
        o = step.net(b["pc1"], b["pc2"], b["ft1"], b["ft2"], mseg, "train")
        loss = step.loss_obj.forward_ragged(b["pc1"], b["pc2"], o[0], b["ft1"][:, 0], c1, c2, b["flow_label"].transpose(2, 1), o[2], o[1],
                                            b["gt_trans"], mseg, dyn, b["radar_u"], b["radar_v"], b["opt_flow"])[0]
        step.bucket.zero()
        loss.backward()
        join_side_streams()
        step.bucket.all_reduce_mean()
        step.opt.step()


def run_ragged(step, bs):
    for b in bs:
        step.step_ragged(b)


variants = [("dense step, B = 1 per frame", (lambda st: (lambda: run_single(st)))(new_step()))]
for B in (8, 16, 64):
    if B <= frames:
        variants.append(("step_ragged, B = %d" % B, (lambda st, bs: (lambda: run_ragged(st, bs)))(new_step(), batches(B))))

times = {name: [] for name, _ in variants}
for name, fn in variants:                           # warm-up: every shape of every variant, twice
    fn(); fn()
torch.cuda.synchronize()
for _ in range(repeats):
    for name, fn in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t0)

print("ragged training probe (eval-mode BatchNorm): %d frames, %d-%d points in cloud 1, %d-%d in cloud 2; %d repeats, variants "
      "alternating; %s" % (frames, int(n1.min()), int(n1.max()), int(n2.min()), int(n2.max()), repeats, torch.cuda.get_device_name(0)))
print("%-28s %12s %22s %14s" % ("variant", "frames/s", "spread (min - max)", "ms per frame"))
base = None
for name, _ in variants:
    fps = sorted(frames / t for t in times[name])
    med = statistics.median(fps)
    base = base or med
    print("%-28s %12.0f %10.0f - %-9.0f %14.3f   x%.2f" % (name, med, fps[0], fps[-1], 1e3 / med, med / base))
