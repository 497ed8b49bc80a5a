"""The loss on whole frames of their own sizes, two ways, in frames per second:

  (a) make_labels + RadarFlowLoss.forward per frame at B = 1 with cloud 2 cropped / the frame cropped to min(n1, n2) points: what the
      dense interface allows (one N for both clouds) -- a different quantity, timed as the cost of the workaround;
  (b) make_labels_ragged + RadarFlowLoss.forward_ragged over B = 8 / 16 / 64 frames padded to the batch's largest clouds.

Both with gradient outputs (the network outputs require grad; backward itself only scales saved buffers and is not timed).  Frames are
synthetic with the sizes of tools/ragged_infer_probe.py; every variant is warmed up on all the shapes it will see, every timed region
ends in a device synchronise, the regions of the variants alternate inside each repeat, and the table gives the median and the spread
(min - max) over the repeats.

    python tools/ragged_loss_probe.py [frames=64] [repeats=7] > profiles/ragged_loss_probe.txt
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmflow_amd import synth
from cmflow_amd.losses import RadarFlowLoss, make_labels, make_labels_ragged

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 64
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)

g = torch.Generator().manual_seed(0)
n1 = torch.randint(180, 401, (frames,), generator=g)
n2 = (n1 + torch.randint(-33, 38, (frames,), generator=g)).clamp(min=8)
nmax = int(max(n1.max(), n2.max()))
pool = synth.make_batch(frames, nmax, seed=4, train_extras=True)
pool["pred_f"] = pool["flow_label"].transpose(2, 1).contiguous() + 0.3 * torch.randn(frames, 3, nmax, generator=g)
pool["mseg_pre"] = torch.sigmoid(2.0 * torch.randn(frames, 1, nmax, generator=g))
pool["pre_trans"] = pool["gt_trans"].clone()
CH1, CH2, ROW1 = ("pc1", "ft1", "pred_f", "mseg_pre"), ("pc2", "ft2"), ("flow_label", "fg_mask", "radar_u", "radar_v", "opt_flow")


def cut(sl, m1, m2):
    out = {}
    for k, v in pool.items():
        v = v[sl]
        v = v[:, :, :m1] if k in CH1 else v[:, :, :m2] if k in CH2 else v[:, :m1] if k in ROW1 else v
        out[k] = v.contiguous().to(dev)
    for k in ("pred_f", "mseg_pre", "pre_trans"):
        out[k].requires_grad_(True)
    return out


singles = []
for i in range(frames):
    m = int(min(n1[i], n2[i]))
    singles.append(cut(slice(i, i + 1), m, m))


def batches(B):
    out = []
    for s in range(0, frames, B):
        sl = slice(s, min(frames, s + B))
        b = cut(sl, int(n1[sl].max()), int(n2[sl].max()))
        b["n1"], b["n2"] = n1[sl].to(dev, torch.int32), n2[sl].to(dev, torch.int32)
        out.append(b)
    return out


def run_single():
    for b in singles:
        dyn, mseg = make_labels(b, 0.3)
        crit(b["pc1"], b["pc2"], b["pred_f"], b["ft1"][:, 0], b["flow_label"].transpose(2, 1), b["pre_trans"], b["mseg_pre"],
             b["gt_trans"], mseg, dyn, b["radar_u"], b["radar_v"], b["opt_flow"])


def run_ragged(bs):
    for b in bs:
        dyn, mseg = make_labels_ragged(b, 0.3)
        crit.forward_ragged(b["pc1"], b["pc2"], b["pred_f"], b["ft1"][:, 0], b["n1"], b["n2"], b["flow_label"].transpose(2, 1),
                            b["pre_trans"], b["mseg_pre"], b["gt_trans"], mseg, dyn, b["radar_u"], b["radar_v"], b["opt_flow"])


variants = [("forward, B = 1 per cropped frame", run_single)]
for B in (8, 16, 64):
    if B <= frames:
        variants.append(("forward_ragged, B = %d" % B, (lambda bs: (lambda: run_ragged(bs)))(batches(B))))

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

print("ragged loss probe (labels + loss + gradients): %d frames, %d-%d points in cloud 1, %d-%d in cloud 2; %d repeats, variants "
      "alternating; %s" % (frames, int(n1.min()), int(n1.max()), int(n2.min()), int(n2.max()), repeats, torch.cuda.get_device_name(0)))
print("%-34s %12s %22s %14s" % ("variant", "frames/s", "spread (min - max)", "ms per frame"))
base = None
for name, _ in variants:
    fps = sorted(frames / t for t in times[name])
    med = statistics.median(fps)
    base = base or med
    print("%-34s %12.0f %10.0f - %-9.0f %14.3f   x%.2f" % (name, med, fps[0], fps[-1], 1e3 / med, med / base))
