"""What clustering a test run's moving points costs: instances.cluster over all frames of the synthetic test partition of
tools/results_probe.py (256 whole frames with View-of-Delft's sizes, 87-461 points), ``which='pred'`` on the store an evaluation
epoch left and ``which='gt'`` on the split's labels, at eps 2 / min_points 2 with and without the displacement term.  Not run by
any test; needs the GPU (no fallback).

  (single)     one call between two device events, the median over ``--rounds`` calls: the fills and the launch latency included;
  (stream)     ``--reps`` calls back to back between two device events, per call, the median over ``--rounds`` (a ``'pred'`` call
               copies ``store.done`` to the host before it launches, so consecutive calls do not overlap: this is what a user gets);
  (kernel)     ``--reps`` calls of the C entry point ``cmf_cluster_moving`` itself back to back on prepared arguments, per call: the
               kernel's own time.  It is compute, not traffic: every pair distance of a frame's candidates is formed once, in float64
               out of LDS, by one workgroup per frame;
  (torch)      for context only, the same LABELS from batched torch ops on the device: the frames padded to (F, 461), all pair
               distances at once in float64, the core test, min-label propagation with pointer jumping until a round changes
               nothing (one read-back per round: the loop is data-dependent), the borders by a masked arg-min, the numbering by a
               sort -- and whether its labels equal the kernel's.

There is no bar: the parent commit has nothing to compare with.  The parent process writes the split and never opens the GPU; the
measurement is a child process under a time limit.

    python tools/instances_probe.py [--frames 256] [--rounds 9] [--reps 50] [--limit 400] [--out profiles/instances_probe.txt]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _run_probe as P                               # noqa: E402

SETTINGS = ((2.0, 2, 0.0), (2.0, 2, 2.5))                       # eps, min_points, flow_weight


def torch_labels(sp, flow, moving, T, eps, min_points, weight):
    """Batched float64 torch ops -> label (sum n1) int64 as cluster gives them."""
    import torch
    dev = sp.tab1.device
    F, off = len(sp), sp.off1.long()
    n = off[1:] - off[:-1]
    N = int(sp.counts_host[0].max())
    slot = torch.arange(N, device=dev)[None, :]
    valid = slot < n[:, None]
    row = (off[:-1, None] + slot).clamp(max=sp.tab1.shape[0] - 1)
    p = sp.tab1[row, :3].double()
    Tm = T.reshape(F, 4, 4).double()
    d = p + flow[row].double() - ((Tm[:, None, :3, :3] @ p[..., None])[..., 0] + Tm[:, None, :3, 3])
    cand = valid & moving[row]
    D2 = ((p[:, :, None] - p[:, None, :]) ** 2).sum(-1) + weight * weight * ((d[:, :, None] - d[:, None, :]) ** 2).sum(-1)
    near = (D2 <= eps * eps) & cand[:, :, None] & cand[:, None, :]
    core = cand & (near.sum(-1) >= min_points)
    link = near & core[:, :, None] & core[:, None, :]
    big = N
    lab = torch.where(core, slot.expand(F, N), torch.full((F, N), big, device=dev))
    while True:
        pulled = torch.where(link, lab[:, None, :].expand(F, N, N), torch.full((), big, device=dev)).min(-1).values
        new = torch.minimum(lab, pulled)
        new = torch.where(core, torch.gather(lab, 1, new.clamp(max=N - 1)), new)
        if bool((new == lab).all()):
            break
        lab = new
    reach = torch.where(near & core[:, None, :] & ~core[:, :, None], D2, torch.full((), float("inf"), dtype=D2.dtype, device=dev))
    has = torch.isfinite(reach).any(-1)
    lab = torch.where(has, torch.gather(lab, 1, reach.argmin(-1)), lab)
    root = core & (lab == slot)
    number = torch.cumsum(root.long(), 1) - 1
    inst = torch.where(lab < big, torch.gather(number, 1, lab.clamp(max=N - 1)), torch.full((F, N), -1, device=dev))
    return inst[valid]


def measure(a):
    import torch
    from cmflow_amd import _lib, instances as I
    sp, store = P.synthetic_store(a)
    F, counts = len(sp), sp.counts_host[0]
    print("split: %d frames of %d-%d points, %d points (%d moving in the prediction, %d in the labels); device: %s; %d rounds, %d calls per "
          "stream window" % (F, counts.min(), counts.max(), sp.tab1.shape[0], int((store.mask == 0).sum()), int((sp.tab1[:, 9] == 0).sum()),
                             torch.cuda.get_device_name(0), a.rounds, a.reps))
    for which in I.WHICH:
        for eps, min_points, weight in SETTINGS:
            call = lambda: I.cluster(sp, store if which == "pred" else None, which=which, eps=eps, min_points=min_points, flow_weight=weight)
            inst = call()
            torch.cuda.synchronize()
            single = statistics.median(P.timed(call, 1) for _ in range(a.rounds))
            stream = statistics.median(P.timed(call, a.reps) for _ in range(a.rounds))
            p, i32, u8, f32 = _lib.dev_ptr, torch.int32, torch.uint8, torch.float32
            gt = which == "gt"
            flow, mask, T = (None, None, sp.trans) if gt else (store.flow, store.mask, store.pred_trans)
            args = (F, F, None, p(sp.off1, i32), sp.tab1.shape[0], p(sp.tab1, f32), sp.tab1.shape[1], p(flow, f32), p(mask, u8),
                    p(T.reshape(-1, 16), f32), int(gt), eps * eps, weight * weight, min_points, p(inst.label, i32), p(inst.kind, u8),
                    p(inst.count, i32), p(inst.size, i32), p(inst.seed, i32), p(inst.centroid, f32), p(inst.disp, f32), p(inst.lo, f32),
                    p(inst.hi, f32), _lib.stream_ptr())
            entry = _lib.lib().cmf_cluster_moving
            kernel = statistics.median(P.timed(lambda: entry(*args), a.reps) for _ in range(a.rounds))
            t_flow, t_moving = (sp.tab1[:, 6:9], sp.tab1[:, 9] == 0) if gt else (store.flow, store.mask == 0)
            ref = lambda: torch_labels(sp, t_flow, t_moving, T, eps, min_points, weight)
            same = int((ref() == inst.label.long()).sum())
            t_torch = statistics.median(P.timed(ref, 3) for _ in range(min(a.rounds, 5)))
            members = inst.kind >= 2
            print("%-4s eps %.1f min_points %d flow_weight %.1f: %5d instances, %6d member points, %6d noise: single %7.1f us, stream %7.1f us per "
                  "call, kernel %7.1f us; torch float64 %9.1f us (x%.0f the call), %d of %d labels equal"
                  % (which, eps, min_points, weight, int(inst.count.sum()), int(members.sum()), int((inst.kind == 1).sum()), single, stream, kernel,
                     t_torch, t_torch / stream, same, inst.label.numel()))


if __name__ == "__main__":
    P.run("instances_probe", measure, (("--rounds", 9, None), ("--reps", 50, P.REPS_HELP)))
