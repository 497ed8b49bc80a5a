"""What keeping every frame's results costs an evaluation epoch: evaluate.eval_split on a synthetic test partition of a few hundred
whole frames with View-of-Delft's sizes (87-461 points), three ways.  Not run by any test; needs the GPU (no fallback).

  (plain)      eval_split without a hook: epoch averages and the two transform arrays only;
  (collector)  evaluate.test_split: a results.ResultCollector as the hook -- per batch cmf_pack_results, two copies into kept scratch
               and cmf_eval_metrics_frames, nothing read back;
  (per_frame)  eval_split with a hook that does what the reference's save_res branch does (main_util.py:149-156): for every frame of
               the batch pc1, pc2, pred_f, pred_m and pred_t copied to the host with .cpu() -- five waits for the device per frame
               (the JSON encoding and the file writes that follow in the reference are left out: they are host work either way).

The three alternate in ONE process: after a warm-up epoch of each, every round times `--epochs` epochs of each variant (ending in a
device synchronise) with the order rotated from round to round, so clock and cache state are shared.  Per variant: the median over
the rounds of the wall-clock ms per frame, the smallest and largest round (the spread), and "host": the time until the epochs'
loops returned -- for the first two the enqueue time, for the third it contains the waits.  No threshold is attached to any number.

The parent process writes the split and never opens the GPU; the measurement is a child process under a time limit.

    python tools/results_probe.py [--frames 256] [--batch 16] [--epochs 5] [--rounds 7] [--limit 400]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _run_probe as P                               # noqa: E402
from tools._run_probe import EvalArgs, PER_CLIP, clips_of     # noqa: E402,F401  (the other probes' split is this one)

VARIANTS = ("plain", "collector", "per_frame")


def measure(a):
    import torch
    from cmflow_amd import evaluate as EV
    net, sp = P.synthetic_net_split(a)
    print("split: %d frames, %d + %d points; device: %s; batch %d; %d rounds of %d epochs per variant, order rotated"
          % (len(sp), sp.tab1.shape[0], sp.tab2.shape[0], torch.cuda.get_device_name(0), a.batch, a.rounds, a.epochs))

    def reference_copies(batch, out):
        n1, n2 = batch["n1"].cpu().tolist(), batch["n2"].cpu().tolist()
        for s in range(len(n1)):
            keep = (batch["pc1"][s, :, :n1[s]].cpu(), batch["pc2"][s, :, :n2[s]].cpu(), out[0][s, :, :n1[s]].cpu(),
                    out[3][s, :n1[s]].cpu(), out[2][s].cpu())
        return keep

    run = {"plain": lambda: EV.eval_split(net, sp, a.batch),
           "collector": lambda: EV.test_split(net, sp, a.batch),
           "per_frame": lambda: EV.eval_split(net, sp, a.batch, on_batch=reference_copies)}
    for v in VARIANTS:                                            # warm-up: first launches, allocator, scratch
        run[v]()
    torch.cuda.synchronize()
    total, host = {v: [] for v in VARIANTS}, {v: [] for v in VARIANTS}
    for r in range(a.rounds):
        for v in VARIANTS[r % 3:] + VARIANTS[:r % 3]:
            t0 = time.perf_counter()
            for _ in range(a.epochs):
                run[v]()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            per = 1e3 / (a.epochs * len(sp))
            total[v].append((t2 - t0) * per)
            host[v].append((t1 - t0) * per)
    for v in VARIANTS:
        print("%-10s %7.3f ms per frame (median of %d rounds; min %7.3f, max %7.3f), host %7.3f"
              % (v, statistics.median(total[v]), a.rounds, min(total[v]), max(total[v]), statistics.median(host[v])))
    base = statistics.median(total["plain"])
    print("collector - plain: %+.3f ms per frame; per_frame - plain: %+.3f ms per frame (medians)"
          % (statistics.median(total["collector"]) - base, statistics.median(total["per_frame"]) - base))


if __name__ == "__main__":
    P.run("results_probe", measure, (("--batch", 16, None), ("--epochs", 5, None), ("--rounds", 7, None)), out=False)
