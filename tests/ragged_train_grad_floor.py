"""Not a test -- the measurement behind the gradient bounds of tests/test_gpu_ragged_train.py (tests/ragged_train_case.py FLOORS): the
reference gradient of a ragged training step -- the mean over the samples of the CPU oracle's B = 1 eval-mode gradients on the
truncated samples -- evaluated in fp32 and in fp64, and the figures of _check_gradients between the two.  Two correct fp32
implementations cannot agree tighter than this.

    python tests/ragged_train_grad_floor.py > profiles/ragged_train_grad_floor.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_loss_case as RC
import ragged_train_case as TC

torch.set_num_threads(8)
print("oracle fp32 vs fp64, mean over the samples of the B = 1 eval-mode gradients on the truncated samples; %d threads, torch %s"
      % (torch.get_num_threads(), torch.__version__))
runs = [(name, counts, seed, False, None) for name, (counts, seed) in TC.CASES.items()]
runs.append(("clip_t", RC.COUNTS5, RC.SEED5, True, TC.SEED_T2))
for name, counts, seed, t, seed2 in runs:
    batch = RC.make_case(counts, seed)[0]
    batch2 = RC.make_case(counts, seed2)[0] if seed2 is not None else None
    sd = TC.weights(t)
    g = {}
    for dt in (torch.float32, torch.float64):
        t0 = time.time()
        g[dt], totals, _, _ = TC.oracle_mean_gradient(sd, batch, counts, dt, t=t, batch2=batch2)
        print("%s %s: per-sample totals %s (%.1f s)" % (name, dt, ["%.6f" % v for v in totals], time.time() - t0), flush=True)
    rows, whole = TC.gradient_metrics(g[torch.float32], g[torch.float64])
    arr = np.array([r[1:] for r in rows])
    for j, what in enumerate(("norm", "1-cos", "element")):
        i = int(arr[:, j].argmax())
        print("%s %-8s median %.3g  p90 %.3g  max %.3g (%s)" % (name, what, np.median(arr[:, j]), np.percentile(arr[:, j], 90), arr[i, j], rows[i][0]))
    print("%s whole gradient: relative error %.3g, 1 - cos %.3g" % (name, whole[0], whole[1]))
    print("%s FLOORS entry: ((%.3g, %.3g, %.3g), (%.3g, %.3g))" % (name, arr[:, 0].max(), arr[:, 1].max(), arr[:, 2].max(), whole[0], whole[1]), flush=True)
