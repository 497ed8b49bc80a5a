#!/usr/bin/env python3
"""Twelve consecutive frames of the REFERENCE's own saved results (its ``--eval --save_res`` run, checkpoints/raflow_cvpr/results/
delft_12/<frame>.json) as the fixture of the accumulation tests: recorded data, nothing computed here.  Build container only.

    python tests/golden/make_golden_accumulate.py   ->  tests/golden/saved_results_delft_12_w12.npz

Frames 727 .. 738, packed like a split: off (13) int64, pc1 (sum n, 3), pred_f (sum n, 3) float32, pred_m (sum n) uint8, pred_t (12,4,4)
float32, first_frame.  The frames are consecutive scan pairs -- pc2 of a frame is pc1 of the next, asserted here -- which is the
contract ``accumulate`` relies on.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

FIRST, COUNT = 727, 12


def main():
    pc1, pred_f, pred_m, pred_t, prev = [], [], [], [], None
    for k in range(FIRST, FIRST + COUNT):
        rec = json.load(open(os.path.join(REF, "checkpoints/raflow_cvpr/results/delft_12/%d.json" % k)))
        p1, p2 = np.array(rec["pc1"], dtype=np.float32).T, np.array(rec["pc2"], dtype=np.float32).T
        assert np.array_equal(np.array(rec["pc1"]).T, p1.astype(np.float64)), "pc1 is not float32 data"
        assert prev is None or np.array_equal(prev, p1), "frame %d does not start where frame %d ended" % (k, k - 1)
        prev = p2
        m = np.array(rec["pred_m"])
        assert set(np.unique(m)) <= {0.0, 1.0}
        pc1.append(p1)
        pred_f.append(np.array(rec["pred_f"], dtype=np.float32).T)
        pred_m.append(m.astype(np.uint8))
        pred_t.append(np.array(rec["pred_t"], dtype=np.float32))
    off = np.concatenate(([0], np.cumsum([p.shape[0] for p in pc1]))).astype(np.int64)
    out = os.path.join(HERE, "saved_results_delft_12_w12.npz")
    np.savez_compressed(out, off=off, pc1=np.concatenate(pc1), pred_f=np.concatenate(pred_f), pred_m=np.concatenate(pred_m),
                        pred_t=np.stack(pred_t), first_frame=np.int64(FIRST))
    print("%d frames, %d points, %d moving, %d bytes" % (COUNT, off[-1], int((np.concatenate(pred_m) == 0).sum()), os.path.getsize(out)))


if __name__ == "__main__":
    main()
