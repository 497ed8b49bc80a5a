"""Building a split from raw scans: cmflow_amd.prepare.SplitBuilder against the numpy restatement of the reference's preprocess step
(tests/prepare_ref.py, which leaves out what the reference also pays for: one process per pair, open3d, file reads, the JSON dump).
Not run by any test; needs the GPU (no fallback).

  (a) prepare_ref.make_sample over every pair of a synthetic chain of scans (tests/prepare_case.py: about --rows raw rows a scan, five
      tracked boxes a scan) -- host clock;
  (b) SplitBuilder.add + finish on the same arrays, everything included (host 4 x 4 products and match_boxes, uploads, the two kernels,
      the copy of the counts, the concatenation) -- host clock around work that ends in a device synchronise, after one warm-up build;
  (c) cmf_prepare_count and cmf_prepare_pairs alone, device events over --launches back-to-back calls on resident inputs;
  (d) filter_scans with nmax given (one launch per call), device events.

    python tools/prepare_probe.py [--pairs 256] [--rows 600] [--repeat 5] [--launches 200]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import prepare_case as PC  # noqa: E402
import prepare_ref as R  # noqa: E402
from cmflow_amd import _lib  # noqa: E402
from cmflow_amd import prepare as P  # noqa: E402


def events_us(fn, launches):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--rows", type=int, default=600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_probe: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    case = PC.chain(5, [int(n) for n in rng.integers(a.rows // 2, a.rows * 3 // 2, a.pairs + 1)], "gt", K=5)
    calib = PC.product_calib(case)
    scans, tracks = case.packed_scans, case.packed_tracks

    t0 = time.perf_counter()
    for f, (s1, s2) in enumerate(case.pairs):
        R.make_sample(case.scans[s1], case.scans[s2], case.calib[s1], case.calib[s2], case.odom[s1], case.odom[s2], case.tracks[s1],
                      case.tracks[s2], case.mode)
    ref_s = time.perf_counter() - t0

    def build():
        b = P.SplitBuilder(calib, case.mode, dev)
        b.add(scans, case.scan_off, case.pairs, case.odom, tracks, case.track_off)
        out = b.finish()
        torch.cuda.synchronize()
        return out

    split, kept = build()                                                  # warm-up: code objects, allocator
    times = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        build()
        times.append(time.perf_counter() - t0)
    print("device: %s; %d pairs of scans of %d-%d raw rows, %d kept pairs, %d + %d points after the filter, %d track rows"
          % (torch.cuda.get_device_name(0), a.pairs, a.rows // 2, a.rows * 3 // 2, len(kept), split.tab1.shape[0], split.tab2.shape[0], len(tracks)))
    print("(a) numpy restatement, one pair at a time:      %8.2f ms per pair (one pass, host clock)" % (ref_s / a.pairs * 1e3))
    print("(b) SplitBuilder.add + finish, all included:    %8.3f ms per pair (median of %d builds; min %.3f, max %.3f)"
          % (np.median(times) / a.pairs * 1e3, a.repeat, min(times) / a.pairs * 1e3, max(times) / a.pairs * 1e3))

    # (c) the kernels alone, on resident inputs
    d_scans = torch.from_numpy(scans).to(dev)
    d_off = P._i32(case.scan_off, dev)
    keep, uv, count = P._count(d_scans, d_off, calib, dev)
    us_count = events_us(lambda: P._count(d_scans, d_off, calib, dev), a.launches)
    cnt = count.cpu().numpy().astype(np.int64)
    n1, n2 = cnt[case.pairs[:, 0]], cnt[case.pairs[:, 1]]
    off1, off2 = np.concatenate([[0], np.cumsum(n1)]), np.concatenate([[0], np.cumsum(n2)])
    cal = [calib] * len(case.scans)
    odom_radar = [case.odom[s] @ calib.t_camera_radar for s in range(len(case.scans))]
    tinv = np.stack([np.linalg.inv(np.linalg.inv(odom_radar[s1]) @ odom_radar[s2]) for s1, s2 in case.pairs])
    boxes = [P.match_boxes(case.tracks[s1], case.tracks[s2], cal[s1], cal[s2]) for s1, s2 in case.pairs]
    box_off = np.cumsum([0] + [len(b) for b in boxes])
    d64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    held = (P._i32(case.pairs, dev), P._i32(off1, dev), P._i32(off2, dev), d64(tinv.reshape(-1, 16)),
            d64(np.concatenate(boxes + [np.zeros((1, P.BOX_DOUBLES))])), P._i32(box_off, dev))
    tab1 = torch.empty((int(off1[-1]), 14), dtype=torch.float32, device=dev)
    tab2 = torch.empty((int(off2[-1]), 6), dtype=torch.float32, device=dev)

    def pairs_kernel():
        _lib.check(_lib.lib().cmf_prepare_pairs(len(case.pairs), d_scans.shape[1], P._ptr(d_scans), P._ptr(d_off), P._ptr(keep), P._ptr(uv),
                                                *(P._ptr(t) for t in held), 0, None, 1936, 1216, P._ptr(tab1), P._ptr(tab2),
                                                _lib.stream_ptr()), "cmf_prepare_pairs")

    us_pairs = events_us(pairs_kernel, a.launches)
    print("(c) cmf_prepare_count over %d scans (with its output allocations): %.1f us per call; cmf_prepare_pairs over %d pairs, %d boxes: "
          "%.1f us per call (device events over %d back-to-back calls, host launch path included)"
          % (len(case.scans), us_count, len(case.pairs), box_off[-1], us_pairs, a.launches))
    us_scans = events_us(lambda: P.filter_scans(d_scans, case.scan_off, calib, dev, nmax=1024), a.launches)
    print("(d) filter_scans(nmax=1024) over %d scans: %.1f us per call (the offsets are uploaded in every call)" % (len(case.scans), us_scans))


if __name__ == "__main__":
    main()
