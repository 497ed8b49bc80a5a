"""What pictures of a test run cost: vis.render alone and SplitResults.write_vis (render + copy + encode + file) per frame, on the
synthetic test partition of tools/results_probe.py (256 whole frames with View-of-Delft's sizes, 87-461 points) at the default view
(1200 x 600, 60 m x 30 m, radius 3.5 px, guides on).  Not run by any test; needs the GPU (no fallback).

  (render)     vis.render of 64 frames at a time over the whole split, layers flow and seg_gt: device events around each call -- the
               two launches, nothing read back; `--reps` passes over the split per timed window, the median over the rounds,
               per frame, and the epoch's own forward beside it;
  (write_vis)  SplitResults.write_vis of the whole split into a scratch directory, wall clock per picture, split into
               device + copy (render and the chunk's device-to-host copy), encode (vis.encode_png: zlib) and file (open / write),
               the last two timed on the host around the same calls write_vis makes.

There is no bar: the parent commit has nothing to compare with, and the reference's matplotlib loop (two figures at dpi 200 per
frame) does not run here.  The parent process writes the split and never opens the GPU; the measurement is a child process under a
time limit.

    python tools/vis_probe.py [--frames 256] [--chunk 64] [--rounds 5] [--reps 100] [--limit 400] [--out profiles/vis_probe.txt]
"""
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _run_probe as P                               # noqa: E402

LAYERS = ("flow", "seg_gt")


def measure(a):
    import torch
    from cmflow_amd import evaluate as EV, vis
    net, sp = P.synthetic_net_split(a)
    EV.test_split(net, sp, 16)                                  # warm-up of the forward
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, store = EV.test_split(net, sp, 16)
    torch.cuda.synchronize()
    forward_ms = 1e3 * (time.perf_counter() - t0) / len(sp)
    view = vis.BevView()
    F = len(sp)
    print("split: %d frames, %d points; device: %s; view %d x %d, radius %.1f px, guides %s; chunks of %d; %d rounds"
          % (F, sp.tab1.shape[0], torch.cuda.get_device_name(0), view.width, view.height, view.radius_px, view.guides, a.chunk, a.rounds))
    print("the epoch itself (evaluate.test_split, batch 16): %.3f ms per frame" % forward_ms)

    chunks = [list(range(c, min(c + a.chunk, F))) for c in range(0, F, a.chunk)]
    for layer in LAYERS:                                        # warm-up: first launches, allocator
        vis.render(store, sp, layer, chunks[0], view)
    torch.cuda.synchronize()
    for layer in LAYERS:
        per = []
        for _ in range(a.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.reps):
                for c in chunks:
                    vis.render(store, sp, layer, c, view)
            stop.record()
            stop.synchronize()
            per.append(1e3 * start.elapsed_time(stop) / (F * a.reps))
        print("render     %-7s %7.2f us per frame on the device (median of %d rounds of %d passes over the split; min %7.2f, max %7.2f)"
              % (layer, statistics.median(per), a.rounds, a.reps, min(per), max(per)))

    with tempfile.TemporaryDirectory(prefix="cmf_vis_probe_") as out:
        t0 = time.perf_counter()
        paths = store.write_vis(out, sp, LAYERS, None, view, a.chunk)
        whole = time.perf_counter() - t0
        size = sum(os.path.getsize(p) for p in paths)
        # the parts, around the same calls: render + copy per chunk, then encode and write per picture
        dev_s = enc_s = file_s = 0.0
        for layer in LAYERS:
            for c in chunks:
                t0 = time.perf_counter()
                images = vis.render(store, sp, layer, c, view).cpu().numpy()
                t1 = time.perf_counter()
                dev_s += t1 - t0
                for f, image in zip(c, images):
                    t2 = time.perf_counter()
                    data = vis.encode_png(image)
                    t3 = time.perf_counter()
                    with open(os.path.join(out, "part_%s_%d.png" % (layer, f)), "wb") as fh:
                        fh.write(data)
                    enc_s += t3 - t2
                    file_s += time.perf_counter() - t3
    n = len(paths)
    print("write_vis  %d pictures (%d frames x %d layers): %7.3f ms per picture wall clock, %.1f kB per file"
          % (n, F, len(LAYERS), 1e3 * whole / n, size / n / 1e3))
    print("  of which device + copy %7.3f, encode %7.3f, file %7.3f ms per picture (timed apart, on a second pass)"
          % (1e3 * dev_s / n, 1e3 * enc_s / n, 1e3 * file_s / n))


if __name__ == "__main__":
    P.run("vis_probe", measure, (("--chunk", 64, None), ("--rounds", 5, None),
                                 ("--reps", 100, "passes over the split inside one timed window of render")))
