"""What accumulating a test run's clouds costs: accumulate.accumulate over all frames of the synthetic test partition of
tools/results_probe.py (256 whole frames with View-of-Delft's sizes, 87-461 points, taken as ONE clip so that every window is
full), windows 8 and 32, the three ``dynamic`` modes, ``which='pred'`` on the store an evaluation epoch left.  Not run by any test;
needs the GPU (no fallback).

  (single)     one call between two device events, the median over ``--rounds`` calls: launch latency included;
  (stream)     ``--reps`` calls back to back between two device events, per call, the median over ``--rounds`` (a ``'pred'`` call
               copies ``store.done`` to the host before it launches, so consecutive calls do not overlap: this is what a user gets);
  (kernel)     ``--reps`` calls of the C entry point ``cmf_accumulate`` itself back to back on prepared arguments (a few microseconds
               of host time each, so the device is never idle between them), per call: the kernel's own time;
  (bytes)      the algorithmic traffic of one call, from the shapes: per output row 1 mask byte read and 17 bytes written (xyz 12,
               src 4, age 1), 12 bytes of position read per row that holds a point, 12 bytes of flow per propagated point, 48 bytes
               per transform of every target's window, 8 bytes of offsets per target -- over the (kernel) time, as achieved bytes/s
               against the 8 TB/s of the device's memory;
  (torch)      the same result from batched float32 torch ops on the device (the chain as ``window - 1`` batched 4x4 products, one
               gather of the matrices per row, the flow term for ``propagate``, a boolean selection for ``drop`` -- which waits for
               the device once), its row indices built beforehand and not timed: the only comparison there is, and its largest
               deviation from the kernel's float64 definition.

There is no bar: the parent commit has nothing to compare with.  The parent process writes the split and never opens the GPU; the
measurement is a child process under a time limit.

    python tools/accumulate_probe.py [--frames 256] [--rounds 9] [--reps 50] [--limit 400] [--out profiles/accumulate_probe.txt]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _run_probe as P                               # noqa: E402

WINDOWS = (8, 32)
PEAK = 8.0e12                                                   # bytes/s


def torch_accumulate(sp, store, window, dynamic, idx):
    """float32 torch ops -> xyz of every output row (of the kept rows under 'drop')."""
    import torch
    F = len(sp)
    T = store.pred_trans
    C = torch.eye(4, device=T.device).repeat(F, window, 1, 1)
    for g in range(1, window):
        C[g:, g] = C[g:, g - 1] @ T[:F - g]
    target, src, age = idx
    p = sp.tab1[src, :3]
    M = C[target, age]
    q = (M[:, :3, :3] @ p[:, :, None])[:, :, 0] + M[:, :3, 3]
    moving = (store.mask[src] == 0) & (age > 0)
    if dynamic == "propagate":
        Ti = T[target - age]
        d = p + store.flow[src] - ((Ti[:, :3, :3] @ p[:, :, None])[:, :, 0] + Ti[:, :3, 3])
        N = C[target, (age - 1).clamp(min=0)]
        q = torch.where(moving[:, None], q + age[:, None].float() * (N[:, :3, :3] @ d[:, :, None])[:, :, 0], q)
    return q[~moving] if dynamic == "drop" else q


def measure(a):
    import numpy as np
    import torch
    from cmflow_amd import _lib, accumulate as A
    sp, store = P.synthetic_store(a)
    dev = sp.device
    F = len(sp)
    counts = sp.counts_host[0]
    print("split: %d frames as one clip, %d points (%d moving in the prediction); device: %s; %d rounds, %d calls per stream window"
          % (F, sp.tab1.shape[0], int((store.mask == 0).sum()), torch.cuda.get_device_name(0), a.rounds, a.reps))
    for window in WINDOWS:
        first, ages, cap_off = A.plan(counts, None, np.arange(F), window)
        R = int(cap_off[-1])
        target = torch.from_numpy(np.repeat(np.arange(F), np.diff(cap_off))).to(dev)
        off1 = np.concatenate(([0], np.cumsum(counts)))
        src = torch.from_numpy(np.concatenate([np.arange(off1[j - g + 1], off1[j + 1]) for j, g in enumerate(ages)])).to(dev)
        frame_of = torch.from_numpy(np.repeat(np.arange(F), counts)).to(dev)
        idx = (target, src, target - frame_of[src])
        for dynamic in A.DYNAMIC:
            call = lambda: A.accumulate(sp, store, window=window, dynamic=dynamic)
            acc = call()
            torch.cuda.synchronize()
            single = statistics.median(P.timed(call, 1) for _ in range(a.rounds))
            stream = statistics.median(P.timed(call, a.reps) for _ in range(a.rounds))
            first_d = torch.from_numpy(first).to(dev)
            p, i32, u8, f32 = _lib.dev_ptr, torch.int32, torch.uint8, torch.float32
            args = (F, F, None, p(first_d, i32), p(sp.off1, i32), sp.tab1.shape[0], p(sp.tab1, f32), sp.tab1.shape[1], p(store.flow, f32),
                    p(store.mask, u8), p(store.pred_trans.reshape(-1, 16), f32), window, A.DYNAMIC.index(dynamic), 0, p(acc.off, i32), R,
                    p(acc.xyz, f32), p(acc.src, i32), p(acc.age, u8), p(acc.count, i32), _lib.stream_ptr())
            entry = _lib.lib().cmf_accumulate
            kernel = statistics.median(P.timed(lambda: entry(*args), a.reps) for _ in range(a.rounds))
            held = int(acc.count.sum())
            moved = int(((store.mask[acc.src.clamp(min=0).long()] == 0) & (acc.age >= 1) & (acc.age != 255)).sum()) if dynamic == "propagate" else 0
            nbytes = R * (1 + 17) + held * 12 + moved * 12 + int((ages - 1).sum()) * 48 + F * 8
            ref = lambda: torch_accumulate(sp, store, window, dynamic, idx)
            got = ref()
            mine = acc.xyz[acc.src >= 0] if dynamic == "drop" else acc.xyz
            dev_max = float((got - mine).abs().max())
            t_torch = statistics.median(P.timed(ref, 5) for _ in range(a.rounds))
            print("window %2d %-9s %8d rows (%8d hold points): single %7.1f us, stream %7.1f us per call, kernel %7.1f us; %6.2f MB algorithmic -> "
                  "%5.3f TB/s achieved by the kernel, %4.1f%% of 8 TB/s; torch float32 %9.1f us (x%.0f the call), max deviation %.2e m"
                  % (window, dynamic, R, held, single, stream, kernel, nbytes / 1e6, nbytes / kernel / 1e6, 100 * nbytes / (kernel * 1e-6) / PEAK,
                     t_torch, t_torch / stream, dev_max))


if __name__ == "__main__":
    P.run("accumulate_probe", measure, (("--rounds", 9, None), ("--reps", 50, P.REPS_HELP)))
