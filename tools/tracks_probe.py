"""What tracking a test run's instances costs: tracks.track over the instances of (a) the synthetic test partition of
tools/results_probe.py (256 whole frames with View-of-Delft's sizes, clustered from the store an evaluation epoch left and from the
labels) taken as 32 clips of 8 frames and as ONE clip of 256, and (b) the coherent world of tests/tracks_ref.py (rigid objects at
constant velocity under a turning ego-motion) repeated to 288 frames in 32 clips.  The synthetic partition's frames are NOT temporally
coherent -- consecutive frames are unrelated clouds -- so most instances there open tracks instead of continuing one: (a) times the
kernel on many births and few matches, (b) on what it is for.  Not run by any test; needs the GPU (no fallback).

  (single)     one call between two device events, the median over ``--rounds`` calls: the fills, the clip upload and the launch latency
               included;
  (stream)     ``--reps`` calls back to back between two device events, per call, the median over ``--rounds``;
  (kernel)     ``--reps`` calls of the C entry point ``cmf_track_instances`` itself back to back on prepared arguments, per call: the
               kernel's own time.  One workgroup per clip walks its frames in sequence, so the launch keeps as many CUs busy as there
               are clips and lasts as long as its longest clip;
  (host)       for context only, the per-frame loop a user would write without the kernel: the tables copied to the host and the
               restatement of tests/tracks_ref.py (numpy, float64) over them, once, wall clock -- and whether its tracks equal the kernel's.

Every figure comes with the smallest and largest round (the spread).  There is no bar: the parent commit has nothing to compare with.
The parent process writes the split and never opens the GPU; the measurement is a child process under a time limit.

    python tools/tracks_probe.py [--frames 256] [--rounds 9] [--reps 50] [--limit 400] [--out profiles/tracks_probe.txt]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _run_probe as P                               # noqa: E402

GATE, MAX_GAP = 2.0, 2


def measure(a):
    import numpy as np
    import torch
    import tracks_ref as ref
    from cmflow_amd import _lib, tracks as K
    print("device: %s; gate %.1f, max_gap %d; %d rounds, %d calls per stream window; median [smallest .. largest round]"
          % (torch.cuda.get_device_name(0), GATE, MAX_GAP, a.rounds, a.reps))

    def case(name, sp, store, inst):                            # its tensors and tables are dropped before the next case
        call = lambda: K.track(inst, sp, store, gate=GATE, max_gap=MAX_GAP)
        tr = call()
        torch.cuda.synchronize()
        single, stream = P.spread(call, 1, a.rounds), P.spread(call, a.reps, a.rounds)
        p, i32, f32 = _lib.dev_ptr, torch.int32, torch.float32
        T = store.pred_trans if inst.which == "pred" else sp.trans
        outs = (tr.track, tr.prev_row, tr.gap, tr.age, tr.pred, tr.point_track, tr.birth, tr.last, tr.hits)
        args = (len(tr), len(sp), p(tr.clips, i32), p(sp.off1, i32), sp.tab1.shape[0], p(inst.count, i32), p(inst.label, i32), p(inst.centroid, f32),
                p(inst.disp, f32), p(T.reshape(-1, 16), f32), GATE * GATE, MAX_GAP, *(p(t, f32 if t.dtype == f32 else i32) for t in outs),
                p(tr.ntracks, i32), p(tr.overflow, i32), _lib.stream_ptr())
        entry = _lib.lib().cmf_track_instances
        kernel = P.spread(lambda: entry(*args), a.reps, a.rounds)
        t0 = time.perf_counter()
        off1 = sp.off1.cpu().numpy()
        want = ref.track(off1, int(off1[-1]), inst.count.cpu().numpy(), inst.label.cpu().numpy(), inst.centroid.cpu().numpy(), inst.disp.cpu().numpy(),
                         T.reshape(-1, 16).cpu().numpy(), tr.clips_host, GATE, MAX_GAP)
        host = 1e3 * (time.perf_counter() - t0)
        same = all(np.array_equal(getattr(tr, k).cpu().numpy().view(np.int32), want[k].view(np.int32)) for k in ref.KEYS)
        inst_n, matched = int(inst.count.sum()), int((tr.age > 1).sum())
        print("%-34s %3d clips (longest %3d frames), %5d instances, %5d tracks, %5d matches: single %s, stream %s per call, kernel %s; host loop "
              "%8.1f ms once, outputs %s" % (name, len(tr), int((tr.clips_host[:, 1] - tr.clips_host[:, 0]).max()), inst_n, int(tr.ntracks.sum()), matched,
                                             single, stream, kernel, host, "equal" if same else "DIFFER"))

    for name, sp, store, inst in P.tracking_cases(a):
        case(name, sp, store, inst)


if __name__ == "__main__":
    P.run("tracks_probe", measure, (("--rounds", 9, None), ("--reps", 50, P.REPS_HELP)))
