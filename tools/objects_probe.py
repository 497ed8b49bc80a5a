"""What the object states of a test run cost: objects.estimate over the tracks of (a) the synthetic test partition of
tools/results_probe.py (256 whole frames with View-of-Delft's sizes, clustered and tracked from the store an evaluation epoch left
and from the labels) taken as 32 clips of 8 frames and as ONE clip of 256, and (b) the coherent world of tests/tracks_ref.py (rigid
objects at constant velocity under a turning ego-motion) repeated to 288 frames in 32 clips.  The synthetic partition's frames are
NOT temporally coherent -- consecutive frames are unrelated clouds -- so most tracks there are single matches: (a) times the kernel
on many short chains, (b) on what it is for.  Not run by any test; needs the GPU (no fallback).

  (single)     one call between two device events, the median over ``--rounds`` calls: the fills, the pose chain and both launch
               latencies included;
  (stream)     ``--reps`` calls back to back between two device events, per call, the median over ``--rounds``;
  (kernel)     ``--reps`` calls of the C entry point ``cmf_track_states`` itself back to back on prepared arguments, per call: the
               kernel's own time.  One workgroup per clip, so the launch keeps as many CUs busy as there are clips and lasts as long
               as its longest clip;
  (host)       for context only, the loop a user would write without the kernel: the tables copied to the host and the restatement
               of tests/objects_ref.py (numpy, float64) over them, once, wall clock -- and whether its outputs equal the kernel's.

Every figure comes with the smallest and largest round (the spread).  There is no bar: the parent commit has nothing to compare with.
The parent process writes the split and never opens the GPU; the measurement is a child process under a time limit.

    python tools/objects_probe.py [--frames 256] [--rounds 9] [--reps 50] [--limit 400] [--out profiles/objects_probe.txt]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _run_probe as P                               # noqa: E402

GATE, MAX_GAP = 2.0, 2


def measure(a):
    import torch
    import objects_ref as ref
    from cmflow_amd import _lib, objects as O, tracks as K
    print("device: %s; sigma_pos %.2f, sigma_disp %.2f, sigma_acc %.2f, min_disp %.2f; %d rounds, %d calls per stream window; "
          "median [smallest .. largest round]" % ((torch.cuda.get_device_name(0),) + ref.PARAMS + (a.rounds, a.reps)))

    def case(name, sp, store, inst):                            # its tensors and tables are dropped before the next case
        trk = K.track(inst, sp, store, gate=GATE, max_gap=MAX_GAP)
        call = lambda: O.estimate(trk, sp, store)
        obj = call()
        torch.cuda.synchronize()
        single, stream = P.spread(call, 1, a.rounds), P.spread(call, a.reps, a.rounds)
        p, i32, f32 = _lib.dev_ptr, torch.int32, torch.float32
        outs = [getattr(obj, k) for k in ref.KEYS]
        rp, rd, q, m2 = (v * v for v in ref.PARAMS)
        args = (len(trk), len(sp), p(trk.clips, i32), p(sp.off1, i32), sp.tab1.shape[0], p(inst.count, i32), p(inst.label, i32), p(inst.centroid, f32),
                p(inst.disp, f32), p(trk.track, i32), p(trk.prev_row, i32), p(trk.gap, i32), p(sp.tab1, f32), sp.tab1.shape[1], obj.poses.data_ptr(),
                rp, rd, q, m2, *(p(t, t.dtype) for t in outs), _lib.stream_ptr())
        entry = _lib.lib().cmf_track_states
        kernel = P.spread(lambda: entry(*args), a.reps, a.rounds)
        t0 = time.perf_counter()
        off1 = sp.off1.cpu().numpy()
        want = ref.states(off1, int(off1[-1]), inst.count.cpu().numpy(), inst.label.cpu().numpy(), inst.centroid.cpu().numpy(), inst.disp.cpu().numpy(),
                          trk.track.cpu().numpy(), trk.prev_row.cpu().numpy(), trk.gap.cpu().numpy(), sp.tab1.cpu().numpy(), obj.poses.cpu().numpy(),
                          trk.clips_host, *ref.PARAMS)
        host = 1e3 * (time.perf_counter() - t0)
        try:
            ref.same({k: getattr(obj, k).cpu().numpy() for k in ref.KEYS}, want)
            same = "equal"
        except AssertionError:
            same = "DIFFER"
        chains = ref.chains(want, int(off1[-1]))
        print("%-34s %3d clips (longest %3d frames), %5d instances, %5d tracks (longest %3d matches), %5d headings from velocity: single %s, stream %s "
              "per call, kernel %s; host loop %8.1f ms once, outputs %s"
              % (name, len(trk), int((trk.clips_host[:, 1] - trk.clips_host[:, 0]).max()), int(inst.count.sum()), len(chains), max(len(c) for c in chains),
                 int((obj.heading_src == 1).sum()), single, stream, kernel, host, same))

    for name, sp, store, inst in P.tracking_cases(a):
        case(name, sp, store, inst)


if __name__ == "__main__":
    P.run("objects_probe", measure, (("--rounds", 9, None), ("--reps", 50, P.REPS_HELP)))
