"""What scoring a test run's tracks and objects costs: score.score of the predicted chain against the labels' over (a) the synthetic
test partition of tools/results_probe.py (256 whole frames with View-of-Delft's sizes, clustered, tracked and smoothed from the
store an evaluation epoch left and from the labels) taken as 32 clips of 8 frames and as ONE clip of 256, and (b) the coherent world
of tests/tracks_ref.py (rigid objects at constant velocity under a turning ego-motion) repeated to 288 frames in 32 clips.  The
synthetic partition's frames are NOT temporally coherent and its synthetic-weights net predicts nothing useful, so the two sides
share few instances there: (a) times the kernel on whole frames of real size, (b) on what it is for.  Not run by any test; needs the
GPU (no fallback).

  (single)     one call between two device events, the median over ``--rounds`` calls: the fills and the launch latency included;
  (stream)     ``--reps`` calls back to back between two device events, per call, the median over ``--rounds``;
  (kernel)     ``--reps`` calls of the C entry point ``cmf_score_tracks`` itself back to back on prepared arguments, per call: the
               kernel's own time.  One workgroup per clip, so the launch keeps as many CUs busy as there are clips and lasts as long
               as its longest clip;
  (host)       for context only, the loop a user would write without the kernel: the tables copied to the host and the restatement
               of tests/score_ref.py (numpy) over them, once, wall clock -- and whether its outputs equal the kernel's.

Every figure comes with the smallest and largest round (the spread).  There is no bar: the parent commit has nothing to compare with.
The parent process writes the split and never opens the GPU; the measurement is a child process under a time limit.

    python tools/score_probe.py [--frames 256] [--rounds 9] [--reps 50] [--limit 400] [--out profiles/score_probe.txt]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _run_probe as P                               # noqa: E402

GATE, MAX_GAP, IOU = 2.0, 2, 0.5


def measure(a):
    import torch
    import score_ref as ref
    from cmflow_amd import _lib, objects as O, score as S, tracks as K
    print("device: %s; iou %.2f, gate %.1f, max_gap %d; %d rounds, %d calls per stream window; median [smallest .. largest round]"
          % (torch.cuda.get_device_name(0), IOU, GATE, MAX_GAP, a.rounds, a.reps))
    sides = {}

    def tables(obj):
        return {"count": obj.inst.count.cpu().numpy(), "label": obj.inst.label.cpu().numpy(), "track": obj.trk.track.cpu().numpy(),
                "prev_row": obj.trk.prev_row.cpu().numpy()}

    def case(name, sp, pred, gt):                               # its tensors and tables are dropped before the next case
        call = lambda: S.score(pred, gt, sp, iou=IOU)
        sc = call()
        torch.cuda.synchronize()
        single, stream = P.spread(call, 1, a.rounds), P.spread(call, a.reps, a.rounds)
        p, i32 = _lib.dev_ptr, torch.int32
        outs = [getattr(sc, k) for k in ref.KEYS]
        args = (len(sc), len(sp), p(pred.clips, i32), p(sp.off1, i32), sp.tab1.shape[0], IOU, p(gt.inst.count, i32), p(gt.inst.label, i32),
                p(gt.trk.track, i32), p(gt.trk.prev_row, i32), p(pred.inst.count, i32), p(pred.inst.label, i32), p(pred.trk.track, i32),
                *(p(t, t.dtype) for t in outs), _lib.stream_ptr())
        entry = _lib.lib().cmf_score_tracks
        kernel = P.spread(lambda: entry(*args), a.reps, a.rounds)
        t0 = time.perf_counter()
        off1 = sp.off1.cpu().numpy()
        want = ref.score(off1, int(off1[-1]), pred.clips_host, IOU, tables(gt), tables(pred))
        host = 1e3 * (time.perf_counter() - t0)
        try:
            ref.same({k: getattr(sc, k).cpu().numpy() for k in ref.KEYS}, want)
            same = "equal"
        except AssertionError:
            same = "DIFFER"
        print("%-30s %3d clips (longest %3d frames), instances %5d pred / %5d gt: tp %5d fp %5d fn %5d, %3d id switches, %3d fragmentations: single %s, "
              "stream %s per call, kernel %s; host loop %8.1f ms once, outputs %s"
              % (name, len(sc), int((sc.clips_host[:, 1] - sc.clips_host[:, 0]).max()), int(pred.inst.count.sum()), int(gt.inst.count.sum()),
                 int(want["tp"].sum()), int(want["fp"].sum()), int(want["fn"].sum()), int(want["ids"].sum()), int(want["frags"].sum()),
                 single, stream, kernel, host, same))

    # tracking_cases yields a world's 'pred' case and then its 'gt' case over the same clips: score once both sides of a pairing exist
    for name, sp, store, inst in P.tracking_cases(a):
        which = inst.which
        trk = K.track(inst, sp, store if which == "pred" else None, gate=GATE, max_gap=MAX_GAP)
        key = tuple(w for w in name.split() if w not in ("pred", "gt"))
        sides[key, which] = (sp, O.estimate(trk, sp, store if which == "pred" else None))
        if which == "gt":
            for (k, w), (sp2, obj) in list(sides.items()):
                if w == "pred" and (k, "gt") in sides:
                    case(" ".join(k), sp2, obj, sides[k, "gt"][1])
                    del sides[k, "pred"], sides[k, "gt"]


if __name__ == "__main__":
    P.run("score_probe", measure, (("--rounds", 9, None), ("--reps", 50, P.REPS_HELP)))
