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
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from tools.results_probe import EvalArgs, PER_CLIP, clips_of   # noqa: E402  (the same split as the results probe)

GATE, MAX_GAP = 2.0, 2
WORLD_REPEATS = 16


def child(a):
    import numpy as np
    import torch
    import instances_ref as iref
    import objects_ref as ref
    import tracks_ref as tref
    from cmflow_amd import _lib, dataset as D, evaluate as EV, instances as I, objects as O, results as R, synth, tracks as K
    from cmflow_amd.cmflow import CMFlow
    if not torch.cuda.is_available():
        raise SystemExit("objects_probe: needs the GPU")
    dev = torch.device("cuda:0")
    print("device: %s; sigma_pos %.2f, sigma_disp %.2f, sigma_acc %.2f, min_disp %.2f; %d rounds, %d calls per stream window; "
          "median [smallest .. largest round]" % ((torch.cuda.get_device_name(0),) + ref.PARAMS + (a.rounds, a.reps)))

    def timed(fn, reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop) / reps                      # us per call

    def spread(fn, reps):
        v = [timed(fn, reps) for _ in range(a.rounds)]
        return "%7.1f [%7.1f .. %7.1f] us" % (statistics.median(v), min(v), max(v))

    def measure(name, sp, store, inst):
        trk = K.track(inst, sp, store, gate=GATE, max_gap=MAX_GAP)
        call = lambda: O.estimate(trk, sp, store)
        obj = call()
        torch.cuda.synchronize()
        single, stream = spread(call, 1), spread(call, a.reps)
        p, i32, f32 = _lib.dev_ptr, torch.int32, torch.float32
        outs = [getattr(obj, k) for k in ref.KEYS]
        rp, rd, q, m2 = (v * v for v in ref.PARAMS)
        args = (len(trk), len(sp), p(trk.clips, i32), p(sp.off1, i32), sp.tab1.shape[0], p(inst.count, i32), p(inst.label, i32), p(inst.centroid, f32),
                p(inst.disp, f32), p(trk.track, i32), p(trk.prev_row, i32), p(trk.gap, i32), p(sp.tab1, f32), sp.tab1.shape[1], obj.poses.data_ptr(),
                rp, rd, q, m2, *(p(t, t.dtype) for t in outs), _lib.stream_ptr())
        entry = _lib.lib().cmf_track_states
        kernel = spread(lambda: entry(*args), a.reps)
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

    # ---- (a) the synthetic partition
    gold = os.path.join(REPO, "tests", "golden")
    net = CMFlow(EvalArgs())
    net.load_state_dict(synth.synth_state_dict(json.load(open(os.path.join(gold, "state_manifest_cmflow.json"))), seed=1234,
                                               calib=os.path.join(gold, "bn_calib_cmflow.npz")))
    sp = D.DeviceSplit.from_dataset(D.vodDataset(EvalArgs(), a.root, "test"), dev)
    _, store = EV.test_split(net.to(dev).eval(), sp, 16)
    F, counts = len(sp), sp.counts_host[0]
    print("synthetic partition (frames not coherent in time): %d frames of %d-%d points" % (F, counts.min(), counts.max()))
    for which in I.WHICH:
        inst = I.cluster(sp, store if which == "pred" else None, which=which)
        for clips in ([(c, min(c + PER_CLIP, F)) for c in range(0, F, PER_CLIP)], None):
            sp.clips = clips
            measure("synthetic %-4s %s" % (which, "clips of %d" % PER_CLIP if clips else "one clip"), sp, store, inst)
    # ---- (b) the coherent world, repeated
    frames, _ = tref.build_world()
    n = len(frames)
    frames = frames * WORLD_REPEATS
    clips = [(r * n + c0, r * n + c1) for r in range(WORLD_REPEATS) for c0, c1 in tref.WORLD_CLIPS]
    wsp = D.DeviceSplit.from_items(iref.as_items(frames), dev, clips)
    wst = R.SplitResults.empty(wsp)
    wst.flow.copy_(torch.from_numpy(np.concatenate([fr["flow"] for fr in frames])))
    wst.mask.copy_(torch.from_numpy(np.concatenate([fr["mask"] for fr in frames])))
    wst.pred_trans.copy_(torch.from_numpy(np.stack([fr["pred_t"] for fr in frames])))
    wst.done.fill_(1)
    print("coherent world: %d frames of %d-%d points" % (len(wsp), wsp.counts_host[0].min(), wsp.counts_host[0].max()))
    for which in I.WHICH:
        measure("coherent  %-4s" % which, wsp, wst, I.cluster(wsp, wst if which == "pred" else None, which=which))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50, help="calls back to back inside one timed window")
    ap.add_argument("--limit", type=int, default=400, help="seconds for the measurement")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    from cmflow_amd import dataset as D
    with tempfile.TemporaryDirectory(prefix="cmf_objects_probe_") as root:
        D.write_synthetic_split(root, seed=11, clips=clips_of(a.frames))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--frames", str(a.frames),
               "--rounds", str(a.rounds), "--reps", str(a.reps)]
        try:
            done = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit("objects_probe: the measurement did not finish in %d s" % a.limit)
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            raise SystemExit("objects_probe: the measurement ended with status %d" % done.returncode)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(done.stdout)


if __name__ == "__main__":
    main()
