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
    import tracks_ref as ref
    from cmflow_amd import _lib, dataset as D, evaluate as EV, instances as I, results as R, synth, tracks as K
    from cmflow_amd.cmflow import CMFlow
    if not torch.cuda.is_available():
        raise SystemExit("tracks_probe: needs the GPU")
    dev = torch.device("cuda:0")
    print("device: %s; gate %.1f, max_gap %d; %d rounds, %d calls per stream window; median [smallest .. largest round]"
          % (torch.cuda.get_device_name(0), GATE, MAX_GAP, a.rounds, a.reps))

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
        call = lambda: K.track(inst, sp, store, gate=GATE, max_gap=MAX_GAP)
        tr = call()
        torch.cuda.synchronize()
        single, stream = spread(call, 1), spread(call, a.reps)
        p, i32, f32 = _lib.dev_ptr, torch.int32, torch.float32
        T = store.pred_trans if inst.which == "pred" else sp.trans
        outs = (tr.track, tr.prev_row, tr.gap, tr.age, tr.pred, tr.point_track, tr.birth, tr.last, tr.hits)
        args = (len(tr), len(sp), p(tr.clips, i32), p(sp.off1, i32), sp.tab1.shape[0], p(inst.count, i32), p(inst.label, i32), p(inst.centroid, f32),
                p(inst.disp, f32), p(T.reshape(-1, 16), f32), GATE * GATE, MAX_GAP, *(p(t, f32 if t.dtype == f32 else i32) for t in outs),
                p(tr.ntracks, i32), p(tr.overflow, i32), _lib.stream_ptr())
        entry = _lib.lib().cmf_track_instances
        kernel = spread(lambda: entry(*args), a.reps)
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
    frames, _ = ref.build_world()
    n = len(frames)
    frames = frames * WORLD_REPEATS
    clips = [(r * n + c0, r * n + c1) for r in range(WORLD_REPEATS) for c0, c1 in ref.WORLD_CLIPS]
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
    with tempfile.TemporaryDirectory(prefix="cmf_tracks_probe_") as root:
        D.write_synthetic_split(root, seed=11, clips=clips_of(a.frames))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--frames", str(a.frames),
               "--rounds", str(a.rounds), "--reps", str(a.reps)]
        try:
            done = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit("tracks_probe: the measurement did not finish in %d s" % a.limit)
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            raise SystemExit("tracks_probe: the measurement ended with status %d" % done.returncode)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(done.stdout)


if __name__ == "__main__":
    main()
