"""What the probes of a test run's analysis chain share (results_probe, vis_probe, accumulate_probe, instances_probe, tracks_probe,
objects_probe, score_probe): the parent/child runner, the timing of a call between two device events, and the two fixtures they measure on.

    run(name, measure, options)   the parent parses the command line, writes the synthetic split and never opens the GPU; the
                                  measurement -- measure(a), a.root the split's directory -- is a child process under --limit
    timed / spread                us per call between two device events; spread: median [smallest .. largest round]
    synthetic_net_split / synthetic_store   the synthetic test partition, the synthetic-weights net, its evaluation epoch's store
    coherent_world / tracking_cases         the coherent world of tests/tracks_ref.py repeated, with its filled store; the cases
                                  tracks_probe, objects_probe and score_probe go through on both
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))                 # the numpy restatements (*_ref.py)

PER_CLIP = 8
WORLD_REPEATS = 16
REPS_HELP = "calls back to back inside one timed window"


class EvalArgs:
    num_points, eval, stat_thres = 256, True, 0.5


def clips_of(frames):
    return tuple(("test", "delft_%d" % (c + 1), tuple(87 + (37 * c + 53 * f) % 375 for f in range(PER_CLIP)))
                 for c in range(frames // PER_CLIP))


def run(name, measure, options, out=True):
    """``options``: (flag, default, help) of the probe's own whole-number options, after --frames and before --limit [--out]."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    for flag, default, text in options:
        ap.add_argument(flag, type=int, default=default, help=text)
    ap.add_argument("--limit", type=int, default=400, help="seconds for the measurement")
    if out:
        ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("%s: needs the GPU" % name)
        return measure(a)
    from cmflow_amd import dataset as D
    with tempfile.TemporaryDirectory(prefix="cmf_%s_" % name) as root:
        D.write_synthetic_split(root, seed=11, clips=clips_of(a.frames))
        cmd = [sys.executable, os.path.abspath(sys.argv[0]), "--child", "--root", root]
        for flag in ["--frames"] + [o[0] for o in options]:
            cmd += [flag, str(getattr(a, flag[2:]))]
        try:
            done = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit("%s: the measurement did not finish in %d s" % (name, a.limit))
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            raise SystemExit("%s: the measurement ended with status %d" % (name, done.returncode))
        if out and a.out:
            with open(a.out, "w") as fh:
                fh.write(done.stdout)


def timed(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps                          # us per call


def spread(fn, reps, rounds):
    v = [timed(fn, reps) for _ in range(rounds)]
    return "%7.1f [%7.1f .. %7.1f] us" % (statistics.median(v), min(v), max(v))


def synthetic_net_split(a):
    """-> (the net with the synthetic weights on the GPU in eval mode, the synthetic partition under a.root as a DeviceSplit)"""
    import torch
    from cmflow_amd import dataset as D, synth
    from cmflow_amd.cmflow import CMFlow
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    net = CMFlow(EvalArgs())
    net.load_state_dict(synth.synth_state_dict(json.load(open(os.path.join(gold, "state_manifest_cmflow.json"))), seed=1234,
                                               calib=os.path.join(gold, "bn_calib_cmflow.npz")))
    sp = D.DeviceSplit.from_dataset(D.vodDataset(EvalArgs(), a.root, "test"), dev)
    return net.to(dev).eval(), sp


def synthetic_store(a):
    """-> (the synthetic partition, the store an evaluation epoch over it left)"""
    from cmflow_amd import evaluate as EV
    net, sp = synthetic_net_split(a)
    return sp, EV.test_split(net, sp, 16)[1]


def coherent_world():
    """-> (the world of tests/tracks_ref.py repeated WORLD_REPEATS times as a DeviceSplit with its clips, its store filled from the world)"""
    import numpy as np
    import torch
    import instances_ref as iref
    import tracks_ref as tref
    from cmflow_amd import dataset as D, results as R
    frames, _ = tref.build_world()
    n = len(frames)
    frames = frames * WORLD_REPEATS
    clips = [(r * n + c0, r * n + c1) for r in range(WORLD_REPEATS) for c0, c1 in tref.WORLD_CLIPS]
    wsp = D.DeviceSplit.from_items(iref.as_items(frames), torch.device("cuda:0"), clips)
    wst = R.SplitResults.empty(wsp)
    wst.flow.copy_(torch.from_numpy(np.concatenate([fr["flow"] for fr in frames])))
    wst.mask.copy_(torch.from_numpy(np.concatenate([fr["mask"] for fr in frames])))
    wst.pred_trans.copy_(torch.from_numpy(np.stack([fr["pred_t"] for fr in frames])))
    wst.done.fill_(1)
    return wsp, wst


def tracking_cases(a):
    """(name, split, store, instances) of (a) the synthetic partition, pred and gt, as clips of PER_CLIP frames and as one clip, and
    (b) the coherent world, pred and gt -- each part announced by its line."""
    from cmflow_amd import instances as I
    sp, store = synthetic_store(a)
    F, counts = len(sp), sp.counts_host[0]
    print("synthetic partition (frames not coherent in time): %d frames of %d-%d points" % (F, counts.min(), counts.max()))
    for which in I.WHICH:
        inst = I.cluster(sp, store if which == "pred" else None, which=which)
        for clips in ([(c, min(c + PER_CLIP, F)) for c in range(0, F, PER_CLIP)], None):
            sp.clips = clips
            yield "synthetic %-4s %s" % (which, "clips of %d" % PER_CLIP if clips else "one clip"), sp, store, inst
    wsp, wst = coherent_world()
    print("coherent world: %d frames of %d-%d points" % (len(wsp), wsp.counts_host[0].min(), wsp.counts_host[0].max()))
    for which in I.WHICH:
        yield "coherent  %-4s" % which, wsp, wst, I.cluster(wsp, wst if which == "pred" else None, which=which)
