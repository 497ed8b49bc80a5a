"""What the augmentation costs on a train_epoch-style step (CMFlow, B = 64, N = 256, one GPU: the batch drawn from a DeviceSplit, then
one TrainStep), and whether this build's step without it is the parent commit's.

    CMF_LIB=<the parent commit's libcmflow_hip.so> python tools/augment_probe.py [--out profiles/augment_probe.txt] [--steps 50] [--rounds 3]

Three variants, each on its own network from the same weights, alternated in ONE process (other work shares the host: only numbers
taken side by side compare), 5 warm-up steps and `--steps` timed steps per variant and round, device events around the timed steps
-- the scheme of tools/ema_probe.py:

  (a) the parent commit's library: a build of the parent in a scratch directory, its path given in CMF_LIB -- every kernel of the
      step comes from it (it reads the loss descriptor without the field this build appends);
  (b) this build (the in-tree library), augmentation off: ``split.draw(...)`` then the step;
  (c) this build, ``split.draw(..., augment=Augment(10, True))`` then the step: one launch more, and the loss reads a calibration
      per sample.

Both libraries are loaded side by side and ``cmflow_amd._lib`` is pointed at the one a variant belongs to in front of its steps.  Then
``augment_batch`` alone on a resident batch, an event pair around each call (median) and around a train of calls.  (b) - (a) is to be
read against the spread of (a)'s own rounds; (c) - (b) is what the feature costs."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench                                       # noqa: E402  (Args, load_weights: the benchmark's model and weights)
from cmflow_amd import _lib, synth                 # noqa: E402
from cmflow_amd.cmflow import CMFlow               # noqa: E402
from cmflow_amd.dataset import Augment, DeviceSplit, augment_batch     # noqa: E402
from cmflow_amd.train import TrainStep             # noqa: E402

IN_TREE = os.path.join(ROOT, "cmflow_amd", "libcmflow_hip.so")


def load(path, need_all):
    """A library handle with the ctypes signatures of _lib.lib(); the parent's lacks the symbols this build adds."""
    handle = ctypes.CDLL(path)
    for name, argtypes in _lib.SIGNATURES.items():
        fn = getattr(handle, name, None)
        if fn is None:
            if need_all:
                raise RuntimeError("%s has no %s" % (path, name))
            continue
        fn.argtypes = argtypes
        fn.restype = _lib.RESTYPES.get(name, _lib._ci)
    handle.cmf_version.restype = ctypes.c_char_p
    return handle


def make_net(dev):
    net = CMFlow(bench.Args())
    net.load_state_dict(bench.load_weights("cmflow"))
    return net.to(dev).train()


def make_split(frames, dev):
    """`frames` whole frames of 200 .. 330 points cut from seeded synthetic scenes (around the 256 a batch is resampled to)."""
    items = []
    for k in range(frames):
        n1, n2 = 200 + (37 * k) % 131, 200 + (53 * k) % 131
        b = synth.make_batch(1, N=max(n1, n2), seed=9000 + k, train_extras=True)
        rows = lambda key, n: np.ascontiguousarray(b[key][0].t().numpy()[:n])
        items.append((rows("pc1", n1), rows("pc2", n2), rows("ft1", n1), rows("ft2", n2), b["gt_trans"][0].numpy(),
                      b["flow_label"][0].numpy()[:n1], b["fg_mask"][0].numpy()[:n1], 0.1, b["radar_u"][0].numpy()[:n1],
                      b["radar_v"][0].numpy()[:n1], b["opt_flow"][0].numpy()[:n1]))
    return DeviceSplit.from_items(items, dev)


def timed_ms(fn, steps):
    """ms per call over `steps` calls, device events around all of them."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def each_us(fn, calls):
    """Median us of one call, an event pair around each."""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(1e3 * a.elapsed_time(b) for a, b in pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_probe.txt"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--yaw", type=float, default=10.0)
    a = ap.parse_args()
    parent_path = os.environ.get("CMF_LIB")
    if not parent_path or os.path.abspath(parent_path) == os.path.abspath(IN_TREE) or not os.path.exists(parent_path):
        sys.exit("augment_probe: set CMF_LIB to a build of the parent commit's library (variant (a)); without it nothing compares")
    if not torch.cuda.is_available():
        sys.exit("augment_probe: needs a GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    libs = {"parent": load(parent_path, False), "this": load(IN_TREE, True)}
    if hasattr(libs["parent"], "cmf_augment_batch"):
        sys.exit("augment_probe: %s already has cmf_augment_batch -- it is not the parent's library" % parent_path)

    def use(which):
        _lib._lib = libs[which]

    use("this")
    split = make_split(a.batch, dev)
    frames = torch.arange(a.batch, dtype=torch.int32, device=dev)
    aug = Augment(a.yaw, True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    class Variant:
        def __init__(self, name, which, augment):
            self.name, self.which, self.augment = name, which, augment
            self.step = TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres)
            self.tcr = self.step.loss_obj.t_camera_radar
            self.draws = 0

        def __call__(self):                         # what train_epoch does per step: draw (and augment) on the device, then the step
            self.draws += 1
            self.step(split.draw(frames, 256, 1234, self.draws, 0, self.augment, None, self.tcr if self.augment is not None else None))

    variants = [Variant("(a) parent's library", "parent", None), Variant("(b) this build, augmentation off", "this", None),
                Variant("(c) this build, %r" % (aug,), "this", aug)]
    say("CMFlow B = %d, N = 256 drawn from a DeviceSplit of %d frames, %s; parent %s, this build %s"
        % (a.batch, len(split), torch.cuda.get_device_name(dev), libs["parent"].cmf_version().decode(), libs["this"].cmf_version().decode()))
    results = {v.name: [] for v in variants}
    for r in range(a.rounds):
        for v in variants[r % 3:] + variants[:r % 3]:      # the order rotates: no variant always runs behind the same one
            use(v.which)
            for _ in range(a.warmup):
                v()
            torch.cuda.synchronize()
            results[v.name].append(timed_ms(v, a.steps))
            torch.cuda.synchronize()
    say("ms per draw + training step, %d timed steps behind %d warm-ups, rounds in order (round r starts with variant r mod 3):" % (a.steps, a.warmup))
    for v in variants:
        x = results[v.name]
        say("  %-46s %s   median %.3f, spread (max - min) %.3f" % (v.name, "  ".join("%.3f" % t for t in x), statistics.median(x), max(x) - min(x)))
    names = [v.name for v in variants]
    for hi, lo in ((1, 0), (2, 1), (2, 0)):
        d = [x - y for x, y in zip(results[names[hi]], results[names[lo]])]
        say("  %s - %s, per round: %s ms; of the medians %+.3f ms"
            % (names[hi][:3], names[lo][:3], "  ".join("%+.3f" % x for x in d),
               statistics.median(results[names[hi]]) - statistics.median(results[names[lo]])))
    same = all(torch.equal(p, q) for p, q in zip(variants[0].step.net.parameters(), variants[1].step.net.parameters()))
    say("  parameters after %d steps each: (a) == (b) bit for bit: %s" % (a.rounds * (a.warmup + a.steps), same))

    # the launch alone, on resident batches: the dense training batch and a ragged one of whole frames
    use("this")
    tcr = variants[2].tcr
    say("augment_batch alone (us; an event pair around each of 200 calls, median | 200 calls back to back, per call; %d rounds):" % a.rounds)
    for what, batch in (("drawn batch (%d, 3, 256)" % a.batch, split.draw(frames, 256, 1234, 0)),
                        ("whole frames, ragged", split.draw_frames(frames))):
        call = lambda: augment_batch(batch, aug, 1234, 7, 0, tcr)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        one, train = zip(*[(each_us(call, 200), 1e3 * timed_ms(call, 200)) for _ in range(a.rounds)])
        say("  %-32s %s | %s   medians %.1f | %.1f   (pc1 %s)" % (what, "  ".join("%.1f" % x for x in one), "  ".join("%.1f" % x for x in train),
                                                                 statistics.median(one), statistics.median(train), tuple(batch["pc1"].shape)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
