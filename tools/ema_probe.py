"""What the averaged weights cost on the benchmark's training step (CMFlow, B = 64, N = 256, one GPU), and whether turning the
optimizer kernels into template instantiations changed the step without them.

    CMF_LIB=<the parent commit's libcmflow_hip.so> python tools/ema_probe.py [--out profiles/ema_probe.txt] [--steps 50] [--rounds 3]

Three variants, each on its own network from the same weights, alternated in ONE process (other work shares the host: only numbers
taken side by side compare), 5 warm-up steps and `--steps` timed steps per variant and round, device events around the timed steps:

  (a) the parent commit's library: a build of the parent in a scratch directory, its path given in CMF_LIB -- every kernel of the
      step comes from it;
  (b) this build (the in-tree library), averaged weights off;
  (c) this build, TrainStep(ema_decay=0.999).

Both libraries are loaded side by side and ``cmflow_amd._lib`` is pointed at the one a variant belongs to in front of its steps.  Then
the optimizer launches alone on a resident bucket -- ``opt.step()`` of the three variants, an event pair around each call (median)
and around a train of calls -- and one ``ema_weights()`` enter + exit pair.  (b) - (a) is to be read against the spread of (a)'s own
rounds: it is the parent's kernel re-instantiated.  (c) - (b) is what the feature costs: one more read and one more write of the
bucket's floats per step."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench                                       # noqa: E402  (Args, load_weights: the benchmark's model and weights)
from cmflow_amd import _lib, synth                 # noqa: E402
from cmflow_amd.cmflow import CMFlow               # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_probe.txt"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--decay", type=float, default=0.999)
    a = ap.parse_args()
    parent_path = os.environ.get("CMF_LIB")
    if not parent_path or os.path.abspath(parent_path) == os.path.abspath(IN_TREE) or not os.path.exists(parent_path):
        sys.exit("ema_probe: set CMF_LIB to a build of the parent commit's library (variant (a)); without it nothing compares")
    if not torch.cuda.is_available():
        sys.exit("ema_probe: needs a GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    libs = {"parent": load(parent_path, False), "this": load(IN_TREE, True)}
    if hasattr(libs["parent"], "cmf_param_exchange"):
        sys.exit("ema_probe: %s already has cmf_param_exchange -- it is not the parent's library" % parent_path)

    def use(which):
        _lib._lib = libs[which]

    batch = {k: v.to(dev) for k, v in synth.make_batch(a.batch, seed=1234, train_extras=True).items()}
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    use("this")
    variants = [("(a) parent's library", "parent", TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres)),
                ("(b) this build, average off", "this", TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres)),
                ("(c) this build, ema_decay=%g" % a.decay, "this", TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres, ema_decay=a.decay))]
    numel = variants[0][2].bucket.numel
    say("CMFlow B = %d, N = 256, %s; bucket %d floats (%.1f MB); parent %s, this build %s"
        % (a.batch, torch.cuda.get_device_name(dev), numel, numel * 4 / 1e6, libs["parent"].cmf_version().decode(),
           libs["this"].cmf_version().decode()))
    results = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, which, step in variants[r % 3:] + variants[:r % 3]:      # the order rotates: no variant always runs behind the same one
            use(which)
            for _ in range(a.warmup):
                step(batch)
            torch.cuda.synchronize()
            results[name].append(timed_ms(lambda: step(batch), a.steps))
            torch.cuda.synchronize()
    say("ms per training step, %d timed steps behind %d warm-ups, rounds in order (round r starts with variant r mod 3):" % (a.steps, a.warmup))
    for name, _, _ in variants:
        v = results[name]
        say("  %-32s %s   median %.3f, spread (max - min) %.3f" % (name, "  ".join("%.3f" % x for x in v), statistics.median(v), max(v) - min(v)))
    names = [name for name, _, _ in variants]
    for hi, lo in ((1, 0), (2, 1), (2, 0)):
        d = [x - y for x, y in zip(results[names[hi]], results[names[lo]])]
        say("  %s - %s, per round: %s ms; of the medians %+.3f ms"
            % (names[hi][:3], names[lo][:3], "  ".join("%+.3f" % x for x in d),
               statistics.median(results[names[hi]]) - statistics.median(results[names[lo]])))
    same = all(torch.equal(p, q) for p, q in zip(variants[0][2].net.parameters(), variants[1][2].net.parameters()))
    same_c = all(torch.equal(p, q) for p, q in zip(variants[1][2].net.parameters(), variants[2][2].net.parameters()))
    say("  parameters after %d steps each: (a) == (b) bit for bit: %s; (b) == (c): %s" % (a.rounds * (a.warmup + a.steps), same, same_c))

    # the optimizer launches alone: the buckets hold the last step's gradient, nothing else runs
    alone = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, which, step in variants[r % 3:] + variants[:r % 3]:
            use(which)
            for _ in range(20):
                step.opt.step()
            torch.cuda.synchronize()
            alone[name].append((each_us(step.opt.step, 200), 1e3 * timed_ms(step.opt.step, 200)))
            torch.cuda.synchronize()
    say("optimizer launch alone, bucket resident (us; an event pair around each of 200 calls, median | 200 calls back to back, per call;")
    say("%d rounds in the same rotating order, then their medians):" % a.rounds)
    rows = []
    for name, _, _ in variants:
        one, train = zip(*alone[name])
        rows.append((name, statistics.median(one), statistics.median(train)))
        say("  %-32s %s | %s" % (name, "  ".join("%.1f" % x for x in one), "  ".join("%.1f" % x for x in train)))
    for name, one, train in rows:
        say("  %-32s %8.1f | %8.1f" % (name, one, train))
    say("  %-32s %+8.1f | %+8.1f" % ("(b) - (a)", rows[1][1] - rows[0][1], rows[1][2] - rows[0][2]))
    say("  %-32s %+8.1f | %+8.1f" % ("(c) - (b)", rows[2][1] - rows[1][1], rows[2][2] - rows[1][2]))
    use("this")
    opt = variants[2][2].opt

    def pair():
        with opt.ema_weights():
            pass
    for _ in range(20):
        pair()
    torch.cuda.synchronize()
    say("  %-32s %8.1f | %8.1f   (two cmf_param_exchange launches)" % ("ema_weights() enter + exit", each_us(pair, 200), 1e3 * timed_ms(pair, 200)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
