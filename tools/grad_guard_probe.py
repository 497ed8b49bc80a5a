"""What the guarded optimizer step costs on the benchmark's training step (CMFlow, B = 64, N = 256, one GPU).

    python tools/grad_guard_probe.py [--out profiles/grad_guard_probe.txt] [--steps 50] [--rounds 3]

Three variants, each on its own network from the same weights, alternated in ONE process (other work shares the host: only numbers
taken side by side compare), 5 warm-up steps and `--steps` timed steps per variant and round, device events around the timed steps:

  (a) TrainStep, guard off;
  (b) TrainStep(max_grad_norm = the run's median norm, skip_nonfinite=True): cmf_grad_sumsq + cmf_adam_step_guarded;
  (c) torch.nn.utils.clip_grad_norm_(bucket.params, the same norm) in front of the unguarded step: what one would write without (b).

and the optimizer launches alone on a resident bucket: ``opt.step()`` guarded and unguarded, an event pair around each call (median)
and around a train of calls.  (b) - (a) is to be read against the spread of (a) over the rounds; (c) is context."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench                                       # noqa: E402  (Args, load_weights: the benchmark's model and weights)
from cmflow_amd import dp, synth                   # noqa: E402
from cmflow_amd.cmflow import CMFlow               # noqa: E402
from cmflow_amd.train import TrainStep             # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard_probe.txt"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grad_guard_probe: needs a GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    batch = {k: v.to(dev) for k, v in synth.make_batch(a.batch, seed=1234, train_extras=True).items()}
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    # the run's median norm: the first steps of the benchmark's run, the norm of each step's bucket read between the steps
    scout = TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres, skip_nonfinite=True)
    norms = []
    for _ in range(a.warmup + 10):
        scout(batch)
        norms.append(float(dp.grad_norm(scout.bucket)))
    median = statistics.median(norms)
    say("CMFlow B = %d, N = 256, %s; bucket %d floats (%.1f MB), %d workgroups in the sum of squares"
        % (a.batch, torch.cuda.get_device_name(dev), scout.bucket.numel, scout.bucket.numel * 4 / 1e6, scout.opt._partials.numel()))
    say("gradient norm over the first %d steps: median %.6g, min %.6g, max %.6g; record %s"
        % (len(norms), median, min(norms), max(norms), [round(v, 6) for v in scout.opt.guard_stats().tolist()]))
    del scout

    plain = TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres)
    guarded = TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres, max_grad_norm=median, skip_nonfinite=True)
    by_hand = TrainStep(make_net(dev), vr_thres=bench.Args.vr_thres)
    unclipped_step = by_hand.opt.step

    def clipped_step():
        torch.nn.utils.clip_grad_norm_(by_hand.bucket.params, median)
        return unclipped_step()
    by_hand.opt.step = clipped_step
    variants = [("(a) guard off", plain), ("(b) guard on", guarded), ("(c) clip_grad_norm_ + step", by_hand)]
    results = {name: [] for name, _ in variants}
    for r in range(a.rounds):
        for name, step in variants:
            for _ in range(a.warmup):
                step(batch)
            torch.cuda.synchronize()
            results[name].append(timed_ms(lambda: step(batch), a.steps))
    say("ms per training step, %d timed steps behind %d warm-ups, rounds in order:" % (a.steps, a.warmup))
    for name, _ in variants:
        v = results[name]
        say("  %-28s %s   median %.3f, spread (max - min) %.3f" % (name, "  ".join("%.3f" % x for x in v), statistics.median(v), max(v) - min(v)))
    base = results["(a) guard off"]
    for name in ("(b) guard on", "(c) clip_grad_norm_ + step"):
        d = [x - y for x, y in zip(results[name], base)]
        say("  %s - (a), per round: %s ms; of the medians %+.3f ms" % (name[:3], "  ".join("%+.3f" % x for x in d),
                                                                      statistics.median(results[name]) - statistics.median(base)))
    rec = guarded.opt.guard_stats().tolist()
    say("  (b) record: %d calls, %d non-finite, %d clipped, last norm %.6g, last scale %.6g" % (rec[0], rec[1], rec[2], rec[6], rec[7]))

    # the optimizer launches alone: the buckets hold the last step's gradient, nothing else runs
    for _ in range(20):
        plain.opt.step(); guarded.opt.step()
    torch.cuda.synchronize()
    rows = []
    for name, opt in (("cmf_adam_step", plain.opt), ("cmf_grad_sumsq + cmf_adam_step_guarded", guarded.opt)):
        rows.append((name, each_us(opt.step, 200), 1e3 * timed_ms(opt.step, 200)))
    norm_us = each_us(lambda: dp.grad_norm(guarded.bucket), 200)
    say("optimizer launches alone, bucket resident (us; an event pair around each of 200 calls, median | 200 calls back to back, per call):")
    for name, one, train in rows:
        say("  %-42s %8.1f | %8.1f" % (name, one, train))
    say("  %-42s %+8.1f | %+8.1f" % ("guarded - unguarded", rows[1][1] - rows[0][1], rows[1][2] - rows[0][2]))
    say("  %-42s %8.1f   (two launches and two small allocations)" % ("dp.grad_norm", norm_us))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
