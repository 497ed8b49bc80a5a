"""One evaluation epoch over whole frames, three ways, on a synthetic test partition of a few hundred frames with View-of-Delft's
sizes (87-461 points).  Not run by any test; needs the GPU (no fallback).

  (split)     evaluate.eval_split on a DeviceSplit: frames drawn on the GPU (cmf_draw_frames), forward_ragged, eval_batch_ragged,
              nothing read back inside the loop -- in frame order and with sort_by_size;
  (collated)  DataLoader(vodDataset, collate_fn=collate_ragged) -> extract_data_info_ragged -> forward_ragged -> eval_batch_ragged:
              the same batches assembled on the host (JSON decode, padding, thirteen host-to-device copies per batch);
  (per_frame) DataLoader(vodDataset, batch_size=1) -> extract_data_info -> dense forward -> eval_batch: the reference's own loop
              (main.py:203).

Per run: wall-clock ms per frame over timed epochs that end in a device synchronise (one warm-up epoch first), and "host": the
time until the epoch's loop returns.  For eval_split, which never waits for the device, that is the enqueue time, and a total
above it is GPU time the host did not cover.  The two loader loops wait for the stream in every blocking host-to-device copy, so
their "host" contains the GPU time of all batches but the last and says nothing about which side bounds them.  Also, from the frame sizes alone, the padded share of cloud-1
positions (dataset.padding_share) of shuffled epochs cut with bucket = 1 and bucket = 4, and of the two sweeps.

The parent process writes the split and never opens the GPU; every run is a child process of its own under a time limit, and the
first one that fails or runs out of time ends the probe.

    python tools/device_eval_probe.py [--frames 256] [--batch 16] [--epochs 20] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
RUNS = ("split", "collated", "per_frame")
PER_CLIP = 8


class EvalArgs:
    num_points, eval, stat_thres = 256, True, 0.5


def clips_of(frames):
    return tuple(("test", "delft_%d" % (c + 1), tuple(87 + (37 * c + 53 * f) % 375 for f in range(PER_CLIP)))
                 for c in range(frames // PER_CLIP))


def timed(epochs, one_epoch):
    """one_epoch() enqueues an epoch and returns its frame count -> (ms per frame, host ms per frame) over `epochs` timed epochs."""
    import torch
    one_epoch()                                       # warm-up: page cache, worker start, first launches
    torch.cuda.synchronize()
    frames, host, t0 = 0, 0.0, time.perf_counter()
    for _ in range(epochs):
        t = time.perf_counter()
        frames += one_epoch()
        host += time.perf_counter() - t
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames, host * 1e3 / frames


def child(a):
    import torch
    from torch.utils.data import DataLoader
    from cmflow_amd import dataset as D, eval_util as E, evaluate as EV, synth
    from cmflow_amd.cmflow import CMFlow
    if not torch.cuda.is_available():
        raise SystemExit("device_eval_probe: needs the GPU")
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    net = CMFlow(EvalArgs())
    net.load_state_dict(synth.synth_state_dict(json.load(open(os.path.join(gold, "state_manifest_cmflow.json"))), seed=1234,
                                               calib=os.path.join(gold, "bn_calib_cmflow.npz")))
    net = net.to(dev).eval()
    ds = D.vodDataset(EvalArgs(), a.root, "test")
    if a.only == "split":
        t0 = time.perf_counter()
        sp = D.DeviceSplit.from_dataset(ds, dev)
        torch.cuda.synchronize()
        print("split: %d frames, %d + %d points, packed once in %.2f s (JSON decode included); device: %s; batch %d; %d timed epochs"
              % (len(sp), sp.tab1.shape[0], sp.tab2.shape[0], time.perf_counter() - t0, torch.cuda.get_device_name(0), a.batch, a.epochs))
        n1 = sp.counts_host[0]
        for bucket in (1, 4):
            shares = [D.padding_share(n1, D.ragged_batches(n1, sp._order(len(sp), 1, e).tolist(), a.batch, bucket)) for e in range(8)]
            print("padding_share, shuffled epochs, bucket = %d: %.3f (mean of 8 epochs)" % (bucket, sum(shares) / len(shares)))
        for sort in (False, True):
            order = sorted(range(len(sp)), key=lambda f: (int(n1[f]), f)) if sort else range(len(sp))
            share = D.padding_share(n1, D.ragged_batches(n1, order, a.batch))

            def epoch():
                EV.eval_split(net, sp, a.batch, sort_by_size=sort)
                return len(sp)
            ms, host = timed(a.epochs, epoch)
            print("eval_split, sort_by_size = %-5s (padding_share %.3f):             %7.3f ms per frame, host %7.3f" % (sort, share, ms, host))
    elif a.only == "collated":
        dl = DataLoader(ds, batch_size=a.batch, shuffle=False, collate_fn=D.collate_ragged)

        def epoch():
            acc, frames = torch.zeros(14, dtype=torch.float64, device=dev), 0
            with torch.no_grad():
                for data in dl:
                    pc1, pc2, ft1, ft2, trans, gt, mask, _, _, _, _, n1, n2 = D.extract_data_info_ragged(data, device=dev)
                    sf, _, pt, mk = net.forward_ragged(pc1, pc2, ft1, ft2, n1, n2)
                    m = E.eval_batch_ragged(pc1, sf.transpose(1, 2).contiguous(), gt, mask, mk.float(), trans, pt, n1)
                    acc = acc + pc1.shape[0] * torch.stack([v for d in m for v in d.values()])
                    frames += pc1.shape[0]
            return frames
        ms, host = timed(a.epochs, epoch)
        print("DataLoader + collate_ragged, batch %d, forward_ragged:                    %7.3f ms per frame, host %7.3f" % (a.batch, ms, host))
    else:
        dl = DataLoader(ds, batch_size=1, shuffle=False)

        def epoch():
            acc, frames = torch.zeros(14, dtype=torch.float64, device=dev), 0
            with torch.no_grad():
                for data in dl:
                    pc1, pc2, ft1, ft2, trans, gt, mask = D.extract_data_info(data, device=dev)[:7]
                    sf, _, pt, mk = net(pc1, pc2, ft1, ft2, None, "test")
                    m = E.eval_batch(pc1, sf.transpose(1, 2).contiguous(), gt, mask, mk.float(), trans, pt)
                    acc = acc + torch.stack([v for d in m for v in d.values()])
                    frames += 1
            return frames
        ms, host = timed(a.epochs, epoch)
        print("DataLoader batch_size = 1, dense forward (the reference's loop):          %7.3f ms per frame, host %7.3f" % (ms, host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds per run")
    ap.add_argument("--only", choices=RUNS, help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.only:
        return child(a)
    from cmflow_amd import dataset as D
    with tempfile.TemporaryDirectory(prefix="cmf_eval_probe_") as root:
        D.write_synthetic_split(root, seed=11, clips=clips_of(a.frames))
        for run in RUNS:
            cmd = [sys.executable, os.path.abspath(__file__), "--only", run, "--root", root, "--frames", str(a.frames),
                   "--batch", str(a.batch), "--epochs", str(a.epochs)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit("device_eval_probe: run '%s' did not finish in %d s; nothing further is started" % (run, a.limit))
            if rc != 0:
                raise SystemExit("device_eval_probe: run '%s' ended with status %d; nothing further is started" % (run, rc))


if __name__ == "__main__":
    main()
