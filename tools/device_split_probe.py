"""Feeding the train step: items per second of the reference-style loader against a device-resident split, and the time of one
cmf_draw_batch.  Not run by any test; needs the GPU (no fallback).

  (a) DataLoader(vodDataset) over a synthetic split written to disk (dataset.write_synthetic_split with enlarged ``clips``): JSON
      decode, numpy resampling, default_collate, then extract_data_info (eleven host-to-device copies, four transposes) -- with
      0 and with --workers worker processes;
  (b) DeviceSplit.epoch over the same frames: one kernel per batch, nothing on the host but the launch;
  (c) one cmf_draw_batch at B = 64, N = 256, timed with device events over many launches.

Every figure is a host clock around work that ends in a device synchronise (a, b) or device events (c); the split's frames have
the sizes write_synthetic_split uses elsewhere (180-400 points).

    python tools/device_split_probe.py [--frames 512] [--batch 64] [--workers 2] [--epochs 3]
"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from cmflow_amd import dataset as D  # noqa: E402


class TrainArgs:
    num_points, eval = 256, False


class EvalArgs:
    num_points, eval = 256, True


def loader_rate(root, batch, workers, epochs, dev):
    ds = D.vodDataset(TrainArgs(), root, "train")
    dl = DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True, num_workers=workers)
    items, t0 = 0, None
    for e in range(epochs + 1):                      # epoch 0 warms up (page cache, worker start, first copies)
        if e == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for data in dl:
            b = D.as_batch_dict(D.extract_data_info(data, device=dev))
            items += b["pc1"].shape[0] if e else 0
    torch.cuda.synchronize()
    return items / (time.perf_counter() - t0)


def split_rate(sp, batch, epochs):
    items, t0 = 0, None
    for e in range(epochs + 1):
        if e == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for b in sp.epoch(batch, 256, seed=1, epoch=e):
            items += b["pc1"].shape[0] if e else 0
    torch.cuda.synchronize()
    return items / (time.perf_counter() - t0)


def draw_time_us(sp, batch, launches=2000):
    g = torch.Generator(device=sp.device)
    g.manual_seed(3)
    frames = torch.randint(len(sp), (batch,), generator=g, device=sp.device, dtype=torch.int32)
    for i in range(20):
        sp.draw(frames, 256, 1, i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(launches):
        sp.draw(frames, 256, 1, i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_split_probe: needs the GPU")
    dev = torch.device("cuda:0")
    per_clip = 32
    clips = tuple(("train", "delft_%d" % (c + 1), tuple(180 + (37 * c + 53 * f) % 221 for f in range(per_clip)))
                  for c in range(a.frames // per_clip))
    with tempfile.TemporaryDirectory(prefix="cmf_split_probe_") as root:
        D.write_synthetic_split(root, seed=11, clips=clips)
        t0 = time.perf_counter()
        sp = D.DeviceSplit.from_dataset(D.vodDataset(EvalArgs(), root, "train"), dev)
        torch.cuda.synchronize()
        pack_s = time.perf_counter() - t0
        mb = (sp.tab1.numel() + sp.tab2.numel()) * 4 / 2 ** 20
        print("split: %d frames, %d + %d points, %.1f MiB on the device, packed once in %.2f s (JSON decode included)"
              % (len(sp), sp.tab1.shape[0], sp.tab2.shape[0], mb, pack_s))
        print("device: %s, batch %d, 256 points, %d timed epochs after one warm-up epoch" % (torch.cuda.get_device_name(0), a.batch, a.epochs))
        for w in sorted({0, a.workers}):
            print("DataLoader(vodDataset), %d workers + extract_data_info: %10.0f items/s" % (w, loader_rate(root, a.batch, w, a.epochs, dev)))
        print("DeviceSplit.epoch (one cmf_draw_batch per batch):          %10.0f items/s" % split_rate(sp, a.batch, a.epochs))
        us = draw_time_us(sp, 64)
        print("cmf_draw_batch B = 64, N = 256: %.1f us per call back to back (device events over 2000 launches, host launch path "
              "included) = %.0f items/s" % (us, 64 / (us * 1e-6)))


if __name__ == "__main__":
    main()
