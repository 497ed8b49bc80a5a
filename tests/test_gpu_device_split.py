"""GPU: cmf_draw_batch / DeviceSplit -- the drawn indices equal the host restatement of the sampling rule (tests/draw_ref.py)
exactly, every output is a bit-exact gather of the packed frames in extract_data_info's layout, a slot does not depend on the rest
of the batch, the epoch iterators visit what the existing loaders list, and a train step runs on the drawn batches."""
import numpy as np
import pytest
import torch
from torch.utils.data import default_collate

import draw_ref as R
from cmflow_amd import dataset as D
from cmflow_amd import synth

pytestmark = pytest.mark.gpu
SEED = 0x1234567887654321            # both words of the 64-bit seed are in use
N1 = [1, 7, 15, 16, 17, 48, 1000, 4096]
N2 = [300, 1, 16, 5, 256, 4096, 17, 33]
CAP = D.DRAW_MAX_POINTS
KEYS = D.DeviceSplit.KEYS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float32), 0.1 + 0.01 * n1,
            r(n1), r(n1), r(n1, 2))


@pytest.fixture(scope="module")
def small(dev):
    rng = np.random.default_rng(7)
    cpu = D.DeviceSplit.from_items([_item(a, b, rng) for a, b in zip(N1, N2)], "cpu")
    return cpu, cpu.to(dev)


@pytest.fixture(scope="module")
def at_cap(dev):
    rng = np.random.default_rng(8)
    cpu = D.DeviceSplit.from_items([_item(CAP, CAP - 1, rng), _item(CAP - 1, CAP, rng)], "cpu")
    return cpu, cpu.to(dev)


def host_batch(cpu, frames, idx1, idx2):
    """The batch gathered on the host from the packed frames through the given indices, in extract_data_info's layout."""
    rows1 = [cpu.tab1[cpu.off1[f]:cpu.off1[f + 1]][i.long()] for f, i in zip(frames, idx1)]
    rows2 = [cpu.tab2[cpu.off2[f]:cpu.off2[f + 1]][i.long()] for f, i in zip(frames, idx2)]
    a, b = torch.stack(rows1), torch.stack(rows2)                         # (B,N,14), (B,N,6)
    cm = lambda t: t.transpose(2, 1).contiguous()
    fr = torch.as_tensor(frames).long()
    return {"pc1": cm(a[:, :, 0:3]), "pc2": cm(b[:, :, 0:3]), "ft1": cm(a[:, :, 3:6]), "ft2": cm(b[:, :, 3:6]),
            "gt_trans": cpu.trans[fr].reshape(-1, 4, 4), "flow_label": a[:, :, 6:9].contiguous(), "fg_mask": a[:, :, 9].contiguous(),
            "interval": cpu.interval[fr], "radar_u": a[:, :, 10].contiguous(), "radar_v": a[:, :, 11].contiguous(),
            "opt_flow": a[:, :, 12:14].contiguous()}


def _check(cpu, gpu, frames, N, draw):
    out = gpu.draw(frames, N, SEED, draw)
    torch.cuda.synchronize()
    n1 = [int(cpu.off1[f + 1] - cpu.off1[f]) for f in frames]
    n2 = [int(cpu.off2[f + 1] - cpu.off2[f]) for f in frames]
    r1, r2 = R.draw_ref(n1, n2, N, SEED, draw)
    idx1, idx2 = out["idx1"].cpu(), out["idx2"].cpu()
    assert idx1.dtype == torch.int32 and idx1.shape == (len(frames), N)
    assert np.array_equal(idx1.numpy(), r1) and np.array_equal(idx2.numpy(), r2)
    want = host_batch(cpu, frames, idx1, idx2)
    for k in KEYS:
        got = out[k].cpu()
        assert got.shape == want[k].shape and got.dtype == torch.float32 and out[k].is_contiguous(), k
        assert torch.equal(got.view(torch.int32), want[k].view(torch.int32)), k           # bit for bit
    return out


@pytest.mark.parametrize("N", [16, 256])
def test_indices_equal_the_host_restatement_and_gather_is_exact(small, N):
    cpu, gpu = small
    frames = list(range(8)) + [3, 3, 0, 7, 6, 5, 1, 2]                     # B = 16: every frame, some twice, one three times
    _check(cpu, gpu, frames, N, draw=5)
    _check(cpu, gpu, frames, N, draw=(1 << 40) + 9)                        # the high word of the draw counter


def test_frames_at_the_cap(at_cap):
    cpu, gpu = at_cap
    _check(cpu, gpu, [0, 1, 1], 256, draw=2)


def test_a_slot_does_not_depend_on_the_batch(small):
    cpu, gpu = small
    mixed = [6, 7, 0, 4, 5, 1, 2, 3]
    a = gpu.draw(mixed, 16, SEED, 11)
    for s, f in enumerate(mixed):
        b = gpu.draw([f] * len(mixed), 16, SEED, 11)
        for k in (*KEYS, "idx1", "idx2"):
            assert torch.equal(a[k][s], b[k][s]), (k, s)
    other = gpu.draw(mixed, 16, SEED, 12)
    assert not torch.equal(other["idx1"], a["idx1"])
    lone = gpu.draw([mixed[0]], 16, SEED, 11)                              # B = 1: slot 0 alone
    assert all(torch.equal(lone[k][0], a[k][0]) for k in (*KEYS, "idx1", "idx2"))


def test_bad_arguments_and_bad_frame_ids(small):
    cpu, gpu = small
    with pytest.raises(RuntimeError):
        gpu.draw([0], 0, SEED, 0)                                          # N >= 1
    with pytest.raises(RuntimeError):
        gpu.draw([], 16, SEED, 0)                                          # B >= 1
    a = gpu.draw([-5, 10 ** 6], 16, SEED, 0)                               # clamped to the first / last frame
    b = gpu.draw([0, len(gpu) - 1], 16, SEED, 0)
    assert all(torch.equal(a[k], b[k]) for k in a)


class TrainArgs:
    num_points, eval, mini_clip_len, update_len = 256, False, 2, 1


class EvalArgs(TrainArgs):
    eval = True


def _frame_of(gpu, batch):
    """The frame behind every slot: the one frame whose point idx1[s, 0] has the coordinates of output position 0 (the synthetic
    frames share their transform, their random coordinates are distinct)."""
    tab, off = gpu.tab1.cpu(), gpu.off1.cpu().tolist()
    first, pos0 = batch["idx1"][:, 0].cpu().tolist(), batch["pc1"][:, :, 0].cpu()
    frames = []
    for s, i in enumerate(first):
        hit = [f for f in range(len(off) - 1) if i < off[f + 1] - off[f] and torch.equal(tab[off[f] + i, 0:3], pos0[s])]
        assert len(hit) == 1, (s, hit)
        frames.append(hit[0])
    return frames


def test_epoch_visits_every_frame_once_in_the_loaders_layout(dev, tmp_path):
    D.write_synthetic_split(str(tmp_path))
    gpu = D.DeviceSplit.from_dataset(D.vodDataset(EvalArgs(), str(tmp_path), "train"), dev)
    loader_ds = D.vodDataset(TrainArgs(), str(tmp_path), "train")
    want = D.as_batch_dict(D.extract_data_info(default_collate([loader_ds[0], loader_ds[1]]), device=dev))
    for bs, sizes in ((2, [2, 2]), (3, [3, 1])):
        batches = list(gpu.epoch(batch_size=bs, npoints=256, seed=SEED, epoch=1, drop_last=False))
        assert [b["pc1"].shape[0] for b in batches] == sizes
        assert sorted(sum((_frame_of(gpu, b) for b in batches), [])) == [0, 1, 2, 3]
    assert len(list(gpu.epoch(3, 256, SEED, 1))) == 1                      # drop_last
    b = batches[0]
    assert [k for k in b if k not in ("idx1", "idx2")] == list(want) and list(b)[-2:] == ["idx1", "idx2"]
    for k, w in want.items():
        assert b[k].shape[1:] == w.shape[1:] and b[k].dtype == w.dtype and b[k].device == w.device and b[k].is_contiguous(), k
    orders = [sum((_frame_of(gpu, x) for x in gpu.epoch(1, 256, SEED, e)), []) for e in range(6)]
    assert orders[0] == sum((_frame_of(gpu, x) for x in gpu.epoch(1, 256, SEED, 0)), [])      # same (seed, epoch), same order
    assert len({tuple(o) for o in orders}) > 1                                                # the epoch reshuffles


def test_epoch_clips_yields_the_clip_loaders_mini_clips(dev, tmp_path):
    clips = (("train", "delft_1", (60, 70, 80, 90, 100)), ("train", "delft_3", (50,)), ("train", "delft_7", (65, 75, 85, 95)))
    D.write_synthetic_split(str(tmp_path), seed=5, clips=clips)
    whole = D.vodClipDataset(EvalArgs(), str(tmp_path), "train")
    gpu = D.DeviceSplit.from_dataset(whole, dev)
    frame = {p: i for i, p in enumerate(whole.samples)}
    want = sorted(tuple(frame[p] for p in mini) for mini in D.vodClipDataset(TrainArgs(), str(tmp_path), "train").mini_samples)
    assert want == [(0, 1), (2, 3), (6, 7), (8, 9)]
    steps = list(gpu.epoch_clips(batch_size=3, mini_clip_len=2, npoints=256, seed=SEED, epoch=0))
    assert [len(s) for s in steps] == [2, 2] and [s[0]["pc1"].shape[0] for s in steps] == [3, 1]
    got = []
    for s in steps:
        got += list(zip(*(_frame_of(gpu, d) for d in s)))
        assert all(d["pc1"].shape == (s[0]["pc1"].shape[0], 3, 256) for d in s)
    assert sorted(got) == want
    # a split without clip ranges serves no mini-clips
    plain = D.DeviceSplit.from_dataset(D.vodDataset(EvalArgs(), str(tmp_path), "train"), dev)
    with pytest.raises(ValueError):
        next(plain.epoch_clips(2, 2, 256, SEED, 0))


def test_train_steps_on_drawn_batches(dev, manifest, golden_dir, args, tmp_path):
    """Two TrainStep steps on the batches of one epoch over the synthetic split: finite loss, every gradient of the bucket written;
    then the loss of a drawn batch equals, bit for bit, the loss of the same batch assembled on the host through idx1 / idx2."""
    import os
    from cmflow_amd.cmflow import CMFlow
    from cmflow_amd.train import TrainStep
    D.write_synthetic_split(str(tmp_path))
    cpu = D.DeviceSplit.from_dataset(D.vodDataset(EvalArgs(), str(tmp_path), "train"), "cpu")
    gpu = cpu.to(dev)
    net = CMFlow(args)
    net.load_state_dict(synth.synth_state_dict(manifest, seed=1234, calib=os.path.join(golden_dir, "bn_calib_cmflow.npz")))
    net = net.to(dev).train()
    step = TrainStep(net, vr_thres=args.vr_thres)
    batches = list(gpu.epoch(batch_size=2, npoints=args.num_points, seed=SEED, epoch=0))
    assert len(batches) == 2
    for b in batches:
        loss, _, _, _ = step(b)
        assert torch.isfinite(loss).item()
        assert torch.isfinite(step.bucket.flat).all()
        names = {id(p): k for k, p in net.named_parameters()}
        unwritten = [names[id(p)] for p in step.bucket.params if p.dim() >= 2 and not p.grad.any()]
        assert not unwritten, unwritten
    b = batches[0]
    frames = _frame_of(gpu, b)
    host = {k: v.to(dev) for k, v in host_batch(cpu, frames, b["idx1"].cpu(), b["idx2"].cpu()).items()}
    for k in KEYS:
        assert torch.equal(host[k], b[k]), k
    drawn = step.forward_loss(b)[0].detach()
    again = step.forward_loss(host)[0].detach()
    assert torch.equal(drawn, again) and torch.isfinite(drawn).item()
