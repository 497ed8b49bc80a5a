"""GPU: data-parallel epochs and evaluation from a DeviceSplit.  One process: a draw at ``slot0`` is the rows of the whole draw; the
ranks' batches of ``epoch`` / ``epoch_clips`` concatenate, bit for bit, to the batches one process draws at the global batch size;
``epoch_ragged`` / ``sweep`` hand every rank its slice of the global id lists.  Two ranks on cuda:0 over gloo
(tests/dp_split_worker.py): ``eval_split`` / ``eval_split_clips`` return the single-process result on both ranks, and two TrainStep
steps fed by ``epoch(..., rank, world)`` obey the project's parity rule (rank r = a single-process run on shard r)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dp_split_worker as W
import draw_ref as R
from cmflow_amd import dataset as D

pytestmark = pytest.mark.gpu
SEED = W.SEED
NPOINTS = 128
# npoints = 128 takes both branches of the draw on either cloud: below (top-up) 3, 64, 127; from 128 on (sort) 128, 129, 300
N1 = [3, 64, 127, 128, 129, 300, 300, 129, 128, 127, 64, 3]
N2 = [128, 129, 300, 3, 64, 127, 64, 3, 300, 129, 127, 128]
CLIPS = [(0, 5), (5, 9), (9, 12)]                      # L = 2: mini-clips at 0, 2 | 5, 7 | 9 -- five of them
KEYS = D.DeviceSplit.KEYS
DRAWN = (*KEYS, "idx1", "idx2")
RAGGED = (*KEYS, "n1", "n2", "frames")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float32), 0.1 + 0.01 * n1,
            r(n1), r(n1), r(n1, 2))


@pytest.fixture(scope="module")
def gpu(dev):
    rng = np.random.default_rng(17)
    return D.DeviceSplit.from_items([_item(a, b, rng) for a, b in zip(N1, N2)], dev, clips=CLIPS)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _cat(dicts, keys):
    return {k: torch.cat([d[k] for d in dicts], dim=0) for k in keys}


def _rows(d, keys, lo, hi):
    return {k: d[k][lo:hi] for k in keys}


def test_draw_at_slot0_is_the_rows_of_the_whole_draw(gpu, dev):
    """Fails on the parent commit: draw has no slot0 there."""
    frames = [0, 5, 2, 3, 11, 1, 6, 4]                                      # 8 slots; slots 5..7: n1 = 64, 300, 129; n2 = 129, 64, 64
    draw = (1 << 40) + 9
    whole = gpu.draw(frames, NPOINTS, SEED, draw)
    tail = gpu.draw(frames[5:8], NPOINTS, SEED, draw, slot0=5)
    head = gpu.draw(frames[0:3], NPOINTS, SEED, draw, slot0=0)
    assert list(tail) == list(whole) and tail["pc1"].shape == (3, 3, NPOINTS)
    _same(tail, _rows(whole, DRAWN, 5, 8), DRAWN, "slots 5..7")
    _same(head, _rows(whole, DRAWN, 0, 3), DRAWN, "slots 0..2")
    r1, r2 = R.draw_ref([N1[f] for f in frames[5:8]], [N2[f] for f in frames[5:8]], NPOINTS, SEED, draw, slots=range(5, 8))
    assert np.array_equal(tail["idx1"].cpu().numpy(), r1) and np.array_equal(tail["idx2"].cpu().numpy(), r2)
    unshifted = gpu.draw(frames[5:8], NPOINTS, SEED, draw)
    assert not torch.equal(unshifted["idx1"], tail["idx1"])                 # the slot number is part of the draw
    assert torch.equal(unshifted["gt_trans"], tail["gt_trans"])             # ... and of nothing else
    # the limits of slot0: 0 <= slot0, slot0 + B <= INT_MAX
    top = 2 ** 31 - 1
    last = gpu.draw([5, 2], NPOINTS, SEED, 3, slot0=top - 2)
    r1, r2 = R.draw_ref([N1[5], N1[2]], [N2[5], N2[2]], NPOINTS, SEED, 3, slots=[top - 2, top - 1])
    assert np.array_equal(last["idx1"].cpu().numpy(), r1) and np.array_equal(last["idx2"].cpu().numpy(), r2)
    for bad in (-1, top - 1, top):
        with pytest.raises(RuntimeError):
            gpu.draw([5, 2], NPOINTS, SEED, 3, slot0=bad)


def test_cmf_draw_batch_is_slot0_zero(gpu, dev):
    """The entry point that stays in the ABI, called as it always was, against draw (which goes through cmf_draw_batch_at)."""
    from cmflow_amd import _lib
    frames = torch.tensor([7, 0, 5, 9, 2], dtype=torch.int32, device=dev)
    want = gpu.draw(frames, NPOINTS, SEED, 21)
    out = {k: torch.empty_like(v) for k, v in want.items()}
    fp, ip = (lambda t: _lib.dev_ptr(t, torch.float32)), (lambda t: _lib.dev_ptr(t, torch.int32))
    _lib.check(_lib.lib().cmf_draw_batch(
        5, NPOINTS, len(gpu), gpu.max_points, fp(gpu.tab1), fp(gpu.tab2), ip(gpu.off1), ip(gpu.off2), fp(gpu.trans), fp(gpu.interval),
        ip(frames), SEED, 21, *(fp(out[k]) for k in KEYS), ip(out["idx1"]), ip(out["idx2"]), _lib.stream_ptr()), "cmf_draw_batch")
    _same(out, want, DRAWN, "cmf_draw_batch")
    r1, r2 = R.draw_ref([N1[f] for f in frames.tolist()], [N2[f] for f in frames.tolist()], NPOINTS, SEED, 21)
    assert np.array_equal(out["idx1"].cpu().numpy(), r1) and np.array_equal(out["idx2"].cpu().numpy(), r2)


@pytest.mark.parametrize("world", [2, 4])
def test_epoch_of_all_ranks_is_the_single_process_epoch(gpu, world):
    B = 2
    single = list(gpu.epoch(world * B, NPOINTS, SEED, 1))
    ranks = [list(gpu.epoch(B, NPOINTS, SEED, 1, rank=r, world=world)) for r in range(world)]
    assert len(single) == 12 // (world * B) and all(len(steps) == len(single) for steps in ranks)
    for t, want in enumerate(single):
        assert all(steps[t]["pc1"].shape == (B, 3, NPOINTS) for steps in ranks)
        _same(_cat([steps[t] for steps in ranks], DRAWN), want, DRAWN, (world, t))
    assert not torch.equal(ranks[0][0]["idx1"], ranks[1][0]["idx1"])


def test_epoch_clips_of_all_ranks_is_the_single_process_epoch(gpu):
    """Five mini-clips, global batch 4.  One process keeps the short last step; two ranks drop it (equal step counts).  The draw
    number counts the steps of an epoch, so with a leftover the two agree in epoch 0 only -- from epoch 1 on a run at world > 1
    is compared with runs at other world sizes of the same global batch, which all drop the same mini-clips."""
    B, L = 2, 2
    single = list(gpu.epoch_clips(2 * B, L, NPOINTS, SEED, 0))
    ranks = [list(gpu.epoch_clips(B, L, NPOINTS, SEED, 0, rank=r, world=2)) for r in range(2)]
    assert [len(s) for s in single] == [L, L] and [s[0]["pc1"].shape[0] for s in single] == [4, 1]      # the leftover step
    assert all(len(steps) == 1 and len(steps[0]) == L for steps in ranks)                               # ... and none here
    for j in range(L):
        _same(_cat([steps[0][j] for steps in ranks], DRAWN), single[0][j], DRAWN, j)
    starts = sorted(int(f) for f in _first_frames(gpu, single))
    assert starts == [0, 2, 5, 7, 9]
    two = [list(gpu.epoch_clips(B, L, NPOINTS, SEED, 3, rank=r, world=2)) for r in range(2)]
    four = [list(gpu.epoch_clips(1, L, NPOINTS, SEED, 3, rank=r, world=4)) for r in range(4)]
    assert all(len(steps) == 1 for steps in two + four)
    for j in range(L):
        _same(_cat([steps[0][j] for steps in two], DRAWN), _cat([steps[0][j] for steps in four], DRAWN), DRAWN, j)


def _first_frames(gpu, steps):
    """The frame behind every slot of frame 0 of every step: the frame whose interval (0.1 + 0.01 * n1) and transform match."""
    trans = gpu.trans.reshape(-1, 4, 4)
    out = []
    for s in steps:
        for row in s[0]["gt_trans"]:
            hit = [f for f in range(len(gpu)) if torch.equal(trans[f], row)]
            assert len(hit) == 1
            out.append(hit[0])
    return out


@pytest.mark.parametrize("bucket", [1, 2])
@pytest.mark.parametrize("world", [2, 3])
def test_epoch_ragged_hands_every_rank_its_slice(gpu, world, bucket):
    B = 2
    n1 = gpu.counts_host[0]
    want = D.ragged_batches(n1, gpu._order(12, 5, 2).tolist(), world * B, bucket, True)
    assert len(want) == 12 // (world * B) and all(len(b) == world * B for b in want)
    ranks = [list(gpu.epoch_ragged(B, 5, 2, bucket=bucket, rank=r, world=world)) for r in range(world)]
    assert all(len(steps) == len(want) for steps in ranks)
    for t, ids in enumerate(want):
        assert sum((steps[t]["frames"].tolist() for steps in ranks), []) == ids
        for steps in ranks:
            _same(steps[t], gpu.draw_frames(steps[t]["frames"].tolist()), RAGGED, (world, bucket, t))
    assert sorted(sum(want, [])) == list(range(12))


@pytest.mark.parametrize("sort_by_size", [False, True])
@pytest.mark.parametrize("world,B", [(2, 2), (3, 3), (5, 1)])
def test_sweep_of_all_ranks_visits_every_frame_once(gpu, world, B, sort_by_size):
    """(5, 1): global batches of 5 over 12 frames -- the last one holds 2 frames, fewer than ranks: ranks 2..4 skip it."""
    n1 = gpu.counts_host[0]
    order = sorted(range(12), key=lambda f: (int(n1[f]), f)) if sort_by_size else list(range(12))
    G = world * B
    want = [order[i:i + G] for i in range(0, 12, G)]
    ranks = [list(gpu.sweep(B, sort_by_size, rank=r, world=world)) for r in range(world)]
    shares = [[s for s in D.shard_batches(want, r, world) if s] for r in range(world)]
    assert [[b["frames"].tolist() for b in steps] for steps in ranks] == shares
    for t, ids in enumerate(want):
        assert sum((shares[r][t] for r in range(world) if t < len(shares[r])), []) == ids
    for steps in ranks:
        for b in steps:
            _same(b, gpu.draw_frames(b["frames"].tolist()), RAGGED, (world, B))
    assert sorted(f for steps in ranks for b in steps for f in b["frames"].tolist()) == list(range(12))
    if (world, B) == (5, 1):
        assert [len(steps) for steps in ranks] == [3, 3, 2, 2, 2]


# ---- two ranks on cuda:0 over gloo ------------------------------------------------------------------------------------------------
def _two_ranks(tmp_path, mode):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "dp_split_worker.py"), str(tmp_path), mode]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=dict(os.environ))
    assert out.returncode == 0, out.stderr[-3000:]
    return [torch.load(os.path.join(tmp_path, "rank%d.pt" % r)) for r in range(2)]


def test_two_rank_evaluation_is_the_single_process_result(dev, tmp_path):
    """eval_split (CMFlow, 10 whole frames of 40 .. 120 points, batch_size 2) and eval_split_clips (CMFlow-T, three clips, update_len 3)
    at world = 2: both ranks return the same; the two transform arrays equal the single-process ones bit for bit (every frame is
    written by one rank, zero elsewhere, and summed); every metric agrees within relative 1e-12 -- the ranks' float64 sums of <= 10
    terms are added in another order, bounded by 10 * 2^-53 relative, three orders below -- and is NaN where the single-process one is."""
    from cmflow_amd import evaluate as EV
    from cmflow_amd import eval_util as E
    ranks = _two_ranks(tmp_path, "eval")
    split = W.eval_split_of(dev)
    single = {"eval_split": W.cpu_result(EV.eval_split(W.model("cmflow", dev), split, W.EVAL_BATCH)),
              "eval_split_clips": W.cpu_result(EV.eval_split_clips(W.model("cmflow_t", dev), split, W.EVAL_BATCH, W.UPDATE_LEN))}
    # who ran what: slices of the global batches of 4; schedule groups 0, 2 | 1
    assert ranks[0]["batches"] == [[0, 1], [4, 5], [8]] and ranks[1]["batches"] == [[2, 3], [6, 7], [9]]
    schedule = EV.clip_test_schedule(EV.clip_test_resets(split.clips, 10, W.UPDATE_LEN), 10, W.EVAL_BATCH)
    assert len(schedule) == 3
    for r in range(2):
        assert ranks[r]["clip_batches"] == [step for group in schedule[r::2] for step in group]
    for what, want in single.items():
        a, b = ranks[0][what], ranks[1][what]
        assert list(a["metrics"]) == list(E.SF_KEYS + E.SEG_KEYS + E.POSE_KEYS)
        for k in ("gt_trans_all", "pre_trans_all"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)
            assert a[k].shape == (10, 4, 4) and torch.equal(_bits(a[k]), _bits(want[k])), (what, k)
        assert float(want["pre_trans_all"].abs().sum(dim=(1, 2)).min()) > 0                # every frame was written
        for k, w in want["metrics"].items():
            va, vb, w = float(a["metrics"][k]), float(b["metrics"][k]), float(w)
            print("%s %s: 2 ranks %.17g, single %.17g" % (what, k, va, w))
            assert a["metrics"][k].dtype == torch.float64
            assert va == vb or (np.isnan(va) and np.isnan(vb)), (what, k)
            if np.isnan(w):
                assert np.isnan(va), (what, k)
            else:
                assert abs(va - w) <= 1e-12 * abs(w), (what, k, va, w)
        assert sum(np.isfinite(float(v)) for v in want["metrics"].values()) >= 7, what


def test_two_rank_training_on_epoch_batches(dev, tmp_path):
    """Two TrainStep steps on split.epoch(2, 256, seed, 0, rank, world = 2).  The ranks' batches are the slices of the single-process
    epoch(4, ...) batches bit for bit; the all-reduced buckets and the final parameters are identical on both ranks; for the first
    step rank r's local bucket equals a single-process run on that shard and the averaged bucket the mean of the two, within the
    bounds of test_two_rank_cmflow_step_matches_single_rank_shards (1e-6 of the largest magnitude)."""
    import bench
    from cmflow_amd.fused_blocks import join_side_streams
    from cmflow_amd.train import TrainStep
    ranks = _two_ranks(tmp_path, "train")
    split = W.train_split_of(dev)
    B = W.TRAIN_BATCH
    single = list(split.epoch(2 * B, W.TRAIN_POINTS, SEED, 0))
    assert len(single) == W.TRAIN_STEPS and all(len(r["steps"]) == W.TRAIN_STEPS for r in ranks)
    for t, want in enumerate(single):
        for r in range(2):
            got = {k: v.to(dev) for k, v in ranks[r]["steps"][t]["batch"].items()}
            assert list(got) == list(want)
            _same(got, _rows(want, DRAWN, r * B, (r + 1) * B), DRAWN, (t, r))
        assert torch.equal(ranks[0]["steps"][t]["averaged"], ranks[1]["steps"][t]["averaged"]), t
    for k, v in ranks[0]["params"].items():
        assert torch.equal(v, ranks[1]["params"][k]), k

    def close(a, b, what):
        a, b = a.double(), b.double()
        assert float((a - b).abs().max()) <= 1e-6 * max(1e-30, float(b.abs().max())), what

    singles = []
    for r in range(2):
        net = W.model("cmflow", dev).train()
        step = TrainStep(net, vr_thres=bench.Args.vr_thres)
        loss = step.forward_loss(_rows(single[0], DRAWN, r * B, (r + 1) * B))[0]
        step.bucket.zero()
        loss.backward()
        join_side_streams()
        torch.cuda.synchronize()
        close(ranks[r]["steps"][0]["loss"], loss.detach().cpu(), "loss of rank %d" % r)
        close(ranks[r]["steps"][0]["local"], step.bucket.flat.cpu(), "local gradient bucket of rank %d" % r)
        singles.append(step.bucket.flat.cpu().double())
    mean = (singles[0] + singles[1]) / 2
    assert float((ranks[0]["steps"][0]["averaged"].double() - mean).abs().max()) <= 1e-6 * float(mean.abs().max())
    local = [ranks[r]["steps"][0]["local"].double() for r in range(2)]
    assert float((ranks[0]["steps"][0]["averaged"].double() - (local[0] + local[1]) / 2).abs().max()) <= 1e-6 * float(mean.abs().max())
    assert float(local[0].abs().sum()) > 0 and not torch.equal(local[0], local[1])
