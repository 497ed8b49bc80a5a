"""CPU: the host side of data-parallel epochs from a DeviceSplit -- ``shard_batches`` (dataset.py) and the refusals that come
before any GPU work: unequal step counts at world > 1, an evaluation at world > 1 without a process group."""
import numpy as np
import pytest
import torch

from cmflow_amd import dataset as D
from cmflow_amd import evaluate as EV


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float32), 0.1, r(n1), r(n1),
            r(n1, 2))


@pytest.fixture(scope="module")
def cpu_split():
    rng = np.random.default_rng(1)
    return D.DeviceSplit.from_items([_item(a, b, rng) for a, b in zip((5, 1, 9, 300, 17), (8, 12, 1, 64, 65))], "cpu")


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_batches_partitions_every_list_in_order(world):
    lengths = [0, 1, world - 1, world, 2 * world + 1]
    rng = np.random.default_rng(world)
    batches = [[int(f) for f in rng.integers(0, 1000, n)] for n in lengths]
    before = [list(b) for b in batches]
    shares = [D.shard_batches(batches, r, world) for r in range(world)]
    assert batches == before                                                # the argument is left alone
    for i, b in enumerate(batches):
        parts = [shares[r][i] for r in range(world)]
        assert sum(parts, []) == b, (world, i)                              # a partition, in order
        sizes = [len(p) for p in parts]
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True), sizes      # as even as possible, larger first
        assert all(type(f) is int for p in parts for f in p)
    assert all(len(s) == len(batches) for s in shares)                      # one share per list, an empty one included
    if world > 1:
        assert shares[world - 1][1] == [] and shares[0][1] == batches[1]    # a list of one id: rank 0 has it
    assert D.shard_batches([], 0, world) == []
    assert D.shard_batches([np.arange(5)], 0, 1) == [[0, 1, 2, 3, 4]]       # any sequence of ids
    assert D.DeviceSplit.shard_batches(batches, 0, world) == shares[0]      # also reachable from the class


def test_shard_batches_is_shard_batchs_rule():
    """Where dp.shard_batch is defined (lengths that are multiples of world) the two agree."""
    from cmflow_amd.dp import shard_batch
    ids = torch.arange(24)
    for world in (1, 2, 3, 4, 8):
        for r in range(world):
            assert D.shard_batches([ids.tolist()], r, world) == [shard_batch({"f": ids}, r, world)["f"].tolist()]


@pytest.mark.parametrize("rank,world", [(0, 0), (0, -1), (-1, 2), (2, 2), (1, 1), (8, 8)])
def test_bad_rank_or_world(cpu_split, rank, world):
    with pytest.raises(ValueError):
        D.shard_batches([[1, 2, 3]], rank, world)
    with pytest.raises(ValueError):
        next(iter(cpu_split.epoch(2, 16, 0, 0, rank=rank, world=world)))
    with pytest.raises(ValueError):
        next(iter(cpu_split.epoch_ragged(2, 0, 0, rank=rank, world=world)))
    with pytest.raises(ValueError):
        next(iter(cpu_split.sweep(2, rank=rank, world=world)))
    clips = D.DeviceSplit(cpu_split.tab1, cpu_split.tab2, cpu_split.off1, cpu_split.off2, cpu_split.trans, cpu_split.interval,
                          cpu_split.max_points, clips=[(0, 5)])
    with pytest.raises(ValueError):
        next(iter(clips.epoch_clips(2, 2, 16, 0, 0, rank=rank, world=world)))


def test_unequal_steps_are_refused_before_the_gpu_is_asked_for(cpu_split):
    """world > 1 with drop_last=False: ValueError, although the split is on the CPU (where every draw is a RuntimeError)."""
    with pytest.raises(ValueError):
        next(iter(cpu_split.epoch(2, 16, 0, 0, drop_last=False, rank=0, world=2)))
    with pytest.raises(ValueError):
        next(iter(cpu_split.epoch_ragged(2, 0, 0, drop_last=False, rank=1, world=2)))
    # the controls: the same calls with equal steps, or in one process, get as far as the GPU check
    with pytest.raises(RuntimeError):
        next(iter(cpu_split.epoch(2, 16, 0, 0, drop_last=True, rank=0, world=2)))
    with pytest.raises(RuntimeError):
        next(iter(cpu_split.epoch_ragged(2, 0, 0, drop_last=True, rank=1, world=2)))
    with pytest.raises(RuntimeError):
        next(iter(cpu_split.epoch(2, 16, 0, 0, drop_last=False)))
    with pytest.raises(RuntimeError):
        next(iter(cpu_split.epoch_ragged(2, 0, 0, drop_last=False)))
    with pytest.raises(RuntimeError):
        next(iter(cpu_split.sweep(2, rank=1, world=2)))


def test_eval_at_world_2_needs_a_process_group(cpu_split, args):
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    assert not torch.distributed.is_initialized()
    net, net_t = CMFlow(args), CMFlow_T(args)
    rng = np.random.default_rng(2)
    clip_split = D.DeviceSplit.from_items([_item(9, 9, rng) for _ in range(3)], "cpu", clips=[(0, 3)])
    for training in (True, False):
        net.train(training), net_t.train(training)
        with pytest.raises(ValueError):
            EV.eval_split(net, cpu_split, 2, rank=0, world=2)
        with pytest.raises(ValueError):
            EV.eval_split_clips(net_t, clip_split, 2, 3, rank=1, world=2)
        with pytest.raises(ValueError):
            EV.eval_split(net, cpu_split, 2, rank=2, world=2)
        with pytest.raises(ValueError):
            EV.eval_split(net, cpu_split, 2, rank=0, world=0)
        assert net.training == training and net_t.training == training    # refused before net.eval()
    with pytest.raises(RuntimeError):
        EV.eval_split(net, cpu_split, 2, rank=0, world=1)                    # one process: as far as the GPU check, as before
