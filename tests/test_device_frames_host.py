"""CPU: the host side of whole-frame batches from a DeviceSplit -- ragged_batches / padding_share (dataset.py), the restated reset
rule of CMFlow-T's test loop and its segment-parallel schedule (evaluate.py), and the refusals of a split that is not on the GPU."""
import numpy as np
import pytest
import torch

from cmflow_amd import dataset as D
from cmflow_amd import evaluate as EV

F, BS, K = 48, 4, 3                                   # F is a multiple of K * BS
N1 = np.random.default_rng(3).integers(87, 462, F)    # the span of View-of-Delft frames


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float32), 0.1, r(n1), r(n1),
            r(n1, 2))


@pytest.fixture(scope="module")
def cpu_split():
    rng = np.random.default_rng(1)
    return D.DeviceSplit.from_items([_item(a, b, rng) for a, b in zip((5, 1, 9, 300, 17), (8, 12, 1, 64, 65))], "cpu")


def test_bucket_1_cuts_the_order_into_consecutive_batches():
    order = list(np.random.default_rng(0).permutation(F - 2))
    got = D.ragged_batches(N1, order, BS)
    assert got == [[int(f) for f in order[i:i + BS]] for i in range(0, F - 2, BS)]
    assert len(got[-1]) == (F - 2) % BS and sorted(sum(got, [])) == list(range(F - 2))          # every frame once, a short last batch
    dropped = D.ragged_batches(N1, order, BS, drop_last=True)
    assert dropped == got[:-1]
    assert D.ragged_batches(N1, order[:BS * 3], BS, drop_last=True) == got[:3]                  # nothing to drop
    assert D.ragged_batches(N1, [], BS) == []
    for bad in ((0, 1), (BS, 0)):
        with pytest.raises(ValueError):
            D.ragged_batches(N1, order, *bad)


@pytest.mark.parametrize("count", [F, F - 2, F - 5])
def test_bucket_k_sorts_by_size_and_id_inside_windows(count):
    order = [int(f) for f in np.random.default_rng(1).permutation(F)[:count]]
    n1 = N1.copy()
    n1[order[0]] = n1[order[1]]                       # a tie inside the first window: the frame id decides
    for drop_last in (False, True):
        got = D.ragged_batches(n1, order, BS, bucket=K, drop_last=drop_last)
        kept = order[:count // BS * BS] if drop_last else order
        assert sorted(sum(got, [])) == sorted(kept)
        assert all(len(b) == BS for b in got[:-1]) and (len(got[-1]) == BS or not drop_last)
        flat = sum(got, [])
        for w in range(0, len(kept), K * BS):
            assert flat[w:w + K * BS] == sorted(kept[w:w + K * BS], key=lambda f: (n1[f], f)), w


def test_bucketing_never_pads_more():
    """Among the splits of a window into groups of equal size, consecutive groups of the sorted window have the smallest sum of
    maxima, so with F a multiple of K * BS (every window full in both cuts) the padded share cannot grow."""
    for seed in range(5):
        order = list(np.random.default_rng(seed).permutation(F))
        plain, bucketed = D.ragged_batches(N1, order, BS), D.ragged_batches(N1, order, BS, bucket=K)
        a, b = D.padding_share(N1, plain), D.padding_share(N1, bucketed)
        assert 0.0 <= b <= a < 1.0, (seed, a, b)
    assert D.padding_share([5, 5, 7, 7], [[0, 1], [2, 3]]) == 0.0
    assert D.padding_share([1, 3], [[0, 1]]) == pytest.approx(1.0 - 4.0 / 6.0)


def test_the_epochs_order_is_a_function_of_seed_and_epoch(cpu_split):
    n1 = cpu_split.counts_host[0]
    batches = lambda seed, epoch: D.ragged_batches(n1, cpu_split._order(len(cpu_split), seed, epoch).tolist(), 2, bucket=2)
    assert batches(11, 3) == batches(11, 3)
    assert len({str(batches(11, e)) for e in range(8)}) > 1
    assert all(sorted(sum(batches(11, e), [])) == list(range(len(cpu_split))) for e in range(8))


def test_clip_test_resets_hand_worked():
    clips = [(0, 4), (4, 7), (7, 8)]
    # update_len 3: 0 (clip 0, now waiting for 4), 3 (multiple; now waiting for 7 -- the start at 4 is missed), 6 (multiple), 7 (clip 2)
    assert EV.clip_test_resets(clips, 8, 3) == [0, 3, 6, 7]
    # update_len 5: 0, 4 (clip 1), 5 (multiple), 7 (clip 2)
    assert EV.clip_test_resets(clips, 8, 5) == [0, 4, 5, 7]
    assert EV.clip_test_resets([(0, 7)], 7, 3) == [0, 3, 6]
    with pytest.raises(ValueError):
        EV.clip_test_resets([], 7, 3)
    with pytest.raises(ValueError):
        EV.clip_test_resets(clips, 8, 0)


@pytest.mark.parametrize("resets,n,bs", [([0, 3, 6, 7], 8, 3), ([0, 3, 6, 7], 8, 1), ([0, 4, 5, 7], 8, 2), ([0, 3, 6], 7, 8),
                                         ([0, 1, 2, 10, 11, 19, 20], 23, 4)])
def test_clip_test_schedule(resets, n, bs):
    groups = EV.clip_test_schedule(resets, n, bs)
    seen = [f for g in groups for step in g for f in step]
    assert sorted(seen) == list(range(n))                                                     # every frame exactly once
    segments = [list(range(a, b)) for a, b in zip(resets, resets[1:] + [n])]
    assert len(groups) == -(-len(segments) // bs)
    for gi, g in enumerate(groups):
        own = segments[gi * bs:(gi + 1) * bs]
        assert sorted(g[0]) == [s[0] for s in own] and len(g) == max(len(s) for s in own)     # bs segments, in segment order
        lengths = {s[0]: len(s) for s in own}
        assert g[0] == sorted(g[0], key=lambda f: (-lengths[f], f))                           # longest first, ties by first frame
        for t, step in enumerate(g):
            # slot s of every step is frame t of the segment that slot s of step 0 started: consecutive steps of one group, a prefix
            assert step == [first + t for first in g[0][:len(step)]]
            assert all(lengths[first] > t for first in g[0][:len(step)])
            assert all(lengths[first] <= t for first in g[0][len(step):])
    if (resets, n, bs) == ([0, 3, 6, 7], 8, 3):
        assert groups == [[[0, 3, 6], [1, 4], [2, 5]], [[7]]]
    with pytest.raises(ValueError):
        EV.clip_test_schedule(resets, n, 0)
    with pytest.raises(ValueError):
        EV.clip_test_schedule([1, 3], n, bs)


def test_counts_host_and_cpu_refusals(cpu_split):
    n1, n2 = cpu_split.counts_host
    assert n1.dtype == np.int32 and n2.dtype == np.int32
    assert np.array_equal(n1, np.diff(cpu_split.off1.numpy())) and np.array_equal(n2, np.diff(cpu_split.off2.numpy()))
    assert n1.tolist() == [5, 1, 9, 300, 17] and n2.tolist() == [8, 12, 1, 64, 65]
    assert cpu_split.counts_host[0] is n1                                                     # taken once
    with pytest.raises(RuntimeError):
        cpu_split.draw_frames([0, 1])
    with pytest.raises(RuntimeError):
        next(iter(cpu_split.epoch_ragged(2, seed=1, epoch=0)))
    with pytest.raises(RuntimeError):
        next(iter(cpu_split.sweep(2)))


def test_eval_split_refuses_before_any_launch(cpu_split, args):
    """The checks that need no GPU: a model without a ragged forward, the wrong driver for the model, a frame above the ragged cap,
    a split without clip ranges."""
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    from cmflow_amd.raflow import RaFlow

    class A:
        num_points, stat_thres, rigid_thres = 256, 0.5, 0.15
    with pytest.raises(NotImplementedError):
        EV.eval_split(RaFlow(A()), cpu_split, 2)
    net, net_t = CMFlow(args), CMFlow_T(args)
    with pytest.raises(ValueError):
        EV.eval_split(net_t, cpu_split, 2)
    with pytest.raises(ValueError):
        EV.eval_split_clips(net, cpu_split, 2, 3)
    with pytest.raises(ValueError):
        EV.eval_split_clips(net_t, cpu_split, 2, 3)                                           # no clip ranges
    rng = np.random.default_rng(2)
    big = D.DeviceSplit.from_items([_item(CMFlow.RAGGED_MAX_POINTS + 1, 9, rng)], "cpu")
    net.train()
    with pytest.raises(ValueError):
        EV.eval_split(net, big, 1)
    assert net.training                                                                       # refused before net.eval()
    with pytest.raises(RuntimeError):
        EV.eval_split(net, cpu_split, 2)                                                      # a split that is not on the GPU
    clip_split = D.DeviceSplit.from_items([_item(9, 9, rng) for _ in range(3)], "cpu", clips=[(0, 3)])
    net_t.train()
    with pytest.raises(RuntimeError):
        EV.eval_split_clips(net_t, clip_split, 2, 3)
    assert net.training and net_t.training
    with pytest.raises(RuntimeError):
        cpu_split.draw_frame_batches([[0], [1, 2]])
