"""CPU: the device-resident split's host side -- packing (DeviceSplit.from_dataset / from_items) and the host restatement of
cmf_draw_batch's sampling rule (tests/draw_ref.py): its generator against the published known answers, its structure, and its
distribution.  The distribution bounds are conditions on a uniform sampler under a fixed seed (deterministic), not measurements."""
import os
import re

import numpy as np
import pytest
import torch

import draw_ref as R
from cmflow_amd import dataset as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240607                         # chosen once; every statistic below is a deterministic function of it


class EvalArgs:
    num_points, eval, mini_clip_len, update_len = 256, True, 2, 1


@pytest.fixture(scope="module")
def split_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("split"))
    D.write_synthetic_split(root)
    return root


def test_packing_equals_the_items(split_root):
    ds = D.vodDataset(EvalArgs(), split_root, "train")
    sp = D.DeviceSplit.from_dataset(ds, "cpu")
    assert len(sp) == 4 and sp.clips is None
    n1 = [180, 256, 400, 300]
    assert sp.off1.dtype == torch.int32 and sp.off2.dtype == torch.int32
    assert sp.off1.tolist() == [0] + list(np.cumsum(n1))
    items = [ds[i] for i in range(len(ds))]
    assert sp.off2.tolist() == [0] + list(np.cumsum([it[1].shape[0] for it in items]))
    assert sp.max_points == max(max(it[0].shape[0], it[1].shape[0]) for it in items)
    assert sp.tab1.shape == (sum(n1), 14) and sp.tab2.shape == (sp.off2[-1].item(), 6)
    assert all(t.dtype == torch.float32 for t in (sp.tab1, sp.tab2, sp.trans, sp.interval))
    for f, it in enumerate(items):
        pos1, pos2, ft1, ft2, trans, labels, mask, interval, ru, rv, opt = it
        a = sp.tab1[sp.off1[f]:sp.off1[f + 1]].numpy()
        b = sp.tab2[sp.off2[f]:sp.off2[f + 1]].numpy()
        assert a.shape[0] == pos1.shape[0] and b.shape[0] == pos2.shape[0]
        for got, want in ((a[:, 0:3], pos1), (a[:, 3:6], ft1), (a[:, 6:9], labels), (a[:, 9], mask), (a[:, 10], ru), (a[:, 11], rv),
                          (a[:, 12:14], opt), (b[:, 0:3], pos2), (b[:, 3:6], ft2)):
            assert np.array_equal(got, want)
        assert np.array_equal(sp.trans[f].numpy().reshape(4, 4), trans)
        assert sp.interval[f].item() == np.float32(interval)


def test_clip_dataset_records_the_clip_ranges(split_root):
    ds = D.vodClipDataset(EvalArgs(), split_root, "train")
    sp = D.DeviceSplit.from_dataset(ds, "cpu")
    assert sp.clips == [(0, 3), (3, 4)] and len(sp) == 4

    class TrainArgs(EvalArgs):
        eval = False
    with pytest.raises(ValueError):
        D.DeviceSplit.from_dataset(D.vodClipDataset(TrainArgs(), split_root, "train"), "cpu")


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float64), 0.1, r(n1), r(n1), r(n1, 2))


def test_refusals():
    rng = np.random.default_rng(0)
    ok = _item(5, 7, rng)
    for bad in (_item(0, 7, rng), _item(5, 0, rng)):
        with pytest.raises(ValueError):
            D.DeviceSplit.from_items([ok, bad], "cpu")
    with pytest.raises(ValueError):
        D.DeviceSplit.from_items([], "cpu")
    with pytest.raises(ValueError):
        D.DeviceSplit.from_items([ok, _item(D.DRAW_MAX_POINTS + 1, 3, rng)], "cpu")
    D.DeviceSplit.from_items([_item(D.DRAW_MAX_POINTS, 3, rng)], "cpu")                # the cap itself is served
    sp = D.DeviceSplit.from_items([ok], "cpu")
    with pytest.raises(RuntimeError):
        sp.draw([0], 16, 1, 0)
    with pytest.raises(RuntimeError):
        next(sp.epoch(1, 16, 1, 0))


def test_cap_agrees_with_the_header():
    text = open(os.path.join(REPO, "include", "cmflow_hip.h")).read()
    cap = int(re.search(r"#define\s+CMF_DRAW_MAX_POINTS\s+(\d+)", text).group(1))
    assert cap == D.DRAW_MAX_POINTS and cap >= 8192
    assert cap * 8 <= 160 * 1024 < 2 * cap * 8                # the sort keys of one cloud fill what one workgroup's LDS can hold


def test_philox_known_answers():
    """Random123's published known-answer vectors for philox4x32-10 (kat_vectors: counter, key -> output)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == want
    got = R.philox4x32_10((np.array([0, 0xffffffff]),) * 4, (0, 0))                     # vectorised over the counter
    assert int(got[0][0]) == 0x6627e8d5


@pytest.mark.parametrize("n", [1, 7, 15, 16, 17, 48, 1000])
def test_draw_ref_structure(n):
    """Eight slots per call: at n = 15 one slot holds a single draw from 15 values, so "a change of seed, draw or slot changes the
    result" is asked of the eight slots together (a coincidence has probability 15^-8), for every n alike."""
    N, B = 16, 8
    i1, i2 = R.draw_ref([n] * B, [n] * B, N, SEED, 3)
    assert i1.shape == (B, N) and i1.dtype == np.int32
    for row in (*i1, *i2):
        assert row.min() >= 0 and row.max() < n
        if n < N:
            assert np.array_equal(row[:n], np.arange(n))
        else:
            assert len(set(row.tolist())) == N
    again = R.draw_ref([n] * B, [n] * B, N, SEED, 3)
    assert np.array_equal(again[0], i1) and np.array_equal(again[1], i2)
    assert np.array_equal(R.draw_ref([n], [n], N, SEED, 3, slots=[5])[0][0], i1[5])      # a slot does not depend on the batch
    if n > 1:                                                                            # n = 1 has one possible result
        assert not np.array_equal(R.draw_ref([n] * B, [n] * B, N, SEED + 1, 3)[0], i1)
        assert not np.array_equal(R.draw_ref([n] * B, [n] * B, N, SEED, 4)[0], i1)
        assert not np.array_equal(R.draw_ref([n] * B, [n] * B, N, SEED, 3, slots=range(B, 2 * B))[0], i1)
        assert not np.array_equal(i2, i1)                                                # cloud


def _five_sigma(counts, trials, p):
    sigma = np.sqrt(trials * p * (1 - p))
    return np.abs(np.asarray(counts) - trials * p).max() <= 5 * sigma


def test_draw_ref_distribution_subset():
    n, N, slots, draws = 12, 4, 64, 200
    idx = np.concatenate([R.draw_ref([n] * slots, [n] * slots, N, SEED, d)[0] for d in range(draws)])
    trials = slots * draws
    assert idx.shape == (trials, N) and trials == 12800
    assert _five_sigma(np.bincount(idx.reshape(-1), minlength=n), trials, N / n)         # inclusion: binomial(12800, 1/3)
    assert _five_sigma(np.bincount(idx[:, 0], minlength=n), trials, 1 / n)               # position 0: binomial(12800, 1/12)


def test_draw_ref_distribution_top_up():
    n, N, slots, draws = 5, 16, 64, 200
    idx = np.concatenate([R.draw_ref([n] * slots, [n] * slots, N, SEED, d)[0] for d in range(draws)])
    trials = slots * draws
    assert np.array_equal(idx[:, :n], np.tile(np.arange(n), (trials, 1)))
    for pos in range(n, N):                                                              # the eleven top-up positions
        assert _five_sigma(np.bincount(idx[:, pos], minlength=n), trials, 1 / n), pos
