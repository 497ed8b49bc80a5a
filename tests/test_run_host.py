"""Host: the bookkeeping behind whole training runs from device-resident splits -- DeviceSplit.save / load, the frame arithmetic of
the in-order iterators (``dataset.sweep_shares``, ``mini_clip_starts``), ``train.make_schedule`` against StepLR on a plain Adam, the
best-checkpoint rule, and every refusal of ``train.fit`` / ``evaluate.eval_epoch`` / ``eval_epoch_clips`` (raised before the network's
mode changes).  Every test fails on the parent commit: none of the names exists there."""
import math

import numpy as np
import pytest
import torch

import bench
from cmflow_amd import dataset as D
from cmflow_amd import evaluate as EV
from cmflow_amd import train as T
from cmflow_amd.cmflow import CMFlow, CMFlow_T
from cmflow_amd.raflow import RaFlow


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float32), 0.1 + 0.01 * n1,
            r(n1), r(n1), r(n1, 2))


def _split(clips=None, sizes=((20, 31), (400, 64), (256, 255), (77, 300), (33, 21), (128, 129), (90, 45))):
    rng = np.random.default_rng(3)
    return D.DeviceSplit.from_items([_item(a, b, rng) for a, b in sizes], "cpu", clips=clips)


# ---- DeviceSplit.save / load --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clips", [None, [(0, 3), (3, 7)]])
def test_split_file_round_trip(tmp_path, clips):
    split = _split(clips)
    path = str(tmp_path / "val.split")
    split.save(path)
    assert [p.name for p in tmp_path.iterdir()] == ["val.split"]                       # the temporary name is gone
    back = D.DeviceSplit.load(path, "cpu")
    for k in ("tab1", "tab2", "off1", "off2", "trans", "interval"):
        a, b = getattr(split, k), getattr(back, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert back.clips == clips and back.max_points == split.max_points == 400 and len(back) == 7
    assert all(np.array_equal(a, b) for a, b in zip(back.counts_host, split.counts_host))


def test_split_file_of_another_version_is_refused(tmp_path):
    path = str(tmp_path / "s.split")
    _split().save(path)
    rec = torch.load(path)
    assert rec["version"] == D.SPLIT_FORMAT_VERSION
    torch.save(dict(rec, version=D.SPLIT_FORMAT_VERSION + 1), path)
    with pytest.raises(ValueError):
        D.DeviceSplit.load(path, "cpu")
    torch.save({"tab1": rec["tab1"]}, path)                                            # not a split file at all
    with pytest.raises(ValueError):
        D.DeviceSplit.load(path, "cpu")


# ---- the in-order iterators' frame arithmetic ---------------------------------------------------------------------------------------
def _frames(count, batch_size, rank, world):
    nb, shares = D.sweep_shares(count, batch_size, rank, world)
    return nb, {b: list(range(first, last)) for b, first, last in shares}


def test_sweep_shares_single_process_keeps_the_short_last_batch():
    assert D.sweep_shares(7, 3) == (3, [(0, 0, 3), (1, 3, 6), (2, 6, 7)])
    assert D.sweep_shares(6, 3) == (2, [(0, 0, 3), (1, 3, 6)])
    assert D.sweep_shares(2, 3) == (1, [(0, 0, 2)])
    assert D.sweep_shares(0, 3) == (0, [])


@pytest.mark.parametrize("count,B", [(7, 3), (7, 2), (12, 2), (5, 4), (9, 1)])
@pytest.mark.parametrize("world", [1, 2])
def test_sweep_shares_of_all_ranks_are_the_single_process_batches(count, B, world):
    """The ranks' shares of global batch b, in rank order, are batch b of one process at the global batch size -- and b is the number
    the draw is keyed by, the same on every rank."""
    nb, single = _frames(count, world * B, 0, 1)
    assert nb == -(-count // (world * B)) and sorted(single) == list(range(nb))
    assert sum(single.values(), []) == list(range(count))                             # every frame once, in order, none dropped
    ranks = [_frames(count, B, r, world) for r in range(world)]
    assert all(n == nb for n, _ in ranks)
    for b in range(nb):
        assert sum((shares.get(b, []) for _, shares in ranks), []) == single[b], b
        assert all(len(shares.get(b, [])) <= B for _, shares in ranks)


def test_sweep_shares_empty_share_yields_nothing():
    """7 frames, 3 per rank, 2 ranks: the last global batch holds frame 6 only -- rank 1 has no entry for it."""
    assert D.sweep_shares(7, 3, 0, 2) == (2, [(0, 0, 3), (1, 6, 7)])
    assert D.sweep_shares(7, 3, 1, 2) == (2, [(0, 3, 6)])
    assert D.sweep_shares(2, 2, 1, 2) == (1, [])
    for rank, world in ((2, 2), (-1, 1), (0, 0)):
        with pytest.raises(ValueError):
            D.sweep_shares(7, 3, rank, world)
    with pytest.raises(ValueError):
        D.sweep_shares(7, 0)


def test_mini_clip_starts_and_their_steps():
    """Clips of 7 and 5 frames, L = 2: the remainders (frames 6 and 11) are dropped; a step of 4 mini-clips spans both clips."""
    clips = [(0, 7), (7, 12)]
    starts = D.mini_clip_starts(clips, 2)
    assert starts == [0, 2, 4, 7, 9]
    assert D.mini_clip_starts(clips, 5) == [0, 7] and D.mini_clip_starts(clips, 8) == [] and D.mini_clip_starts(clips, 1) == list(range(12))
    steps, shares = D.sweep_shares(len(starts), 4)
    assert steps == 2 and [starts[a:b] for _, a, b in shares] == [[0, 2, 4, 7], [9]]   # the short last step is kept
    two = [D.sweep_shares(len(starts), 2, r, 2)[1] for r in range(2)]
    assert [[starts[a:b] for _, a, b in s] for s in two] == [[[0, 2], [9]], [[4, 7]]]
    with pytest.raises(ValueError):
        D.mini_clip_starts(clips, 0)


def test_sweeps_refuse_a_cpu_split_and_a_split_without_clips():
    cpu = _split([(0, 7)])
    with pytest.raises(RuntimeError):
        next(cpu.sweep_resampled(3, 256, 1))
    with pytest.raises(RuntimeError):
        next(cpu.sweep_clips(3, 2, 256, 1))
    with pytest.raises(ValueError):
        next(_split().sweep_clips(3, 2, 256, 1))
    with pytest.raises(ValueError):
        next(cpu.sweep_resampled(3, 256, 1, rank=1, world=1))


# ---- the schedule and the best rule -------------------------------------------------------------------------------------------------
def _rates(opt, sched, epochs):
    out = []
    for _ in range(epochs):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("decay_epochs", [1, 2])
def test_schedule_is_steplr_and_survives_a_checkpoint(decay_epochs, tmp_path):
    adam = lambda: torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, weight_decay=1e-4)
    ref = adam()
    want = _rates(ref, torch.optim.lr_scheduler.StepLR(ref, decay_epochs, gamma=0.9), 5)
    opt = adam()
    assert _rates(opt, T.make_schedule(opt, decay_epochs, 0.9), 5) == want
    assert want[0] == 1e-3 and want[4] < want[0] and len(set(want)) == (5 if decay_epochs == 1 else 3)
    # two epochs, a save / load of optimizer and scheduler state into fresh objects, three more epochs
    opt = adam()
    sched = T.make_schedule(opt, decay_epochs, 0.9)
    head = _rates(opt, sched, 2)
    T.save_atomic({"optimizer": opt.state_dict(), "scheduler": sched.state_dict()}, str(tmp_path / "s.pt"))
    state = torch.load(str(tmp_path / "s.pt"))
    opt = adam()
    sched = T.make_schedule(opt, decay_epochs, 0.9)
    opt.load_state_dict(state["optimizer"])
    sched.load_state_dict(state["scheduler"])
    assert head + _rates(opt, sched, 3) == want


def test_best_rule_is_the_references():
    """main.py:143 on a scripted list: a tie replaces, NaN never does, a worse score does not."""
    best, replaced = math.inf, []
    for epoch, score in enumerate([0.5, 0.5, float("nan"), 0.4, math.inf]):
        if T.replaces_best(best, score):
            best = score
            replaced.append(epoch)
    assert replaced == [0, 1, 3] and best == 0.4
    assert T.replaces_best(math.inf, math.inf) and not T.replaces_best(math.inf, float("nan"))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    a = bench.Args()
    return {"cmflow": CMFlow(a), "cmflow_t": CMFlow_T(a), "raflow": RaFlow(a), "other": torch.nn.Linear(3, 3)}


FIT = dict(epochs=2, batch_size=2, val_batch_size=3, num_points=256)


@pytest.mark.parametrize("training", [True, False])
def test_fit_refusals_leave_the_mode_alone(nets, training):
    plain, clipped = _split(), _split([(0, 3), (3, 7)])
    cases = [("cmflow", plain, plain, dict(FIT), RuntimeError),                        # splits on the CPU
             ("raflow", plain, plain, dict(FIT), RuntimeError),
             ("cmflow_t", clipped, clipped, dict(FIT), RuntimeError),
             ("cmflow_t", plain, clipped, dict(FIT), ValueError),                      # CMFlow_T without clip ranges: training split
             ("cmflow_t", clipped, plain, dict(FIT), ValueError),                      # ... validation split
             ("cmflow", plain, plain, dict(FIT, epochs=0), ValueError),
             ("cmflow", plain, plain, dict(FIT, rank=0, world=2), ValueError),         # world > 1 without a process group
             ("cmflow", plain, plain, dict(FIT, rank=1, world=1), ValueError),
             ("other", plain, plain, dict(FIT), NotImplementedError)]
    for name, train_split, val_split, kw, error in cases:
        net = nets[name].train(training)
        with pytest.raises(error):
            T.fit(net, train_split, val_split, **kw)
        assert net.training == training and all(m.training == training for m in net.modules()), (name, kw)


@pytest.mark.parametrize("training", [True, False])
def test_eval_epoch_refusals_leave_the_mode_alone(nets, training):
    plain, clipped = _split(), _split([(0, 3), (3, 7)])
    cases = [(EV.eval_epoch, "cmflow", (plain, 3, 256, 1), {}, RuntimeError),          # a split on the CPU
             (EV.eval_epoch, "raflow", (plain, 3, 256, 1), {}, RuntimeError),          # RaFlow is accepted: it gets as far as the device check
             (EV.eval_epoch, "cmflow_t", (clipped, 3, 256, 1), {}, ValueError),        # the wrong model class for the driver
             (EV.eval_epoch, "other", (plain, 3, 256, 1), {}, NotImplementedError),
             (EV.eval_epoch, "cmflow", (plain, 3, 256, 1), dict(rank=2, world=2), ValueError),
             (EV.eval_epoch, "cmflow", (plain, 3, 256, 1), dict(rank=0, world=2), ValueError),      # no process group
             (EV.eval_epoch_clips, "cmflow_t", (clipped, 2, 2, 256, 1), {}, RuntimeError),
             (EV.eval_epoch_clips, "cmflow", (clipped, 2, 2, 256, 1), {}, ValueError),
             (EV.eval_epoch_clips, "raflow", (clipped, 2, 2, 256, 1), {}, ValueError),
             (EV.eval_epoch_clips, "cmflow_t", (plain, 2, 2, 256, 1), {}, ValueError),              # no clip ranges
             (EV.eval_epoch_clips, "cmflow_t", (clipped, 2, 2, 256, 1), dict(rank=0, world=0), ValueError),
             (EV.eval_epoch_clips, "cmflow_t", (clipped, 2, 2, 256, 1), dict(rank=1, world=2), ValueError)]
    for fn, name, pos, kw, error in cases:
        net = nets[name].train(training)
        with pytest.raises(error):
            fn(net, *pos, **kw)
        assert net.training == training and all(m.training == training for m in net.modules()), (fn.__name__, name, kw)
