"""CPU: the argument checks the stages of a test run's analysis chain share (cmflow_amd/_frames.py).  For ``accumulate``, ``cluster``,
``track`` and ``estimate`` every argument error their docstrings list is raised with the caller's name in front and before any device
work -- the splits here are on the CPU, so a call that got as far as the device would raise RuntimeError instead -- and a call that
is wrong in two ways raises what comes first in the stage's own order; the number and whole-number checks refuse what is no number,
not finite, or just outside a bound, and take numpy's scalars; the frame selection gives the same ids for None, a list and an int64
tensor."""
import numpy as np
import pytest
import torch

from cmflow_amd import _frames
from cmflow_amd import accumulate as A
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import objects as O
from cmflow_amd import results as R
from cmflow_amd import tracks as K

f32 = np.float32
COUNTS = [5, 1, 9, 4]


def _cpu_split(counts=COUNTS, clips=None):
    rng = np.random.default_rng(0)
    z = lambda *s: np.zeros(s, dtype=f32)
    items = [(rng.standard_normal((n, 3)).astype(f32), z(4, 3) + 1, z(n, 3), z(4, 3), np.eye(4, dtype=f32), z(n, 3), z(n), 0.1, z(n), z(n), z(n, 2))
             for n in counts]
    return D.DeviceSplit.from_items(items, "cpu", clips)


def _cpu_instances(split, which="gt"):
    total, F = split.tab1.shape[0], len(split)
    t = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    tables = (t(total), t(total), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32), t(total, 3, dt=torch.float32))
    off = np.concatenate(([0], np.cumsum(split.counts_host[0])))
    return I.FrameInstances(split.off1, torch.arange(F), t(total) - 1, t(total, dt=torch.uint8), t(F), tables, split.interval, which, 2.0, 2, 0.0,
                            off, np.arange(F))


def _cpu_tracks(split, which="gt"):
    total, F = split.tab1.shape[0], len(split)
    t = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    arrays = (t(total) - 1, t(total) - 1, t(total), t(total), t(total, 3, dt=torch.float32), t(total) - 1, t(total) - 1, t(total) - 1, t(total))
    clips = K.plan_clips(F, split.clips)
    return K.InstanceTracks(_cpu_instances(split, which), arrays, t(len(clips)), t(len(clips)), torch.from_numpy(clips), clips, 2.0, 2)


@pytest.fixture(scope="module")
def world():
    split = _cpu_split()
    store = R.SplitResults.empty(split)                                     # nothing done
    done = R.SplitResults.empty(split)
    done.done.fill_(1)
    other_rows, other_frames = R.SplitResults.empty(_cpu_split([5, 1, 9, 5])), R.SplitResults.empty(_cpu_split([5, 1, 13]))
    return {"split": split, "store": store, "done": done, "others": (other_rows, other_frames)}


def _refused(what, call):
    """ValueError (never the RuntimeError of a call that reached the device), the caller's name in front"""
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value).startswith(what + ": "), str(e.value)
    return str(e.value)


NO_NUMBER = (True, float("nan"), float("inf"), -float("inf"), "2", None)


def test_accumulate_refuses_every_listed_error_under_its_name(world):
    split, store, done = world["split"], world["store"], world["done"]
    for window in (0, 65, 2.0, "8") + NO_NUMBER:
        assert "window" in _refused("accumulate", lambda: A.accumulate(split, None, window=window, which="gt"))
    assert "which" in _refused("accumulate", lambda: A.accumulate(split, done, which="label"))
    assert "dynamic" in _refused("accumulate", lambda: A.accumulate(split, done, dynamic="trail"))
    assert "store" in _refused("accumulate", lambda: A.accumulate(split, None, which="pred"))
    for other in world["others"]:
        assert "not the one" in _refused("accumulate", lambda: A.accumulate(split, other))
    assert "no results" in _refused("accumulate", lambda: A.accumulate(split, store, window=2, frames=[2]))
    for frames in ([4], [-1], torch.tensor([0, 7])):
        assert "outside" in _refused("accumulate", lambda: A.accumulate(split, done, frames=frames))
    F, n = 64, 2 ** 24
    off = torch.arange(F + 1, dtype=torch.int64).mul(n).to(torch.int32)
    large = D.DeviceSplit(torch.zeros((0, 14)), torch.zeros((0, 6)), off, off, torch.zeros((F, 16)), torch.zeros(F), n)
    assert "2^31" in _refused("accumulate", lambda: A.accumulate(large, None, window=3, which="gt"))
    # the stage's own order: which, dynamic, the store, the selection's type, the window, the selection's bounds, done
    assert "which" in _refused("accumulate", lambda: A.accumulate(split, None, window=0, which="label", dynamic="trail"))
    assert "dynamic" in _refused("accumulate", lambda: A.accumulate(split, None, window=0, dynamic="trail"))
    assert "store" in _refused("accumulate", lambda: A.accumulate(split, None, window=0, frames=[9]))
    assert "int64" in _refused("accumulate", lambda: A.accumulate(split, store, window=0, frames=torch.tensor([9], dtype=torch.int32)))
    assert "window" in _refused("accumulate", lambda: A.accumulate(split, store, window=0, frames=[9]))
    assert "outside" in _refused("accumulate", lambda: A.accumulate(split, store, window=2, frames=[9]))
    with pytest.raises(RuntimeError, match="GPU"):                          # everything in order: only the device is wrong
        A.accumulate(split, done, window=np.int64(2), frames=[2, 3])


def test_cluster_refuses_every_listed_error_under_its_name(world):
    split, store, done = world["split"], world["store"], world["done"]
    gt = lambda **kw: I.cluster(split, None, which="gt", **kw)
    assert "which" in _refused("cluster", lambda: I.cluster(split, done, which="label"))
    assert "store" in _refused("cluster", lambda: I.cluster(split, None))
    for other in world["others"]:
        assert "not the one" in _refused("cluster", lambda: I.cluster(split, other))
    for eps in (0.0, -1e-9) + NO_NUMBER:
        assert "eps" in _refused("cluster", lambda: gt(eps=eps))
    for weight in (-1e-9,) + NO_NUMBER:
        assert "flow_weight" in _refused("cluster", lambda: gt(flow_weight=weight))
    for min_points in (0, 2 ** 31, 2.0) + NO_NUMBER:
        assert "min_points" in _refused("cluster", lambda: gt(min_points=min_points))
    for frames in ([4], [-1], torch.tensor([0, 7])):
        assert "outside" in _refused("cluster", lambda: gt(frames=frames))
    assert "1025 points" in _refused("cluster", lambda: I.cluster(_cpu_split([3, 1025]), None, which="gt"))
    assert "no results" in _refused("cluster", lambda: I.cluster(split, store, frames=[0, 2]))
    # the stage's own order: which, the store, eps, flow_weight, min_points, the selection, the frame sizes, done
    assert "store" in _refused("cluster", lambda: I.cluster(split, None, eps=0, flow_weight=-1, min_points=0, frames=[9]))
    assert "eps" in _refused("cluster", lambda: I.cluster(split, store, eps=0, flow_weight=-1, min_points=0, frames=[9]))
    assert "flow_weight" in _refused("cluster", lambda: I.cluster(split, store, flow_weight=-1, min_points=0, frames=[9]))
    assert "min_points" in _refused("cluster", lambda: I.cluster(split, store, min_points=0, frames=[9]))
    assert "outside" in _refused("cluster", lambda: I.cluster(split, store, frames=[9]))
    with pytest.raises(RuntimeError, match="GPU"):
        I.cluster(split, done, eps=np.float32(0.5), min_points=np.int32(3), flow_weight=0, frames=[1, 0])


def test_track_refuses_every_listed_error_under_its_name(world):
    split, done = world["split"], world["done"]
    inst, pred = _cpu_instances(split), _cpu_instances(split, "pred")
    assert "cluster()" in _refused("track", lambda: K.track({"label": None}, split))
    assert "store" in _refused("track", lambda: K.track(pred, split))
    for counts in ([5, 1, 9, 5], [5, 1, 13]):
        assert "instances belong" in _refused("track", lambda: K.track(inst, _cpu_split(counts)))
    for other in world["others"]:
        assert "results belong" in _refused("track", lambda: K.track(pred, split, other))
    for gate in (0.0, -1e-9) + NO_NUMBER:
        assert "gate" in _refused("track", lambda: K.track(inst, split, gate=gate))
    for max_gap in (-1, 17, 2.0) + NO_NUMBER:
        assert "max_gap" in _refused("track", lambda: K.track(inst, split, max_gap=max_gap))
    for clips, word in (([(0, 3), (2, 4)], "overlaps"), ([(3, 1)], "descends")):
        assert word in _refused("track", lambda: K.track(inst, _cpu_split(COUNTS, clips)))
    # the stage's own order: inst, the store, the split, gate, max_gap, the clips
    assert "store" in _refused("track", lambda: K.track(pred, _cpu_split([5, 1, 13]), gate=0, max_gap=-1))
    assert "instances belong" in _refused("track", lambda: K.track(inst, _cpu_split([5, 1, 13]), gate=0, max_gap=-1))
    assert "gate" in _refused("track", lambda: K.track(inst, _cpu_split(COUNTS, [(3, 1)]), gate=0, max_gap=-1))
    assert "max_gap" in _refused("track", lambda: K.track(inst, _cpu_split(COUNTS, [(3, 1)]), max_gap=-1))
    with pytest.raises(RuntimeError, match="GPU"):
        K.track(pred, split, done, gate=np.float64(1.5), max_gap=np.int64(16))


def test_estimate_refuses_every_listed_error_under_its_name(world):
    split, done = world["split"], world["done"]
    trk, pred = _cpu_tracks(split), _cpu_tracks(split, "pred")
    assert "track()" in _refused("estimate", lambda: O.estimate(trk.inst, split))
    assert "store" in _refused("estimate", lambda: O.estimate(pred, split))
    for counts in ([5, 1, 9, 5], [5, 1, 13]):
        assert "tracks belong" in _refused("estimate", lambda: O.estimate(trk, _cpu_split(counts)))
    for other in world["others"]:
        assert "results belong" in _refused("estimate", lambda: O.estimate(pred, split, other))
    for name in ("sigma_pos", "sigma_disp"):
        for v in (0.0, -1e-9) + NO_NUMBER:
            assert name in _refused("estimate", lambda: O.estimate(trk, split, **{name: v}))
    for name in ("sigma_acc", "min_disp"):
        for v in (-1e-9,) + NO_NUMBER:
            assert name in _refused("estimate", lambda: O.estimate(trk, split, **{name: v}))
    # the stage's own order: trk, the store, the split, the four numbers as they stand in the signature
    assert "store" in _refused("estimate", lambda: O.estimate(pred, _cpu_split([5, 1, 13]), sigma_pos=0))
    assert "tracks belong" in _refused("estimate", lambda: O.estimate(trk, _cpu_split([5, 1, 13]), sigma_pos=0))
    assert "sigma_pos" in _refused("estimate", lambda: O.estimate(trk, split, sigma_pos=0, sigma_disp=0, sigma_acc=-1, min_disp=-1))
    assert "sigma_disp" in _refused("estimate", lambda: O.estimate(trk, split, sigma_disp=0, sigma_acc=-1, min_disp=-1))
    assert "sigma_acc" in _refused("estimate", lambda: O.estimate(trk, split, sigma_acc=-1, min_disp=-1))
    with pytest.raises(RuntimeError, match="GPU"):
        O.estimate(pred, split, done, sigma_pos=np.float32(1), sigma_disp=2, sigma_acc=0, min_disp=np.float64(0.0))


def test_number_and_whole_number_checks():
    for zero_ok in (False, True):
        for v in NO_NUMBER + (-1e-300, -1, np.float64("nan"), np.float32("inf"), [1.0], 1 + 0j):
            with pytest.raises(ValueError, match=r"^who: x = .* \(in words\)$"):
                _frames.number("who", "x", v, zero_ok, "in words")
        for v in (1e-300, 1, 2.5, np.float32(0.5), np.float64(3.0), np.int64(4), np.uint8(1)):
            got = _frames.number("who", "x", v, zero_ok, "in words")
            assert type(got) is float and got == float(v)
    with pytest.raises(ValueError, match="x = 0"):
        _frames.number("who", "x", 0, False, "in words")
    with pytest.raises(ValueError, match=r"x = .*0\.0"):
        _frames.number("who", "x", np.float64(0.0), False, "in words")
    assert _frames.number("who", "x", 0, True, "in words") == 0.0 and _frames.number("who", "x", np.float32(0.0), True, "in words") == 0.0

    for lo, hi in ((1, 64), (0, 16), (1, None)):
        top = 2 ** 31 - 1 if hi is None else hi
        words = r"\(a whole number, %d or above\)$" % lo if hi is None else r"\(a whole number from %d to %d\)$" % (lo, hi)
        for v in NO_NUMBER + (lo - 1, top + 1, float(lo), np.float64(lo), np.int64(lo - 1), np.int64(top + 1), [lo]):
            with pytest.raises(ValueError, match=r"^who: n = .* " + words):
                _frames.whole("who", "n", v, lo, hi)
        for v in (lo, top, np.int32(lo), np.int64(top), np.uint8(lo + 1)):
            got = _frames.whole("who", "n", v, lo, hi)
            assert type(got) is int and got == int(v)


def test_selection_gives_the_same_ids_for_none_a_list_and_a_tensor():
    F = 6
    everything = _frames.selected(None, F, "who")
    assert everything.dtype == np.int64 and everything.tolist() == list(range(F))
    for got in (_frames.selected(list(range(F)), F, "who"), _frames.selected(torch.arange(F), F, "who"), _frames.selected(range(F), F, "who")):
        assert got.dtype == np.int64 and np.array_equal(got, everything)
    picked = [4, 0, 4, 5]                                                    # order and repeats are the caller's
    for got in (_frames.selected(picked, F, "who"), _frames.selected(torch.tensor(picked), F, "who"), _frames.selected(np.array(picked), F, "who")):
        assert got.dtype == np.int64 and got.tolist() == picked
    assert _frames.selected([], F, "who").size == 0 and _frames.selected(torch.zeros(0, dtype=torch.int64), F, "who").size == 0
    for bad in (torch.tensor([1], dtype=torch.int32), torch.tensor([[1, 2]]), torch.tensor(1), torch.tensor([1.0])):
        with pytest.raises(ValueError, match="^who: frames is a list or a 1-d int64 tensor"):
            _frames.selected(bad, F, "who")
    for bad in ([F], [-1], torch.tensor([0, F]), [0, -1, 2]):
        with pytest.raises(ValueError, match="^who: frames outside 0 .. 5$"):
            _frames.selected(bad, F, "who")
        assert _frames.selected(bad, F, "who", bounds=False).tolist() == [int(f) for f in bad]


def test_the_public_names_stay_where_they_were():
    assert A.WHICH is I.WHICH is _frames.WHICH and A.WHICH == ("pred", "gt")
    assert A._to_device is _frames.to_device
    t = A._to_device(np.arange(3), torch.int32, torch.device("cpu"))
    assert t.dtype == torch.int32 and t.tolist() == [0, 1, 2]
    off = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    assert _frames.per_row(torch.tensor([0.1, 0.2, 0.4]), off, 5).tolist() == pytest.approx([0.1, 0.1, 0.4, 0.4, 0.4])
