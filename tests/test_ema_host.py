"""Host: what the averaged weights decide without a device -- the checks of ``ema_decay``, the refusal on a CPU model (torch's Adam
keeps no average, and nothing falls back), the argument checks of the new launchers, the keywords, and the float64 reference of the
GPU tests.  Every test fails on the parent commit: the symbols and the keyword do not exist there."""
import inspect

import numpy as np
import pytest
import torch

import ema_ref as E
from cmflow_amd import _lib, dp
from cmflow_amd import train as T
from cmflow_amd.train import TrainStep


@pytest.mark.parametrize("good", [0.5, 0.9, 0.999, 1e-6, 1.0 - 2.0 ** -30])
def test_ema_options_accept_the_open_interval(good):
    assert dp.ema_options(good) == good and type(dp.ema_options(good)) is float
    assert dp.ema_options(None) is None and dp.ema_options() is None


@pytest.mark.parametrize("bad", [True, False, 0, 0.0, 1, 1.0, -0.5, -1, 1.5, float("nan"), float("inf"), -float("inf"), "0.9"])
def test_ema_decay_must_lie_inside_0_1(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        dp.ema_options(bad)
    with pytest.raises(ValueError, match="ema_decay"):
        TrainStep(torch.nn.Linear(3, 2), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):                # checked before the optimizer looks at the device
        dp.FlatAdam(dp.FlatGradBucket(torch.nn.Linear(3, 2)), ema_decay=bad)


def test_cpu_model_refuses_the_average_and_is_unchanged_without_it():
    with pytest.raises(ValueError, match="GPU"):
        TrainStep(torch.nn.Linear(3, 2), ema_decay=0.9)
    with pytest.raises(ValueError, match="GPU"):
        dp.FlatAdam(dp.FlatGradBucket(torch.nn.Linear(3, 2)), ema_decay=0.9)
    assert type(TrainStep(torch.nn.Linear(3, 2)).opt) is torch.optim.Adam       # off: torch's own Adam, as before


def test_fit_refuses_a_bad_ema_decay_first():
    with pytest.raises(ValueError, match="ema_decay"):
        T.fit(torch.nn.Linear(3, 3), None, None, epochs=1, batch_size=2, val_batch_size=2, num_points=256, ema_decay=1.0)


def test_keywords():
    for fn in (T.fit, TrainStep.__init__, dp.FlatAdam.__init__):
        p = inspect.signature(fn).parameters["ema_decay"]
        assert p.default is None, fn


def test_launchers_refuse_bad_arguments_before_any_launch():
    """A null or misaligned ``ema`` / ``flat``, a decay outside (0, 1) or NaN, total <= 0: hipErrorInvalidValue (1) from the argument
    checks in front of the launch (no device is touched)."""
    _lib.build()
    L = _lib.lib()
    args = (1, 256, 256, 8, 256, 256, 256, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    guard = (1.0, 1, 256, 256)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert L.cmf_adam_step_ema(*args, 256, bad, None) == 1, bad
        assert L.cmf_adam_step_guarded_ema(*args, *guard, 256, bad, None) == 1, bad
    for ema in (None, 256 + 2):
        assert L.cmf_adam_step_ema(*args, ema, 0.9, None) == 1
        assert L.cmf_adam_step_guarded_ema(*args, *guard, ema, 0.9, None) == 1
    assert L.cmf_adam_step_ema(*(args[:3] + (0,) + args[4:]), 256, 0.9, None) == 1
    assert L.cmf_adam_step_guarded_ema(*args, 1.0, 1, None, 256, 256, 0.9, None) == 1      # the guard's own checks still hold
    assert L.cmf_param_exchange(1, 256, 256, 8, None, None) == 1 and L.cmf_param_exchange(1, 256, 256, 8, 256 + 1, None) == 1
    assert L.cmf_param_exchange(0, 256, 256, 8, 256, None) == 1 and L.cmf_param_exchange(1, 256, 256, 0, 256, None) == 1
    assert L.cmf_param_exchange(1, None, 256, 8, 256, None) == 1 and L.cmf_param_exchange(1, 256, None, 8, 256, None) == 1


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999])
def test_recurrence_on_a_constant_sequence(decay):
    """p = e0 at every step: the lerp form's fixed point, so e is e0 exactly, and the bound is of the order of an ulp -- it converges
    to 2^-23 |e0| / omd from below and is 2^-23 |e0| after one step."""
    e0 = torch.randn(257, generator=torch.Generator().manual_seed(2)).numpy()
    e, b = E.ema_recurrence([e0] * 1, e0, decay)
    assert e.dtype == np.float64 and b.dtype == np.float64 and np.array_equal(e, e0.astype(np.float64))
    assert np.array_equal(b, 2.0 ** -23 * np.abs(e0.astype(np.float64)))
    e, b = E.ema_recurrence([e0] * 7, e0, decay)
    omd = float(np.float32(1.0 - decay))
    assert np.array_equal(e, e0.astype(np.float64))
    assert (b >= 2.0 ** -23 * np.abs(e)).all() and (b <= 2.0 ** -23 * np.abs(e) / omd * (1 + 1e-12)).all()


def test_recurrence_follows_a_step():
    """One hand-checked step: e0 = 0, p = 1, decay 0.5 -> e = 0.5; then p = 1 again -> 0.75."""
    e, b = E.ema_recurrence([np.ones(1, np.float32)] * 2, np.zeros(1, np.float32), 0.5)
    assert e.tolist() == [0.75] and 0 < b[0] < 4 * 2.0 ** -23


def test_odd_bucket_straddles_every_boundary():
    bucket = dp.FlatGradBucket(E.odd_module("cpu"))
    assert bucket.numel == E.ODD_TOTAL == 4101 and bucket.numel % 4 != 0
    offs = np.cumsum((0,) + E.ODD_SIZES)
    assert all(c not in offs for c in range(1024, E.ODD_TOTAL, 1024))           # every chunk boundary inside a tensor
    assert all(o % 1024 != 0 for o in offs[1:-1])                                # every tensor boundary inside a chunk
