"""Host: what the guarded optimizer step decides without a device -- the partition of the gradient-norm kernel (cmf_grad_norm_parts is
host arithmetic on `total` alone), the checks of ``max_grad_norm``, and the refusal of a guard on a CPU model (torch's Adam has none,
and nothing falls back).  Every test fails on the parent commit: the symbol and the keywords do not exist there."""
import os
import subprocess
import sys

import pytest
import torch

import grad_guard_ref as G
from cmflow_amd import _lib, dp
from cmflow_amd.train import TrainStep

TOTALS = [1, 2, 1023, 1024, 1025, 4096, 4097, 4 * 1024 + 3, 8192, 8193, 300001, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1,
          4218880, 2 ** 31 + 5, 2 ** 40]


def _parts(total):
    return _lib.lib().cmf_grad_norm_parts(total)


def test_parts_range_and_monotony():
    _lib.build()
    got = [_parts(t) for t in TOTALS]
    assert all(1 <= p <= 256 for p in got), got
    assert got == sorted(got), got                                   # non-decreasing in total
    assert all(_parts(t) == 1 for t in range(1, 1025)) and _parts(4097) == 2
    assert _parts(1024 * 1024) == 256 and _parts(2 ** 40) == 256     # saturates
    dense = [_parts(t) for t in range(1, 1024 * 1100, 509)]          # ... and every step on the way up is 0 or +1 slab group
    assert all(0 <= b - a <= 1 for a, b in zip(dense, dense[1:])) and dense[-1] == 256
    assert _parts(0) == 0 and _parts(-5) == 0                         # not a count: the launchers refuse total <= 0


def test_parts_are_the_same_in_another_process():
    """A function of `total` alone: a second process, with another environment, gives the same answers."""
    _lib.build()
    code = ("from cmflow_amd import _lib; print([_lib.lib().cmf_grad_norm_parts(t) for t in %r])" % (TOTALS,))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="3")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert eval(out.stdout.strip().splitlines()[-1]) == [_parts(t) for t in TOTALS]


def test_launchers_refuse_bad_arguments_before_any_launch():
    """total <= 0, null pointers, a gradient pointer that is not 16-byte aligned, a NaN max_grad_norm: hipErrorInvalidValue (1),
    returned by the argument checks in front of the launch (no device is touched)."""
    _lib.build()
    L = _lib.lib()
    assert L.cmf_grad_sumsq(0, 256, 256, None) == 1 and L.cmf_grad_sumsq(8, None, 256, None) == 1 and L.cmf_grad_sumsq(8, 256, None, None) == 1
    assert L.cmf_grad_sumsq(8, 256 + 4, 256, None) == 1 and L.cmf_grad_sumsq(8, 256 + 8, 256, None) == 1     # float-aligned is not enough
    assert L.cmf_grad_norm(8, 256, 256, None, None) == 1 and L.cmf_grad_norm(8, 256 + 4, 256, 256, None) == 1
    args = (1, 256, 256, 8, 256, 256, 256, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    assert L.cmf_adam_step_guarded(*args, 1.0, 1, None, 256, None) == 1 and L.cmf_adam_step_guarded(*args, 1.0, 1, 256, None, None) == 1
    assert L.cmf_adam_step_guarded(*args, float("nan"), 1, 256, 256, None) == 1


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.0, float("nan"), float("inf"), "1", True])
def test_max_grad_norm_must_be_positive_and_finite(bad):
    with pytest.raises(ValueError):
        dp.guard_options(bad, False)
    with pytest.raises(ValueError):
        TrainStep(torch.nn.Linear(3, 2), max_grad_norm=bad)
    with pytest.raises(ValueError):                                   # checked before the optimizer looks at the device
        dp.FlatAdam(dp.FlatGradBucket(torch.nn.Linear(3, 2)), max_grad_norm=bad)


def test_guard_options_pass_good_values():
    assert dp.guard_options() == (None, False) and dp.guard_options(2, 1) == (2.0, True) and dp.guard_options(1e-3, False) == (1e-3, False)


def test_cpu_train_step_refuses_a_guard_and_is_unchanged_without_one():
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(max_grad_norm=1.0, skip_nonfinite=True)):
        with pytest.raises(ValueError, match="GPU"):
            TrainStep(torch.nn.Linear(3, 2), **kw)
    net = torch.nn.Linear(3, 2)
    step = TrainStep(net)                                             # no guard: torch's own Adam, as before
    assert type(step.opt) is torch.optim.Adam and step.opt.defaults["lr"] == 1e-3 and step.opt.defaults["weight_decay"] == 1e-4
    assert [p.data_ptr() for p in step.opt.param_groups[0]["params"]] == [p.data_ptr() for p in net.parameters()]
    before = [p.detach().clone() for p in net.parameters()]
    step.bucket.zero()
    net(torch.ones(4, 3)).sum().backward()
    step.opt.step()
    assert all(not torch.equal(a, p) for a, p in zip(before, net.parameters()))


def test_fit_refuses_a_bad_max_grad_norm_first():
    from cmflow_amd import train as T
    with pytest.raises(ValueError, match="max_grad_norm"):
        T.fit(torch.nn.Linear(3, 3), None, None, epochs=1, batch_size=2, val_batch_size=2, num_points=256, max_grad_norm=0)


def test_ragged_case_of_the_gpu_test_is_sound():
    """The two frames of the whole-frame GPU test hold both motion-segmentation classes and a static point each (an empty class makes
    the class-balanced BCE NaN by itself: the GPU test must see a NaN only where it plants one)."""
    import ragged_loss_case as RC
    from oracle import train_oracle as TO
    batch, outs = RC.make_case(G.RAGGED_COUNTS, G.RAGGED_SEED)
    for i in range(len(G.RAGGED_COUNTS)):
        dyn, mseg = TO.make_labels(RC.sample(batch, outs, G.RAGGED_COUNTS, i)[0])
        assert int((mseg == 0).sum()) >= 1 and int((mseg == 1).sum()) >= 1 and int((dyn == 0).sum()) >= 1, i
    pb = G.ragged_batch()
    assert pb["n1"].tolist() == [256, 33] and all(torch.isfinite(v).all() for v in pb.values() if v.is_floating_point())


def test_exact_reference_is_exact():
    x = torch.tensor([3e38, -3e38, 1e-20, 1.0], dtype=torch.float32)
    big = float(torch.tensor(3e38, dtype=torch.float32)) ** 2
    assert G.exact_sumsq(x) == 2 * big                               # finite (an fp32 sum is not); 1 is far below the last bit of 1.8e77
    assert G.exact_sumsq(torch.tensor([3.0, 4.0])) == 25.0
    assert G.clip_scale(2.0, 1.0) < 0.5 and G.clip_scale(0.5, 1.0) == 1.0
