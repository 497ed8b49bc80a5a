"""GPU: the guarded optimizer step -- the gradient norm on the device (cmf_grad_sumsq / cmf_grad_norm), clipping by it and skipping a
non-finite step (cmf_adam_step_guarded), through ``dp.grad_norm``, ``dp.FlatAdam``, ``TrainStep`` and ``train.fit``.

The norm is held to an EXACT reference (math.fsum of the exact float64 squares) within total * 2^-52: the squares are exact in double
and only the additions round, so the bound is gamma_n with a factor 2 of margin -- derived, not measured.  The guarded step is held bit
for bit to the unguarded ``FlatAdam`` on a bucket scaled by hand, and within the existing optimizer test's bound to
``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam``.  Every test fails on the parent commit: the symbols and keywords are new."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import grad_guard_ref as G
import run_dp_worker as R
from cmflow_amd import _lib, dp
from cmflow_amd import train as T
from cmflow_amd.train import TrainStep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    """Two dicts of tensors, bit for bit."""
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _same_but_nan(a, b, what):
    """... where NaN equals NaN whatever its payload."""
    for k in a:
        na, nb = torch.isnan(a[k]), torch.isnan(b[k])
        assert torch.equal(na, nb) and torch.equal(_bits(a[k][~na]), _bits(b[k][~nb])), (what, k)


# ---- 1, 2. the norm -------------------------------------------------------------------------------------------------------------------
def _norm(flat):
    """cmf_grad_norm on a 1-d fp32 device tensor -> (out[2], partials[P], the two entries behind the P partials), host float64."""
    L = _lib.lib()
    n = flat.numel()
    P = L.cmf_grad_norm_parts(n)
    partials = torch.full((P + 2,), math.nan, dtype=torch.float64, device=flat.device)
    out = torch.full((2,), math.nan, dtype=torch.float64, device=flat.device)
    _lib.check(L.cmf_grad_norm(n, _lib.dev_ptr(flat, torch.float32), partials.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "cmf_grad_norm")
    partials = partials.cpu().numpy()
    return out.cpu().numpy(), partials[:P], partials[P:]


@pytest.mark.parametrize("total", G.SUMSQ_TOTALS)
def test_norm_against_the_exact_sum(total, dev):
    x = G.wide_range_values(total, seed=total)
    want = G.exact_sumsq(x)
    flat = x.to(dev)
    out, partials, behind = _norm(flat)
    err = abs(out[0] - want) / want
    print("total %d: P = %d, sumsq %.17g, exact %.17g, relative error %.3g (bound %.3g)" % (total, partials.size, out[0], want, err, G.sumsq_bound(total)))
    assert err <= G.sumsq_bound(total)
    assert out[1] == math.sqrt(out[0])
    assert partials.size == _lib.lib().cmf_grad_norm_parts(total) and (total <= 4096 or partials.size > 1)
    assert np.isfinite(partials).all() and np.isnan(behind).all()               # exactly P entries written
    again = _norm(flat)
    assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == partials.tobytes()      # bit-reproducible
    # a view at an offset of one float is not 16-byte aligned: an argument error, nothing launched
    if total > 1:
        L = _lib.lib()
        scratch = torch.zeros(4, dtype=torch.float64, device=dev)
        assert L.cmf_grad_norm(total - 1, flat[1:].data_ptr(), scratch.data_ptr(), scratch.data_ptr(), _lib.stream_ptr()) == 1


def test_norm_range(dev):
    """+-3e38 everywhere: the squares (9e76) overflow an fp32 accumulator, the double sum is finite and within the same bound.  One NaN,
    +Inf or -Inf -- first element, last element, first element of the second slab -- makes the sum of squares non-finite."""
    n = G.RANGE_TOTAL
    sign = torch.where(torch.arange(n) % 3 == 0, -1.0, 1.0)
    x = (sign * 3e38).float()
    want = G.exact_sumsq(x)
    out = _norm(x.to(dev))[0]
    assert math.isfinite(out[0]) and abs(out[0] - want) / want <= G.sumsq_bound(n) and out[1] == math.sqrt(out[0])
    assert not math.isfinite(float((x * x).sum()))                              # what an fp32 accumulator gives
    base = G.wide_range_values(n, seed=7).to(dev)
    for where in (0, n - 1, 1024):
        for bad in (math.nan, math.inf, -math.inf):
            flat = base.clone()
            flat[where] = bad
            out = _norm(flat)[0]
            assert not math.isfinite(out[0]) and not math.isfinite(out[1]), (where, bad, out)
            assert math.isnan(out[0]) == math.isnan(bad), (where, bad, out)      # Inf^2 is +Inf, never Inf - Inf


# ---- 3. the guarded step, composed from the unguarded one ----------------------------------------------------------------------------
def _pair(dev, **guard):
    """Two copies of the small module, their buckets, a guarded FlatAdam on the first and an unguarded one on the second."""
    a, b = G.small_module(dev), G.small_module(dev)
    b.load_state_dict(a.state_dict())
    ba, bb = dp.FlatGradBucket(a), dp.FlatGradBucket(b)
    return a, b, ba, bb, dp.FlatAdam(ba, lr=1e-3, weight_decay=1e-4, **guard), dp.FlatAdam(bb, lr=1e-3, weight_decay=1e-4)


def _gradient(net, bucket, x):
    bucket.zero()
    net(x).square().mean().backward()


def _opt_state(net, opt):
    d = {"p.%s" % k: p.detach() for k, p in net.named_parameters()}
    d.update(exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq)
    return d


def _inputs(dev, steps=5):
    g = torch.Generator().manual_seed(11)
    return [torch.randn(64, 37, generator=g).to(dev) for _ in range(steps)]


def test_bucket_straddles_chunks_and_parts(dev):
    bucket = dp.FlatGradBucket(G.small_module(dev))
    assert bucket.numel == 37 * 129 + 2 * 129 + 129 * 5 + 5 and bucket.numel % 1024 != 0 and _lib.lib().cmf_grad_norm_parts(bucket.numel) == 2


def test_skip_only_guard_on_finite_gradients_is_the_unguarded_step(dev):
    """(a) and (c): nothing to skip, nothing clipped (no max_grad_norm / ten times the norm) -> bit-identical to FlatAdam after every
    step, and the record counts it."""
    xs = _inputs(dev)
    records = []
    for guard in (dict(skip_nonfinite=True), None):
        if guard is None:                                              # (c): ten times the largest norm of run (a)
            guard = dict(max_grad_norm=10.0 * records[0][4], skip_nonfinite=True)
        a, b, ba, bb, oa, ob = _pair(dev, **guard)
        total, biggest = 0.0, 0.0
        for k, x in enumerate(xs):
            _gradient(a, ba, x)
            bb.flat.copy_(ba.flat)
            norm = dp.grad_norm(ba)
            assert norm.dtype == torch.float64 and norm.dim() == 0 and norm.is_cuda
            before = ba.flat.clone()
            oa.step(); ob.step()
            assert torch.equal(_bits(ba.flat), _bits(before))          # the bucket is left as it was
            _same(_opt_state(a, oa), _opt_state(b, ob), ("step", k, guard))
            rec = oa.guard_stats().tolist()
            normf = float(norm.float())
            total += normf
            biggest = max(biggest, normf)
            assert rec[:5] == [k + 1, 0, 0, total, biggest] and rec[6] == normf and rec[7] == 1.0, (k, rec)
            assert rec[5] > 0 and float(torch.tensor(math.sqrt(rec[5]), dtype=torch.float64).float()) == normf
        records.append(rec)
    assert records[0] == records[1]


def test_clipped_step_is_the_unguarded_step_on_a_scaled_bucket(dev):
    """(b) max_grad_norm = half the first norm: after every step bit-identical to FlatAdam on the bucket multiplied elementwise, in
    fp32, by record[7]; record[7] is torch's clip coefficient in fp32 from record[6]; record[2] counts the clipped steps."""
    xs = _inputs(dev)
    probe, _, pb, _, _, _ = _pair(dev)
    _gradient(probe, pb, xs[0])
    c = 0.5 * float(dp.grad_norm(pb))
    a, b, ba, bb, oa, ob = _pair(dev, max_grad_norm=c)
    clipped = 0
    for k, x in enumerate(xs):
        _gradient(a, ba, x)
        oa.step()
        rec = oa.guard_stats().tolist()
        assert rec[6] == float(dp.grad_norm(ba).float())
        assert rec[7] == G.clip_scale(rec[6], c), (k, rec)
        clipped += rec[7] < 1.0
        assert rec[0] == k + 1 and rec[1] == 0 and rec[2] == clipped
        bb.flat.copy_(ba.flat * torch.tensor(rec[7], dtype=torch.float32, device=dev))
        ob.step()
        _same(_opt_state(a, oa), _opt_state(b, ob), ("step", k))
    assert clipped >= 1                                                # the first step is, by construction
    assert oa.guard_stats(reset=True).tolist() == rec and oa.guard_stats().tolist() == [0.0] * 8


def test_nonfinite_step_is_skipped_and_t_counts_calls(dev):
    """(d) a NaN in the bucket, skip on: parameters and both moment arrays bit-unchanged, record[1] = 1; the following finite steps
    equal an unguarded optimizer whose step count was advanced by the skipped call."""
    xs = _inputs(dev)
    a, b, ba, bb, oa, ob = _pair(dev, skip_nonfinite=True)
    for k, x in enumerate(xs):
        _gradient(a, ba, x)
        if k == 2:
            ba.flat[1500] = math.nan
            before = {n: t.clone() for n, t in _opt_state(a, oa).items()}
            oa.step()
            _same(before, _opt_state(a, oa), "skipped step")
            rec = oa.guard_stats().tolist()
            assert rec[0] == 3 and rec[1] == 1 and math.isnan(rec[5]) and math.isnan(rec[6]) and rec[7] == 1.0
            ob.steps += 1                                              # t counts calls
            continue
        bb.flat.copy_(ba.flat)
        oa.step(); ob.step()
        _same(_opt_state(a, oa), _opt_state(b, ob), ("step", k))
    rec = oa.guard_stats().tolist()
    assert oa.steps == ob.steps == 5 and rec[0] == 5 and rec[1] == 1 and math.isfinite(rec[3]) and math.isfinite(rec[6])


@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_nonfinite_step_without_skip_is_the_unguarded_step(bad, dev):
    """(e) skip off, max_grad_norm = 1: a non-finite norm means 'guard off' -- scale 1, the unguarded update, NaNs included."""
    a, b, ba, bb, oa, ob = _pair(dev, max_grad_norm=1.0)
    _gradient(a, ba, _inputs(dev, 1)[0])
    ba.flat[7] = bad
    bb.flat.copy_(ba.flat)
    oa.step(); ob.step()
    got, want = _opt_state(a, oa), _opt_state(b, ob)
    _same_but_nan(got, want, "unskipped")
    assert int(torch.isnan(oa.exp_avg).sum()) == (1 if math.isnan(bad) else 0) and not torch.isfinite(oa.exp_avg).all()
    rec = oa.guard_stats().tolist()
    assert rec[:3] == [1, 1, 0] and rec[3] == 0 and rec[7] == 1.0


def test_guard_record_survives_a_checkpoint(dev, tmp_path):
    """(f) state_dict / load_state_dict keep the record; a checkpoint without 'guard' loads (record zeroed); an unguarded optimizer's
    state has no 'guard' and ignores one."""
    a, b, ba, bb, oa, ob = _pair(dev, max_grad_norm=1e-3, skip_nonfinite=True)
    for x in _inputs(dev, 2):
        _gradient(a, ba, x)
        oa.step()
    path = str(tmp_path / "opt.pt")
    torch.save(oa.state_dict(), path)
    sd = torch.load(path)
    assert set(sd["flat"]) == {"exp_avg", "exp_avg_sq", "steps", "guard"} and set(ob.state_dict()["flat"]) == {"exp_avg", "exp_avg_sq", "steps"}
    fresh = dp.FlatAdam(ba, lr=1e-3, weight_decay=1e-4, max_grad_norm=1e-3, skip_nonfinite=True)
    fresh.load_state_dict(copy.deepcopy(sd))
    assert fresh.steps == 2 and fresh.guard_stats().tolist() == oa.guard_stats().tolist() and fresh.guard_stats().tolist()[2] == 2
    _same({"m": fresh.exp_avg, "v": fresh.exp_avg_sq}, {"m": oa.exp_avg, "v": oa.exp_avg_sq}, "moments")
    old = copy.deepcopy(sd)
    del old["flat"]["guard"]
    fresh.load_state_dict(old)
    assert fresh.steps == 2 and fresh.guard_stats().tolist() == [0.0] * 8
    ob.load_state_dict(copy.deepcopy(sd))                              # guard off: the record is not this optimizer's business
    assert ob.steps == 2 and not hasattr(ob, "record")
    with pytest.raises(RuntimeError):
        ob.guard_stats()


# ---- 4. torch as an independent reference ----------------------------------------------------------------------------------------------
def test_clipped_adam_matches_torch_clip_grad_norm_and_adam(dev):
    """clip_grad_norm_(params, c) + torch.optim.Adam (lr 1e-3, weight decay 1e-4), 5 steps, within the bound of
    test_flat_adam_matches_torch_adam (rtol 2e-6, atol 2e-7).  Adam's update is invariant to a common scale of g up to eps, so the
    one extra rounding of the scale (torch takes its norm in fp32) does not widen the bound."""
    xs = _inputs(dev)
    a, b = G.small_module(dev), G.small_module(dev)
    b.load_state_dict(a.state_dict())
    bucket = dp.FlatGradBucket(a)
    _gradient(a, bucket, xs[0])
    c = 0.5 * float(dp.grad_norm(bucket))
    oa = dp.FlatAdam(bucket, lr=1e-3, weight_decay=1e-4, max_grad_norm=c)
    ob = torch.optim.Adam(b.parameters(), lr=1e-3, weight_decay=1e-4)
    for k, x in enumerate(xs):
        _gradient(a, bucket, x)
        oa.step()
        ob.zero_grad()
        b(x).square().mean().backward()
        torch.nn.utils.clip_grad_norm_(b.parameters(), c)
        ob.step()
        for (name, p), q in zip(a.named_parameters(), b.parameters()):
            np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=2e-6, atol=2e-7, err_msg="%s step %d" % (name, k))
    assert oa.guard_stats().tolist()[2] >= 1


# ---- 5. on the model ------------------------------------------------------------------------------------------------------------------
def _cmflow(dev):
    import ragged_train_case as TC
    from cmflow_amd.cmflow import CMFlow
    net = CMFlow(TC.Args())
    net.load_state_dict(TC.weights())
    return net.to(dev)


def _run_state(step):
    d = {k: v.detach() for k, v in step.net.state_dict().items()}                # parameters and BatchNorm buffers
    d.update(exp_avg=step.opt.exp_avg, exp_avg_sq=step.opt.exp_avg_sq)
    return d


def _trained_state(step):
    d = {k: p.detach().clone() for k, p in step.net.named_parameters()}
    d.update(exp_avg=step.opt.exp_avg.clone(), exp_avg_sq=step.opt.exp_avg_sq.clone())
    return d


def _plant_nan(step):
    """The fused loss takes a gradient term only where its residual is > 0 (csrc/loss.hip), so a NaN LABEL makes the loss item NaN and
    drops out of the analytic gradient: no label reaches the bucket as a NaN.  The non-finite gradient is therefore planted where the
    SVD backward would leave one -- in the bucket, behind the all-reduce and in front of opt.step(), inside the step's own call."""
    reduce = step.bucket.all_reduce_mean

    def reduce_then_plant(*args, **kw):
        reduce(*args, **kw)
        step.bucket.flat[12345] = math.nan
    step.bucket.all_reduce_mean = reduce_then_plant


def test_guarded_train_step_on_cmflow(dev):
    """B = 2, N = 256, train-mode BatchNorm.  A guard that never acts (max_grad_norm 1e9, skip on) against the plain TrainStep: after 2
    steps parameters, moments and BN buffers are bit-identical.  Then a step with flow_label[0, 0, 0] = NaN and one NaN gradient element
    (see _plant_nan: measured on an MI355X, the NaN label alone leaves the gradient finite, norm 699.78 before and a finite norm with it):
    the guarded step leaves parameters and moments bit-unchanged and counts one non-finite call; the plain step's moments hold NaN."""
    from cmflow_amd import synth
    batch = {k: v.to(dev) for k, v in synth.make_batch(2, seed=3, train_extras=True).items()}
    guarded, plain = TrainStep(_cmflow(dev).train(), max_grad_norm=1e9, skip_nonfinite=True), TrainStep(_cmflow(dev).train())
    for k in range(2):
        la, lb = guarded(batch)[0], plain(batch)[0]
        assert torch.isfinite(la) and torch.equal(la, lb), k
        _same(_run_state(guarded), _run_state(plain), ("step", k))
    rec = guarded.opt.guard_stats().tolist()
    print("CMFlow B = 2: record", rec)
    assert rec[:3] == [2, 0, 0] and rec[7] == 1.0 and 0 < rec[6] <= rec[4] < 1e9
    bad = dict(batch, flow_label=batch["flow_label"].clone())
    bad["flow_label"][0, 0, 0] = math.nan
    before = _trained_state(guarded)
    _plant_nan(guarded); _plant_nan(plain)
    guarded(bad)
    plain(bad)
    _same(before, _trained_state(guarded), "skipped step")
    rec = guarded.opt.guard_stats().tolist()
    assert rec[0] == 3 and rec[1] == 1 and not math.isfinite(rec[5])
    assert torch.isnan(plain.opt.exp_avg).any() and torch.isnan(plain.opt.exp_avg_sq).any()
    assert guarded.opt.steps == plain.opt.steps == 3


def test_guarded_step_ragged_on_cmflow(dev):
    """The same through step_ragged on whole frames of 256 and 33 points (eval-mode BatchNorm): a clean step trains and counts a finite
    norm, the step with the NaN label and the planted NaN gradient is skipped; the plain step's moments hold NaN."""
    pb = {k: v.to(dev) for k, v in G.ragged_batch().items()}
    guarded, plain = TrainStep(_cmflow(dev).eval(), skip_nonfinite=True), TrainStep(_cmflow(dev).eval())
    start = _trained_state(guarded)
    loss = guarded.step_ragged(pb)[0]
    rec = guarded.opt.guard_stats().tolist()
    print("CMFlow ragged (256, 33): loss %.6g, record %s" % (float(loss), rec))
    assert torch.isfinite(loss) and rec[:3] == [1, 0, 0] and math.isfinite(rec[6]) and rec[6] > 0
    before = _trained_state(guarded)
    assert any(not torch.equal(before[k], start[k]) for k in before)            # it trained
    bad = dict(pb, flow_label=pb["flow_label"].clone())
    bad["flow_label"][0, 0, 0] = math.nan
    _plant_nan(guarded); _plant_nan(plain)
    guarded.step_ragged(bad)
    _same(before, _trained_state(guarded), "skipped ragged step")
    rec = guarded.opt.guard_stats().tolist()
    assert rec[0] == 2 and rec[1] == 1 and not math.isfinite(rec[5])
    plain.step_ragged(bad)
    assert torch.isnan(plain.opt.exp_avg).any() and torch.isnan(plain.opt.exp_avg_sq).any()


# ---- 6. fit ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def splits(dev):
    return R.train_split_of(dev), R.val_split_of(dev)


def _fit(splits, epochs, **kw):
    return T.fit(R.model("cmflow", dev=splits[0].device), splits[0], splits[1], epochs=epochs, batch_size=R.BATCH,
                 val_batch_size=R.VAL_BATCH, num_points=R.NPOINTS, seed=R.SEED, mini_clip_len=R.MINI_CLIP_LEN, **kw)


def _same_numbers(a, b, what):
    assert len(a) == len(b) and np.array_equal(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), equal_nan=True), (what, a, b)


def _same_guarded_history(a, b, what):
    assert set(a) == G.HISTORY_KEYS | set(G.GUARD_KEYS) and set(b) == set(a), what
    for k in ("train_loss", "val_score", "lr") + G.GUARD_KEYS:
        _same_numbers(a[k], b[k], (what, k))
    for e, (x, y) in enumerate(zip(a["loss_items"], b["loss_items"])):
        assert list(x) == list(y)
        _same_numbers(list(x.values()), list(y.values()), (what, "loss_items", e))
    _same_numbers([a["best"]], [b["best"]], (what, "best"))


def test_guarded_fit_reports_and_resumes_exactly(splits, tmp_path):
    """The splits and sizes of tests/test_gpu_run.py::test_resume_is_exact, two epochs.  The typical norm is read from a first
    guarded epoch (skip only); the run then clips at half of it."""
    probe = _fit(splits, 1, skip_nonfinite=True)
    assert set(probe) == G.HISTORY_KEYS | set(G.GUARD_KEYS) and probe["clipped_steps"] == [0] and probe["skipped_steps"] == [0]
    typical = probe["grad_norm_mean"][0]
    assert math.isfinite(typical) and 0 < typical <= probe["grad_norm_max"][0]
    c = 0.5 * typical
    whole, first, second = (str(tmp_path / d) for d in ("whole", "first", "second"))
    records = []
    want = _fit(splits, 2, max_grad_norm=c, out_dir=whole, on_epoch=lambda e, r: records.append(r))
    print("guarded fit at max_grad_norm %.6g (typical norm %.6g):" % (c, typical), {k: want[k] for k in G.GUARD_KEYS})
    assert all(len(want[k]) == 2 for k in G.GUARD_KEYS + ("train_loss", "val_score"))
    assert sum(want["clipped_steps"]) > 0 and want["skipped_steps"] == [0, 0]
    assert all(0 <= n <= 2 for n in want["clipped_steps"])                       # 10 frames at batch 4: two steps an epoch
    assert all(math.isfinite(v) and v > 0 for v in want["grad_norm_mean"] + want["grad_norm_max"])
    assert all(m <= x for m, x in zip(want["grad_norm_mean"], want["grad_norm_max"]))
    assert [[r[k] for k in G.GUARD_KEYS] for r in records] == [[want[k][e] for k in G.GUARD_KEYS] for e in range(2)]
    head = _fit(splits, 1, max_grad_norm=c, out_dir=first)
    point = os.path.join(first, "last.pt")
    stored = torch.load(point)
    assert stored["settings"]["max_grad_norm"] == c and stored["settings"]["skip_nonfinite"] is False
    assert set(stored["settings"]) == G.SETTINGS_KEYS | {"max_grad_norm", "skip_nonfinite"}
    assert set(stored["optimizer"]["flat"]) == {"exp_avg", "exp_avg_sq", "steps", "guard"}
    _same_numbers(head["grad_norm_mean"], want["grad_norm_mean"][:1], "first epoch")
    for other in (dict(max_grad_norm=2 * c), dict(), dict(max_grad_norm=c, skip_nonfinite=True)):      # another guard, or none
        with pytest.raises(ValueError):
            _fit(splits, 2, resume=point, **other)
    got = _fit(splits, 2, max_grad_norm=c, out_dir=second, resume=point)
    _same_guarded_history(got, want, "resumed")
    a, b = torch.load(os.path.join(whole, "last.pt")), torch.load(os.path.join(second, "last.pt"))
    assert a["epoch"] == b["epoch"] == 2 and a["settings"] == b["settings"] and a["training"] == b["training"]
    _same(a["model"], b["model"], "parameters and buffers")
    fa, fb = a["optimizer"]["flat"], b["optimizer"]["flat"]
    assert fa["steps"] == fb["steps"] == 4
    _same({k: fa[k] for k in ("exp_avg", "exp_avg_sq", "guard")}, {k: fb[k] for k in ("exp_avg", "exp_avg_sq", "guard")}, "Adam moments and record")
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"] and a["scheduler"] == b["scheduler"]
    _same_guarded_history(a["history"], b["history"], "last.pt")


def test_unguarded_fit_keeps_its_format_and_refuses_a_guarded_resume(splits, tmp_path):
    """Guard off: history, the on_epoch record and last.pt have the keys they had before the guard existed (settings included), and a
    guarded run does not resume from it."""
    records = []
    out = str(tmp_path / "plain")
    history = _fit(splits, 1, out_dir=out, on_epoch=lambda e, r: records.append(r))
    assert set(history) == G.HISTORY_KEYS
    assert set(records[0]) == {"lr", "train_loss", "loss_items", "val_score", "best", "is_best"}
    last = torch.load(os.path.join(out, "last.pt"))
    assert set(last) == G.LAST_PT_KEYS and set(last["settings"]) == G.SETTINGS_KEYS and set(last["history"]) == G.HISTORY_KEYS
    assert set(last["optimizer"]) == {"state", "param_groups", "flat"} and set(last["optimizer"]["flat"]) == {"exp_avg", "exp_avg_sq", "steps"}
    with pytest.raises(ValueError):
        _fit(splits, 2, resume=os.path.join(out, "last.pt"), skip_nonfinite=True)
