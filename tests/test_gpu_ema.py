"""GPU: averaged weights -- the exponential moving average of the parameters inside the flat Adam step (cmf_adam_step_ema /
cmf_adam_step_guarded_ema), the exchange that runs the module on it (cmf_param_exchange), through ``dp.FlatAdam``, ``TrainStep`` and
``train.fit``.

Parameters and moments are held bit for bit to the optimizer without the average; the average is held to its recurrence in float64
(tests/ema_ref.py) within a bound derived from the two roundings of the kernel's expression, not measured; everything that copies
(exchange, checkpoint, resume) is held bit for bit.  Every test fails on the parent commit: the symbols and the keyword are new."""
import copy
import math
import os
import statistics

import numpy as np
import pytest
import torch

import ema_ref as E
import grad_guard_ref as G
import run_dp_worker as R
from cmflow_amd import _lib, dp
from cmflow_amd import train as T
from cmflow_amd.train import TrainStep

pytestmark = pytest.mark.gpu
MODULES = ("odd", "small")


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


def _flat(bucket):
    """The bucket's parameters as one flat tensor in bucket order (a copy)."""
    return torch.cat([p.detach().reshape(-1) for p in bucket.params])


def _state(bucket, opt):
    d = {"p": _flat(bucket), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone()}
    if opt.ema_decay is not None:
        d["ema"] = opt.ema.clone()
    return d


def _make(name, dev, **kw):
    net = E.modules(dev)[name]
    bucket = dp.FlatGradBucket(net)
    return net, bucket, dp.FlatAdam(bucket, lr=1e-3, weight_decay=kw.pop("weight_decay", 1e-4), **kw)


def _grads(bucket, steps, seed, dev):
    return [g.to(dev) for g in E.gradients(bucket.numel, steps, seed)]


def test_buckets_straddle_chunks(dev):
    sizes = {name: dp.FlatGradBucket(net).numel for name, net in E.modules(dev).items()}
    assert sizes == {"odd": E.ODD_TOTAL, "small": 37 * 129 + 2 * 129 + 129 * 5 + 5}
    assert all(n % 4 != 0 and n % 1024 != 0 and n > 4096 for n in sizes.values())          # more than one workgroup, a ragged end


# ---- 1. parameters and moments are the plain step's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", ["plain", "clip", "skip"])
@pytest.mark.parametrize("name", MODULES)
def test_parameters_and_moments_are_those_of_the_step_without_the_average(name, guard, dev):
    """Two copies, the same 6 gradients, FlatAdam(ema_decay=None) against ema_decay=0.9: p, exp_avg, exp_avg_sq bit for bit after every
    step -- unguarded, clipping at the median norm of the 6 gradients (so that some steps clip and some do not), and skip only."""
    probe = dp.FlatGradBucket(E.modules(dev)[name])
    grads = _grads(probe, 6, 21, dev)
    kw = {}
    if guard == "clip":
        kw = dict(max_grad_norm=statistics.median(float(g.double().norm()) for g in grads))
    elif guard == "skip":
        kw = dict(skip_nonfinite=True)
    _, ba, oa = _make(name, dev, **kw)
    _, bb, ob = _make(name, dev, ema_decay=0.9, **kw)
    _same({"p": _flat(ba)}, {"p": _flat(bb)}, "start")
    for k, g in enumerate(grads):
        ba.flat.copy_(g); bb.flat.copy_(g)
        oa.step(); ob.step()
        got = _state(bb, ob)
        moved = not torch.equal(got.pop("ema"), got["p"])
        _same(_state(ba, oa), got, (name, guard, "step", k))
        assert moved                                                       # the average lags the parameters: it is not a copy of them
    if guard == "clip":
        rec = ob.guard_stats().tolist()
        assert rec[0] == 6 and 0 < rec[2] < 6 and rec == oa.guard_stats().tolist(), rec


# ---- 2. the average follows the recurrence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999])
@pytest.mark.parametrize("name", MODULES)
def test_average_follows_the_recurrence(name, decay, dev):
    """12 steps; the parameters are read back after every step and |ema - e_ref| <= b element-wise after every step, (e_ref, b) from
    ema_ref.ema_recurrence on the kernel's own parameter sequence."""
    _, bucket, opt = _make(name, dev, ema_decay=decay)
    e0 = _flat(bucket).cpu().numpy()
    assert np.array_equal(opt.ema.cpu().numpy().view(np.int32), e0.view(np.int32))          # initialised to the parameters
    p_seq, worst = [], 0.0
    for k, g in enumerate(_grads(bucket, 12, 33, dev)):
        bucket.flat.copy_(g)
        opt.step()
        p_seq.append(_flat(bucket).cpu().numpy())
        e_ref, b = E.ema_recurrence(p_seq, e0, decay)
        err = np.abs(opt.ema.cpu().numpy().astype(np.float64) - e_ref)
        ratio = float(np.max(err[b > 0] / b[b > 0])) if (b > 0).any() else 0.0
        worst = max(worst, ratio)
        assert (err <= b).all(), (name, decay, k, ratio, float(err.max()))
    print("%s, decay %g: worst |ema - e_ref| / b over 12 steps %.3f" % (name, decay, worst))
    assert not np.array_equal(p_seq[-1], p_seq[0]) and np.isfinite(e_ref).all()


# ---- 3. fixed point ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", [dict(), dict(max_grad_norm=1.0, skip_nonfinite=True)])
@pytest.mark.parametrize("name", MODULES)
def test_fixed_point(name, guard, dev):
    """Zero gradient, zero weight decay, fresh moments: the parameters do not move and ema stays bit-equal to them for 5 steps."""
    _, bucket, opt = _make(name, dev, weight_decay=0.0, ema_decay=0.9, **guard)
    start = _flat(bucket)
    for k in range(5):
        bucket.zero()
        opt.step()
        _same({"p": _flat(bucket), "ema": opt.ema}, {"p": start, "ema": start}, (name, "step", k))
    assert opt.steps == 5 and not opt.exp_avg.any() and not opt.exp_avg_sq.any()


# ---- 4. a skipped step touches nothing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODULES)
def test_skipped_step_touches_nothing(name, dev):
    _, bucket, opt = _make(name, dev, ema_decay=0.9, skip_nonfinite=True)
    grads = _grads(bucket, 3, 44, dev)
    for g in grads[:2]:
        bucket.flat.copy_(g)
        opt.step()
    before = _state(bucket, opt)
    assert not torch.equal(before["ema"], before["p"])
    bucket.flat.copy_(grads[2])
    bucket.flat[bucket.numel - 2] = math.nan
    opt.step()
    _same(before, _state(bucket, opt), (name, "skipped step"))
    rec = opt.guard_stats().tolist()
    assert opt.steps == 3 and rec[0] == 3 and rec[1] == 1


@pytest.mark.parametrize("guard", [dict(), dict(max_grad_norm=1.0)])
@pytest.mark.parametrize("name", MODULES)
def test_unskipped_nan_reaches_the_average_where_it_reaches_the_parameter(name, guard, dev):
    _, bucket, opt = _make(name, dev, ema_decay=0.9, **guard)
    grads = _grads(bucket, 2, 45, dev)
    bucket.flat.copy_(grads[0])
    opt.step()
    where = 1025
    bucket.flat.copy_(grads[1])
    bucket.flat[where] = math.nan
    opt.step()
    p, ema = _flat(bucket), opt.ema
    want = torch.zeros(bucket.numel, dtype=torch.bool, device=dev)
    want[where] = True
    assert torch.equal(torch.isnan(p), want) and torch.equal(torch.isnan(ema), want)
    assert torch.isfinite(ema[~want]).all()


# ---- 5. exchange ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODULES)
def test_param_exchange_swaps_and_swaps_back(name, dev):
    """cmf_param_exchange itself, on a flat array with NaN canaries on either side: the parameters hold the former flat, flat the former
    parameters; a second call restores both; bit for bit; nothing outside flat[0:total] is written.  total is not a multiple of 4."""
    _, bucket, opt = _make(name, dev)
    n = bucket.numel
    assert n % 4 != 0
    room = torch.full((n + 8,), math.nan, dtype=torch.float32, device=dev)
    flat = room[4:4 + n]
    flat.copy_(torch.randn(n, generator=torch.Generator().manual_seed(8)).to(dev))
    p0, f0 = _flat(bucket), flat.clone()

    def exchange():
        _lib.check(_lib.lib().cmf_param_exchange(len(bucket.params), opt._offs.data_ptr(), opt._pt.data_ptr(), n, flat.data_ptr(),
                                                 _lib.stream_ptr()), "cmf_param_exchange")
    exchange()
    _same({"p": _flat(bucket), "flat": flat}, {"p": f0, "flat": p0}, (name, "exchanged"))
    exchange()
    _same({"p": _flat(bucket), "flat": flat}, {"p": p0, "flat": f0}, (name, "back"))
    assert torch.isnan(room[:4]).all() and torch.isnan(room[4 + n:]).all()


@pytest.mark.parametrize("name", MODULES)
def test_ema_weights_context(name, dev):
    _, bucket, opt = _make(name, dev, ema_decay=0.9)
    for g in _grads(bucket, 3, 55, dev):
        bucket.flat.copy_(g)
        opt.step()
    live, avg = _flat(bucket), opt.ema.clone()
    assert not torch.equal(live, avg)
    versions = [p._version for p in bucket.params]
    with opt.ema_weights() as inside:
        assert inside is opt
        _same({"p": _flat(bucket), "ema": opt.ema}, {"p": avg, "ema": live}, (name, "inside"))
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.ema_state_dict(torch.nn.Module())
        _same({"p": _flat(bucket), "ema": opt.ema}, {"p": avg, "ema": live}, (name, "still inside"))      # the refusals changed nothing
    _same({"p": _flat(bucket), "ema": opt.ema}, {"p": live, "ema": avg}, (name, "after"))
    if hasattr(torch.autograd.graph, "increment_version"):
        assert [p._version for p in bucket.params] == [v + 2 for v in versions]                # both exchanges count as writes
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("the body raises")
    _same({"p": _flat(bucket), "ema": opt.ema}, {"p": live, "ema": avg}, (name, "after a raising body"))
    assert opt.steps == 3
    bucket.zero()
    opt.step()                                                             # ... and the optimizer steps again
    assert opt.steps == 4
    plain = _make(name, dev)[2]
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass


# ---- 6. checkpoint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODULES)
def test_checkpoint_and_state_dict(name, dev, tmp_path):
    net, bucket, opt = _make(name, dev, ema_decay=0.9)
    for g in _grads(bucket, 3, 66, dev):
        bucket.flat.copy_(g)
        opt.step()
    path = str(tmp_path / "opt.pt")
    torch.save(opt.state_dict(), path)
    sd = torch.load(path)
    assert set(sd["flat"]) == {"exp_avg", "exp_avg_sq", "steps", "ema"}
    fresh = dp.FlatAdam(bucket, lr=1e-3, weight_decay=1e-4, ema_decay=0.9)
    _same({"ema": fresh.ema}, {"ema": _flat(bucket)}, "a fresh optimizer starts from the parameters")
    fresh.load_state_dict(copy.deepcopy(sd))
    assert fresh.steps == 3
    _same(_state(bucket, fresh), _state(bucket, opt), (name, "restored"))
    old = copy.deepcopy(sd)
    del old["flat"]["ema"]
    fresh.ema.fill_(7.0)
    fresh.load_state_dict(old)                                             # averaging starts from the parameters as they are now
    _same({"ema": fresh.ema, "m": fresh.exp_avg}, {"ema": _flat(bucket), "m": opt.exp_avg}, (name, "no ema in the checkpoint"))
    off = dp.FlatAdam(bucket, lr=1e-3, weight_decay=1e-4)
    assert set(off.state_dict()["flat"]) == {"exp_avg", "exp_avg_sq", "steps"}
    off.load_state_dict(copy.deepcopy(sd))                                 # off: a stored average is ignored
    assert off.steps == 3 and not hasattr(off, "ema")
    with pytest.raises(RuntimeError, match="ema_decay"):
        off.ema_state_dict(net)
    # ema_state_dict: the module's state dict as it is inside ema_weights(), key by key; outside, nothing was touched
    live = {k: v.detach().clone() for k, v in net.state_dict().items()}
    averaged = opt.ema_state_dict(net)
    _same({k: v.detach() for k, v in net.state_dict().items()}, live, (name, "ema_state_dict touched the module"))
    store = opt.ema.untyped_storage().data_ptr()
    for k, p in net.named_parameters():                                    # clones: neither the parameter nor a view of opt.ema
        assert averaged[k].data_ptr() != p.data_ptr() and averaged[k].untyped_storage().data_ptr() != store, k
    with opt.ema_weights():
        inside = {k: v.detach().clone() for k, v in net.state_dict().items()}
    _same(averaged, inside, (name, "ema_state_dict"))
    assert any(not torch.equal(averaged[k], live[k]) for k in live)
    _same({k: v.detach() for k, v in net.state_dict().items()}, live, (name, "after the context"))


# ---- 7. on the model ------------------------------------------------------------------------------------------------------------------
def _cmflow(dev):
    import ragged_train_case as TC
    from cmflow_amd.cmflow import CMFlow
    net = CMFlow(TC.Args())
    net.load_state_dict(TC.weights())
    return net.to(dev)


def _forward(net, batch):
    with torch.no_grad():
        out = net(batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"], None, "test")
    return {str(i): o.clone() for i, o in enumerate(out) if torch.is_tensor(o)}


def test_train_step_and_averaged_forward_on_cmflow(dev):
    """B = 2, N = 64, train-mode BatchNorm, 3 steps: TrainStep(ema_decay=0.9) leaves the parameters, BN buffers and moments of the same
    3 steps without it, bit for bit.  Then in eval mode under no_grad: the forward inside ema_weights() equals, bit for bit, the
    forward of a second CMFlow into which ema_state_dict was loaded (a fresh network stands for the deep copy: the module's cached
    launch plans hold raw pointers and do not deep-copy) -- a weight cache that went stale behind the raw-pointer write would show
    here -- and after the context the live forward is the one taken before it."""
    from cmflow_amd import synth
    batch = {k: v.to(dev) for k, v in synth.make_batch(2, N=64, seed=3, train_extras=True).items()}
    averaged, plain = TrainStep(_cmflow(dev).train(), ema_decay=0.9), TrainStep(_cmflow(dev).train())
    for k in range(3):
        la, lb = averaged(batch)[0], plain(batch)[0]
        assert torch.isfinite(la) and torch.equal(la, lb), k
        _same({k_: v.detach() for k_, v in averaged.net.state_dict().items()}, {k_: v.detach() for k_, v in plain.net.state_dict().items()},
              ("step", k))
        _same({"m": averaged.opt.exp_avg, "v": averaged.opt.exp_avg_sq}, {"m": plain.opt.exp_avg, "v": plain.opt.exp_avg_sq}, ("step", k))
    net = averaged.net.eval()
    before = _forward(net, batch)                                          # also fills whatever the eval-mode forward caches
    twin = _cmflow(dev)
    twin.load_state_dict(averaged.opt.ema_state_dict(net))
    want = _forward(twin.eval(), batch)
    with averaged.opt.ema_weights():
        got = _forward(net, batch)
    _same(got, want, "forward on the averaged weights")
    assert any(not torch.equal(got[k], before[k]) for k in got)            # the averaged model is another model
    _same(_forward(net, batch), before, "live forward after the context")


# ---- 8. fit --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def splits(dev):
    return R.train_split_of(dev), R.val_split_of(dev)


def _fit(splits, epochs, **kw):
    return T.fit(R.model("cmflow", dev=splits[0].device), splits[0], splits[1], epochs=epochs, batch_size=R.BATCH, val_batch_size=R.VAL_BATCH, num_points=R.NPOINTS, seed=R.SEED, mini_clip_len=R.MINI_CLIP_LEN, **kw)


def _same_numbers(a, b, what):
    assert len(a) == len(b) and np.array_equal(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), equal_nan=True), (what, a, b)


def _same_history(a, b, what):
    assert set(a) == G.HISTORY_KEYS and set(b) == G.HISTORY_KEYS, what     # the average adds no key
    for k in ("train_loss", "val_score", "lr"):
        _same_numbers(a[k], b[k], (what, k))
    for e, (x, y) in enumerate(zip(a["loss_items"], b["loss_items"])):
        assert list(x) == list(y)
        _same_numbers(list(x.values()), list(y.values()), (what, "loss_items", e))
    _same_numbers([a["best"]], [b["best"]], (what, "best"))


def test_fit_scores_and_keeps_the_averaged_model_and_resumes_exactly(splits, tmp_path, monkeypatch):
    """The splits and sizes of tests/test_gpu_run.py::test_resume_is_exact, 3 epochs at ema_decay = 0.9."""
    made = []

    class Spy(T.TrainStep):                                                # fit's own TrainStep, so that on_epoch can reach its optimizer
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(T, "TrainStep", Spy)
    whole, first, second, plain = (str(tmp_path / d) for d in ("whole", "first", "second", "plain"))
    kept, records = {}, []

    def on_epoch(epoch, record):
        records.append(record)
        if record["is_best"]:
            step = made[-1]
            kept.update(epoch=epoch, averaged=step.opt.ema_state_dict(step.net), live=R.state_of(step.net))
    want = _fit(splits, 3, ema_decay=0.9, out_dir=whole, on_epoch=on_epoch)
    assert set(want) == G.HISTORY_KEYS and len(want["val_score"]) == 3 and all(math.isfinite(v) for v in want["val_score"])
    assert set(records[0]) == {"lr", "train_loss", "loss_items", "val_score", "best", "is_best"}
    assert kept and want["val_score"][kept["epoch"]] == want["best"]
    best = torch.load(os.path.join(whole, T.BEST_FILE))
    _same(best, kept["averaged"], "model.best.t7 is the averaged model")
    assert any(not torch.equal(best[k], kept["live"][k]) for k in best)    # ... and not the live one
    R.model("cmflow", splits[0].device).load_state_dict(best)              # the reference's file format: it loads, strictly
    last = torch.load(os.path.join(whole, "last.pt"))
    assert set(last) == G.LAST_PT_KEYS and set(last["settings"]) == G.SETTINGS_KEYS | {"ema_decay"} and last["settings"]["ema_decay"] == 0.9
    assert set(last["optimizer"]["flat"]) == {"exp_avg", "exp_avg_sq", "steps", "ema"} and last["optimizer"]["flat"]["steps"] == 6
    _same(last["model"], R.state_of(made[0].net), "last.pt stores the live model")
    _same({"ema": last["optimizer"]["flat"]["ema"]}, {"ema": made[0].opt.ema}, "last.pt stores the average")
    # training is what it is without the average; the score is another model's
    off = _fit(splits, 1, out_dir=plain)
    _same_numbers(off["train_loss"], want["train_loss"][:1], "training does not see the average")
    assert off["val_score"][0] != want["val_score"][0]
    # 2 epochs, then 1 more from the resume point
    head = _fit(splits, 2, ema_decay=0.9, out_dir=first)
    _same_numbers(head["val_score"], want["val_score"][:2], "first two epochs")
    point = os.path.join(first, "last.pt")
    with pytest.raises(ValueError):
        _fit(splits, 3, resume=point)                                      # the average off against a point with it
    with pytest.raises(ValueError):
        _fit(splits, 3, resume=point, ema_decay=0.99)                      # another decay
    with pytest.raises(ValueError):
        _fit(splits, 3, resume=os.path.join(plain, "last.pt"), ema_decay=0.9)      # a point without it counts as off
    got = _fit(splits, 3, ema_decay=0.9, out_dir=second, resume=point)
    _same_history(got, want, "resumed")
    a, b = last, torch.load(os.path.join(second, "last.pt"))
    assert a["epoch"] == b["epoch"] == 3 and a["settings"] == b["settings"] and a["training"] == b["training"]
    _same(a["model"], b["model"], "parameters and buffers")
    fa, fb = a["optimizer"]["flat"], b["optimizer"]["flat"]
    assert fa["steps"] == fb["steps"] == 6
    _same({k: fa[k] for k in ("exp_avg", "exp_avg_sq", "ema")}, {k: fb[k] for k in ("exp_avg", "exp_avg_sq", "ema")}, "Adam moments and average")
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"] and a["scheduler"] == b["scheduler"]
    _same_history(a["history"], b["history"], "last.pt")
