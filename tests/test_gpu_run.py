"""GPU: whole training runs from device-resident splits -- ``evaluate.eval_epoch`` / ``eval_epoch_clips``, ``train.train_epoch`` /
``train_epoch_clips`` and ``train.fit`` (with resume and two ranks) against the same loops WRITTEN OUT here from pieces that exist
without them and are pinned to the reference by the other suites: ``DeviceSplit.draw`` / ``epoch`` / ``epoch_clips``, ``TrainStep``,
``net.forward``, ``eval_util.eval_batch``, StepLR.  A training step is bit-reproducible (tests/test_gpu_stress.py), so the
comparisons are bit for bit; only a float64 sum taken in another order (the ranks' parts of a validation) gets rtol 1e-12, the
bound tests/test_gpu_ragged.py uses for the same thing.  The shapes (tests/run_dp_worker.py): 10 training frames at batch 4
(drop_last drops two), 7 validation frames at batch 3 (a short last batch), 256 points, 3 epochs; CMFlow-T on clips of 7 and 5
frames, L = 2.  Every test fails on the parent commit: the names do not exist there."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import run_dp_worker as R
from cmflow_amd import eval_util as E
from cmflow_amd import evaluate as EV
from cmflow_amd import train as T
from cmflow_amd.train import TrainStep

pytestmark = pytest.mark.gpu
SEED, NP, B, VB, L = R.SEED, R.NPOINTS, R.BATCH, R.VAL_BATCH, R.MINI_CLIP_LEN
METRICS = E.SF_KEYS + E.SEG_KEYS + E.POSE_KEYS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def train_split(dev):
    return R.train_split_of(dev)


@pytest.fixture(scope="module")
def val_split(dev):
    return R.val_split_of(dev)


@pytest.fixture(scope="module")
def clip_split(dev):
    return R.clip_split_of(dev)


class no_host_waits:
    """Every wait of the host for the device is an error inside (torch's synchronisation check), the mode restored on the way out."""

    def __enter__(self):
        torch.cuda.synchronize()
        self.mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        return False


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_state(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k].to(a[k].device))), (what, k)


def _same_numbers(a, b, what):
    """Two lists of floats, equal as numbers and NaN in the same places."""
    assert len(a) == len(b) and np.array_equal(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), equal_nan=True), (what, a, b)


def _same_history(a, b, what):
    assert set(a) == {"train_loss", "loss_items", "val_score", "lr", "best"} and set(b) == set(a), what
    for k in ("train_loss", "val_score", "lr"):
        _same_numbers(a[k], b[k], (what, k))
    assert len(a["loss_items"]) == len(b["loss_items"])
    for e, (x, y) in enumerate(zip(a["loss_items"], b["loss_items"])):
        assert list(x) == list(y)
        _same_numbers(list(x.values()), list(y.values()), (what, "loss_items", e))
    _same_numbers([a["best"]], [b["best"]], (what, "best"))


# ---- the loops, written out ---------------------------------------------------------------------------------------------------------
def hand_eval(net, split, batch_size, seed, epoch, recurrent=False, starts=None):
    """eval_one_epoch (main_util.py:93-206) / eval_one_epoch_seq (clip_util.py:99-178) on frames drawn in order: per batch the dense
    forward and one eval_batch, B * metric summed as Python floats (float64), divided by the number of frames evaluated."""
    net.eval()
    raflow = hasattr(net, "fd_layer")
    F = len(split)
    sums, count = np.zeros(len(METRICS)), 0
    gt_all, pre_all = torch.zeros(F, 4, 4, device=split.device), torch.zeros(F, 4, 4, device=split.device)
    ids = starts if recurrent else list(range(F))
    nb = -(-len(ids) // batch_size)
    with torch.no_grad():
        for b in range(nb):
            own = ids[b * batch_size:(b + 1) * batch_size]
            gfeat = None
            for j in range(L if recurrent else 1):
                frames = [f + j for f in own]
                batch = split.draw(frames, NP, seed, (epoch * nb + b) * L + j if recurrent else epoch * nb + b)
                pc1, pc2, ft1, ft2 = (batch[k] for k in ("pc1", "pc2", "ft1", "ft2"))
                if recurrent:
                    pred_f, _, pred_t, pred_m, gfeat = net(pc1, pc2, ft1, ft2, None, 'test', gfeat)
                elif raflow:
                    _, pred_f, pred_t, pred_m = net(pc1, pc2, ft1, ft2, batch["interval"])
                else:
                    pred_f, _, pred_t, pred_m = net(pc1, pc2, ft1, ft2, None, 'test')
                groups = E.eval_batch(pc1, pred_f.transpose(2, 1).contiguous(), batch["flow_label"], batch["fg_mask"], pred_m,
                                      batch["gt_trans"], pred_t)
                sums = sums + len(frames) * np.array([v.item() for d in groups for v in d.values()])
                gt_all[frames], pre_all[frames] = batch["gt_trans"], pred_t
                count += len(frames)
    return sums / count, gt_all, pre_all


def hand_train_epoch(step, split, epoch):
    """train_one_epoch (main_util.py:39-90): loss.item() on every step, np.mean of the items' lists."""
    total, examples, lists = 0.0, 0, {}
    for batch in split.epoch(B, NP, SEED, epoch):
        loss, items = step(batch)[:2]
        size = batch["pc1"].size(0)
        examples += size
        total += loss.item() * size
        for k, v in items.items():
            lists.setdefault(k, []).append(v.item())
    return total * 1.0 / examples, {k: float(np.mean(np.array(v))) for k, v in lists.items()}


def hand_train_epoch_clips(step, split, epoch):
    """train_one_epoch_seq (clip_util.py:20-78); a step is weighted by its number of mini-clips."""
    total, examples, lists = 0.0, 0, {}
    step.net.train()
    for clip in split.epoch_clips(B, L, NP, SEED, epoch):
        step.reset_clip()
        iter_loss, iter_items = 0, {}
        for batch in clip:
            loss, items = step(batch)[:2]
            iter_loss += loss
            for k, v in items.items():
                iter_items.setdefault(k, []).append(v.item())
        iter_loss = iter_loss / L
        size = clip[-1]["pc1"].size(0)
        examples += size
        total += iter_loss.item() * size
        for k, v in iter_items.items():
            lists.setdefault(k, []).append(np.mean(np.array(v)))
    return total / examples, {k: float(np.mean(np.array(v))) for k, v in lists.items()}


def hand_fit(net, train_split, val_split, epochs, recurrent=False, val_batch=VB, starts=None):
    """train() (main.py:104-170) -> (history, the network's state after every epoch, the TrainStep)."""
    step = TrainStep(net, vr_thres=0.3, lr=1e-3)
    scheduler = torch.optim.lr_scheduler.StepLR(step.opt, 1, gamma=0.9)
    history = {"train_loss": [], "loss_items": [], "val_score": [], "lr": [], "best": np.inf}
    states = []
    for epoch in range(epochs):
        history["lr"].append(step.opt.param_groups[0]["lr"])
        total, items = (hand_train_epoch_clips if recurrent else hand_train_epoch)(step, train_split, epoch)
        score = float(hand_eval(net, val_split, val_batch, SEED + 1, epoch, recurrent, starts)[0][0])
        history["train_loss"].append(total)
        history["loss_items"].append(items)
        history["val_score"].append(score)
        if history["best"] >= score:
            history["best"] = score
        scheduler.step()
        states.append(R.state_of(net))
    return history, states, step


def _numbers(result):
    return np.array([v.item() for d in result[:3] for v in d.values()])


def _assert_epoch_result(got, want, what):
    numbers, gt_all, pre_all = want
    assert [k for d in got[:3] for k in d] == list(METRICS)
    assert all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for d in got[:3] for v in d.values())
    have = _numbers(got)
    print(what, "driver", have.tolist(), "written out", numbers.tolist())
    assert np.array_equal(np.isnan(have), np.isnan(numbers)), what
    ok = ~np.isnan(numbers)
    assert ok[0] and ok.sum() >= 10, what                                             # the score and most of the rest are numbers
    assert np.all(np.abs(have[ok] - numbers[ok]) <= 1e-12 * np.abs(numbers[ok])), what
    assert torch.equal(_bits(got[3]), _bits(gt_all)) and torch.equal(_bits(got[4]), _bits(pre_all)), what


# ---- 1. validation epochs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cmflow", "raflow"])
def test_eval_epoch_is_the_written_out_loop(name, val_split, dev):
    net = R.model(name, dev)
    want = hand_eval(net, val_split, VB, SEED + 1, 2)
    assert float(want[2].abs().sum(dim=(1, 2)).min()) > 0                             # every frame was written
    net.train()
    seen = []
    with no_host_waits():
        got = EV.eval_epoch(net, val_split, VB, NP, SEED + 1, epoch=2, on_batch=lambda b, o: seen.append(b["frames"]))
    assert not net.training                                                            # net.eval(), not restored
    assert [f.tolist() for f in seen] == [[0, 1, 2], [3, 4, 5], [6]]                   # in order, the short last batch kept
    _assert_epoch_result(got, want, "eval_epoch " + name)
    other = _numbers(EV.eval_epoch(net, val_split, VB, NP, SEED + 1, epoch=1))
    assert other[0] != _numbers(got)[0]                                                # the epoch keys the draws


def test_sweep_resampled_ranks_are_the_rows_of_the_global_batches(val_split):
    """Two ranks of 2 frames: the ranks' batches concatenated are, bit for bit, the batches of one process at 4 frames (the last
    global batch holds 3: rank 1 gets one of them).  Two ranks of 3 frames: the last global batch holds one frame and rank 1
    yields nothing for it."""
    single = list(val_split.sweep_resampled(4, NP, SEED, 5))
    ranks = [list(val_split.sweep_resampled(2, NP, SEED, 5, rank=r, world=2)) for r in range(2)]
    assert [b["frames"].tolist() for b in single] == [[0, 1, 2, 3], [4, 5, 6]]
    assert [[b["frames"].tolist() for b in steps] for steps in ranks] == [[[0, 1], [4, 5]], [[2, 3], [6]]]
    for t, want in enumerate(single):
        for k in want:
            assert torch.equal(_bits(torch.cat([steps[t][k] for steps in ranks])), _bits(want[k])), (t, k)
    by_hand = val_split.draw([4, 5, 6], NP, SEED, 5 * 2 + 1)
    assert all(torch.equal(_bits(single[1][k]), _bits(by_hand[k])) for k in by_hand)
    three = [list(val_split.sweep_resampled(3, NP, SEED, 0, rank=r, world=2)) for r in range(2)]      # 7 = 6 + 1: an empty share
    assert [[b["frames"].tolist() for b in steps] for steps in three] == [[[0, 1, 2], [6]], [[3, 4, 5]]]


def test_eval_epoch_clips_is_the_written_out_loop(val_split, dev):
    from cmflow_amd.dataset import mini_clip_starts
    net = R.model("cmflow_t", dev)
    starts = mini_clip_starts(val_split.clips, L)
    assert starts == [0, 3, 5]
    want = hand_eval(net, val_split, R.CLIP_VAL_BATCH, SEED + 1, 1, True, starts)
    assert [i for i in range(7) if float(want[2][i].abs().sum()) == 0] == [2]         # the remainder of clip 0 is not visited
    net.train()
    forward, states, frames = net.forward, [], []

    def spy(pc1, pc2, ft1, ft2, label_m, mode, gfeat):
        out = forward(pc1, pc2, ft1, ft2, label_m, mode, gfeat)
        states.append((gfeat, out[4]))
        return out

    net.forward = spy
    try:
        with no_host_waits():
            got = EV.eval_epoch_clips(net, val_split, R.CLIP_VAL_BATCH, L, NP, SEED + 1, epoch=1,
                                      on_batch=lambda b, o: frames.append(b["frames"]))
    finally:
        del net.forward
    assert not net.training
    assert [f.tolist() for f in frames] == [[0, 3], [1, 4], [5], [6]]                  # steps of 2 and 1 mini-clips, L = 2 frames each
    assert len(states) == 4
    for t, (given, returned) in enumerate(states):
        if t % L == 0:
            assert given is None, t                                                    # frame 0 of every step
        else:
            assert given is states[t - 1][1], t                                        # the state the previous frame returned
    _assert_epoch_result(got, want, "eval_epoch_clips")


# ---- 2. training epochs -------------------------------------------------------------------------------------------------------------
def _moments(step):
    return {"exp_avg": step.opt.exp_avg, "exp_avg_sq": step.opt.exp_avg_sq}


def _assert_epoch_statistics(got, want, what):
    total, items = got
    assert total.dtype == torch.float64 and total.dim() == 0 and total.is_cuda
    assert all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in items.values())
    print(what, "driver", total.item(), {k: v.item() for k, v in items.items()}, "written out", want)
    assert math.isfinite(want[0]) and total.item() == want[0], what
    assert list(items) == list(want[1])
    _same_numbers([v.item() for v in items.values()], list(want[1].values()), what)


@pytest.mark.parametrize("name,training", [("cmflow", True), ("cmflow", False), ("raflow", True)])
def test_train_epoch_is_the_written_out_loop(name, training, train_split, dev):
    a, b = R.model(name, dev).train(training), R.model(name, dev).train(training)
    hand, step = TrainStep(a, vr_thres=0.3), TrainStep(b, vr_thres=0.3)
    want = [hand_train_epoch(hand, train_split, e) for e in (0, 1)]
    assert hand.opt.steps == 4                                                         # 10 frames at batch 4: two steps an epoch
    got = [T.train_epoch(step, train_split, B, NP, SEED, 0)]                           # a network's first step builds its plans
    with no_host_waits():                                                              # ... the next epoch only enqueues
        got.append(T.train_epoch(step, train_split, B, NP, SEED, 1))
    assert b.training == training and all(m.training == training for m in b.modules())            # left as found, both ways
    for e in (0, 1):
        _assert_epoch_statistics(got[e], want[e], "train_epoch %s epoch %d" % (name, e))
    assert step.opt.steps == 4
    _same_state(R.state_of(a), R.state_of(b), "parameters and buffers")
    _same_state(_moments(hand), _moments(step), "Adam moments")
    fresh = R.state_of(R.model(name, dev))
    assert any(not torch.equal(v, fresh[k]) for k, v in R.state_of(b).items())         # ... and it trained


def test_train_epoch_clips_is_the_written_out_loop(clip_split, dev):
    a, b = R.model("cmflow_t", dev), R.model("cmflow_t", dev).eval()
    hand, step = TrainStep(a, vr_thres=0.3), TrainStep(b, vr_thres=0.3)
    want = [hand_train_epoch_clips(hand, clip_split, e) for e in (0, 1)]
    assert hand.opt.steps == 2 * 2 * L                                                 # 5 mini-clips at batch 4: steps of 4 and 1
    resets, reset_clip = [], step.reset_clip
    step.reset_clip = lambda: (resets.append(step.opt.steps), reset_clip())[1]
    got = [T.train_epoch_clips(step, clip_split, B, L, NP, SEED, 0)]                   # both step sizes, 4 and 1, build their plans
    with no_host_waits():
        got.append(T.train_epoch_clips(step, clip_split, B, L, NP, SEED, 1))
    assert b.training and all(m.training for m in b.modules())                          # net.train() at entry (clip_util.py:25)
    assert resets == [0, L, 2 * L, 3 * L]                                              # before frame 0 of every step
    for e in (0, 1):
        _assert_epoch_statistics(got[e], want[e], "train_epoch_clips epoch %d" % e)
    _same_state(R.state_of(a), R.state_of(b), "parameters and buffers")
    _same_state(_moments(hand), _moments(step), "Adam moments")


# ---- 3. fit -------------------------------------------------------------------------------------------------------------------------
def _fit(net, train_split, val_split, epochs, **kw):
    kw.setdefault("val_batch_size", VB)
    return T.fit(net, train_split, val_split, epochs=epochs, batch_size=B, num_points=NP, seed=SEED, mini_clip_len=L, **kw)


def _mode_spy(net, modes, epoch_of):
    """A forward pre-hook: the mode of every forward that records a graph (the training forwards), with the epoch it ran in."""
    return net.register_forward_pre_hook(lambda m, a: modes.append((epoch_of(), bool(m.training))) if torch.is_grad_enabled() else None)


def test_fit_is_the_references_train(train_split, val_split, dev, tmp_path):
    want, want_states, _ = hand_fit(R.model("cmflow", dev), train_split, val_split, R.EPOCHS)
    net = R.model("cmflow", dev)
    states, records, modes = [], [], []
    _mode_spy(net, modes, lambda: len(states))

    def on_epoch(epoch, record):
        assert epoch == len(states)
        states.append(R.state_of(net))
        records.append(record)

    out = str(tmp_path / "run")
    got = _fit(net, train_split, val_split, R.EPOCHS, out_dir=out, on_epoch=on_epoch)
    print("fit", got, "written out", want)
    _same_history(got, want, "fit")
    assert len(states) == R.EPOCHS
    for e in range(R.EPOCHS):
        _same_state(states[e], want_states[e], "after epoch %d" % e)
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(ref, 1, gamma=0.9)
    for e in range(R.EPOCHS):
        assert got["lr"][e] == ref.param_groups[0]["lr"], e
        ref.step()
        sched.step()
    assert got["lr"][0] == 1e-3 and got["lr"][2] < got["lr"][1] < got["lr"][0]
    # train-mode BatchNorm in epoch 0, eval-mode from epoch 1 on: the first validation's net.eval() sticks
    assert modes == [(0, True)] * 2 + [(1, False)] * 2 + [(2, False)] * 2
    assert not net.training
    assert all(math.isfinite(v) for v in got["val_score"]) and got["best"] == min(got["val_score"])
    assert [r["is_best"] for r in records] == [s <= min(got["val_score"][:e + 1]) for e, s in enumerate(got["val_score"])]
    assert [r["val_score"] for r in records] == got["val_score"] and records[-1]["best"] == got["best"]
    # model.best.t7: the state dict alone, as the reference writes it; loaded into a fresh network it scores the best
    assert sorted(os.listdir(out)) == ["last.pt", "models"] and os.listdir(os.path.join(out, "models")) == ["model.best.t7"]
    best_epoch = max(e for e in range(R.EPOCHS) if got["val_score"][e] == got["best"])
    sd = torch.load(os.path.join(out, "models", "model.best.t7"))
    _same_state(states[best_epoch], sd, "model.best.t7")
    fresh = R.model("cmflow", dev)
    fresh.load_state_dict(sd)
    assert EV.eval_epoch(fresh, val_split, VB, NP, SEED + 1, epoch=best_epoch)[0]["rne"].item() == got["best"]
    last = torch.load(os.path.join(out, "last.pt"))
    assert last["epoch"] == R.EPOCHS and last["training"] is False
    _same_history(last["history"], got, "last.pt")


def test_fit_keeps_cmflow_t_in_train_mode(clip_split, val_split, dev):
    from cmflow_amd.dataset import mini_clip_starts
    starts = mini_clip_starts(val_split.clips, L)
    want, want_states, _ = hand_fit(R.model("cmflow_t", dev), clip_split, val_split, 2, True, R.CLIP_VAL_BATCH, starts)
    net = R.model("cmflow_t", dev)
    states, modes = [], []
    _mode_spy(net, modes, lambda: len(states))
    got = _fit(net, clip_split, val_split, 2, val_batch_size=R.CLIP_VAL_BATCH, on_epoch=lambda e, r: states.append(R.state_of(net)))
    print("fit cmflow_t", got, "written out", want)
    _same_history(got, want, "fit cmflow_t")
    for e in range(2):
        _same_state(states[e], want_states[e], "after epoch %d" % e)
    assert modes == [(0, True)] * 2 * L + [(1, True)] * 2 * L                          # train mode in every training epoch
    assert not net.training                                                            # ... and the validation's eval mode after it


# ---- 4. resume ----------------------------------------------------------------------------------------------------------------------
def test_resume_is_exact(train_split, val_split, dev, tmp_path):
    whole, first, second = (str(tmp_path / d) for d in ("whole", "first", "second"))
    want = _fit(R.model("cmflow", dev), train_split, val_split, R.EPOCHS, out_dir=whole)
    head = _fit(R.model("cmflow", dev), train_split, val_split, 1, out_dir=first)
    assert head["val_score"] == want["val_score"][:1]
    point = os.path.join(first, "last.pt")
    stored = torch.load(point)
    assert stored["epoch"] == 1 and stored["training"] is False                        # written after the validation: eval mode
    net = R.model("cmflow", dev)                                                       # fresh, in train mode
    modes, epochs = [], []
    _mode_spy(net, modes, lambda: 1 + len(epochs))
    with pytest.raises(ValueError):
        T.fit(net, train_split, val_split, epochs=R.EPOCHS, batch_size=B + 1, val_batch_size=VB, num_points=NP, seed=SEED,
              mini_clip_len=L, resume=point)
    assert net.training and not modes                                                  # refused before anything ran
    got = _fit(net, train_split, val_split, R.EPOCHS, out_dir=second, resume=point, on_epoch=lambda e, r: epochs.append(e))
    assert epochs == [1, 2]                                                            # continues at the stored epoch
    assert modes == [(1, False)] * 2 + [(2, False)] * 2                                # last.pt restored eval mode for CMFlow
    _same_history(got, want, "resumed")
    a, b = torch.load(os.path.join(whole, "last.pt")), torch.load(os.path.join(second, "last.pt"))
    assert a["epoch"] == b["epoch"] == R.EPOCHS and a["settings"] == b["settings"] and a["training"] == b["training"]
    _same_state(a["model"], b["model"], "parameters and buffers")
    _same_state(a["optimizer"]["flat"] | {"steps": torch.tensor(a["optimizer"]["flat"]["steps"])},
                b["optimizer"]["flat"] | {"steps": torch.tensor(b["optimizer"]["flat"]["steps"])}, "Adam moments")
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"] and a["scheduler"] == b["scheduler"]
    _same_history(a["history"], b["history"], "last.pt")
    best, where = math.inf, None                                                       # the run that wrote the best model last
    for e, score in enumerate(got["val_score"]):
        if best >= score:
            best, where = score, (first if e == 0 else second)
    assert best == got["best"] and where is not None
    _same_state(*(torch.load(os.path.join(d, "models", "model.best.t7")) for d in (whole, where)), "model.best.t7")


# ---- 5. two ranks on cuda:0 over gloo ------------------------------------------------------------------------------------------------
def test_two_rank_fit(val_split, dev, tmp_path):
    """fit at world = 2 (2 + 2 training frames and 2 + 2 validation frames per global batch): both ranks return the same history and
    end every epoch with the same parameters and (rank 0's, broadcast before the validation) BatchNorm buffers, only rank 0 writes, and every epoch's score is what a single process computes for
    that epoch's network at the global validation batch size -- the ranks' rows are the rows of its batches, and 'rne' is a mean
    over the points of a batch, so the two differ by the order of float64 sums only (rtol 1e-12)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "run_dp_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=dict(os.environ))
    assert out.returncode == 0, out.stderr[-3000:]
    ranks = [torch.load(os.path.join(tmp_path, "rank%d.pt" % r)) for r in range(2)]
    _same_history(ranks[0]["history"], ranks[1]["history"], "two ranks")
    history = ranks[0]["history"]
    assert len(history["val_score"]) == R.DP_EPOCHS and all(math.isfinite(v) for v in history["val_score"] + history["train_loss"])
    for e in range(R.DP_EPOCHS):
        _same_state(ranks[0]["states"][e], ranks[1]["states"][e], "epoch %d" % e)
    assert ranks[0]["modes"] == ranks[1]["modes"] == [True] * 2 + [False] * 2          # 10 frames, global batch 4: two steps an epoch
    assert sorted(os.listdir(os.path.join(tmp_path, "out0"))) == ["last.pt", "models"]
    assert not os.path.exists(os.path.join(tmp_path, "out1"))                          # only rank 0 writes
    net = R.model("cmflow", dev)
    for e in range(R.DP_EPOCHS):
        net.load_state_dict(ranks[0]["states"][e])
        single = EV.eval_epoch(net, val_split, 2 * R.DP_VAL_BATCH, NP, SEED + 1, epoch=e)[0]["rne"].item()
        print("epoch %d: two ranks %.17g, one process %.17g" % (e, history["val_score"][e], single))
        assert abs(history["val_score"][e] - single) <= 1e-12 * abs(single), e
