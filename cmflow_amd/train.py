"""The reference's training-step sequence (main_util.py:63-76 / clip_util.py:34-62) on device.

    labels -> net(..., mseg_gt, 'train') -> RadarFlowLoss -> zero_grad / backward / [all-reduce] / step

``TrainStep`` owns the optimizer (Adam lr 1e-3, weight decay 1e-4: main.py:107), the flat
gradient bucket and the loss module; ``__call__(batch)`` runs one optimizer step and returns
(loss, items) as device tensors.

Around the step, on a ``dataset.DeviceSplit``: ``train_epoch`` / ``train_epoch_clips`` are the reference's ``train_one_epoch``
(main_util.py:39-90) / ``train_one_epoch_seq`` (clip_util.py:20-78) without a host read inside the epoch, and ``fit`` is its
``train()`` (main.py:104-170): epochs, a validation epoch after each (``evaluate.eval_epoch`` / ``eval_epoch_clips``), StepLR,
``model.best.t7`` by validation RNE, and a resume point from which a run continues bit for bit.
"""
import contextlib
import math
import os

import torch
import torch.distributed as dist

from . import synth
from .dataset import Augment
from .dp import FlatAdam, FlatGradBucket, SegmentedReducer, ema_options, guard_options
from .fused_blocks import join_side_streams
from .losses import RadarFlowLoss, make_labels, make_labels_ragged


class TrainStep:
    def __init__(self, net, vr_thres=0.3, lr=0.001, weight_decay=1e-4, camera_projection=None, t_camera_radar=None, group=None,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None):
        """``max_grad_norm`` / ``skip_nonfinite``: the guard of the optimizer step (dp.FlatAdam) -- clip by the L2 norm of the whole
        gradient, leave parameters and moments untouched when that norm is not finite.  It runs inside ``opt.step()``, behind the
        all-reduce, so every rank sees the same bucket and takes the same decision without a further collective.  On a CPU model a
        requested guard raises ValueError: torch's Adam has none and nothing here falls back.
        ``ema_decay``: averaged weights (dp.FlatAdam: an exponential moving average of the parameters, updated inside the optimizer's
        launch; ``opt.ema_weights()`` / ``opt.ema_state_dict(net)`` use it).  None: off, nothing changes.  Refused on a CPU model
        like the guard."""
        max_grad_norm, skip_nonfinite = guard_options(max_grad_norm, skip_nonfinite)
        ema_decay = ema_options(ema_decay)
        self.net = net
        self.group = group                                         # the process group of the gradient all-reduce (None: the default one)
        dev = next(net.parameters()).device
        self.vr_thres = vr_thres
        self.loss_obj = RadarFlowLoss(camera_projection or synth.CAMERA_PROJECTION,
                                      t_camera_radar or synth.T_CAMERA_RADAR).to(dev)
        self.bucket = FlatGradBucket(net)
        # the reference's Adam (main.py:107) as one launch over the flat bucket (dp.FlatAdam; torch's fused Adam: six launches at the
        # tail of the step); on a CPU model torch's own
        if dev.type != "cuda" and (max_grad_norm is not None or skip_nonfinite):
            raise ValueError("TrainStep: max_grad_norm / skip_nonfinite need the GPU optimizer (dp.FlatAdam); the model is on the CPU")
        if dev.type != "cuda" and ema_decay is not None:
            raise ValueError("TrainStep: ema_decay needs the GPU optimizer (dp.FlatAdam); the model is on the CPU")
        self.opt = (FlatAdam(self.bucket, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                             ema_decay=ema_decay)
                    if dev.type == "cuda" else torch.optim.Adam(self.bucket.params, lr=lr, weight_decay=weight_decay))
        self.recurrent = hasattr(net, "gru")
        self.self_supervised = hasattr(net, "fd_layer")
        # the scales of an encoder run on side streams while the gradient bucket lives on the main stream
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
        self.gfeat = None
        # diagnostics (bench.py --force-allreduce): run the gradient all-reduce even with a single rank
        self.force_allreduce = False
        # The all-reduce can be cut into three segments in the order backward completes them -- heads + second encoder
        # (+ GRU), cost volume, first encoder -- each launched from a tensor hook as soon as its chains have been enqueued
        # (models/model.py:40-42: nn.DataParallel reduces inside backward too).  Opt-in (CMF_OVERLAP_ALLREDUCE=1 or
        # overlap_allreduce = True): measured on one MI355X with a world-1 RCCL group inside every step (bench.py
        # --force-allreduce, same box) the step is 22.22 ms without a collective, 22.79 ms with ONE all-reduce after backward
        # and 23.00 ms with the three overlapped segments -- RCCL's stream is a fifth busy hardware queue next to the four
        # the step uses (more queues are slower on this part), so running it DURING backward costs more
        # than the 0.2-0.3 ms of ring time it could hide at 8 GPUs.  Both forms leave bit-identical buckets (tests/test_dp.py,
        # the two-rank GPU tests run the overlapped one).
        self.overlap_allreduce = os.environ.get("CMF_OVERLAP_ALLREDUCE") == "1"
        self.reducer = None
        enc2 = net._second_encoder() if hasattr(net, "_second_encoder") else None
        if enc2 is not None and hasattr(net, "fc_layer") and hasattr(net, "mse_layer") and not self.self_supervised:
            try:
                late = [m for m in (enc2, getattr(net, "gru", None), net.fp, net.mp) if m is not None]
                segs = [self.bucket.segment_of(late), self.bucket.segment_of([net.fc_layer]), self.bucket.segment_of([net.mse_layer])]
                self.reducer = SegmentedReducer(self.bucket, segs, group)
            except ValueError:                                   # a model whose parameter order does not follow the data flow
                self.reducer = None

    def reset_clip(self):
        """clip_util.py:51-52: the first frame of a mini-clip starts from gfeat=None."""
        self.gfeat = None

    def forward_loss(self, batch):
        """``batch["t_camera_radar"]`` (B,4,4), when present -- an augmented batch (dataset.augment_batch) -- is the calibration per
        sample the loss projects through; it must have been derived from this step's ``loss_obj.t_camera_radar`` (the iterators'
        ``t_camera_radar`` argument; ``train_epoch`` / ``train_epoch_clips`` pass it)."""
        pc1, pc2, ft1, ft2 = batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"]
        if self.self_supervised:                                   # model 'raflow': main_util.py:57-60
            output, pred_f, pre_trans, mask_s = self.net(pc1, pc2, ft1, ft2, batch["interval"])
            loss, items = self.loss_obj(pc1, pc2, pred_f, ft1[:, 0])
            return loss, items, (pred_f, output, pre_trans, mask_s), (None, None)
        dyn_mask, mseg_gt = make_labels(batch, self.vr_thres)
        if self.recurrent:
            g = self.gfeat.detach() if self.gfeat is not None else None          # clip_util.py:54
            pred_f, mseg_pre, pre_trans, mask, self.gfeat = self.net(pc1, pc2, ft1, ft2, mseg_gt, 'train', g)
        else:
            pred_f, mseg_pre, pre_trans, mask = self.net(pc1, pc2, ft1, ft2, mseg_gt, 'train')
        loss, items = self.loss_obj(pc1, pc2, pred_f, ft1[:, 0], batch["flow_label"].transpose(2, 1), pre_trans,
                                    mseg_pre, batch["gt_trans"], mseg_gt, dyn_mask, batch["radar_u"],
                                    batch["radar_v"], batch["opt_flow"], t_camera_radar=batch.get("t_camera_radar"))
        return loss, items, (pred_f, mseg_pre, pre_trans, mask), (dyn_mask, mseg_gt)

    def _segment_ready(self, i):
        """Tensor hook (autograd thread): everything that writes segment i has been enqueued.  Parameter gradients are
        accumulated in place by kernels on the side streams (fused_blocks.grad_sink), so the pool is joined into this
        stream first; the collective then waits for this stream."""
        if self.reducer is not None and self.reducer.active:
            join_side_streams()
            self.reducer.launch(i)

    def __call__(self, batch):
        overlap = self.overlap_allreduce and self.reducer is not None and self.reducer.begin(self.force_allreduce)
        self.net._grad_ready = self._segment_ready if overlap else None
        try:
            loss, items, outs, labels = self.forward_loss(batch)
        finally:
            self.net._grad_ready = None
        self.bucket.zero()
        loss.backward()
        if loss.is_cuda:
            join_side_streams()                     # gradient sinks written on side streams (fused_blocks.grad_sink)
        if overlap:
            self.reducer.finish()
        else:
            self.bucket.all_reduce_mean(self.group, force=self.force_allreduce)
        self.opt.step()
        return loss.detach(), items, outs, labels

    # ---- whole frames of their own sizes (dataset.collate_ragged / as_batch_dict_ragged) -------------------------------------------
    def forward_loss_ragged(self, batch, validate=False):
        """forward_loss on a RAGGED batch (``dataset.as_batch_dict_ragged``: padded tensors plus ``n1``, ``n2``):
        make_labels_ragged -> forward_ragged_train -> RadarFlowLoss.forward_ragged.  The network must be in eval mode (BatchNorm on
        its running statistics while gradients flow -- the reference's regime after its first epoch); the loss is the mean of the
        per-frame totals (the reference's protocol at batch size 1).  -> (loss, items, outs, labels) as forward_loss, with
        ``items["per_sample"]`` the (B,9) per-frame values (column 0 the total, then losses.ITEM_KEYS)."""
        if self.self_supervised:
            raise NotImplementedError("RaFlow has no ragged-batch training step: its SFR module normalises by the padded point count")
        pc1, pc2, ft1, ft2, n1, n2 = (batch[k] for k in ("pc1", "pc2", "ft1", "ft2", "n1", "n2"))
        if self.net.training:
            raise RuntimeError("step_ragged needs eval-mode BatchNorm: call net.eval() first (train-mode batch statistics over padded "
                               "rows are a different computation)")
        dyn_mask, mseg_gt = make_labels_ragged(batch, self.vr_thres)
        if self.recurrent:
            g = self.gfeat.detach() if self.gfeat is not None else None          # clip_util.py:54
            pred_f, mseg_pre, pre_trans, mask, self.gfeat = self.net.forward_ragged_train(pc1, pc2, ft1, ft2, n1, n2, mseg_gt, g,
                                                                                          validate=validate)
        else:
            pred_f, mseg_pre, pre_trans, mask = self.net.forward_ragged_train(pc1, pc2, ft1, ft2, n1, n2, mseg_gt, validate=validate)
        loss, items, per_sample = self.loss_obj.forward_ragged(pc1, pc2, pred_f, ft1[:, 0], n1, n2, batch["flow_label"].transpose(2, 1),
                                                               pre_trans, mseg_pre, batch["gt_trans"], mseg_gt, dyn_mask,
                                                               batch["radar_u"], batch["radar_v"], batch["opt_flow"], validate=validate,
                                                               t_camera_radar=batch.get("t_camera_radar"))
        items = dict(items, per_sample=per_sample)
        return loss, items, (pred_f, mseg_pre, pre_trans, mask), (dyn_mask, mseg_gt)

    def step_ragged(self, batch, validate=False):
        """One optimizer step on a ragged batch: forward_loss_ragged -> zero the bucket -> backward -> join the side streams ->
        all-reduce -> Adam.  Returns what __call__ returns."""
        loss, items, outs, labels = self.forward_loss_ragged(batch, validate)
        self.bucket.zero()
        loss.backward()
        join_side_streams()                         # gradient sinks written on side streams (fused_blocks.grad_sink)
        self.bucket.all_reduce_mean(self.group, force=self.force_allreduce)
        self.opt.step()
        return loss.detach(), items, outs, labels


# ---- epochs (main_util.py:39-90, clip_util.py:20-78) ---------------------------------------------------------------------------------
def _epoch_statistics(rows, weights, dev):
    """rows: per step a (1 + K,) tensor [loss, items...]; weights: the steps' batch sizes (host ints) -> (sum loss * B / sum B, the
    items' means over the steps), float64 on the device, every sum taken in step order as the reference's host loop takes them."""
    if not rows:
        raise ValueError("an epoch without a step: the split holds fewer frames (mini-clips) than one global batch")
    total = torch.zeros((), dtype=torch.float64, device=dev)
    items = torch.zeros(rows[0].numel() - 1, dtype=torch.float64, device=dev)
    for row, B in zip(rows, weights):
        row = row.double()
        total = total + row[0] * B
        items = items + row[1:]
    return total / _count(sum(weights), dev), items / _count(len(rows), dev)


def _count(n, dev):
    """n as a 0-d float64 device tensor (a fill, no copy): dividing by it is a true division, as the reference's host arithmetic
    is -- dividing a device tensor by a Python number multiplies by the rounded reciprocal."""
    return torch.full((), float(n), dtype=torch.float64, device=dev)


def train_epoch(step, split, batch_size, npoints, seed, epoch, rank=0, world=1, augment=None):
    """train_one_epoch (main_util.py:39-90) for CMFlow / RaFlow: ``step`` (a TrainStep) on every batch of
    ``split.epoch(batch_size, npoints, seed, epoch, drop_last=True, rank, world)`` -- the reference's shuffled loader with drop_last
    (main.py:207).  -> (total_loss, loss_items): ``total_loss = sum loss * B / sum B`` and, per key of the step's items, the mean
    over the steps, as 0-d float64 device tensors (the reference takes the same sums of ``.item()`` values on the host, in float64;
    here they are taken in step order, which is numpy's order below 8 steps and differs from its pairwise order in the last
    bits above).  Inside the loop the host only enqueues: nothing is read back, so it never waits for the device.
    Like the reference it does NOT touch ``net.training``: whoever called ``net.eval()`` last decides the BatchNorm regime (``fit``).
    At world > 1 the statistics are this rank's own (``fit`` averages them over the ranks once per epoch).
    ``augment`` (a ``dataset.Augment``; None: off) goes to ``split.epoch`` together with the step's own shared calibration
    (``step.loss_obj.t_camera_radar``), from which every batch's per-sample calibration is derived."""
    rows, weights = [], []
    for batch in split.epoch(batch_size, npoints, seed, epoch, True, rank, world, augment, _calibration_of(step, augment)):
        loss, items = step(batch)[:2]
        rows.append(torch.stack([loss, *items.values()]))
        weights.append(int(batch["pc1"].shape[0]))
        keys = list(items)
    total, means = _epoch_statistics(rows, weights, split.device)
    return total, {k: means[i] for i, k in enumerate(keys)}


def _calibration_of(step, augment):
    """The shared radar-to-camera matrix an augmented iterator starts from: the one the step's loss object holds."""
    return step.loss_obj.t_camera_radar if augment is not None else None


def train_epoch_clips(step, split, batch_size, mini_clip_len, npoints, seed, epoch, rank=0, world=1, augment=None):
    """train_one_epoch_seq (clip_util.py:20-78) for CMFlow_T over ``split.epoch_clips(...)``: ``net.train()`` at entry (:25 -- unlike
    train_one_epoch, so CMFlow-T trains every epoch under train-mode BatchNorm), then per step ``step.reset_clip()`` and one
    optimizer step per frame of the mini-clips, the recurrent state carried (detached) from frame to frame.  A step's loss is the
    float32 mean over its L frames (:64,68), its items the float64 means over the frames (:70); ``total_loss`` weights the steps by
    their number of mini-clips (the last step of ``epoch_clips`` may be short at world = 1) and the items are averaged over the
    steps (:71-76).  Returns and the no-read-back rule as in train_epoch.  ``augment`` as in train_epoch: a mini-clip keeps one
    transform across its frames (``DeviceSplit.epoch_clips``)."""
    step.net.train()
    L = int(mini_clip_len)
    rows, weights = [], []
    for clip in split.epoch_clips(batch_size, L, npoints, seed, epoch, rank, world, augment, _calibration_of(step, augment)):
        step.reset_clip()
        frames = []
        for batch in clip:
            loss, items = step(batch)[:2]
            frames.append((loss, torch.stack(list(items.values()))))
            keys = list(items)
        iter_loss = frames[0][0]
        iter_items = frames[0][1].double()
        for loss, vals in frames[1:]:
            iter_loss = iter_loss + loss
            iter_items = iter_items + vals.double()
        rows.append(torch.cat(((iter_loss / L).double().reshape(1), iter_items / _count(L, split.device))))
        weights.append(int(clip[0]["pc1"].shape[0]))
    total, means = _epoch_statistics(rows, weights, split.device)
    return total, {k: means[i] for i, k in enumerate(keys)}


# ---- the run (main.py:104-170) -------------------------------------------------------------------------------------------------------
BEST_FILE = os.path.join("models", "model.best.t7")               # main.py:147-149, under out_dir
LAST_FILE = "last.pt"
RESUME_VERSION = 1
GUARD_KEYS = ("grad_norm_mean", "grad_norm_max", "clipped_steps", "skipped_steps")      # history / on_epoch entries of a guarded fit


def make_schedule(opt, decay_epochs, decay_rate):
    """The reference's schedule (main.py:108): torch's own StepLR on the step's optimizer, stepped once per epoch.  The scheduler
    itself and not ``lr * decay_rate ** (epoch // decay_epochs)``: it multiplies the current rate by gamma at every decay, and
    that recursive product differs from the closed form in the last bits."""
    return torch.optim.lr_scheduler.StepLR(opt, int(decay_epochs), gamma=float(decay_rate))


def replaces_best(best, score):
    """main.py:143: ``best_val_res >= eval_score`` -- a tie replaces the kept model, a NaN score never does."""
    return bool(best >= score)


def save_atomic(obj, path):
    """torch.save to a temporary name in the same directory, then os.replace: a killed run leaves the previous whole file."""
    tmp = "%s.tmp%d" % (path, os.getpid())
    torch.save(obj, tmp)
    os.replace(tmp, path)


def _broadcast_buffers(net, group):
    """Rank 0's buffers (the BatchNorm running statistics and counters) to every rank.  The parameters are identical on all ranks
    (one averaged gradient), the running statistics are each rank's own; nn.DataParallel keeps those of its first replica
    (models/model.py:40-42), and so does this -- once per epoch, before the validation, so that all ranks validate, and go on
    training, the same network, the one rank 0 writes to disk."""
    src = 0 if group is None else dist.get_global_rank(group, 0)
    for t in net.buffers():
        dist.broadcast(t.data, src=src, group=group)


OPTIONAL_SETTINGS = {"max_grad_norm": None, "skip_nonfinite": False, "ema_decay": None, "augment": None}


def check_resume_settings(stored, given):
    """fit's comparison of a resume point's settings with the call's: every setting of the call must equal the stored one, where
    the options a run only records when they are on (OPTIONAL_SETTINGS: the guard, the average, the augmentation) count as off on
    the side that lacks them.  A difference raises ValueError naming (stored, given) per key."""
    stored, given = dict(OPTIONAL_SETTINGS, **stored), dict(OPTIONAL_SETTINGS, **given)
    differ = {k: (stored.get(k), v) for k, v in given.items() if stored.get(k) != v}
    if differ:
        raise ValueError("fit: the resume point was written by a run with other settings (stored, given): %s" % differ)


def _refuse(net, train_split, val_split, epochs, rank, world, group):
    """fit's refusals, before anything is launched, built or switched."""
    from .cmflow import CMFlow_T
    from .evaluate import _check_epoch
    if int(epochs) < 1:
        raise ValueError("fit: epochs = %d; at least one" % int(epochs))
    recurrent = isinstance(net, CMFlow_T)
    if recurrent and train_split.clips is None:
        raise ValueError("fit: CMFlow_T trains on mini-clips and the training split has no clip ranges (build it with from_dataset "
                         "on a vodClipDataset)")
    rank, world = _check_epoch(net, val_split, "fit", recurrent, rank, world, group)      # model class, val clips, ranks, val on GPU
    train_split._need_gpu("fit")
    if not next(net.parameters()).is_cuda:
        raise RuntimeError("fit: the network is on the CPU; the training step runs on the GPU only")
    return recurrent, rank, world


def fit(net, train_split, val_split, *, epochs, batch_size, val_batch_size, num_points, lr=1e-3, decay_epochs=1, decay_rate=0.9,
        seed=1234, mini_clip_len=5, vr_thres=0.3, out_dir=None, resume=None, on_epoch=None, rank=0, world=1, group=None, args=None,
        max_grad_norm=None, skip_nonfinite=False, ema_decay=None, augment=None):
    """The reference's ``train()`` (main.py:104-170) on two device-resident splits, without its plots and log files; the defaults
    are configs.yaml's.  One TrainStep (Adam, weight decay 1e-4) and one StepLR (``make_schedule``), then per epoch:

      1. train: ``train_epoch`` (CMFlow, RaFlow) or ``train_epoch_clips`` (CMFlow_T) on ``train_split``, batches keyed by
         (seed, epoch, step);
      2. validate: ``evaluate.eval_epoch`` / ``eval_epoch_clips`` on ``val_split`` at ``val_batch_size`` with seed ``seed + 1`` (its
         draws come from another Philox stream than the training draws); the score is ``sf_metric['rne']``;
      3. keep the best: ``replaces_best`` (the reference's ``>=``: a tie replaces, NaN never does); rank 0 then writes
         ``out_dir/models/model.best.t7`` -- ``net.state_dict()`` and nothing else, the reference's file, which its model loads;
      4. ``scheduler.step()``;
      5. rank 0 writes the resume point ``out_dir/last.pt``: model, optimizer (both Adam moment arrays and the step count) and
         scheduler state, the next epoch, ``best``, the histories, ``net.training`` as the validation left it, and the settings.
         Both files are written under a temporary name and renamed;
      6. ``on_epoch(epoch, record)``: the place of the reference's log lines; ``record`` holds the epoch's ``lr``, ``train_loss``,
         ``loss_items``, ``val_score``, ``best`` and ``is_best``.

    -> the history: ``train_loss``, ``loss_items`` (one dict per epoch), ``val_score``, ``lr`` (the rate each epoch trained with), one
    entry per epoch, and ``best``.  The host reads the device once per epoch -- one small vector with the score and the epoch's
    training statistics -- and never inside an epoch.

    BatchNorm regime.  ``fit`` never calls ``net.train()`` for CMFlow / RaFlow, because the reference does not (train_one_epoch,
    main_util.py:39-90): pass a fresh network in train mode and epoch 0 trains under train-mode BatchNorm, the first validation's
    ``net.eval()`` (main_util.py:96) sticks, and every later epoch trains under eval-mode BatchNorm (running statistics, gradients
    still flowing).  CMFlow_T stays in train mode in every training epoch: train_one_epoch_seq calls ``net.train()`` itself
    (clip_util.py:25).  Pass a network in eval mode and all epochs run under eval-mode BatchNorm.

    ``resume=path`` (a ``last.pt``): restores everything listed under 5, ``net.training`` included, and continues at the stored
    epoch; the batches depend on (seed, epoch, step) only, so the continued run is bit for bit the uninterrupted one.  Stored
    settings (model class, batch sizes, num_points, seed, lr, schedule, mini_clip_len, vr_thres, world, the splits' frame
    counts) that differ from the call's raise ValueError -- ``epochs`` may differ, that is how a run is extended.

    Data parallel: ``rank`` / ``world`` / ``group`` go to the iterators (``batch_size`` and ``val_batch_size`` are per rank), to the
    TrainStep's gradient all-reduce and to the validation.  The score is all-reduced inside the validation, so every rank takes the
    same decisions; the epoch's training statistics are averaged over the ranks in one all-reduce per epoch, so every rank returns
    the same history.  BatchNorm's running statistics are per rank during an epoch (as nn.DataParallel's are per replica); before
    every validation rank 0's are broadcast, so all ranks validate and continue with the network rank 0 saves.  Only rank 0 writes files; a resumed run reads the one ``last.pt`` on every rank.  Start the ranks from
    identical parameters (``dp.broadcast_module``).

    Guard.  ``max_grad_norm`` / ``skip_nonfinite`` go to the TrainStep (dp.FlatAdam: clip by the gradient's L2 norm; skip a step whose
    norm is NaN or Inf, so that one bad batch does not put NaN into the Adam moments for good).  With either on, the epoch's one read
    also carries the optimizer's ``guard_stats(reset=True)``, and the history and the ``on_epoch`` record gain ``grad_norm_mean`` (over
    the epoch's steps with a finite norm; NaN if there was none), ``grad_norm_max``, ``clipped_steps`` and ``skipped_steps`` (0 unless
    ``skip_nonfinite``).  They are not averaged over the ranks: the guard reads the all-reduced bucket, so they are identical on
    all of them.  The settings hold the two options only when a guard is on, and a resume point without them compares as "off";
    with the guard off, history, record and ``last.pt`` have exactly the keys they had without it.  The guard protects parameters
    and moments; train-mode BatchNorm updates its running statistics in the forward, so a non-finite INPUT still reaches those.

    Averaged weights.  ``ema_decay`` (a float in (0, 1); None: off) goes to the TrainStep (dp.FlatAdam keeps an exponential moving
    average of the parameters inside the optimizer's launch).  With it on, the epoch's validation runs inside
    ``step.opt.ema_weights()``, so ``val_score`` -- and with it ``best`` -- is the averaged model's, and ``model.best.t7`` is
    ``step.opt.ema_state_dict(net)``: still the reference's file format and nothing else.  BatchNorm's buffers are not averaged;
    the averaged parameters are validated and saved with the live running statistics.  ``last.pt`` stores the live model and the
    optimizer state, which carries ``ema``, and the settings gain ``ema_decay``; a resume point without it compares as "off", a
    mismatch either way raises ValueError, and a resumed run continues bit for bit, ``ema`` included.  With ``ema_decay=None``
    history, record, settings and ``last.pt`` keep exactly their keys and the launches are the same.  Data parallel: nothing is
    exchanged for it -- every rank's parameters are bit-identical (one averaged gradient), so every rank's ``ema`` is; each rank
    swaps its own copy in for the validation and rank 0 writes.

    Augmentation.  ``augment`` (a ``dataset.Augment``; None: off) goes to the TRAINING iterator only (``train_epoch`` /
    ``train_epoch_clips``): every training batch is rotated about the sensor's z axis and, optionally, mirrored, slot by slot, with
    its labels and calibration (``dataset.augment_batch``; one small launch more per step); the validation sweeps are never
    augmented.  The transforms depend on (seed, epoch, step, slot) only, so a resumed run continues bit for bit.  The settings gain
    ``augment`` -- the plain tuple ``(yaw_deg, mirror)`` -- only when it is on; a resume point without it compares as "off" and a
    mismatch either way raises ValueError.  With ``augment=None`` settings and launches are exactly what they were.  Tested: the
    labels' consistency and the loss's invariance; not claimed: any effect on accuracy.

    Refused before anything is launched and before any mode changes: a bad ``max_grad_norm`` or ``ema_decay`` (ValueError), an
    ``augment`` that is not a ``dataset.Augment`` (TypeError), ``epochs < 1``, CMFlow_T with a split without clip ranges, a
    bad rank / world, ``world > 1`` without an initialised process group (ValueError); a model that is not CMFlow / CMFlow_T /
    RaFlow (NotImplementedError); a split or a network that is not on the GPU (RuntimeError).
    Whole-frame training (``epoch_ragged`` / ``step_ragged``) is not driven from here: its epoch 0 would need train-mode BatchNorm
    on ragged batches, which raises by design.  The speed of a run is unmeasured."""
    from . import evaluate as EV
    max_grad_norm, skip_nonfinite = guard_options(max_grad_norm, skip_nonfinite)
    guarded = max_grad_norm is not None or skip_nonfinite
    ema_decay = ema_options(ema_decay)
    if augment is not None and not isinstance(augment, Augment):
        raise TypeError("fit: augment is a dataset.Augment or None (got %s)" % type(augment).__name__)
    recurrent, rank, world = _refuse(net, train_split, val_split, epochs, rank, world, group)
    dev = train_split.device
    settings = {"model": type(net).__name__, "batch_size": int(batch_size), "val_batch_size": int(val_batch_size),
                "num_points": int(num_points), "seed": int(seed), "lr": float(lr), "decay_epochs": int(decay_epochs),
                "decay_rate": float(decay_rate), "mini_clip_len": int(mini_clip_len), "vr_thres": float(vr_thres), "world": world,
                "train_frames": len(train_split), "val_frames": len(val_split)}
    if guarded:
        settings.update(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    if ema_decay is not None:
        settings.update(ema_decay=ema_decay)
    if augment is not None:
        settings.update(augment=tuple(augment))
    state = None
    if resume is not None:
        state = torch.load(resume, map_location=dev)
        if not isinstance(state, dict) or state.get("format") != "cmflow_amd.fit" or state.get("version") != RESUME_VERSION:
            raise ValueError("fit: %s is not a resume point of format version %d" % (resume, RESUME_VERSION))
        check_resume_settings(state["settings"], settings)
    step = TrainStep(net, vr_thres=vr_thres, lr=lr, group=group, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                     ema_decay=ema_decay)
    scheduler = make_schedule(step.opt, decay_epochs, decay_rate)
    history = {"train_loss": [], "loss_items": [], "val_score": [], "lr": [], "best": math.inf}     # main.py:110
    if guarded:
        history.update({k: [] for k in GUARD_KEYS})
    first = 0
    if state is not None:
        net.load_state_dict(state["model"])
        step.opt.load_state_dict(state["optimizer"])
        scheduler.load_state_dict(state["scheduler"])
        net.train(bool(state["training"]))
        history, first = state["history"], int(state["epoch"])
    writes = rank == 0 and out_dir is not None
    if writes:
        os.makedirs(os.path.join(out_dir, "models"), exist_ok=True)
    for epoch in range(first, int(epochs)):
        rate = step.opt.param_groups[0]["lr"]
        if recurrent:
            total, items = train_epoch_clips(step, train_split, batch_size, mini_clip_len, num_points, seed, epoch, rank, world, augment)
        else:
            total, items = train_epoch(step, train_split, batch_size, num_points, seed, epoch, rank, world, augment)
        if world > 1:
            _broadcast_buffers(net, group)
        with step.opt.ema_weights() if ema_decay is not None else contextlib.nullcontext():      # the averaged model is what is scored
            if recurrent:
                sf = EV.eval_epoch_clips(net, val_split, val_batch_size, mini_clip_len, num_points, seed + 1, epoch, args,
                                         rank=rank, world=world, group=group)[0]
            else:
                sf = EV.eval_epoch(net, val_split, val_batch_size, num_points, seed + 1, epoch, args, rank=rank, world=world,
                                   group=group)[0]
        stats = torch.stack([total, *items.values()])
        if world > 1:                                               # this rank's statistics -> the mean over the ranks
            dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=group)
            stats = stats / world
        parts = (sf["rne"].reshape(1), stats) + ((step.opt.guard_stats(reset=True),) if guarded else ())
        numbers = torch.cat(parts).tolist()                                     # the epoch's one read of the device
        score, train_loss = numbers[0], numbers[1]
        guard = {}
        if guarded:                                                 # identical on every rank: the guard reads the reduced bucket
            record = numbers[-8:]
            numbers = numbers[:-8]
            finite = record[0] - record[1]
            guard = {"grad_norm_mean": record[3] / finite if finite > 0 else math.nan, "grad_norm_max": record[4],
                     "clipped_steps": int(record[2]), "skipped_steps": int(record[1]) if skip_nonfinite else 0}
            for k in GUARD_KEYS:
                history[k].append(guard[k])
        history["lr"].append(rate)
        history["train_loss"].append(train_loss)
        history["loss_items"].append(dict(zip(items, numbers[2:])))
        history["val_score"].append(score)
        is_best = replaces_best(history["best"], score)
        if is_best:
            history["best"] = score
            if writes:
                save_atomic(net.state_dict() if ema_decay is None else step.opt.ema_state_dict(net), os.path.join(out_dir, BEST_FILE))
        scheduler.step()
        if writes:
            save_atomic({"format": "cmflow_amd.fit", "version": RESUME_VERSION, "settings": settings, "epoch": epoch + 1,
                         "model": net.state_dict(), "optimizer": step.opt.state_dict(), "scheduler": scheduler.state_dict(),
                         "training": bool(net.training), "history": history}, os.path.join(out_dir, LAST_FILE))
        if on_epoch is not None:
            on_epoch(epoch, {"lr": rate, "train_loss": train_loss, "loss_items": history["loss_items"][-1], "val_score": score,
                             "best": history["best"], "is_best": is_best, **guard})
    return history
