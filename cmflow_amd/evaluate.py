"""Evaluation epochs on a device-resident split -- mirror of ``eval_one_epoch`` (main_util.py:93-206) and of CMFlow-T's
``test_one_epoch_seq`` (clip_util.py:182-298) on WHOLE frames, the reference's published protocol (main.py:203: batch_size = 1, every
frame with its own point counts), batched: ``DeviceSplit.sweep`` / ``draw_frames`` hand out ragged batches drawn on the GPU,
``forward_ragged`` runs them and ``eval_batch_ragged`` returns the mean of the per-frame metrics, so ``B * metric`` summed over the
batches and divided by the frame count is what the reference accumulates frame by frame.  Nothing is read back inside the loops: the
sums are float64 device tensors and the two transform arrays are filled at the frames' own indices.

CMFlow-T's test loop is serial in the reference (one frame per forward, the recurrent state carried) but the state is reset at known
frames, so the runs between two resets are independent: ``clip_test_resets`` restates the reset rule, ``clip_test_schedule`` lays
``batch_size`` such runs side by side, and ``eval_split_clips`` steps through them with the state of the still-running ones carried.

Data parallel (``rank``, ``world``, ``group``): every rank evaluates its share of the frames -- its slices of ``sweep``'s global
batches, or the schedule groups ``g % world == rank`` -- and the sums, the frame count and the two transform arrays are all-reduced
once each AFTER the loop, so every rank returns the result of the whole split.

``test_split`` / ``test_split_clips`` are the same epochs with every frame's outputs and metrics kept on the device (results.py): the
reference's ``--eval --save_res`` run.
"""
import torch
import torch.distributed as dist

from . import eval_util as E
from .cmflow import CMFlow, CMFlow_T
from .raflow import RaFlow

METRIC_KEYS = E.SF_KEYS + E.SEG_KEYS + E.POSE_KEYS


class _Accumulator:
    """main_util.py:176-202: sum of batch_size * metric over the batches, divided by the number of frames at the end; the predicted
    and true transforms of every frame at the frame's index."""

    def __init__(self, split, args):
        F, dev = len(split), split.device
        self.args, self.frames = args, 0
        self.sum = torch.zeros(len(METRIC_KEYS), dtype=torch.float64, device=dev)
        self.gt_trans_all = torch.zeros((F, 4, 4), dtype=torch.float32, device=dev)
        self.pre_trans_all = torch.zeros((F, 4, 4), dtype=torch.float32, device=dev)

    def add(self, batch, pred_f, pred_t, pred_m):
        B = batch["pc1"].shape[0]
        groups = E.eval_batch_ragged(batch["pc1"], pred_f.transpose(1, 2).contiguous(), batch["flow_label"], batch["fg_mask"],
                                     pred_m.float(), batch["gt_trans"], pred_t, batch["n1"], self.args)
        self.sum = self.sum + B * torch.stack([v for d in groups for v in d.values()])
        at = batch["frames"].long()
        self.gt_trans_all[at] = batch["gt_trans"]
        self.pre_trans_all[at] = pred_t
        self.frames += B

    def all_reduce(self, group):
        """The ranks' parts into the whole, on every rank: four all_reduce(SUM).  A frame's rows of the two transform arrays are
        written by the one rank that evaluated it and are zero elsewhere, so their sum is exact."""
        frames = torch.tensor([self.frames], dtype=torch.int64, device=self.sum.device)
        for t in (self.sum, frames, self.gt_trans_all, self.pre_trans_all):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self.frames = frames

    def result(self):
        m = self.sum / self.frames
        pick = lambda keys, first: {k: m[first + i] for i, k in enumerate(keys)}
        return (pick(E.SF_KEYS, 0), pick(E.SEG_KEYS, len(E.SF_KEYS)), pick(E.POSE_KEYS, len(E.SF_KEYS) + len(E.SEG_KEYS)),
                self.gt_trans_all, self.pre_trans_all)


def _check(net, split, what, recurrent, rank=0, world=1, group=None):
    if isinstance(net, RaFlow) or not isinstance(net, CMFlow):
        raise NotImplementedError("%s: only CMFlow%s has a ragged-batch forward (RaFlow's SFR module normalises by the padded point "
                                  "count)" % (what, "-T" if recurrent else ""))
    if isinstance(net, CMFlow_T) != recurrent:
        raise ValueError("%s takes %s" % (what, "CMFlow_T (its recurrent state is carried along the clips)" if recurrent
                                          else "CMFlow; CMFlow_T's test protocol is eval_split_clips"))
    if split.max_points > net.RAGGED_MAX_POINTS:
        raise ValueError("%s: the split has a frame of %d points; forward_ragged covers clouds of up to %d"
                         % (what, split.max_points, net.RAGGED_MAX_POINTS))
    if recurrent and split.clips is None:
        raise ValueError("%s: no clip ranges (build the split with from_dataset on a vodClipDataset)" % what)
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("%s: rank %d of a world of %d" % (what, rank, world))
    if world > 1:
        if not (dist.is_available() and dist.is_initialized()):
            raise ValueError("%s: world = %d, but no process group is initialised (the ranks' results are all-reduced at the end)"
                             % (what, world))
        if dist.get_world_size(group) != world or dist.get_rank(group) != rank:
            raise ValueError("%s: rank %d of %d given, the process group says rank %d of %d"
                             % (what, rank, world, dist.get_rank(group), dist.get_world_size(group)))
    split._need_gpu(what)                                           # every refusal comes before net.eval()
    return rank, world


def eval_split(net, split, batch_size, args=None, sort_by_size=False, on_batch=None, rank=0, world=1, group=None):
    """eval_one_epoch (main_util.py:93-206) for CMFlow on the whole frames of a DeviceSplit: ``split.sweep`` -> ``forward_ragged`` ->
    ``eval_batch_ragged`` per batch under no_grad, ``B * metric`` summed in float64 on the device and divided by the frame count --
    the per-frame average the reference reports at its test batch size of 1, whatever ``batch_size`` is here.  The frame ids of
    the whole sweep go to the device in one copy before the first batch; inside the loop the host only enqueues and never waits
    for the device (a test runs the epoch under torch's synchronisation check).  ``sort_by_size``: batches of frames of similar size (less padding; the per-frame results land
    at the frames' own indices all the same).  ``args.radar_res`` as in eval_util.  ``on_batch(batch, outputs)`` is called after every
    forward with the batch dict of ``draw_frames`` and the tuple ``forward_ragged`` returned -- the place of the reference's
    ``save_res`` branch and the way to see per-frame outputs.
    -> (sf_metric, seg_metric, pose_metric, gt_trans_all (F,4,4), pre_trans_all (F,4,4)); the metrics under eval_util's keys as 0-d
    float64 device tensors.  A frame without static points has a NaN 'stat_rne' and makes the epoch's NaN, as in the reference.

    Calls ``net.eval()`` as the reference does (main_util.py:96) and, like the reference, does not restore the mode afterwards: in
    the reference that call is what switches every later training epoch to eval-mode BatchNorm (train_one_epoch never calls
    net.train()), the regime ``TrainStep.step_ragged`` trains in.
    RaFlow raises NotImplementedError (no ragged forward), a split with a frame above ``RAGGED_MAX_POINTS`` ValueError, a split
    that is not on the GPU RuntimeError -- all before anything is launched and before ``net.eval()``.

    Data parallel: rank ``rank`` of ``world`` processes (``batch_size`` per rank; ``group``: their process group, None = the
    default one) sweeps its share, ``split.sweep(batch_size, sort_by_size, rank, world)``; after the loop -- never inside it -- the
    float64 sums, the frame count and the two transform arrays are all-reduced (SUM) once each, and every rank returns the
    result of the whole split: the transform arrays bit for bit those of a single process, the metrics up to the order of a
    float64 sum.  ``on_batch`` sees the rank's own batches.  ``world`` > 1 without an initialised process group, or a ``rank`` /
    ``world`` that is not the group's, raises ValueError with the other refusals."""
    rank, world = _check(net, split, "eval_split", False, rank, world, group)
    net.eval()
    acc = _Accumulator(split, args)
    with torch.no_grad():
        for batch in split.sweep(batch_size, sort_by_size, rank, world):
            out = net.forward_ragged(batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"], batch["n1"], batch["n2"])
            if on_batch is not None:
                on_batch(batch, out)
            acc.add(batch, out[0], out[2], out[3])
    if world > 1:
        acc.all_reduce(group)
    return acc.result()


def clip_test_resets(clips, n_frames, update_len):
    """The frames at which test_one_epoch_seq (clip_util.py:210-233) starts from an empty recurrent state, restated on the host:
    frame i resets when it is the start of clip ``num_clip`` or a multiple of ``update_len``, and EVERY reset advances ``num_clip``
    (up to the last clip).  The quirk is kept: after a reset that was not a clip start the loop waits for the wrong clip, so a clip
    start that is not a multiple of ``update_len`` can pass without a reset.  ``clips``: [first, last) frame range per clip."""
    starts = [int(c[0]) for c in clips]
    update_len = int(update_len)
    if not starts or update_len < 1:
        raise ValueError("clip_test_resets: at least one clip and update_len >= 1")
    resets, num_clip = [], 0
    for i in range(int(n_frames)):
        if i == starts[num_clip] or i % update_len == 0:
            resets.append(i)
            if num_clip < len(starts) - 1:
                num_clip += 1
    return resets


def clip_test_schedule(resets, n_frames, batch_size):
    """The serial test loop as segment-parallel steps.  A segment is the run of frames from one reset up to the next (the state
    is carried inside it and nowhere else).  -> a list of groups; a group takes ``batch_size`` segments in segment order and sorts
    them by length, longest first (ties: by first frame); it is a list of steps, step t listing frame ``first + t`` of every segment
    longer than t.  The active segments of a step are therefore a PREFIX of the group's step 0, and the state to carry into step
    t + 1 is ``gfeat[:len(step t + 1)]``."""
    resets, batch_size = [int(r) for r in resets], int(batch_size)
    if batch_size < 1:
        raise ValueError("clip_test_schedule: batch_size is at least 1")
    if n_frames > 0 and (not resets or resets[0] != 0):
        raise ValueError("clip_test_schedule: frame 0 starts the first segment")
    segments = [(a, b - a) for a, b in zip(resets, resets[1:] + [int(n_frames)])]
    groups = []
    for g in range(0, len(segments), batch_size):
        group = sorted(segments[g:g + batch_size], key=lambda s: (-s[1], s[0]))
        groups.append([[first + t for first, length in group if length > t] for t in range(group[0][1])])
    return groups


def eval_split_clips(net, split, batch_size, update_len, args=None, on_batch=None, rank=0, world=1, group=None):
    """CMFlow-T's test protocol (test_one_epoch_seq, clip_util.py:182-298) on a DeviceSplit built from a vodClipDataset
    (``split.clips``; ValueError otherwise): every frame once, the recurrent global feature carried from frame to frame and reset
    where ``clip_test_resets(split.clips, len(split), update_len)`` says -- run as ``clip_test_schedule`` lays it out, ``batch_size``
    segments side by side per forward instead of one frame.  Step 0 of a group starts from ``gfeat = None``; a later step takes the
    previous step's state of the segments still running, ``gfeat[:active]``.  As in eval_split the host does not wait for the
    device inside the loop (the frame ids of the whole schedule are sent once).  Accumulation, ``on_batch`` (outputs: the five-tuple of
    ``CMFlow_T.forward_ragged``), the returned tuple and the ``net.eval()`` call are eval_split's.
    Data parallel (``rank``, ``world``, ``group`` as in eval_split): group g of the schedule -- ``batch_size`` segments, which share
    no state with any other group -- is run by rank ``g % world``; the final all-reduce is eval_split's."""
    rank, world = _check(net, split, "eval_split_clips", True, rank, world, group)
    schedule = clip_test_schedule(clip_test_resets(split.clips, len(split), update_len), len(split), batch_size)
    if world > 1:
        schedule = schedule[rank::world]
    net.eval()
    acc = _Accumulator(split, args)
    with torch.no_grad():
        batches = split.draw_frame_batches([step for steps in schedule for step in steps])      # the ids of the epoch in one copy
        for steps in schedule:                                      # one group of the schedule
            gfeat = None
            for step in steps:
                batch = next(batches)
                out = net.forward_ragged(batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"], batch["n1"], batch["n2"],
                                         None if gfeat is None else gfeat[:len(step)])
                gfeat = out[4]
                if on_batch is not None:
                    on_batch(batch, out)
                acc.add(batch, out[0], out[2], out[3])
    if world > 1:
        acc.all_reduce(group)
    return acc.result()


# ---- test epochs that keep every frame's results (the reference's --eval --save_res run; results.py) ----------------------------------
def _collecting(collector, on_batch):
    if on_batch is None:
        return collector

    def both(batch, outputs):
        collector(batch, outputs)
        on_batch(batch, outputs)
    return both


def test_split(net, split, batch_size, args=None, sort_by_size=False, on_batch=None, rank=0, world=1, group=None):
    """``eval_split`` that also keeps what the network predicted for every frame: a ``results.ResultCollector`` is its ``on_batch``
    hook (a given ``on_batch`` is still called, after it), so flow, score, mask, both transforms and the 14 metrics of every frame
    land in a ``results.SplitResults`` on the device without the loop ever waiting for it.  Arguments, refusals (``_check``, before
    anything is allocated) and the epoch itself are eval_split's.  Data parallel: the store is all-reduced after eval_split's own
    all-reduce (``SplitResults.all_reduce``), so every rank returns the whole split's.
    -> (the five-tuple of eval_split, SplitResults)."""
    from .results import ResultCollector
    rank, world = _check(net, split, "test_split", False, rank, world, group)
    collector = ResultCollector(split, args)
    five = eval_split(net, split, batch_size, args, sort_by_size, _collecting(collector, on_batch), rank, world, group)
    if world > 1:
        collector.results.all_reduce(group)
    return five, collector.results


def test_split_clips(net, split, batch_size, update_len, args=None, on_batch=None, rank=0, world=1, group=None):
    """``eval_split_clips`` (CMFlow-T's test protocol) with a ``results.ResultCollector`` as its hook, as ``test_split``.
    -> (the five-tuple of eval_split_clips, SplitResults)."""
    from .results import ResultCollector
    rank, world = _check(net, split, "test_split_clips", True, rank, world, group)
    collector = ResultCollector(split, args)
    five = eval_split_clips(net, split, batch_size, update_len, args, _collecting(collector, on_batch), rank, world, group)
    if world > 1:
        collector.results.all_reduce(group)
    return five, collector.results


test_split.__test__ = test_split_clips.__test__ = False                 # entry points of the product, not tests


# ---- validation epochs: frames resampled to num_points, in order (train()'s eval_one_epoch / eval_one_epoch_seq) -----------------------
class _PooledAccumulator(_Accumulator):
    """_Accumulator for dense batches of resampled frames: one ``eval_batch`` per batch -- the points of the batch pooled, as the
    reference's metrics do at a validation batch size above 1 (main_util.py:175-192) -- weighted by the batch's frame count."""

    def add(self, batch, pred_f, pred_t, pred_m):
        B = batch["pc1"].shape[0]
        groups = E.eval_batch(batch["pc1"], pred_f.transpose(1, 2).contiguous(), batch["flow_label"], batch["fg_mask"], pred_m,
                              batch["gt_trans"], pred_t, self.args)
        self.sum = self.sum + B * torch.stack([v for d in groups for v in d.values()])
        at = batch["frames"].long()
        self.gt_trans_all[at] = batch["gt_trans"]
        self.pre_trans_all[at] = pred_t
        self.frames += B

    def result(self):
        if not torch.is_tensor(self.frames):                        # a true division by the count (a fill, no copy), as the host's is;
            self.frames = torch.full((1,), self.frames, dtype=torch.int64, device=self.sum.device)      # by a Python number: * (1 / n)
        return super().result()


def _check_epoch(net, split, what, recurrent, rank, world, group):
    """The refusals of eval_epoch / eval_epoch_clips, all before ``net.eval()``: the model class, clip ranges, rank / world / group
    (``_check``'s rules and kinds of errors), the split's device."""
    if not isinstance(net, CMFlow):
        raise NotImplementedError("%s: CMFlow, CMFlow_T or RaFlow (got %s)" % (what, type(net).__name__))
    if isinstance(net, CMFlow_T) != recurrent:
        raise ValueError("%s takes %s" % (what, "CMFlow_T (its recurrent state is carried along a mini-clip)" if recurrent
                                          else "CMFlow or RaFlow; CMFlow_T validates on mini-clips: eval_epoch_clips"))
    if recurrent and split.clips is None:
        raise ValueError("%s: no clip ranges (build the split with from_dataset on a vodClipDataset)" % what)
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("%s: rank %d of a world of %d" % (what, rank, world))
    if world > 1:
        if not (dist.is_available() and dist.is_initialized()):
            raise ValueError("%s: world = %d, but no process group is initialised (the ranks' results are all-reduced at the end)"
                             % (what, world))
        if dist.get_world_size(group) != world or dist.get_rank(group) != rank:
            raise ValueError("%s: rank %d of %d given, the process group says rank %d of %d"
                             % (what, rank, world, dist.get_rank(group), dist.get_world_size(group)))
    split._need_gpu(what)
    return rank, world


def eval_epoch(net, split, batch_size, npoints, seed, epoch=0, args=None, on_batch=None, rank=0, world=1, group=None):
    """eval_one_epoch as the reference's ``train()`` uses it after every training epoch (main.py:138 on the loader of main.py:206-208):
    the frames of ``split`` in index order, each resampled to ``npoints`` (``split.sweep_resampled``: ``batch_size`` frames per dense
    batch, the short last batch kept; the draws keyed by (seed, epoch)), and per batch under no_grad the dense
    ``net(pc1, pc2, ft1, ft2, None, 'test')`` -- for RaFlow ``net(pc1, pc2, ft1, ft2, interval)`` and its outputs 1..3 -- then one
    ``eval_util.eval_batch`` (metrics pooled over the batch's points).  ``B_b * metric`` is summed in float64 on the device and
    divided by the frame count at the end (main_util.py:175-202); both transforms of a frame land at the frame's index.  Inside the loop
    the host only enqueues.  ``on_batch(batch, outputs)`` as in eval_split.
    -> the 5-tuple of eval_split.  This is NOT the test protocol (whole frames, per-frame metrics: eval_split); it is the number the
    reference selects ``model.best.t7`` by.

    Calls ``net.eval()`` and does not restore the mode (see eval_split: this call is what puts CMFlow's later training epochs under
    eval-mode BatchNorm).  Before that call it refuses: a model that is not CMFlow / RaFlow (NotImplementedError), CMFlow_T
    (ValueError: eval_epoch_clips), a bad rank / world or a missing process group (ValueError), a split on the CPU (RuntimeError).
    Data parallel: as eval_split -- every rank sweeps its rows of the global batches, and sums, frame count and transform arrays
    are all-reduced once each after the loop."""
    rank, world = _check_epoch(net, split, "eval_epoch", False, rank, world, group)
    net.eval()
    acc = _PooledAccumulator(split, args)
    self_supervised = isinstance(net, RaFlow)
    with torch.no_grad():
        for batch in split.sweep_resampled(batch_size, npoints, seed, epoch, rank, world):
            if self_supervised:                                     # main_util.py:140
                out = net(batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"], batch["interval"])
                pred_f, pred_t, pred_m = out[1], out[2], out[3]
            else:                                                   # main_util.py:142
                out = net(batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"], None, 'test')
                pred_f, pred_t, pred_m = out[0], out[2], out[3]
            if on_batch is not None:
                on_batch(batch, out)
            acc.add(batch, pred_f, pred_t, pred_m)
    if world > 1:
        acc.all_reduce(group)
    return acc.result()


def eval_epoch_clips(net, split, batch_size, mini_clip_len, npoints, seed, epoch=0, args=None, on_batch=None, rank=0, world=1,
                     group=None):
    """eval_one_epoch_seq (clip_util.py:99-178), CMFlow-T's validation inside ``train()``: the mini-clips of ``split`` in order
    (``split.sweep_clips``: ``batch_size`` per step, the short last step kept), the L frames of a step one after the other through
    ``net(pc1, pc2, ft1, ft2, None, 'test', gfeat)`` with ``gfeat = None`` at frame 0 of every step and the returned state carried
    to the next frame.  Accumulation as in eval_epoch, over the frames evaluated (the frames a clip's remainder leaves out are not
    visited: their rows of the two transform arrays stay zero, and they do not count).  Everything else -- ``net.eval()``, the
    refusals (here CMFlow_T is the model it takes; a split without clip ranges: ValueError), ``on_batch``, data parallel -- as
    eval_epoch."""
    rank, world = _check_epoch(net, split, "eval_epoch_clips", True, rank, world, group)
    net.eval()
    acc = _PooledAccumulator(split, args)
    with torch.no_grad():
        for step in split.sweep_clips(batch_size, mini_clip_len, npoints, seed, epoch, rank, world):
            gfeat = None                                            # clip_util.py:131-134
            for batch in step:
                out = net(batch["pc1"], batch["pc2"], batch["ft1"], batch["ft2"], None, 'test', gfeat)
                gfeat = out[4]
                if on_batch is not None:
                    on_batch(batch, out)
                acc.add(batch, out[0], out[2], out[3])
    if world > 1:
        acc.all_reduce(group)
    return acc.result()
