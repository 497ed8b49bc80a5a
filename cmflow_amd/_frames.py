"""What the stages of a test run's analysis chain (``accumulate``, ``instances``, ``tracks``, ``objects``, ``score``, ``vis``) ask of
their arguments, stated once: the ``which`` of a stage, the store or the upstream result that must belong to the split, the two sides
``score`` compares, numbers in their ranges, the frame selection, the ``done`` test, the (flow, mask, transforms) a stage reads, and
the pinned upload of host tables.
Every check takes the caller's name (``what``) for its message.  A stage calls them in its own order -- every ``ValueError`` first,
then ``bind`` / ``on_device`` for the ``RuntimeError``s -- so nothing here touches the device before those two.  Private: the stages'
docstrings are the contract.  The device side of the same rules is csrc/frame_tables.h.
"""
import math

import numpy as np
import torch

WHICH = ("pred", "gt")


def to_device(host, dtype, device):
    """A host array as a tensor of ``dtype`` on ``device``, through pinned memory (no wait) where that is a GPU."""
    return pinned(torch.from_numpy(np.ascontiguousarray(host)).to(dtype), device)


def pinned(t, device):
    device = torch.device(device)
    return t.pin_memory().to(device, non_blocking=True) if t.numel() and device.type == "cuda" else t.to(device)


def check_which(which, what):
    if which not in WHICH:
        raise ValueError("%s: which = %r is not one of %s" % (what, which, ", ".join(WHICH)))


def number(what, name, v, zero_ok, says):
    """``v`` as a float: a finite int or float (numpy's included, no bool) above 0, or 0 and above with ``zero_ok``; ``says``: the
    range in words, for the message."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0 or (v == 0 and not zero_ok):
        raise ValueError("%s: %s = %r (%s)" % (what, name, v, says))
    return float(v)


def within(what, name, v, lo, hi, says):
    """``v`` as a float: a finite int or float (numpy's included, no bool) in [lo, hi); ``says``: the range in words."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not lo <= v < hi:
        raise ValueError("%s: %s = %r (%s)" % (what, name, v, says))
    return float(v)


def whole(what, name, v, lo, hi=None):
    """``v`` as an int: a whole number (numpy's included, no bool) in lo .. hi, or from lo on (below 2^31) without ``hi``."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= (2 ** 31 - 1 if hi is None else hi):
        raise ValueError("%s: %s = %r (a whole number%s)" % (what, name, v, ", %d or above" % lo if hi is None else " from %d to %d" % (lo, hi)))
    return int(v)


def check_frames_tensor(frames, what):
    if frames.dtype != torch.int64 or frames.dim() != 1:
        raise ValueError("%s: frames is a list or a 1-d int64 tensor, not %s of shape %s" % (what, frames.dtype, tuple(frames.shape)))


def in_split(ids, F, what):
    if ids.size and not (0 <= ids.min() and ids.max() < F):
        raise ValueError("%s: frames outside 0 .. %d" % (what, F - 1))
    return ids


def selected(frames, F, what, bounds=True):
    """The frame selection of a stage on the host: None (all ``F``), a list, or a 1-d int64 tensor -> int64 numpy ids; a DEVICE tensor
    is read back (the one wait).  ValueError for another tensor and, with ``bounds``, for ids outside the split."""
    if frames is None:
        return np.arange(F, dtype=np.int64)
    if torch.is_tensor(frames):
        check_frames_tensor(frames, what)
        ids = frames.detach().cpu().numpy()
    else:
        ids = np.asarray([int(f) for f in frames], dtype=np.int64)
    return in_split(ids, F, what) if bounds else ids


def belongs(split, store, what):
    """ValueError unless ``store`` is a store of ``split``: as many frames, as many rows."""
    if len(split) != len(store) or split.tab1.shape[0] != store.flow.shape[0]:
        raise ValueError("%s: the split is not the one these results belong to" % what)


def check_store(split, store, which, what):
    """``'pred'`` needs a store, of this split (``'gt'`` reads none)."""
    if which == "pred":
        if store is None:
            raise ValueError("%s: which='pred' reads a SplitResults store; pass one, or which='gt'" % what)
        belongs(split, store, what)


def check_upstream(split, store, result, rows, what, these, made):
    """The downstream form of ``check_store``: ``result`` (``these``: 'instances' / 'tracks', ``made``: how) with ``rows`` in the
    split's row space belongs to ``split``, and so does the store its ``which='pred'`` needs."""
    if result.which == "pred" and store is None:
        raise ValueError("%s: these %s were %s with which='pred'; pass the SplitResults store their transforms are in" % (what, these, made))
    if len(split) != result.off.numel() - 1 or split.tab1.shape[0] != rows.shape[0]:
        raise ValueError("%s: the split is not the one these %s belong to" % (what, these))
    if result.which == "pred":
        belongs(split, store, what)


def check_sides(split, a, b, what, these):
    """Two results of one stage (``these``: 'object states') that a stage compares: both in the split's row space (as
    ``check_upstream``), with the same offsets and the same clips, on one device."""
    for r in (a, b):
        if len(split) != r.off.numel() - 1 or split.tab1.shape[0] != r.trk.track.shape[0]:
            raise ValueError("%s: the split is not the one these %s belong to" % (what, these))
    if not np.array_equal(a.offsets_host, b.offsets_host):
        raise ValueError("%s: the two sides' offsets differ: not the same split" % what)
    if not np.array_equal(a.clips_host, b.clips_host):
        raise ValueError("%s: the two sides were tracked over different clips" % what)
    if a.device != b.device:
        raise ValueError("%s: the two sides lie on different devices (%s, %s)" % (what, a.device, b.device))


def need_done(store, needed, what, role):
    """ValueError unless every needed frame is ``done`` in the store -- its one copy to the host.  ``needed``: int64 ids (counted and
    named in the caller's order) or a bool mask over the frames."""
    done = store.done.cpu().numpy() != 0
    mask = needed.dtype == bool
    missing = needed & ~done if mask else ~done[needed]
    if missing.any():
        first = missing.argmax() if mask else needed[missing.argmax()]
        raise ValueError("%s: %d %s frames have no results (first: frame %d)" % (what, int(missing.sum()), role, int(first)))


def transforms(split, store, which):
    return split.trans if which == "gt" else store.pred_trans


def bind(split, store, which, what):
    """After every ``ValueError``: the split on the GPU and, for ``'pred'``, the store on the same one (RuntimeError) ->
    (flow, mask, T, gt) as the kernels take them -- ``'gt'``: no flow and no mask (the split's own columns), the split's transforms."""
    split._need_gpu(what)
    if which == "gt":
        return None, None, split.trans, True
    if not (store.flow.is_cuda and store.flow.device == split.device):
        raise RuntimeError("%s: store on %s, split on %s" % (what, store.flow.device, split.device))
    return store.flow, store.mask, store.pred_trans, False


def on_device(split, tensors, what, made):
    """The downstream form of ``bind``: every (name, tensor) of ``tensors`` on the split's GPU, or RuntimeError."""
    split._need_gpu(what)
    for name, t in tensors:
        if not (t.is_cuda and t.device == split.device):
            raise RuntimeError("%s: %s on %s, split on %s (%s are formed on the GPU only, no CPU fallback)" % (what, name, t.device, split.device, made))


def per_row(per_frame, off, total):
    """A per-frame quantity (F) repeated over every frame's rows -> (total); ``off`` (F+1): the row offsets."""
    return torch.repeat_interleave(per_frame, (off[1:] - off[:-1]).long(), output_size=total)
