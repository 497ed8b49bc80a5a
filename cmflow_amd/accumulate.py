"""A test run's clouds accumulated over a window of frames, on the device -- what ego-motion, motion segmentation and scene flow are
for when taken together: a single 4D-radar scan has a few hundred points, and the last W scans of a clip brought into the current
sensor frame give the densified cloud.  Static points go through the chained ego-motion; moving points are left where the chain
puts them (``dynamic='keep'``: a trail), left out (``'drop'``), or carried forward by their own flow (``'propagate'``).

Everything this needs lies on the device already: positions in ``split.tab1``, flow, mask and transforms in a
``results.SplitResults`` store (``which='pred'``) or in the split itself (``which='gt'``: the labels).  ``accumulate`` is one launch
of ``cmf_accumulate`` (csrc/accumulate.hip) -- a definition in float64 with a fixed operation order, stated in include/cmflow_hip.h
and DESIGN.md section 21 and restated in numpy, bit for bit, by tests/accumulate_ref.py -- and ``vis.render_accumulated`` draws the
result with the rasteriser of ``vis.render``.

What this is NOT is a map: there is no loop closure and no registration refinement (the chain is the product of the per-frame
transforms as they are, so its drift grows with the window), no static-point filtering beyond the mask (a point the mask calls
static is trusted), and a moving point under ``'propagate'`` is assumed to repeat, step after step, the displacement its flow shows
in the ego-compensated frame (constant velocity over the window, no turning).
"""
import numpy as np
import torch

from . import _frames, _lib
from ._frames import WHICH, to_device as _to_device         # noqa: F401  (both are reached through this module too)

MAX_WINDOW = 64                                             # CMF_ACCUM_MAX_WINDOW of include/cmflow_hip.h
DYNAMIC = ("keep", "propagate", "drop")                     # CMF_ACCUM_KEEP, CMF_ACCUM_PROPAGATE, CMF_ACCUM_DROP


class AccumulatedClouds:
    """The accumulated clouds of ``nsel`` target frames, packed, on the device:

      ``off`` (nsel+1) int32      capacity offsets: target s owns rows off[s] .. off[s+1]-1, the point count of all its sources
      ``count`` (nsel) int32      the rows of target s that hold points: off[s+1] - off[s] unless ``dynamic='drop'`` left some out
      ``xyz`` (R, 3) float32      positions in the target's scan-1 sensor frame; rows behind ``count`` are 0
      ``src`` (R) int32           the point's row in ``split.tab1`` / the store (any attribute can be gathered by it); -1 behind ``count``
      ``age`` (R) uint8           how many frames back the point was measured (0: the target's own scan); 255 behind ``count``
      ``frames`` (nsel) int64     the target frames
      ``window``, ``which``, ``dynamic``   as given to ``accumulate``

    A target's rows run oldest age first and the current scan last; inside an age they keep the source frame's point order.
    ``offsets_host`` is the host's own copy of ``off`` (the capacities come from the split's host-side counts, nothing is read back)."""

    def __init__(self, off, count, xyz, src, age, frames, window, which, dynamic, offsets_host, frames_host):
        self.off, self.count, self.xyz, self.src, self.age, self.frames = off, count, xyz, src, age, frames
        self.window, self.which, self.dynamic = int(window), which, dynamic
        self.offsets_host, self.frames_host = offsets_host, frames_host
        self.device = xyz.device

    def __len__(self):
        return self.off.numel() - 1


def plan(counts, clips, ids, window):
    """Host arithmetic of ``accumulate``: for the target frames ``ids`` of a split with ``counts`` points per frame and the [first,
    last) ranges ``clips`` (None: one clip), -> (first (nsel) int32: the first frame of every target's clip, ages (nsel) int32:
    G = min(window, id - first + 1), cap_off (nsel+1) int64: the running sum of the sources' point counts).  A frame outside every
    clip is a clip of its own.  ValueError for a window outside 1 .. 64 or an id outside the split."""
    _frames.whole("accumulate", "window", window, 1, MAX_WINDOW)
    counts = np.asarray(counts, dtype=np.int64)
    F = counts.size
    ids = _frames.in_split(np.asarray(ids, dtype=np.int64).reshape(-1), F, "accumulate")
    start_of = np.arange(F, dtype=np.int64)                                 # outside every clip: a clip of one frame
    for a, b in ([(0, F)] if not clips else clips):
        a, b = max(int(a), 0), min(int(b), F)
        if b > a:
            start_of[a:b] = a
    first = start_of[ids]
    ages = np.minimum(window, ids - first + 1)
    csum = np.concatenate(([0], np.cumsum(counts)))
    cap = csum[ids + 1] - csum[ids - ages + 1]                              # the sources are consecutive frames: their rows are one range
    return first.astype(np.int32), ages.astype(np.int32), np.concatenate(([0], np.cumsum(cap))).astype(np.int64)


def accumulate(split, store=None, window=8, which="pred", dynamic="keep", frames=None):
    """The clouds of the selected target frames accumulated over ``window`` frames -> ``AccumulatedClouds`` on the device.

    For a target j of a clip [a, b) the sources are the frames j-g, g = 0 .. min(window, j-a+1)-1: never across a clip boundary
    (``split.clips``; a split without clip ranges is one clip).  Frames of a clip are taken as consecutive scan pairs -- scan 2 of
    frame k is scan 1 of frame k+1, what ``SplitResults.trajectories`` relies on too.  ``which='pred'`` takes flow, mask and
    transforms from ``store`` and needs every source frame ``done``; ``which='gt'`` takes the label flow, the mask column and the
    transforms of the split and reads no store (``store`` may be None).  ``dynamic``: what happens to a point whose mask is 0 (moving)
    when it is older than the target's own scan -- ``'keep'``: through the chain like a static point; ``'drop'``: left out;
    ``'propagate'``: through the chain, plus its age times the displacement its flow shows against the ego-motion.
    ``frames``: None (all), a list, or an int64 tensor.  The capacities come from the split's host-side counts (``counts_host``): with
    None or a host list nothing waits for the device but, for ``'pred'``, the one copy of ``store.done`` (as ``write_vis``).  A DEVICE
    tensor of ids is brought to the host once -- one wait per call; pass a list where the ids are known on the host.
    ValueError, before any launch, for a window outside 1 .. 64, an unknown ``which`` or ``dynamic``, ``'pred'`` without a store or with
    a source frame that is not done, a store of another split, ids outside the split, or 2^31 output rows and more; RuntimeError when
    the split is not on the GPU (no CPU fallback)."""
    _frames.check_which(which, "accumulate")
    if dynamic not in DYNAMIC:
        raise ValueError("accumulate: dynamic = %r is not one of %s" % (dynamic, ", ".join(DYNAMIC)))
    _frames.check_store(split, store, which, "accumulate")
    F = len(split)
    ids = _frames.selected(frames, F, "accumulate", bounds=False)           # plan() takes the window first, then the bounds
    first, ages, cap_off = plan(split.counts_host[0], split.clips, ids, window)
    if which == "pred":
        need = np.zeros(F + 1, dtype=np.int64)                              # the sources of all targets, as a difference array
        np.add.at(need, ids - ages + 1, 1)
        np.add.at(need, ids + 1, -1)
        _frames.need_done(store, np.cumsum(need[:F]) > 0, "accumulate", "source")
    R = int(cap_off[-1])
    if R >= 2 ** 31:
        raise ValueError("accumulate: %d output rows, more than 2^31 - 1 (select fewer frames or a shorter window)" % R)
    flow, mask, T, gt = _frames.bind(split, store, which, "accumulate")
    dev = split.device
    nsel = ids.size
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    off = _to_device(cap_off, i32, dev)
    first_d = _to_device(first, i32, dev)
    sel = None if frames is None else _to_device(ids, torch.int64, dev)
    ids_d = torch.arange(F, dtype=torch.int64, device=dev) if frames is None else sel
    xyz = torch.empty((R, 3), dtype=f32, device=dev)
    src = torch.empty((R,), dtype=i32, device=dev)
    age = torch.empty((R,), dtype=u8, device=dev)
    count = torch.empty((nsel,), dtype=i32, device=dev)
    out = AccumulatedClouds(off, count, xyz, src, age, ids_d, window, which, dynamic, cap_off, ids)
    if nsel == 0:
        return out
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_accumulate(
            nsel, F, None if sel is None else _lib.dev_ptr(sel, torch.int64), _lib.dev_ptr(first_d, i32), _lib.dev_ptr(split.off1, i32),
            split.tab1.shape[0], _lib.dev_ptr(split.tab1, f32), split.tab1.shape[1], _lib.dev_ptr(flow, f32), _lib.dev_ptr(mask, u8),
            _lib.dev_ptr(T.reshape(-1, 16), f32), int(window), DYNAMIC.index(dynamic), int(gt), _lib.dev_ptr(off, i32), R,
            _lib.dev_ptr(xyz, f32), _lib.dev_ptr(src, i32), _lib.dev_ptr(age, u8), _lib.dev_ptr(count, i32), _lib.stream_ptr()),
            "cmf_accumulate")
    return out


def accumulation_error(pred, gt):
    """How far a predicted accumulation lies from the labels': ``pred`` and ``gt`` are two ``accumulate`` results of the same split,
    selection and window, neither with ``dynamic='drop'`` (so row r of one is the same measured point as row r of the other).  With
    e_r = |xyz_pred,r - xyz_gt,r| (Euclidean, float64):

      ``mean``, ``max`` (nsel)    per target, over its rows of age >= 1 (age 0 is a copy on both sides); NaN for a target without such rows
      ``per_age`` (window)        the mean of e_r over all rows of age g, g = 0 .. window-1; NaN for an age no target has

    Batched torch ops in float64 on the device, nothing read back, and deterministic: the sums are differences of a cumulative sum
    over the rows (per age: over the rows sorted by age, a stable sort), the maximum is exact in any order."""
    for a in (pred, gt):
        if not isinstance(a, AccumulatedClouds) or a.dynamic == "drop":
            raise ValueError("accumulation_error: two accumulate() results with dynamic 'keep' or 'propagate'")
    if pred.window != gt.window or pred.device != gt.device or not np.array_equal(pred.frames_host, gt.frames_host) \
            or not np.array_equal(pred.offsets_host, gt.offsets_host):
        raise ValueError("accumulation_error: the two accumulations differ in selection, window, split or device")
    dev, f64 = pred.device, torch.float64
    nsel, R, W = len(pred), pred.xyz.shape[0], pred.window
    nan = torch.full((), float("nan"), dtype=f64, device=dev)
    if nsel == 0 or R == 0:
        return {"mean": nan.expand(nsel).clone(), "max": nan.expand(nsel).clone(), "per_age": nan.expand(W).clone()}
    diff = pred.xyz.to(f64) - gt.xyz.to(f64)
    e = (diff * diff).sum(-1).sqrt()
    old = pred.age >= 1
    off = pred.off.long()
    zero = torch.zeros(1, dtype=f64, device=dev)
    csum = torch.cat((zero, torch.cumsum(torch.where(old, e, torch.zeros_like(e)), 0)))
    cnum = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(old.long(), 0)))
    rows = (cnum[off[1:]] - cnum[off[:-1]]).to(f64)
    mean = (csum[off[1:]] - csum[off[:-1]]) / rows                          # 0 / 0 = NaN where a target has no older rows
    target = torch.repeat_interleave(torch.arange(nsel, device=dev), off[1:] - off[:-1], output_size=R)
    top = torch.full((nsel,), float("-inf"), dtype=f64, device=dev).scatter_reduce(0, target, torch.where(old, e, -torch.ones_like(e)), "amax")
    top = torch.where(rows > 0, top, nan)
    ages = pred.age.to(torch.int16)
    sorted_age, order = torch.sort(ages, stable=True)
    by_age = torch.cat((zero, torch.cumsum(e[order], 0)))
    edge = torch.searchsorted(sorted_age, torch.arange(W + 1, dtype=torch.int16, device=dev))
    per_age = (by_age[edge[1:]] - by_age[edge[:-1]]) / (edge[1:] - edge[:-1]).to(f64)
    return {"mean": mean, "max": top, "per_age": per_age}
