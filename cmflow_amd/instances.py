"""Moving-object instances of a test run, clustered on the device -- the first thing done with "these points move, and this is how":
which moving points belong together, where the object is, how large it is and how it moves against the ground.

Everything this needs lies on the device already: positions in ``split.tab1``, flow, mask and transforms in a
``results.SplitResults`` store (``which='pred'``) or in the split itself (``which='gt'``: the labels).  ``cluster`` is one launch of
``cmf_cluster_moving`` (csrc/instances.hip) over all selected frames -- density-based clustering of every frame's moving points by
position and, weighted by ``flow_weight``, by the displacement they show against the ego-motion (the ``d`` of
``accumulate``'s ``'propagate'`` rule).  A definition in float64 with a fixed operation order and the one order-dependent choice of
DBSCAN pinned (a border point joins its nearest core neighbour, the lowest index among equals), stated in include/cmflow_hip.h and
DESIGN.md section 22 and restated in numpy, bit for bit, by tests/instances_ref.py.  ``vis.render_instances`` draws the result.

What this is NOT: every frame is clustered on its own, so instance 3 of one frame has nothing to do with instance 3 of the next
(``tracks.track`` associates the instances of a clip's frames and gives an object one id), no boxes and no orientation (an
instance has a centroid, an axis-aligned extent and a mean displacement), no ground-truth object ids (the split has none: ``which='gt'`` clusters the labelled moving points by the same
rule, and ``agreement`` compares two clusterings), and nothing is claimed about real data beyond the reference's twelve saved
frames the tests go through.
"""
import numpy as np
import torch

from . import _frames, _lib
from ._frames import WHICH                                  # noqa: F401  (``instances.WHICH``)

MAX_POINTS = 1024                                           # CMF_INST_MAX_POINTS of include/cmflow_hip.h
NONE, NOISE, BORDER, CORE = 0, 1, 2, 3                      # CMF_INST_NONE .. CMF_INST_CORE: the values of ``kind``
IOU_UNIT = 2 ** 30                                          # agreement: an IoU is counted in whole units of 2^-30
TABLES = ("size", "seed", "centroid", "disp", "lo", "hi")


class FrameInstances:
    """The instances of the selected frames of a split, on the device, packed like the split's cloud-1 table:

      ``off`` (F+1) int32         the split's ``off1``: frame f owns rows off[f] .. off[f+1]-1 of everything below
      ``frames`` (nsel) int64     the selected frames; rows of other frames hold label -1 and zeros
      ``label`` (sum n1) int32    the point's instance inside its frame, 0 .. K-1, or -1 (noise, static, or not selected)
      ``kind`` (sum n1) uint8     0 not a candidate (static), 1 noise, 2 border, 3 core
      ``count`` (F) int32         K, the instances of frame f
      ``size``, ``seed`` (sum n1) int32; ``centroid``, ``disp``, ``lo``, ``hi`` (sum n1, 3) float32
                                  the instance tables in the points' row space: instance c of frame f is row off[f] + c (K <= n1
                                  always); ``seed`` is the frame-local index of its lowest core point, ``disp`` the mean
                                  displacement against the ego-motion over one frame interval, ``lo`` / ``hi`` the extent.  Rows
                                  behind K hold size 0, seed -1 (0 in frames that were not selected) and zeros.
      ``which``, ``eps``, ``min_points``, ``flow_weight``   as given to ``cluster``

    ``offsets_host`` / ``frames_host`` are host copies the call had anyway (nothing is read back for them)."""

    def __init__(self, off, frames, label, kind, count, tables, interval, which, eps, min_points, flow_weight, offsets_host, frames_host):
        self.off, self.frames, self.label, self.kind, self.count = off, frames, label, kind, count
        self.size, self.seed, self.centroid, self.disp, self.lo, self.hi = tables
        self.interval = interval
        self.which, self.eps, self.min_points, self.flow_weight = which, float(eps), int(min_points), float(flow_weight)
        self.offsets_host, self.frames_host = offsets_host, frames_host
        self.device = label.device
        self._count_host = None

    def __len__(self):
        return self.frames.numel()

    def frame(self, i):
        """Views of frame ``i`` of the split: label, kind (n1), count (0-d), and the first K rows of size, seed, centroid, disp, lo,
        hi.  The offsets are the host's own; K comes from a host copy of ``count`` made on first use and kept (the one wait)."""
        i = int(i)
        if not 0 <= i < self.off.numel() - 1:
            raise IndexError("FrameInstances.frame: frame %d of %d" % (i, self.off.numel() - 1))
        if self._count_host is None:
            self._count_host = self.count.cpu().numpy()
        a, b, K = int(self.offsets_host[i]), int(self.offsets_host[i + 1]), int(self._count_host[i])
        out = {"label": self.label[a:b], "kind": self.kind[a:b], "count": self.count[i]}
        out.update({k: getattr(self, k)[a:a + K] for k in TABLES})
        return out

    def velocity(self):
        """(sum n1, 3) float32, in the instance tables' row space: ``disp`` over the frame's ``split.interval`` -- the instance's mean
        velocity against the ground in the sensor's scan-1 axes, metres per second.  Rows that hold no instance are 0."""
        return self.disp / _frames.per_row(self.interval, self.off, self.disp.shape[0])[:, None]


def cluster(split, store=None, which="pred", eps=2.0, min_points=2, flow_weight=0.0, frames=None):
    """The moving points of every selected frame grouped into instances -> ``FrameInstances`` on the device.

    ``which='pred'`` takes flow, mask and transforms from ``store`` and needs every selected frame ``done``; ``which='gt'`` takes the
    label flow, the mask column and the transforms of the split and reads no store (``store`` may be None).  A point whose mask is 0
    is a candidate.  Two candidates are neighbours iff |p_i - p_j|^2 + flow_weight^2 |d_i - d_j|^2 <= eps^2, d the displacement a
    point's flow shows against the ego-motion (metres per frame; ``flow_weight=0``: position alone); a candidate with at least
    ``min_points`` neighbours, itself included, is a core point; the instances are the connected components of the core points, a
    candidate that is not core joins its nearest core neighbour's (lowest index among equals) or is noise.  A frame's instances
    are numbered by their lowest core point.  ``frames``: None (all), a list, or an int64 tensor.
    The outputs are filled once (label -1, the rest 0), then there is ONE launch; with None or a host list nothing waits for the
    device but, for ``'pred'``, the one copy of ``store.done`` (as ``accumulate``).  A DEVICE tensor of ids is brought to the host once.
    ValueError, before any launch, for an unknown ``which``, ``'pred'`` without a store or with a store of another split, ``eps``
    not finite or <= 0, ``flow_weight`` negative or not finite, ``min_points < 1``, ids outside the split, a selected frame of more
    than 1024 points, or a selected frame that is not done; RuntimeError when the split is not on the GPU (no CPU fallback)."""
    _frames.check_which(which, "cluster")
    _frames.check_store(split, store, which, "cluster")
    _frames.number("cluster", "eps", eps, False, "a finite number above 0, metres")
    _frames.number("cluster", "flow_weight", flow_weight, True, "a finite number, 0 or above")
    _frames.whole("cluster", "min_points", min_points, 1)
    F = len(split)
    ids = _frames.selected(frames, F, "cluster")
    counts = np.asarray(split.counts_host[0], dtype=np.int64)
    large = counts[ids] > MAX_POINTS
    if large.any():
        raise ValueError("cluster: frame %d has %d points, more than the %d one workgroup clusters in its LDS"
                         % (int(ids[large.argmax()]), int(counts[ids[large.argmax()]]), MAX_POINTS))
    if which == "pred":
        _frames.need_done(store, ids, "cluster", "selected")
    flow, mask, T, gt = _frames.bind(split, store, which, "cluster")
    dev = split.device
    total, nsel = split.tab1.shape[0], ids.size
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    sel = None if frames is None else _frames.to_device(ids, torch.int64, dev)
    ids_d = torch.arange(F, dtype=torch.int64, device=dev) if frames is None else sel
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    label, kind, count = torch.full((total,), -1, dtype=i32, device=dev), z((total,), u8), z((F,), i32)
    tables = (z((total,), i32), z((total,), i32), z((total, 3), f32), z((total, 3), f32), z((total, 3), f32), z((total, 3), f32))
    off_host = np.concatenate(([0], np.cumsum(counts)))
    out = FrameInstances(split.off1, ids_d, label, kind, count, tables, split.interval, which, eps, min_points, flow_weight, off_host, ids)
    if nsel == 0:
        return out
    eps2, w2 = float(eps) * float(eps), float(flow_weight) * float(flow_weight)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_cluster_moving(
            nsel, F, None if sel is None else _lib.dev_ptr(sel, torch.int64), _lib.dev_ptr(split.off1, i32), total,
            _lib.dev_ptr(split.tab1, f32), split.tab1.shape[1], _lib.dev_ptr(flow, f32), _lib.dev_ptr(mask, u8),
            _lib.dev_ptr(T.reshape(-1, 16), f32), int(gt), eps2, w2, int(min_points), _lib.dev_ptr(label, i32), _lib.dev_ptr(kind, u8),
            _lib.dev_ptr(count, i32), _lib.dev_ptr(tables[0], i32), _lib.dev_ptr(tables[1], i32), *(_lib.dev_ptr(t, f32) for t in tables[2:]),
            _lib.stream_ptr()), "cmf_cluster_moving")
    return out


def agreement(pred, gt):
    """How well a clustering ``pred`` recovers the instances of a clustering ``gt``: two ``cluster`` results of the same split and
    selection (usually ``which='pred'`` against ``which='gt'``).  For a point i with a gt instance G and a predicted instance P,
    IoU_i = c / (|G| + |P| - c), c the points of the frame that lie in both; 0 where the point has no predicted instance.

      ``iou`` (nsel) float64         per selected frame, the mean of IoU_i over its points with a gt instance; NaN without such a point
      ``count_pred``, ``count_gt`` (nsel) int32   the instances of the frame on either side

    Batched torch ops on the device without data-dependent shapes (the pair keys are sorted and their runs counted with
    ``searchsorted``), nothing read back.  Exact in any summation order: c / (|G| + |P| - c) is one float64 division, counted in whole
    units of 2^-30 (rounded down), the units are summed as integers, and the mean is one float64 division of that sum by the point
    count times 2^30 -- so ``agreement(x, x)`` is exactly 1 wherever it is defined."""
    for a in (pred, gt):
        if not isinstance(a, FrameInstances):
            raise ValueError("agreement: two cluster() results")
    if pred.device != gt.device or not np.array_equal(pred.frames_host, gt.frames_host) or not np.array_equal(pred.offsets_host, gt.offsets_host):
        raise ValueError("agreement: the two results differ in selection, split or device")
    dev, i64 = pred.device, torch.int64
    F, total = pred.off.numel() - 1, pred.label.shape[0]
    off = pred.off.to(i64)
    frame_of = torch.repeat_interleave(torch.arange(F, dtype=i64, device=dev), off[1:] - off[:-1], output_size=total)
    g, p = gt.label.to(i64), pred.label.to(i64)
    key = (frame_of * (MAX_POINTS + 1) + (g + 1)) * (MAX_POINTS + 1) + (p + 1)
    ordered = torch.sort(key).values
    c = torch.searchsorted(ordered, key, right=True) - torch.searchsorted(ordered, key, right=False)
    base = off[:-1][frame_of]
    size_g, size_p = gt.size.to(i64)[base + g.clamp(min=0)], pred.size.to(i64)[base + p.clamp(min=0)]
    union = (size_g + size_p - c).clamp(min=1)                              # only read where both sizes count the point itself
    units = torch.floor(c.to(torch.float64) / union.to(torch.float64) * float(IOU_UNIT)).to(i64)
    has_g = g >= 0
    units = torch.where(has_g & (p >= 0), units, torch.zeros_like(units))
    zero = torch.zeros(1, dtype=i64, device=dev)
    csum, cnum = torch.cat((zero, torch.cumsum(units, 0))), torch.cat((zero, torch.cumsum(has_g.to(i64), 0)))
    points = (cnum[off[1:]] - cnum[off[:-1]]).to(torch.float64)
    iou = (csum[off[1:]] - csum[off[:-1]]).to(torch.float64) / (points * float(IOU_UNIT))          # 0 / 0 = NaN
    sel = pred.frames
    return {"iou": iou[sel], "count_pred": pred.count[sel], "count_gt": gt.count[sel]}
