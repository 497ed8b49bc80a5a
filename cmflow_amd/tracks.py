"""Moving-object instances tracked across the frames of a clip, on the device -- what ``instances.cluster`` stops short of: which
instance of the next frame is the same object, how long it has been seen, where it was expected.

Everything this needs lies on the device already: an instance carries a centroid and a mean own-motion displacement (``disp``),
the store (``which='pred'``) or the split (``'gt'``) every frame's ego-motion, and the frames of a clip are consecutive scan pairs
(the contract of ``cmf_pose_chain`` and ``accumulate``), so "where will this object be in the next frame" is a defined quantity.
``track`` is one launch of ``cmf_track_instances`` (csrc/tracks.hip) over all clips: a gated greedy nearest-first association of
every frame's instances with the tracks the clip's earlier frames left -- a definition in float64 with a fixed operation order and
every tie decided by the one order (G2, track id, j), stated in include/cmflow_hip.h and DESIGN.md section 23 and restated in numpy,
bit for bit, by tests/tracks_ref.py.  ``vis.render_tracks`` draws the result: an object keeps its colour from frame to frame.

What this is NOT: a filter (a track repeats the displacement of its last match, frame after frame, and is set to the measurement
when matched), re-identification (a track that misses more than ``max_gap`` frames is gone, and the object gets a new id when it
comes back), merge or split handling (two objects clustered as one instance are one track while that lasts), boxes, ground-truth
identities (the split has none: ``which='gt'`` tracks the instances of the labelled moving points by the same rule), and nothing
is claimed about real data beyond the reference's twelve saved frames the tests go through.
"""
import numpy as np
import torch

from . import _frames, _lib
from .instances import FrameInstances

MAX_LIVE = 1024                                             # CMF_TRACK_MAX_LIVE of include/cmflow_hip.h
MAX_GAP = 16                                                # CMF_TRACK_MAX_GAP
PER_INSTANCE = ("track", "prev_row", "gap", "age", "pred")
PER_TRACK = ("birth", "last", "hits")


class InstanceTracks:
    """The tracks of a ``FrameInstances`` result, on the device.  In the instances' row space (instance c of frame f is row off[f] + c):

      ``track`` (sum n1) int32        the instance's track, numbered from 0 inside its clip; -1 behind the frame's K
      ``prev_row`` (sum n1) int32     the row of the instance the track matched before this one; -1 for the first
      ``gap`` (sum n1) int32          the frames since that match (1: the frame before); 0 for the first
      ``age`` (sum n1) int32          the matches of the track so far, this one included
      ``pred`` (sum n1, 3) float32    the position the track predicted for this frame, what the instance was matched against; the
                                      centroid itself for the first
      ``point_track`` (sum n1) int32  per POINT: the track of the point's instance (``inst.label``), or -1

    in the clip's row space (track u of the clip [a, b) is row off[a] + u):

      ``birth``, ``last`` (sum n1) int32   the frames (of the split) of the track's first and last match; -1 behind the clip's tracks
      ``hits`` (sum n1) int32              its matches; 0 behind the clip's tracks

    and per clip ``ntracks`` (C) int32 and ``overflow`` (C) int32 (the frames at which more than 1024 tracks were alive and the
    coasting ones were dropped).  ``clips`` (C,2) int32 / ``clips_host``: the [first, last) ranges the call tracked, ``gate`` and
    ``max_gap`` as given to ``track``; ``off`` / ``offsets_host`` the split's offsets."""

    def __init__(self, inst, arrays, ntracks, overflow, clips, clips_host, gate, max_gap):
        self.inst = inst
        self.off, self.offsets_host, self.which = inst.off, inst.offsets_host, inst.which
        self.track, self.prev_row, self.gap, self.age, self.pred, self.point_track, self.birth, self.last, self.hits = arrays
        self.ntracks, self.overflow, self.clips, self.clips_host = ntracks, overflow, clips, clips_host
        self.gate, self.max_gap = float(gate), int(max_gap)
        self.device = self.track.device

    def __len__(self):
        return self.clips_host.shape[0]

    def frame(self, i):
        """Views of frame ``i`` of the split: the first K rows of track, prev_row, gap, age, pred, and point_track (n1).  K comes from
        the instances' host copy of ``count``, made on first use and kept (the one wait, as ``FrameInstances.frame``)."""
        K = self.inst.frame(i)["centroid"].shape[0]
        a, b = int(self.offsets_host[int(i)]), int(self.offsets_host[int(i) + 1])
        out = {k: getattr(self, k)[a:a + K] for k in PER_INSTANCE}
        out["point_track"] = self.point_track[a:b]
        return out

    def lengths(self):
        """(sum n1) int32 in the clip's row space: the frames from a track's first match to its last, ``last - birth + 1``; 0 in rows
        that hold no track.  Torch ops on the device, nothing read back."""
        return torch.where(self.hits > 0, self.last - self.birth + 1, torch.zeros_like(self.hits))


def plan_clips(F, clips):
    """Host arithmetic of ``track``: the [first, last) ranges ``clips`` of a split of ``F`` frames (None: one clip) clamped to 0 .. F,
    empty ones left out, and every frame outside all of them as a clip of its own (as ``accumulate.plan``) -> (C,2) int32 in frame
    order.  ValueError for a range that descends (last < first) or two that overlap."""
    cover = np.zeros(F, dtype=bool)
    out = []
    for a, b in ([(0, F)] if clips is None else clips):
        a, b = int(a), int(b)
        if b < a:
            raise ValueError("track: the clip range [%d, %d) descends" % (a, b))
        a, b = min(max(a, 0), F), min(max(b, 0), F)
        if cover[a:b].any():
            raise ValueError("track: the clip range [%d, %d) overlaps an earlier one" % (a, b))
        cover[a:b] = True
        if b > a:
            out.append((a, b))
    out += [(int(f), int(f) + 1) for f in np.flatnonzero(~cover)]
    return np.array(sorted(out), dtype=np.int32).reshape(-1, 2)


def track(inst, split, store=None, gate=2.0, max_gap=2):
    """The instances ``inst`` (an ``instances.cluster`` result of ``split``) associated from frame to frame -> ``InstanceTracks``.

    Inside every clip of ``split.clips`` (None: the split is one clip; a frame outside every range is a clip of its own) the frames
    are taken in order.  A track predicts its position in the next frame from its last match: the centroid through that frame's
    ego-motion (``store.pred_trans`` for ``inst.which == 'pred'``, which therefore needs ``store``; the split's ``trans`` for
    ``'gt'``) plus the instance's ``disp``.  An instance and a track may match iff they lie within ``gate`` metres; the candidate
    pairs are taken nearest first (equal distances: the lower track id, then the lower instance), a pair matches iff both are still
    free.  An instance left over opens a new track; a track left over keeps its prediction going (its displacement turned with the
    ego-motion) and is dropped after more than ``max_gap`` frames without a match.  A frame that was not selected when clustering has
    no instances: everything coasts through it.
    The outputs are filled once, then there is ONE launch -- one workgroup per clip, so the call keeps as many CUs busy as there are
    clips and lasts as long as the longest; nothing waits for the device.
    ValueError, before any launch, for an ``inst`` that is no ``FrameInstances``, ``'pred'`` without a store, a split or store the
    instances do not belong to, ``gate`` not finite or <= 0, ``max_gap`` no whole number in 0 .. 16, clip ranges that descend or
    overlap; RuntimeError when the split or the instances are not on the GPU or lie on different devices (no CPU fallback)."""
    if not isinstance(inst, FrameInstances):
        raise ValueError("track: inst is a cluster() result, not %s" % type(inst).__name__)
    _frames.check_upstream(split, store, inst, inst.label, "track", "instances", "clustered")
    _frames.number("track", "gate", gate, False, "a finite number above 0, metres")
    _frames.whole("track", "max_gap", max_gap, 0, MAX_GAP)
    F = len(split)
    clips_host = plan_clips(F, split.clips)
    T = _frames.transforms(split, store, inst.which)
    _frames.on_device(split, (("instances", inst.label), ("transforms", T)), "track", "tracks")
    dev = split.device
    total, C = split.tab1.shape[0], clips_host.shape[0]
    i32, f32 = torch.int32, torch.float32
    full = lambda shape, v, dt=i32: torch.full(shape, v, dtype=dt, device=dev)
    arrays = (full((total,), -1), full((total,), -1), full((total,), 0), full((total,), 0), full((total, 3), 0.0, f32), full((total,), -1),
              full((total,), -1), full((total,), -1), full((total,), 0))
    ntracks, overflow = full((C,), 0), full((C,), 0)
    clips = _frames.to_device(clips_host, i32, dev)
    out = InstanceTracks(inst, arrays, ntracks, overflow, clips, clips_host, gate, max_gap)
    if C == 0:
        return out
    p = _lib.dev_ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_track_instances(
            C, F, p(clips, i32), p(split.off1, i32), total, p(inst.count, i32), p(inst.label, i32), p(inst.centroid, f32), p(inst.disp, f32),
            p(T.reshape(-1, 16), f32), float(gate) * float(gate), int(max_gap), *(p(t, f32 if t.dtype == f32 else i32) for t in arrays),
            p(ntracks, i32), p(overflow, i32), _lib.stream_ptr()), "cmf_track_instances")
    return out
