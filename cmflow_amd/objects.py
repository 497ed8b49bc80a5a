"""Per-track object states of a test run, on the device -- what ``tracks.track`` stops short of: per object and per frame, where it
is, how fast it moves, which way it points and how large it is.

Everything this needs lies on the device already: a track's matches are linked by ``prev_row``, every match has a measured position
(the instance's ``centroid``) and a measured own-motion displacement from the scene flow (``disp``), and ``cmf_pose_chain`` gives
every frame's pose in the clip's axes.  A test run is offline, so the estimator is a fixed-interval smoother, not a causal filter:
``estimate`` is two launches, ``cmf_pose_chain`` on the tracker's clips and then ``cmf_track_states`` (csrc/objects.hip) over all
clips -- per track a constant-velocity Kalman filter forwards over its matches (position and displacement both measured, the
process noise a white acceleration) and a Rauch-Tung-Striebel smoother backwards, in the clip's axes; then per match the smoothed
position and velocity back in the frame's own scan-1 axes, a heading along the smoothed velocity, and a box oriented along that
heading around the instance's points.  A definition in float64 with a fixed operation order (+ - * / and sqrt only), stated in
include/cmflow_hip.h and DESIGN.md section 24 and restated in numpy, bit for bit, by tests/objects_ref.py.

What this is NOT: boxes are not drawn (``vis`` has no line segments yet); a slow object (smoothed speed below ``min_disp`` metres
per frame) gets no principal-axis heading but the axis-aligned box its instance already has (``heading_src`` 0); the filter's state
is per FRAME, so frame intervals that vary inside a clip are not modelled (``velocity()`` divides by the frame's interval
afterwards); no ground-truth identities or boxes (the split has none: ``which='gt'`` smooths the tracks of the labelled moving
points by the same rule); no merge or split handling (two objects clustered as one instance are one box while that lasts); the
tracks are not formed again with the smoothed prediction; a radar sees part of an object in most frames, so a frame's box is the
extent of the points seen, not the object's (``track_size`` takes the largest over a track); and nothing is claimed about real data
beyond the reference's twelve saved frames the tests go through.
"""
import numpy as np
import torch

from . import _frames, _lib
from .tracks import InstanceTracks

PER_INSTANCE = ("row_frame", "next_row", "filt", "fcov", "state", "scov", "pos", "vel", "heading", "heading_src", "box_center", "box_size")


class TrackObjects:
    """The object states of an ``InstanceTracks`` result, on the device, in the instances' row space (instance c of frame f is row
    off[f] + c; the rows behind a frame's K hold row_frame -1, next_row -1, heading_src -1 and zeros):

      ``row_frame`` (sum n1) int32       the frame of the row's instance
      ``next_row`` (sum n1) int32        the row of the track's next match (the inverse of the tracker's ``prev_row``); -1 for the last
      ``filt``, ``state`` (sum n1, 6) float64   the filtered and the smoothed p0 p1 p2 v0 v1 v2 in the CLIP's axes (the scan-1 axes of
                                         the clip's first frame), v in metres per frame
      ``fcov``, ``scov`` (sum n1, 3) float64    their covariance (P_pp, P_pv, P_vv), one for the three axes
      ``pos``, ``vel`` (sum n1, 3) float32      the smoothed position and velocity (metres per frame) in the FRAME's scan-1 axes
      ``heading`` (sum n1, 2) float32    the unit direction of ``vel`` in the x-y plane, or (1, 0)
      ``heading_src`` (sum n1) int32     1: from the velocity; 0: below ``min_disp``, the axis-aligned box
      ``box_center``, ``box_size`` (sum n1, 3) float32   the box around the instance's points along the heading, its normal and z

    ``poses`` (F,16) float64: the pose chain the states were formed with.  ``trk``: the tracks; ``sigma_pos``, ``sigma_disp``,
    ``sigma_acc``, ``min_disp`` as given to ``estimate``."""

    def __init__(self, trk, arrays, poses, clip_base, interval, sigma_pos, sigma_disp, sigma_acc, min_disp):
        self.trk, self.inst = trk, trk.inst
        self.off, self.offsets_host, self.which = trk.off, trk.offsets_host, trk.which
        for k, t in zip(PER_INSTANCE, arrays):
            setattr(self, k, t)
        self.poses, self.clip_base, self.interval = poses, clip_base, interval
        self.clips, self.clips_host = trk.clips, trk.clips_host
        self.sigma_pos, self.sigma_disp, self.sigma_acc, self.min_disp = float(sigma_pos), float(sigma_disp), float(sigma_acc), float(min_disp)
        self.device = self.state.device

    def __len__(self):
        return self.clips_host.shape[0]

    def frame(self, i):
        """Views of frame ``i`` of the split: the first K rows of every array above.  K comes from the instances' host copy of
        ``count``, made on first use and kept (the one wait, as ``InstanceTracks.frame``)."""
        K = self.inst.frame(i)["centroid"].shape[0]
        a = int(self.offsets_host[int(i)])
        return {k: getattr(self, k)[a:a + K] for k in PER_INSTANCE}

    def velocity(self):
        """(sum n1, 3) float32: ``vel`` over the frame's ``split.interval`` -- the smoothed velocity against the ground in the frame's
        scan-1 axes, metres per second (as ``FrameInstances.velocity``).  Rows that hold no instance are 0."""
        return self.vel / _frames.per_row(self.interval, self.off, self.vel.shape[0])[:, None]

    def yaw(self):
        """(sum n1) float32: the heading as an angle, ``atan2(heading_y, heading_x)`` in torch -- a convenience, not part of the
        bit-exact contract."""
        return torch.atan2(self.heading[:, 1], self.heading[:, 0])

    def track_size(self):
        """(sum n1, 3) float32 in the CLIP's row space (track u of the clip [a, b) is row off[a] + u, as ``InstanceTracks.birth``): per
        track the largest ``box_size`` over its matches, coordinate by coordinate; 0 in rows that hold no track.  A radar sees part
        of an object in most frames, so the maximum is the usable size.  One scatter-amax in torch on the device, nothing read back."""
        total = self.box_size.shape[0]
        held = self.row_frame >= 0
        row = self.clip_base[self.row_frame.clamp(min=0).long()] + self.trk.track.clamp(min=0).long()
        row = torch.where(held & (self.trk.track >= 0), row, torch.full_like(row, total)).clamp(max=total)      # the rest: a row of its own
        out = torch.zeros((total + 1, 3), dtype=self.box_size.dtype, device=self.device)
        out.scatter_reduce_(0, row[:, None].expand(-1, 3), self.box_size, "amax", include_self=True)
        return out[:total]


def _sigma(name, v, zero_ok):
    return _frames.number("estimate", name, v, zero_ok, "a finite number %s" % ("0 or above" if zero_ok else "above 0"))


def estimate(trk, split, store=None, sigma_pos=0.5, sigma_disp=0.25, sigma_acc=0.25, min_disp=0.05):
    """The tracks ``trk`` (a ``tracks.track`` result of ``split``) smoothed into per-match object states -> ``TrackObjects``.

    A track's matches are taken in frame order.  A match is measured in the clip's axes: its centroid through the pose of the
    frame's scan 1, its ``disp`` turned by the pose of the frame's scan 2 (``store.pred_trans`` chained for ``trk.which == 'pred'``,
    which therefore needs ``store``; the split's ``trans`` for ``'gt'``).  The filter's state per axis is (position, displacement
    per frame); between two matches ``gap`` frames apart it predicts with a white acceleration of ``sigma_acc`` (metres per frame^2
    per root frame), a match updates it with ``sigma_pos`` (metres) on the position and ``sigma_disp`` (metres per frame) on the
    displacement, and the smoother runs back over the same matches.  A match whose smoothed horizontal speed reaches ``min_disp``
    (metres per frame) gets its heading from the velocity, any other the axis-aligned box.
    The outputs are filled once, then there are TWO launches -- ``cmf_pose_chain`` on the tracker's clips, then ``cmf_track_states``,
    one workgroup per clip; nothing waits for the device.
    ValueError, before any launch, for a ``trk`` that is no ``InstanceTracks``, ``'pred'`` without a store, a split or store the
    tracks do not belong to, ``sigma_pos`` or ``sigma_disp`` not finite or <= 0, ``sigma_acc`` or ``min_disp`` not finite or < 0;
    RuntimeError when the split or the tracks are not on the GPU or lie on different devices (no CPU fallback)."""
    if not isinstance(trk, InstanceTracks):
        raise ValueError("estimate: trk is a track() result, not %s" % type(trk).__name__)
    inst = trk.inst
    _frames.check_upstream(split, store, trk, trk.track, "estimate", "tracks", "formed")
    F = len(split)
    sigma_pos, sigma_disp = _sigma("sigma_pos", sigma_pos, False), _sigma("sigma_disp", sigma_disp, False)
    sigma_acc, min_disp = _sigma("sigma_acc", sigma_acc, True), _sigma("min_disp", min_disp, True)
    T = _frames.transforms(split, store, trk.which)
    _frames.on_device(split, (("tracks", trk.track), ("instances", inst.label), ("transforms", T)), "estimate", "object states")
    dev = split.device
    total, C = split.tab1.shape[0], trk.clips_host.shape[0]
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev)
    arrays = (full((total,), -1, i32), full((total,), -1, i32), full((total, 6), 0.0, f64), full((total, 3), 0.0, f64), full((total, 6), 0.0, f64),
              full((total, 3), 0.0, f64), full((total, 3), 0.0, f32), full((total, 3), 0.0, f32), full((total, 2), 0.0, f32), full((total,), -1, i32),
              full((total, 3), 0.0, f32), full((total, 3), 0.0, f32))
    poses = full((F, 16), float("nan"), f64)
    base = np.zeros(F, dtype=np.int64)                                      # per frame, the first row of its clip: host arithmetic
    for a, b in trk.clips_host:
        base[int(a):int(b)] = int(trk.offsets_host[int(a)])
    out = TrackObjects(trk, arrays, poses, _frames.to_device(base, torch.int64, dev), split.interval, sigma_pos, sigma_disp, sigma_acc, min_disp)
    if C == 0:
        return out
    p = _lib.dev_ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_pose_chain(F, C, p(T.reshape(-1, 16), f32), p(trk.clips, i32), poses.data_ptr(), _lib.stream_ptr()), "cmf_pose_chain")
        _lib.check(_lib.lib().cmf_track_states(
            C, F, p(trk.clips, i32), p(split.off1, i32), total, p(inst.count, i32), p(inst.label, i32), p(inst.centroid, f32), p(inst.disp, f32),
            p(trk.track, i32), p(trk.prev_row, i32), p(trk.gap, i32), p(split.tab1, f32), split.tab1.shape[1], poses.data_ptr(),
            sigma_pos * sigma_pos, sigma_disp * sigma_disp, sigma_acc * sigma_acc, min_disp * min_disp,
            *(p(t, t.dtype) for t in arrays), _lib.stream_ptr()), "cmf_track_states")
    return out
