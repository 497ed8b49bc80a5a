"""From raw radar scans, a calibration, odometry poses and box tracks to a ``DeviceSplit`` -- the reference's offline
``preprocess/`` step (preprocess/utils/get_flow_samples.py:44-248,285-312, optical_flow.py:58-89, vod/frame/transformations.py:285-328)
as array arithmetic on the GPU (csrc/prepare.hip), and the same input filter as a front end of ``CMFlow.forward_ragged``.

What runs where: the filter, the kept-row compaction, the box tests with their 3 m gate, the rigid flow and the label rules are
kernels (``cmf_prepare_count``, ``cmf_prepare_pairs``, ``cmf_prepare_scans``); the 4 x 4 products of a pair (ego-motion, the box
transforms of a handful of tracks: ``match_boxes``) are numpy float64 on the host.  GPU only: the functions that launch raise
RuntimeError without one; argument errors raise ValueError before anything is launched.

Row conventions: a scan row is ``x y z RCS v_r [...]`` (float32, at least 5 columns); a track row is
``h w l x y z rot score id`` (float64; the box in camera coordinates as the tracker writes it).  The reference has no depth test in
its FOV filter -- a point behind the camera whose projection lands in the image is kept -- and neither has this one; a row whose
homogeneous pixel coordinate ``w`` is zero or not finite (undefined in the reference) is dropped.
"""
import numpy as np
import torch

from . import _lib
from .dataset import DRAW_MAX_POINTS, DeviceSplit

BOX_DOUBLES = 32                 # CMF_PREP_BOX_DOUBLES: centre 3 | rotation 9 | half extents 3 | T_b1_b2 16 | score
MODES = {"gt": 0, "pseudo": 1}   # CMF_PREP_MODE_*
INTERVAL = 0.10                  # dataset/vod.py:32


def _mat(what, a, shape):
    a = np.asarray(a)
    if a.dtype != np.float64:
        raise ValueError("%s: float64 expected, got %s" % (what, a.dtype))
    if a.shape[-2:] != shape or a.ndim not in (2, 3):
        raise ValueError("%s: %s or (S,%d,%d) expected, got %s" % (what, shape, shape[0], shape[1], a.shape))
    if not np.isfinite(a).all():
        raise ValueError("%s: not finite" % what)
    return np.ascontiguousarray(a)


class Calibration:
    """``t_camera_radar`` (4,4), ``camera_projection_matrix`` (3,4) and ``t_radar_lidar`` (4,4), float64: one set for all scans, or
    arrays with a leading (S,...) axis, one set per scan.  ``image_size`` = (width, height) and ``height`` = (lowest, highest z
    kept) are the reference's IMG_WIDTH, IMG_HEIGHT (global_param.py:6-7) and [-3, 3].  ``t_radar_camera`` is the inverse of
    ``t_camera_radar``."""

    def __init__(self, t_camera_radar, camera_projection_matrix, t_radar_lidar, image_size=(1936, 1216), height=(-3.0, 3.0)):
        self.t_camera_radar = _mat("Calibration: t_camera_radar", t_camera_radar, (4, 4))
        self.camera_projection_matrix = _mat("Calibration: camera_projection_matrix", camera_projection_matrix, (3, 4))
        self.t_radar_lidar = _mat("Calibration: t_radar_lidar", t_radar_lidar, (4, 4))
        per = {a.shape[0] for a in (self.t_camera_radar, self.camera_projection_matrix, self.t_radar_lidar) if a.ndim == 3}
        if len(per) > 1 or (per and any(a.ndim == 2 for a in (self.t_camera_radar, self.camera_projection_matrix, self.t_radar_lidar))):
            raise ValueError("Calibration: one set of matrices for all scans, or the same number S of each")
        self.per_scan = per.pop() if per else None
        try:
            self.t_radar_camera = np.linalg.inv(self.t_camera_radar)
        except np.linalg.LinAlgError:
            raise ValueError("Calibration: t_camera_radar is singular") from None
        w, h = (int(v) for v in image_size)
        lo, hi = (float(v) for v in height)
        if w < 1 or h < 1 or not lo <= hi:
            raise ValueError("Calibration: image_size = (width, height) >= 1 and height = (lo, hi) with lo <= hi")
        self.image_size, self.height = (w, h), (lo, hi)

    def scan(self, s):
        """The calibration of scan ``s`` as a single-set Calibration."""
        if self.per_scan is None:
            return self
        return Calibration(self.t_camera_radar[s], self.camera_projection_matrix[s], self.t_radar_lidar[s], self.image_size, self.height)

    def _check_scans(self, what, S):
        if self.per_scan is not None and self.per_scan != S:
            raise ValueError("%s: the calibration holds %d sets, the call %d scans" % (what, self.per_scan, S))

    def _device(self, device):
        """(t_camera_radar (k,16), projection (k,12)) float64 on the device, k = 1 or S."""
        to = lambda a, c: torch.from_numpy(a.reshape(-1, c)).to(device)
        return to(self.t_camera_radar, 16), to(self.camera_projection_matrix, 12)


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _box(row, calib):
    """get_bbx_param (get_flow_samples.py:285-303) for the radar: centre, rotation, extent (l, w, h) of a track row."""
    centre = (calib.t_radar_camera @ np.array([row[3], row[4], row[5], 1.0]))[:3]
    rot = calib.t_radar_lidar[:3, :3] @ _rz(-(row[6] + np.pi / 2))
    return centre, rot, np.array([row[2], row[1], row[0]])


def _pose(rot, centre):
    T = np.zeros((4, 4))
    T[:3, :3], T[:3, 3], T[3, 3] = rot, centre, 1.0
    return T


def _tracks(what, a):
    a = np.asarray(a)
    if a.size == 0:
        return np.zeros((0, 9))
    if a.ndim != 2 or a.shape[1] != 9 or a.dtype != np.float64:
        raise ValueError("%s: track rows are (M,9) float64 = h w l x y z rot score id, got %s %s" % (what, a.shape, a.dtype))
    return a


def match_boxes(labels1, labels2, calib1, calib2):
    """The box records of one pair (extract_fg_labels, get_flow_samples.py:178-217, up to its point tests): for every row of
    ``labels1`` in order, the FIRST row of ``labels2`` with the same id (rows without one are skipped; no rows in either frame:
    nothing) -> (K, 32) float64, a record = centre of box 1 (3) | its rotation (9, row-major) | half extents l/2 w/2 h/2 |
    T_b2 inv(T_b1) (16, row-major; T_b = [R | c]) | score of row 1.  ``calib1`` / ``calib2``: single-set Calibrations of the frames."""
    labels1, labels2 = _tracks("match_boxes: labels1", labels1), _tracks("match_boxes: labels2", labels2)
    for c in (calib1, calib2):
        if not isinstance(c, Calibration) or c.per_scan is not None:
            raise ValueError("match_boxes: calib1, calib2 are single-set Calibrations (Calibration.scan(s) of a per-scan one)")
    out = []
    if labels1.shape[0] and labels2.shape[0]:
        for row in labels1:
            nxt = np.where(labels2[:, -1] == row[-1])[0]
            if len(nxt) == 0:
                continue
            c1, r1, ext = _box(row, calib1)
            c2, r2, _ = _box(labels2[nxt[0]], calib2)
            t12 = _pose(r2, c2) @ np.linalg.inv(_pose(r1, c1))
            out.append(np.concatenate([c1, r1.reshape(9), ext / 2, t12.reshape(16), [row[7]]]))
    return np.stack(out) if out else np.zeros((0, BOX_DOUBLES))


def _need_gpu(what, device):
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("%s: device %s -- scans are prepared on the GPU only (no CPU fallback)" % (what, dev))
    return dev


def _offsets(what, off, total, name="scan_off"):
    off = np.asarray(off)
    if off.ndim != 1 or off.size < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("%s: %s is an integer array of S + 1 >= 2 row offsets" % (what, name))
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
        raise ValueError("%s: %s must start at 0, not decrease, and end at the row count %d" % (what, name, total))
    return off


def _check_scans(what, scans, scan_off, calib):
    """-> (scans as a float32 tensor (rows, C), still where it was; scan_off int64 numpy)"""
    if not isinstance(calib, Calibration):
        raise ValueError("%s: calib is a Calibration" % what)
    if not torch.is_tensor(scans):
        scans = np.asarray(scans)
        if scans.dtype != np.float32:
            raise ValueError("%s: scans are float32, got %s" % (what, scans.dtype))
        scans = torch.from_numpy(np.ascontiguousarray(scans))
    if scans.dtype != torch.float32:
        raise ValueError("%s: scans are float32, got %s" % (what, scans.dtype))
    if scans.dim() != 2 or scans.shape[1] < 5:
        raise ValueError("%s: scans are (rows, C >= 5) = x y z RCS v_r ..., got %s" % (what, tuple(scans.shape)))
    if scans.shape[0] >= 2 ** 31:
        raise ValueError("%s: more than 2^31 - 1 rows" % what)
    scan_off = _offsets(what, scan_off, scans.shape[0])
    calib._check_scans(what, scan_off.size - 1)
    return scans, scan_off


def _i32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def _filter_args(scans, scan_off_d, calib, tcr, proj):
    S, C = scan_off_d.numel() - 1, scans.shape[1]
    return (S, C), (_lib.dev_ptr(scan_off_d, torch.int32), _lib.dev_ptr(tcr, torch.float64), _lib.dev_ptr(proj, torch.float64),
                    int(calib.per_scan is not None), calib.image_size[0], calib.image_size[1], calib.height[0], calib.height[1])


def _rows(n, *shape, dtype, device):
    """A tensor for n rows that has storage even when n = 0 (the entry points refuse NULL)."""
    return torch.empty((max(int(n), 1), *shape), dtype=dtype, device=device)[:int(n)]


def _scans_on(scans, dev):
    """The scans on the device; a call without any row still hands the entry points storage (they refuse NULL, and never read it)."""
    if scans.shape[0] == 0:
        return _rows(0, scans.shape[1], dtype=torch.float32, device=dev)
    return scans.to(dev).contiguous()


def count_scans(scans, scan_off, calib, device):
    """The input filter on every raw row (``cmf_prepare_count``) -> (keep (rows,) int32: the row's position among the kept rows of
    its scan, -1 for a dropped row; uv (rows,2) int32: the pixel of a kept row; count (S,) int32), all on the device."""
    scans, scan_off = _check_scans("count_scans", scans, scan_off, calib)
    dev = _need_gpu("count_scans", device)
    return _count(_scans_on(scans, dev), _i32(scan_off, dev), calib, dev)


def _count(scans, scan_off_d, calib, dev):
    tcr, proj = calib._device(dev)
    rows = scans.shape[0]
    keep, uv = _rows(rows, dtype=torch.int32, device=dev), _rows(rows, 2, dtype=torch.int32, device=dev)
    count = torch.empty(scan_off_d.numel() - 1, dtype=torch.int32, device=dev)
    (S, C), rest = _filter_args(scans, scan_off_d, calib, tcr, proj)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_prepare_count(S, C, _ptr(scans), *rest, _ptr(keep), _ptr(uv), _ptr(count), _lib.stream_ptr()),
                   "cmf_prepare_count")
    return keep, uv, count


def _ptr(t):
    """data pointer of a dense device tensor, also of the zero-row view of a one-row allocation"""
    if not t.is_cuda or not t.is_contiguous():
        raise RuntimeError("cmflow_amd.prepare: a dense GPU tensor is expected")
    return t.data_ptr() if t.numel() else t.untyped_storage().data_ptr()


def filter_scans(scans, scan_off, calib, device, nmax=None):
    """The network's input clouds from raw scans (``cmf_prepare_scans``): the filter's kept rows of every scan, in scan order, as
    ``pc`` (S,3,Nmax) = x y z, ``ft`` (S,3,Nmax) = v_r RCS RCS and ``n`` (S,) int32 -- ``forward_ragged``'s padded layout, padded
    slots exact zeros.  ``nmax=None``: Nmax is the largest kept count (one count pass and one device-to-host copy of the counts);
    ``nmax`` given: one launch, nothing read back, a scan with more kept rows is truncated (``n`` says so)."""
    scans, scan_off = _check_scans("filter_scans", scans, scan_off, calib)
    if nmax is not None and not 1 <= int(nmax) <= 32768:
        raise ValueError("filter_scans: nmax in [1, 32768]")
    dev = _need_gpu("filter_scans", device)
    scans, scan_off_d = _scans_on(scans, dev), _i32(scan_off, dev)
    if nmax is None:
        nmax = max(int(_count(scans, scan_off_d, calib, dev)[2].max()), 1)
    S, nmax = scan_off.size - 1, int(nmax)
    pc, ft = (torch.empty((S, 3, nmax), dtype=torch.float32, device=dev) for _ in range(2))
    n = torch.empty(S, dtype=torch.int32, device=dev)
    tcr, proj = calib._device(dev)
    (S, C), rest = _filter_args(scans, scan_off_d, calib, tcr, proj)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_prepare_scans(S, C, nmax, _ptr(scans), *rest, _ptr(pc), _ptr(ft), _ptr(n), _lib.stream_ptr()),
                   "cmf_prepare_scans")
    return pc, ft, n


def _check_pairs(what, pairs, S):
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 or not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError("%s: pairs is an integer array (F >= 1, 2) = scan of frame 1, scan of frame 2" % what)
    if pairs.min() < 0 or pairs.max() >= S:
        raise ValueError("%s: a pair names scan %d, outside the %d scans of the call" % (what, pairs.max() if pairs.max() >= S else pairs.min(), S))
    return pairs.astype(np.int64)


def pair_batch(pc, ft, n, pairs):
    """``filter_scans``' clouds paired up -> the dict ``CMFlow.forward_ragged`` takes: ``pc1, ft1`` = the clouds of ``pairs[:,0]``,
    ``pc2, ft2`` those of ``pairs[:,1]``, ``n1, n2`` their counts, ``interval`` (F,) = 0.10 (all on the clouds' device)."""
    if pc.dim() != 3 or pc.shape[1] != 3 or ft.shape != pc.shape or n.shape != (pc.shape[0],):
        raise ValueError("pair_batch: pc, ft (S,3,Nmax) and n (S,) as filter_scans returns them")
    pairs = _check_pairs("pair_batch", pairs, pc.shape[0])
    i1, i2 = (torch.from_numpy(np.ascontiguousarray(pairs[:, k])).to(pc.device) for k in (0, 1))
    return {"pc1": pc[i1].contiguous(), "pc2": pc[i2].contiguous(), "ft1": ft[i1].contiguous(), "ft2": ft[i2].contiguous(),
            "n1": n[i1].to(torch.int32), "n2": n[i2].to(torch.int32),
            "interval": torch.full((pairs.shape[0],), INTERVAL, dtype=torch.float32, device=pc.device)}


class SplitBuilder:
    """Builds a ``DeviceSplit`` from raw scans on the GPU.  ``mode``: ``"gt"`` -- the labels of the reference's val / test /
    train_anno samples (rigid flow from the ego-motion, the tracked boxes' flow on moving points) -- or ``"pseudo"`` -- those of its
    train samples (box flow on foreground, pixel coordinates, optical flow).  ``add`` takes one chunk of scans with the pairs formed
    among them and may be called any number of times; ``finish`` hands the packed tables to ``DeviceSplit``."""

    def __init__(self, calib, mode, device):
        if not isinstance(calib, Calibration):
            raise ValueError("SplitBuilder: calib is a Calibration")
        if mode not in MODES:
            raise ValueError("SplitBuilder: mode is 'gt' or 'pseudo', got %r" % (mode,))
        self.calib, self.mode, self.device = calib, mode, torch.device(device)
        self._chunks = []                       # (tab1, tab2, n1, n2, trans (F,16) float32, clip tags or None)

    def add(self, scans, scan_off, pairs, t_odom_camera, tracks=None, track_off=None, opt_flow=None, clip=None):
        """One chunk.  ``scans`` (rows, C >= 5) float32 with ``scan_off`` (S+1); ``pairs`` (F,2): indices into THIS call's scans;
        ``t_odom_camera`` (S,4,4) float64, the camera pose of every scan; ``tracks`` (rows,9) float64 with ``track_off`` (S+1): the
        box tracks of every scan (None: no boxes); ``opt_flow`` (mode 'pseudo'): one (height,width,2) float32 image or None per pair
        -- they are on the device for the duration of this call only, so size the chunks by them; ``clip`` (F,): an integer tag per
        pair, consecutive pairs of one tag form a clip of the split.  One device-to-host copy (the kept counts).
        A pair whose filtered cloud has more than ``DRAW_MAX_POINTS`` points is refused (ValueError)."""
        what = "SplitBuilder.add"
        calib = self.calib
        scans, scan_off = _check_scans(what, scans, scan_off, calib)
        S = scan_off.size - 1
        pairs = _check_pairs(what, pairs, S)
        F = pairs.shape[0]
        odom = np.asarray(t_odom_camera)
        if odom.shape != (S, 4, 4) or odom.dtype != np.float64:
            raise ValueError("%s: t_odom_camera is (S,4,4) float64, got %s %s" % (what, odom.shape, odom.dtype))
        if (tracks is None) != (track_off is None):
            raise ValueError("%s: tracks and track_off come together" % what)
        if tracks is not None:
            tracks = _tracks(what, tracks)
            track_off = _offsets(what, track_off, tracks.shape[0], "track_off")
            if track_off.size != S + 1:
                raise ValueError("%s: track_off has S + 1 = %d entries" % (what, S + 1))
        W, H = calib.image_size
        if opt_flow is not None:
            if self.mode != "pseudo":
                raise ValueError("%s: optical flow belongs to mode 'pseudo'" % what)
            if len(opt_flow) != F:
                raise ValueError("%s: opt_flow holds one image (or None) per pair" % what)
            for im in opt_flow:
                if im is not None and (tuple(im.shape) != (H, W, 2) or str(im.dtype).split(".")[-1] != "float32"):
                    raise ValueError("%s: a flow image is (%d,%d,2) float32, got %s %s" % (what, H, W, tuple(im.shape), im.dtype))
        if clip is not None:
            clip = np.asarray(clip)
            if clip.shape != (F,) or not np.issubdtype(clip.dtype, np.integer):
                raise ValueError("%s: clip is an integer tag per pair, (F,)" % what)
        # host: the 4 x 4 products of every pair (get_flow_samples.py:82-89) and its box records
        cal = [calib.scan(s) for s in range(S)] if calib.per_scan is not None else [calib] * S
        odom_radar = [odom[s] @ cal[s].t_camera_radar for s in range(S)]
        tinv, boxes = np.empty((F, 4, 4)), []
        none = np.zeros((0, 9))
        for f, (a, b) in enumerate(pairs):
            try:
                tinv[f] = np.linalg.inv(np.linalg.inv(odom_radar[a]) @ odom_radar[b])
            except np.linalg.LinAlgError:
                raise ValueError("%s: the pose of scan %d or %d is singular" % (what, a, b)) from None
            l1, l2 = (none if tracks is None else tracks[track_off[s]:track_off[s + 1]] for s in (a, b))
            boxes.append(match_boxes(l1, l2, cal[a], cal[b]))
        box_off = np.cumsum([0] + [b.shape[0] for b in boxes])
        boxes = np.concatenate(boxes + [np.zeros((1, BOX_DOUBLES))])       # never empty: the entry point refuses NULL

        dev = _need_gpu(what, self.device)
        scans, scan_off_d = _scans_on(scans, dev), _i32(scan_off, dev)
        keep, uv, count = _count(scans, scan_off_d, calib, dev)
        count = count.cpu().numpy().astype(np.int64)                       # the one device-to-host copy of the call
        n1, n2 = count[pairs[:, 0]], count[pairs[:, 1]]
        if max(n1.max(), n2.max()) > DRAW_MAX_POINTS:
            f = int(np.argmax(np.maximum(n1, n2) > DRAW_MAX_POINTS))
            raise ValueError("%s: pair %d has %d / %d points after the filter, more than the %d a DeviceSplit frame may hold"
                             % (what, f, n1[f], n2[f], DRAW_MAX_POINTS))
        off1, off2 = np.concatenate([[0], np.cumsum(n1)]), np.concatenate([[0], np.cumsum(n2)])
        if max(off1[-1], off2[-1]) >= 2 ** 31:
            raise ValueError("%s: more than 2^31 - 1 points in one chunk" % what)
        tab1 = _rows(off1[-1], 14, dtype=torch.float32, device=dev)
        tab2 = _rows(off2[-1], 6, dtype=torch.float32, device=dev)
        images, flow_ptr = [], None
        if opt_flow is not None and any(im is not None for im in opt_flow):
            images = [None if im is None else torch.as_tensor(im).to(dev).contiguous() for im in opt_flow]
            flow_ptr = torch.tensor([0 if im is None else im.data_ptr() for im in images], dtype=torch.int64).to(dev)
        d64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        held = (_i32(pairs, dev), _i32(off1, dev), _i32(off2, dev), d64(tinv.reshape(F, 16)), d64(boxes), _i32(box_off, dev))
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().cmf_prepare_pairs(
                F, scans.shape[1], _ptr(scans), _ptr(scan_off_d), _ptr(keep), _ptr(uv), *(_ptr(t) for t in held), MODES[self.mode],
                None if flow_ptr is None else _ptr(flow_ptr), W, H, _ptr(tab1), _ptr(tab2), _lib.stream_ptr()), "cmf_prepare_pairs")
            if images:
                torch.cuda.current_stream().synchronize()                  # the images go back to the allocator with this call
        self._chunks.append((tab1, tab2, n1, n2, torch.from_numpy(tinv.reshape(F, 16).astype(np.float32)), clip))

    def finish(self, min_points=(1, 1)):
        """-> (DeviceSplit, kept): the pairs of all chunks in the order they were added, without those whose filtered clouds hold
        fewer than ``min_points`` = (cloud 1, cloud 2) points (both at least 1: a DeviceSplit frame is not empty); ``kept``: the
        indices, in that order, of the pairs that remain.  With ``clip`` tags the split's ``clips`` are the runs of consecutive kept
        pairs of one tag: a clip is cut where the tag changes AND where a pair was dropped, so the frames of a clip are always
        consecutive pairs of the input (CMFlow-T carries its state along them)."""
        m1, m2 = (int(v) for v in min_points)
        if m1 < 1 or m2 < 1:
            raise ValueError("SplitBuilder.finish: min_points are at least 1 (a DeviceSplit frame is not empty)")
        if not self._chunks:
            raise ValueError("SplitBuilder.finish: nothing was added")
        dev = _need_gpu("SplitBuilder.finish", self.device)
        tagged = [c[5] is not None for c in self._chunks]
        if any(tagged) and not all(tagged):
            raise ValueError("SplitBuilder.finish: clip tags on some chunks only")
        n1, n2 = (np.concatenate([c[k] for c in self._chunks]) for k in (2, 3))
        ok = (n1 >= m1) & (n2 >= m2)
        kept = np.nonzero(ok)[0]
        if kept.size == 0:
            raise ValueError("SplitBuilder.finish: no pair has min_points = (%d, %d) points" % (m1, m2))
        tab1, tab2 = (torch.cat([c[k] for c in self._chunks]) for k in (0, 1))
        trans = torch.cat([c[4] for c in self._chunks])
        if kept.size < ok.size:                                            # drop the rows of the dropped pairs
            rows = lambda n: torch.from_numpy(np.repeat(ok, n)).to(dev)
            tab1, tab2, trans = tab1[rows(n1)], tab2[rows(n2)], trans[torch.from_numpy(ok)]
            n1, n2 = n1[ok], n2[ok]
        off1, off2 = np.concatenate([[0], np.cumsum(n1)]), np.concatenate([[0], np.cumsum(n2)])
        if max(off1[-1], off2[-1]) >= 2 ** 31:
            raise ValueError("SplitBuilder.finish: more than 2^31 - 1 points")
        clips = None
        if all(tagged):
            tags = np.concatenate([c[5] for c in self._chunks])
            cut = [0] + [i for i in range(1, kept.size) if kept[i] != kept[i - 1] + 1 or tags[kept[i]] != tags[kept[i - 1]]] + [kept.size]
            clips = [(a, b) for a, b in zip(cut[:-1], cut[1:])]
        split = DeviceSplit(tab1.contiguous(), tab2.contiguous(), _i32(off1, dev), _i32(off2, dev), trans.contiguous().to(dev),
                            torch.full((kept.size,), INTERVAL, dtype=torch.float32, device=dev), int(max(n1.max(), n2.max())), clips)
        return split, kept
