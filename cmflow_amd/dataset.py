"""Sample I/O: the View-of-Delft scene-flow sample format and its Datasets -- mirror of ``dataset/vod.py``
(vodDataset :14-137; format described in src/GETTING_STARTED.md:97-106), of ``dataset/vod_clip.py`` (vodClipDataset
:14-198, the mini-clip loader CMFlow-T trains on) and of ``extract_data_info`` / ``extract_data_info_clip``
(main_util.py:21-36, clip_util.py:81-96); ``collate_ragged`` / ``extract_data_info_ragged`` batch the evaluation-mode items (whole
frames of their own sizes) for ``CMFlow.forward_ragged``; ``DeviceSplit`` keeps a whole split on the device and draws each step's
batch there: resampled to ``num_points`` (``cmf_draw_batch``) or as whole frames in a ragged batch (``cmf_draw_frames``).

One sample = one JSON file ``<root>/<partition>/<clip>/<k>_*.json`` with
    pc1, pc2          [n][5]  x, y, z, RCS, v_r          (features fed to the net: [v_r, RCS, RCS], vod.py:62-63)
    gt_labels, pse_labels [n1][3], gt_mask, pse_mask [n1]  scene-flow labels / static masks (ground truth, pseudo)
    trans             [4][4]  frame-2 -> frame-1 ego transform (the loader inverts it, vod.py:92)
    opt_info          {opt_flow [n1][2], radar_u [n1], radar_v [n1]}   (training partitions only)
``__getitem__`` returns the reference's 11-tuple; in training mode clouds are resampled to ``args.num_points``
(duplicate padding below, random subset above; same numpy RNG call sequence as vod.py:95-121, so a seeded
run reproduces the reference's batches).  The calibration constants are those of dataset/vod_radar_calib.txt.
"""
import json
import math
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import synth


class vodDataset(Dataset):

    def __init__(self, args, root, partition='train', textio=None):
        self.npoints = args.num_points
        self.textio = textio
        self.res = {'r_res': 0.2, 'theta_res': 1.5 * np.pi / 180, 'phi_res': 1.5 * np.pi / 180}
        self.camera_projection_matrix = np.array(synth.CAMERA_PROJECTION, dtype=np.float32)
        self.t_camera_radar = np.array(synth.T_CAMERA_RADAR, dtype=np.float32)
        self.eval = args.eval
        self.partition = partition
        self.root = os.path.join(root, self.partition)
        self.interval = 0.10
        self.clips = sorted(os.listdir(self.root), key=lambda x: int(x.split("_")[1]))
        self.samples = []
        self.clips_info = []
        for clip in self.clips:
            clip_path = os.path.join(self.root, clip)
            files = sorted(os.listdir(clip_path), key=lambda x: int(x.split("_")[0]))
            if self.eval:
                self.clips_info.append({'clip_name': clip, 'index': [len(self.samples), len(self.samples) + len(files)]})
            if clip[:5] == 'delft':
                self.samples.extend(os.path.join(clip_path, f) for f in files)
        if self.textio is not None:
            self.textio.cprint(self.partition + ' : ' + str(len(self.samples)))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        with open(self.samples[index], 'rb') as fp:
            data = json.load(fp)
        return _sample_item(self, data)


def _resample(npoints, n):
    """vod.py:99-111 / vod_clip.py:183-191: keep all n points and pad with random duplicates, or draw a random subset."""
    if n < npoints:
        return np.append(np.arange(0, n), np.random.choice(n, npoints - n, replace=True))
    return np.random.choice(n, npoints, replace=False)


def _sample_item(ds, data):
    """One decoded sample -> the reference's 11-tuple (vod.py:54-124 = vod_clip.py:77-127: the two loaders share this body).
    Training (``not ds.eval``): both clouds resampled to ``ds.npoints`` -- cloud 1's index draw first, then cloud 2's, the numpy RNG
    call order of ``sample_points`` (vod_clip.py:181-193)."""
    d1 = np.array(data["pc1"]).astype('float32')
    d2 = np.array(data["pc2"]).astype('float32')
    pos_1, pos_2 = d1[:, 0:3], d2[:, 0:3]
    feature_1, feature_2 = d1[:, [4, 3, 3]], d2[:, [4, 3, 3]]
    if ds.partition in ('test', 'val', 'train_anno'):            # ground truth for evaluation
        labels = np.array(data["gt_labels"]).astype('float32')
        mask = np.array(data["gt_mask"])
        n1 = pos_1.shape[0]
        opt_flow = np.zeros((n1, 2)).astype('float32')
        radar_u, radar_v = np.zeros(n1).astype('float32'), np.zeros(n1).astype('float32')
    else:                                                         # pseudo labels + optical flow for training
        labels = np.array(data["pse_labels"]).astype('float32')
        mask = np.array(data["pse_mask"])
        info = data["opt_info"]
        opt_flow = np.array(info["opt_flow"]).astype('float32')
        radar_u = np.array(info["radar_u"]).astype('float32')
        radar_v = np.array(info["radar_v"]).astype('float32')
    trans = np.linalg.inv(np.array(data["trans"])).astype('float32')
    if not ds.eval:
        i1 = _resample(ds.npoints, pos_1.shape[0])
        i2 = _resample(ds.npoints, pos_2.shape[0])
        pos_1, pos_2 = pos_1[i1, :], pos_2[i2, :]
        feature_1, feature_2 = feature_1[i1, :], feature_2[i2, :]
        radar_u, radar_v, opt_flow = radar_u[i1], radar_v[i1], opt_flow[i1, :]
        labels, mask = labels[i1, :], mask[i1]
    return pos_1, pos_2, feature_1, feature_2, trans, labels, mask, ds.interval, radar_u, radar_v, opt_flow


class vodClipDataset(Dataset):
    """``dataset/vod_clip.py:14-198``.  Training (``args.eval`` false): item i is the i-th MINI-CLIP -- ``args.mini_clip_len``
    consecutive samples of one clip (clips cut into floor(len / mini_clip_len) mini-clips, the remainder dropped, :40-50) -- as
    eleven arrays with a leading ``(mini_clip_len, ...)`` axis (:131-170); every frame is resampled to ``args.num_points`` in
    file order (one numpy RNG stream).  Evaluation: item i is ONE frame (:69-74), ragged, in clip order, with ``clips_info``
    giving each clip's [first, last) frame range (:34-39)."""

    def __init__(self, args, root, partition='train', textio=None):
        self.npoints = args.num_points
        self.textio = textio
        self.res = {'r_res': 0.2, 'theta_res': 1.5 * np.pi / 180, 'phi_res': 1.5 * np.pi / 180}
        self.camera_projection_matrix = np.array(synth.CAMERA_PROJECTION, dtype=np.float32)
        self.t_camera_radar = np.array(synth.T_CAMERA_RADAR, dtype=np.float32)
        self.eval = args.eval
        self.partition = partition
        self.root = os.path.join(root, self.partition)
        self.interval = 0.10
        self.mini_clip_len = args.mini_clip_len
        self.update_len = args.update_len
        self.clips = sorted(os.listdir(self.root), key=lambda x: int(x.split("_")[1]))
        self.mini_samples = []
        self.samples = []
        self.clips_info = []
        self.mini_clips_info = []
        for clip in self.clips:
            clip_path = os.path.join(self.root, clip)
            files = sorted(os.listdir(clip_path), key=lambda x: int(x.split("/")[-1].split("_")[0]))
            if self.eval:
                self.clips_info.append({'clip_name': clip, 'index': [len(self.samples), len(self.samples) + len(files)]})
                self.samples.extend(os.path.join(clip_path, f) for f in files)
            else:
                for i in range(int(np.floor(len(files) / self.mini_clip_len))):
                    mini = [os.path.join(clip_path, files[i * self.mini_clip_len + j]) for j in range(self.mini_clip_len)]
                    self.samples.extend(mini)
                    self.mini_samples.append(mini)
        if self.textio is not None:
            if self.eval:
                self.textio.cprint(self.partition + ' : ' + str(len(self.samples)) + ' frames')
            else:
                self.textio.cprint(self.partition + ' : ' + str(len(self.mini_samples)) + ' mini_clips')

    def __len__(self):
        return len(self.samples) if self.eval else len(self.mini_samples)

    def get_sample_item(self, data):
        return _sample_item(self, data)

    def get_clip_item(self, index):
        mini = self.mini_samples[index]
        L, n = self.mini_clip_len, self.npoints
        z = lambda *shape: np.zeros(shape).astype('float32')
        out = (z(L, n, 3), z(L, n, 3), z(L, n, 3), z(L, n, 3), z(L, 4, 4), z(L, n, 3), z(L, n), z(L), z(L, n), z(L, n), z(L, n, 2))
        for i, path in enumerate(mini):
            with open(path, 'rb') as fp:
                item = _sample_item(self, json.load(fp))
            for dst, v in zip(out, item):
                dst[i] = v
        return out

    def __getitem__(self, index):
        if not self.eval:
            return self.get_clip_item(index)
        with open(self.samples[index], 'rb') as fp:
            return _sample_item(self, json.load(fp))


def extract_data_info(data, device="cuda"):
    """main_util.py:21-36: a collated batch -> model-layout device tensors
    (pc1, pc2, ft1, ft2 (B,3,N); trans (B,4,4); gt (B,N,3); mask (B,N); interval (B); radar_u/v (B,N); opt_flow (B,N,2))."""
    pc1, pc2, ft1, ft2, trans, gt, mask, interval, radar_u, radar_v, opt_flow = data
    cm = lambda t: torch.as_tensor(t).to(device).transpose(2, 1).contiguous()
    fl = lambda t: torch.as_tensor(t).to(device).float()
    return (cm(pc1), cm(pc2), cm(ft1), cm(ft2), fl(trans), fl(gt), fl(mask), fl(interval), fl(radar_u), fl(radar_v),
            fl(opt_flow))


def extract_data_info_clip(seq_data, idx, device="cuda"):
    """clip_util.py:81-96: frame ``idx`` of a collated mini-clip batch -> the tuple of extract_data_info."""
    return extract_data_info(tuple(t[:, idx] for t in seq_data), device=device)


def collate_ragged(items):
    """``collate_fn`` for the evaluation-mode items of vodDataset / vodClipDataset (the reference's 11-tuples, whole frames of their
    own sizes: dataset/vod.py:92-111 resamples for training only, main.py:203 therefore tests with batch_size = 1): B items -> the
    same eleven arrays with a leading batch axis, per-point arrays padded to ``Nmax1 = max(n1)`` (cloud 1 and everything indexed by
    its points) / ``Nmax2 = max(n2)`` (cloud 2), plus ``n1``, ``n2`` (B,) int32.  Padding repeats the sample's FIRST point (and its
    label / mask / radar_u / radar_v / opt_flow row): coordinates stay in range and an accidental read finds a real point.
    -> (pc1 (B,Nmax1,3), pc2 (B,Nmax2,3), ft1, ft2, trans (B,4,4), labels (B,Nmax1,3), mask (B,Nmax1), interval (B),
        radar_u (B,Nmax1), radar_v (B,Nmax1), opt_flow (B,Nmax1,2), n1, n2) as torch CPU tensors."""
    if len(items) == 0:
        raise ValueError("collate_ragged: empty batch")
    n1 = np.array([np.asarray(it[0]).shape[0] for it in items], dtype=np.int32)
    n2 = np.array([np.asarray(it[1]).shape[0] for it in items], dtype=np.int32)
    if n1.min() < 1 or n2.min() < 1:
        raise ValueError("collate_ragged: a frame without points")
    m1, m2 = int(n1.max()), int(n2.max())

    def pad(k, nmax, dtype=np.float32):
        out = []
        for it in items:
            a = np.asarray(it[k]).astype(dtype)
            out.append(np.concatenate([a, np.repeat(a[:1], nmax - a.shape[0], axis=0)], axis=0))
        return torch.from_numpy(np.stack(out))

    fixed = lambda k: torch.from_numpy(np.stack([np.asarray(it[k], dtype=np.float32) for it in items]))
    return (pad(0, m1), pad(1, m2), pad(2, m1), pad(3, m2), fixed(4), pad(5, m1), pad(6, m1), fixed(7), pad(8, m1), pad(9, m1),
            pad(10, m1), torch.from_numpy(n1), torch.from_numpy(n2))


def extract_data_info_ragged(data, device="cuda"):
    """extract_data_info (main_util.py:21-36) for a ``collate_ragged`` batch -> model-layout device tensors
    (pc1, ft1 (B,3,Nmax1); pc2, ft2 (B,3,Nmax2); trans (B,4,4); gt (B,Nmax1,3); mask (B,Nmax1); interval (B); radar_u/v (B,Nmax1);
    opt_flow (B,Nmax1,2); n1, n2 (B,) int32): the tuple of extract_data_info followed by the two count tensors."""
    return (*extract_data_info(data[:11], device=device), torch.as_tensor(data[11]).to(device=device, dtype=torch.int32),
            torch.as_tensor(data[12]).to(device=device, dtype=torch.int32))


def as_batch_dict(info):
    """The tuple of extract_data_info as the dict TrainStep / RadarFlowLoss take (train partitions: mask = fg_mask)."""
    keys = ("pc1", "pc2", "ft1", "ft2", "gt_trans", "flow_label", "fg_mask", "interval", "radar_u", "radar_v", "opt_flow")
    return dict(zip(keys, info))


def as_batch_dict_ragged(info):
    """The tuple of extract_data_info_ragged as the dict losses.make_labels_ragged / RadarFlowLoss.forward_ragged take: the keys of
    as_batch_dict plus the count tensors ``n1``, ``n2``."""
    d = as_batch_dict(info[:11])
    d["n1"], d["n2"] = info[11], info[12]
    return d


class Augment(tuple):
    """The settings of the label-consistent augmentation (``augment_batch``): ``yaw_deg``, the largest
    rotation about the sensor's z axis in degrees (0 <= yaw_deg < 180; 0: no rotation), and ``mirror``, whether a slot's y axis is
    mirrored with probability 1/2.  Immutable; it IS the tuple ``(yaw_deg, mirror)`` -- it compares equal to it, and ``tuple(a)`` is
    what a resume point stores.  A negative, non-finite or >= 180 ``yaw_deg`` raises ValueError."""
    __slots__ = ()

    def __new__(cls, yaw_deg=0.0, mirror=False):
        try:
            yaw = float(yaw_deg)
        except (TypeError, ValueError):
            raise ValueError("Augment: yaw_deg = %r is not a number" % (yaw_deg,))
        if not (math.isfinite(yaw) and 0.0 <= yaw < 180.0):
            raise ValueError("Augment: yaw_deg = %r; a finite number of degrees in [0, 180)" % (yaw_deg,))
        return tuple.__new__(cls, (yaw, bool(mirror)))

    def __getnewargs__(self):
        return (self[0], self[1])

    yaw_deg = property(lambda self: self[0])
    mirror = property(lambda self: self[1])

    @property
    def tan_half_max(self):
        """tan(yaw_max / 2), the one number cmf_augment_batch takes for the angle (computed here, once, in float64)."""
        return math.tan(math.radians(self[0]) / 2.0)

    def __repr__(self):
        return "Augment(yaw_deg=%r, mirror=%r)" % (self[0], self[1])


def augment_batch(batch, augment, seed, aug_draw, slot0=0, t_camera_radar=None):
    """One transform per slot of an already drawn batch, IN PLACE, in one launch (cmf_augment_batch): a rotation about the sensor's z
    axis by an angle within ``augment.yaw_deg`` after, with ``augment.mirror``, a mirror of the y axis in half of the slots -- the
    transforms under which every label this model trains on stays consistent.  ``batch``: any batch dict on
    the GPU -- ``as_batch_dict``, ``as_batch_dict_ragged``, a ``DeviceSplit.draw`` or ``draw_frames`` result; its ``pc1``, ``pc2``,
    ``flow_label`` and ``gt_trans`` are rewritten (contiguous float32 tensors), everything else -- features, masks, interval, pixel
    measurements, counts -- is invariant and stays.  Padded positions of a ragged batch are transformed like any other.
    Slot s's transform depends on (seed, aug_draw, slot0 + s) only: Philox4x32-10 keyed by (seed, aug_draw), counter
    (slot0 + s, 2, 0, 0) -- a stream the sampling of ``draw`` never touches, so ``aug_draw`` may be the draw id itself.
    ``t_camera_radar``: the shared (4,4) radar-to-camera transform the loss object holds (default ``synth.T_CAMERA_RADAR``, as
    TrainStep's); a tensor on the batch's device is used as it is, anything else is copied there.
    Adds ``batch["aug"]`` (B,4,4), the slot's transform, and ``batch["t_camera_radar"]`` (B,4,4), the slot's calibration, which
    ``TrainStep`` hands to ``RadarFlowLoss``; returns the batch.  CPU tensors raise: there is no fallback."""
    from . import _lib
    if not isinstance(augment, Augment):
        raise TypeError("augment_batch: augment is a dataset.Augment (got %s)" % type(augment).__name__)
    pc1, pc2, fl, gt = (batch[k] for k in ("pc1", "pc2", "flow_label", "gt_trans"))
    if not pc1.is_cuda:
        raise RuntimeError("augment_batch: the batch is on %s; batches are augmented on the GPU only (no CPU fallback)" % pc1.device)
    if pc1.dim() != 3 or pc2.dim() != 3 or pc1.shape[1] != 3 or pc2.shape[:2] != pc1.shape[:2] or \
            fl.shape != (pc1.shape[0], pc1.shape[2], 3) or gt.shape != (pc1.shape[0], 4, 4):
        raise ValueError("augment_batch: pc1 (B,3,N1), pc2 (B,3,N2), flow_label (B,N1,3), gt_trans (B,4,4)")
    B, _, N1 = pc1.shape
    N2 = pc2.shape[2]
    dev = pc1.device
    tcr = synth.T_CAMERA_RADAR if t_camera_radar is None else t_camera_radar
    tcr = torch.as_tensor(tcr, dtype=torch.float32).to(dev).contiguous()
    if tcr.shape != (4, 4):
        raise ValueError("augment_batch: t_camera_radar is the shared (4,4) matrix")
    aug = torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
    calib = torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
    fp = lambda t: _lib.dev_ptr(t, torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_augment_batch(
            int(slot0), B, N1, N2, int(seed) & _MASK64, int(aug_draw) & _MASK64, augment.tan_half_max, int(augment.mirror), fp(tcr),
            fp(pc1), fp(pc2), fp(fl), fp(gt), fp(aug), fp(calib), _lib.stream_ptr()), "cmf_augment_batch")
    batch["aug"], batch["t_camera_radar"] = aug, calib
    return batch


DRAW_MAX_POINTS = 16384          # CMF_DRAW_MAX_POINTS of include/cmflow_hip.h: the per-frame cap of cmf_draw_batch (sort keys in LDS)
_MASK64 = (1 << 64) - 1


def ragged_batches(n1, order, batch_size, bucket=1, drop_last=False):
    """Cut a frame order into the frame-id lists of ragged batches (host only).  ``n1``: cloud-1 point count per frame id;
    ``order``: frame ids in visiting order.  ``bucket = 1``: consecutive batches of ``order``.  ``bucket = k > 1``: ``order`` is cut
    into windows of ``k * batch_size`` frames, every window is sorted by (n1, frame id) and then cut into consecutive batches -- a
    ragged batch pays for its largest frame, and among the ways to split a window into groups of equal size, consecutive groups of
    the sorted window have the smallest sum of maxima.  ``drop_last`` drops the tail of ``order`` that does not fill a batch (the
    frames a DataLoader with drop_last would drop), before any sorting."""
    batch_size, bucket = int(batch_size), int(bucket)
    if batch_size < 1 or bucket < 1:
        raise ValueError("ragged_batches: batch_size and bucket are at least 1")
    order = [int(f) for f in order]
    if drop_last:
        order = order[:len(order) // batch_size * batch_size]
    out = []
    for w in range(0, len(order), bucket * batch_size):
        window = order[w:w + bucket * batch_size]
        if bucket > 1:
            window = sorted(window, key=lambda f: (int(n1[f]), f))
        out += [window[i:i + batch_size] for i in range(0, len(window), batch_size)]
    return out


def _rank_of(what, rank, world):
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("%s: rank %d of a world of %d" % (what, rank, world))
    return rank, world


def shard_batches(batches, rank, world):
    """Rank ``rank``'s contiguous slice of every GLOBAL frame-id list (host only) -- ``dp.shard_batch``'s rule, DataParallel's
    scatter, for id lists.  A list whose length is not a multiple of ``world`` is split as evenly as possible: the first
    ``len % world`` ranks get one id more, so a rank's share may be empty (a list shorter than ``world``).  The shares of the ranks
    0 .. world-1, in that order, concatenate to the list."""
    rank, world = _rank_of("shard_batches", rank, world)
    out = []
    for b in batches:
        q, r = divmod(len(b), world)
        first = rank * q + min(rank, r)
        out.append([int(f) for f in b[first:first + q + (rank < r)]])
    return out


def sweep_shares(count, batch_size, rank=0, world=1):
    """The bookkeeping of an in-order pass over ``count`` things (frames, mini-clips) in global batches of
    ``G = world * batch_size``, the short last batch kept (host only) -> (nbatches, shares): ``nbatches = ceil(count / G)``, and one
    ``(b, first, last)`` per global batch b of which rank ``rank`` holds something -- its rows ``[b * G + rank * batch_size, ...)`` cut
    at ``count``.  A rank whose share of the last global batch is empty has no entry for it; the shares of the ranks 0 .. world-1
    of one b, in that order, are that global batch."""
    rank, world = _rank_of("sweep_shares", rank, world)
    count, batch_size = int(count), int(batch_size)
    if batch_size < 1:
        raise ValueError("sweep_shares: batch_size is at least 1")
    G = world * batch_size
    nbatches = -(-count // G)
    shares = []
    for b in range(nbatches):
        first = b * G + rank * batch_size
        last = min(first + batch_size, count)
        if first < last:
            shares.append((b, first, last))
    return nbatches, shares


def mini_clip_starts(clips, mini_clip_len):
    """The first frame of every mini-clip as vodClipDataset cuts them (vod_clip.py:40-50): floor(len / L) per clip, in clip order,
    the remainder of a clip dropped.  ``clips``: [first, last) frame range per clip."""
    L = int(mini_clip_len)
    if L < 1:
        raise ValueError("mini_clip_starts: mini_clip_len is at least 1")
    return [int(a) + i * L for a, b in clips for i in range((int(b) - int(a)) // L)]


SPLIT_FORMAT_VERSION = 1         # DeviceSplit.save / load


def padding_share(n1, batches):
    """The share of padded cloud-1 positions over the batches of ``ragged_batches``: 1 - sum n1 / sum (B * Nmax1)."""
    valid = sum(int(n1[f]) for b in batches for f in b)
    padded = sum(len(b) * max(int(n1[f]) for f in b) for b in batches)
    return 1.0 - valid / padded


class DeviceSplit:
    """A split decoded once and kept on the device as whole frames; every step's batch is then produced there by one kernel --
    ``cmf_draw_batch`` (``draw``, ``epoch``, ``epoch_clips``: frame choice, the reference's per-frame resampling to ``npoints``, the
    layout of extract_data_info) or ``cmf_draw_frames`` (``draw_frames``, ``epoch_ragged``, ``sweep``: the frames themselves as a
    ragged batch, collate_ragged's padding, the layout of extract_data_info_ragged) -- no workers, no per-step host work, no
    per-step host-to-device copy (``draw_frames`` with ids given on the host copies those ids; the iterators send an epoch's ids
    once).  ``sweep_resampled`` / ``sweep_clips`` are the validation iterators of a training run (every frame / mini-clip in order,
    resampled); ``save`` / ``load`` keep the packed split in one file.

    Packed CSR-style over F frames: ``tab1`` (sum n1, 14) float32 per point of cloud 1 = xyz 3 | features 3 | label 3 | mask |
    radar_u | radar_v | opt_flow 2; ``tab2`` (sum n2, 6) = xyz 3 | features 3; ``off1``, ``off2`` (F+1) int32; ``trans`` (F,16);
    ``interval`` (F); ``clips``: [first, last) frame range of every clip (from_dataset on a vodClipDataset), else None.
    Packing is host code and works on any device; drawing needs the GPU (no CPU fallback)."""

    KEYS = ("pc1", "pc2", "ft1", "ft2", "gt_trans", "flow_label", "fg_mask", "interval", "radar_u", "radar_v", "opt_flow")

    def __init__(self, tab1, tab2, off1, off2, trans, interval, max_points, clips=None):
        self.tab1, self.tab2, self.off1, self.off2, self.trans, self.interval = tab1, tab2, off1, off2, trans, interval
        self.max_points = int(max_points)
        self.clips = clips
        self.device = tab1.device
        self._counts = None

    @property
    def counts_host(self):
        """(n1, n2): the point counts of every frame as two numpy int32 arrays, from off1 / off2 -- brought to the host on first use
        (one device-to-host copy per split) and kept."""
        if self._counts is None:
            off = torch.stack((self.off1, self.off2)).cpu().numpy()
            self._counts = (np.diff(off[0]).astype(np.int32), np.diff(off[1]).astype(np.int32))
        return self._counts

    def __len__(self):
        return self.off1.numel() - 1

    def to(self, device):
        """The same split on another device (pack once on the host, keep a copy per GPU)."""
        return DeviceSplit(*(t.to(device) for t in (self.tab1, self.tab2, self.off1, self.off2, self.trans, self.interval)),
                           self.max_points, self.clips)

    @classmethod
    def from_items(cls, items, device, clips=None):
        """items: whole-frame 11-tuples exactly as ``_sample_item`` returns them when ``ds.eval`` is true (a training partition
        opened with ``args.eval = True`` gives pseudo labels and optical-flow columns, not resampled)."""
        items = list(items)
        if len(items) == 0:
            raise ValueError("DeviceSplit: no frames")
        t1, t2, tr, iv = [], [], [], []
        for k, it in enumerate(items):
            pos1, pos2, f1, f2, trans, labels, mask, interval, ru, rv, opt = (np.asarray(v, dtype=np.float32) for v in it)
            n1, n2 = pos1.shape[0], pos2.shape[0]
            if n1 < 1 or n2 < 1:
                raise ValueError("DeviceSplit: frame %d has no points" % k)
            if max(n1, n2) > DRAW_MAX_POINTS:
                raise ValueError("DeviceSplit: frame %d has %d points, more than the %d cmf_draw_batch sorts in one workgroup's LDS"
                                 % (k, max(n1, n2), DRAW_MAX_POINTS))
            t1.append(np.concatenate([pos1, f1, labels, mask[:, None], ru[:, None], rv[:, None], opt], axis=1))
            t2.append(np.concatenate([pos2, f2], axis=1))
            tr.append(trans.reshape(16))
            iv.append(interval)
        c1, c2 = np.cumsum([0] + [t.shape[0] for t in t1]), np.cumsum([0] + [t.shape[0] for t in t2])
        if max(c1[-1], c2[-1]) >= 2 ** 31:
            raise ValueError("DeviceSplit: more than 2^31 - 1 points")
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        return cls(to(np.concatenate(t1), np.float32), to(np.concatenate(t2), np.float32), to(c1, np.int32), to(c2, np.int32),
                   to(np.stack(tr), np.float32), to(np.array(iv), np.float32),
                   max(int(np.diff(c1).max()), int(np.diff(c2).max())), clips)

    @classmethod
    def from_dataset(cls, ds, device):
        """One pass over a vodDataset / vodClipDataset opened with ``args.eval = True`` (whole frames); the clip dataset's
        ``clips_info`` gives each clip's frame range."""
        if not ds.eval:
            raise ValueError("DeviceSplit.from_dataset: open the dataset with args.eval = True (whole frames, not resampled)")
        clips = [tuple(c["index"]) for c in ds.clips_info] if isinstance(ds, vodClipDataset) else None
        return cls.from_items((ds[i] for i in range(len(ds))), device, clips)

    shard_batches = staticmethod(shard_batches)

    def _calibration(self, t_camera_radar):
        """The shared radar-to-camera matrix of an augmented iterator on the split's device: copied once per iterator, not per step."""
        t = synth.T_CAMERA_RADAR if t_camera_radar is None else t_camera_radar
        return torch.as_tensor(t, dtype=torch.float32).to(self.device).contiguous()

    def draw(self, frames, npoints, seed, draw, slot0=0, augment=None, aug_draw=None, t_camera_radar=None):
        """One batch: slot s holds frame ``frames[s]`` resampled to ``npoints`` as ``dataset._resample`` does (n < npoints: all n
        points in order, then uniform duplicates; n >= npoints: a uniformly random subset in uniformly random order), generator
        Philox4x32-10 keyed by (seed, draw) -- a slot's result depends on (seed, draw, slot, frame) only.  ``slot0``: the batch is
        slots ``slot0 .. slot0 + B - 1`` of a larger (global) one -- row s is then, bit for bit, row ``slot0 + s`` of the draw of
        that whole batch, which is how a data-parallel rank draws its share (``cmf_draw_batch_at``).
        ``augment`` (a ``dataset.Augment``; None: off, nothing more is launched): the drawn batch goes through
        ``augment_batch(batch, augment, seed, aug_draw, slot0, t_camera_radar)`` -- ``aug_draw`` defaults to ``draw`` -- and gains
        ``aug`` and ``t_camera_radar``; bit for bit what the two calls give one after the other.
        -> the dict of as_batch_dict plus ``idx1``, ``idx2`` (B, npoints) int32, the drawn point of every position."""
        from . import _lib
        if not self.tab1.is_cuda:
            raise RuntimeError("DeviceSplit.draw: the split is on %s; batches are drawn on the GPU only (no CPU fallback)" % self.device)
        frames = torch.as_tensor(frames, dtype=torch.int32, device=self.device).contiguous()
        B, N = int(frames.numel()), int(npoints)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        out = dict(zip(self.KEYS, (f32(B, 3, N), f32(B, 3, N), f32(B, 3, N), f32(B, 3, N), f32(B, 4, 4), f32(B, N, 3), f32(B, N), f32(B),
                                   f32(B, N), f32(B, N), f32(B, N, 2))))
        out["idx1"] = torch.empty((B, N), dtype=torch.int32, device=self.device)
        out["idx2"] = torch.empty((B, N), dtype=torch.int32, device=self.device)
        fp, ip = (lambda t: _lib.dev_ptr(t, torch.float32)), (lambda t: _lib.dev_ptr(t, torch.int32))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().cmf_draw_batch_at(
                int(slot0), B, N, len(self), self.max_points, fp(self.tab1), fp(self.tab2), ip(self.off1), ip(self.off2), fp(self.trans),
                fp(self.interval), ip(frames), int(seed) & _MASK64, int(draw) & _MASK64, *(fp(out[k]) for k in self.KEYS),
                ip(out["idx1"]), ip(out["idx2"]), _lib.stream_ptr()), "cmf_draw_batch_at")
        if augment is not None:
            augment_batch(out, augment, seed, draw if aug_draw is None else aug_draw, slot0, t_camera_radar)
        return out

    def _order(self, count, seed, epoch):
        g = torch.Generator(device=self.device)
        g.manual_seed((int(seed) * 0x9E3779B97F4A7C15 + int(epoch)) & _MASK64)
        return torch.randperm(count, generator=g, device=self.device)

    @staticmethod
    def _equal_steps(what, rank, world, drop_last=True):
        rank, world = _rank_of(what, rank, world)
        if world > 1 and not drop_last:
            raise ValueError("%s: drop_last=False at world = %d -- every step ends in a collective, so the ranks take the same number "
                             "of steps and the frames that do not fill a global batch are dropped" % (what, world))
        return rank, world

    def epoch(self, batch_size, npoints, seed, epoch, drop_last=True, rank=0, world=1, augment=None, t_camera_radar=None):
        """One pass over the frames in an order shuffled on the device (torch.randperm, generator seeded by (seed, epoch)): yields
        one batch dict per step; ``draw`` = epoch * steps_per_epoch + step.
        Data parallel (``rank`` of ``world`` processes, ``batch_size`` per rank): the order is the same on every rank, a step is the
        global batch of ``G = world * batch_size`` frames, ``steps = F // G``, and rank r draws rows ``r * batch_size ..`` of it with
        ``slot0 = r * batch_size`` -- the ranks' batches concatenated are, bit for bit, the batches of ``epoch(G, ...)`` in one
        process, whatever ``world`` is.  ``drop_last=False`` is refused at world > 1 (ValueError).
        ``augment`` (a ``dataset.Augment``; None: off): every batch is augmented (``augment_batch``) with ``aug_draw`` = the step's
        draw id and the rank's ``slot0``, so the ranks' batches still concatenate to the single-process batch.  ``t_camera_radar``:
        the shared matrix of the loss object the batches go to (default ``synth.T_CAMERA_RADAR``, TrainStep's default)."""
        rank, world = self._equal_steps("DeviceSplit.epoch", rank, world, drop_last)
        tcr = self._calibration(t_camera_radar) if augment is not None else None
        F, G, at = len(self), world * batch_size, rank * batch_size
        steps = F // G if drop_last else -(-F // G)
        order = self._order(F, seed, epoch).to(torch.int32)
        for step in range(steps):
            yield self.draw(order[step * G + at:step * G + at + batch_size], npoints, seed, epoch * steps + step, at, augment, None, tcr)

    def epoch_clips(self, batch_size, mini_clip_len, npoints, seed, epoch, rank=0, world=1, augment=None, t_camera_radar=None):
        """CMFlow-T: mini-clips cut as vodClipDataset cuts them (floor(len / L) per clip, remainder dropped), their order
        shuffled; every step yields a list of L batch dicts -- frame j of every mini-clip of the batch -- which TrainStep takes
        frame by frame between reset_clip() calls.  The last step holds the mini-clips left over (fewer than batch_size).
        Data parallel (``rank`` of ``world``, ``batch_size`` per rank): as in ``epoch`` -- the same shuffled starts on every rank,
        global batches of ``world * batch_size`` mini-clips, rank r's rows drawn with ``slot0 = r * batch_size``; at world > 1 the
        mini-clips that do not fill a global batch are dropped (equal steps on every rank), at world = 1 the short last step stays.
        ``augment`` / ``t_camera_radar`` as in ``epoch``, with ``aug_draw = epoch * steps + step`` for ALL L frames of a step: a
        mini-clip keeps ONE transform across its frames (their ``aug`` are equal), because CMFlow-T's recurrent feature is carried
        from frame to frame and must see one scene."""
        rank, world = _rank_of("DeviceSplit.epoch_clips", rank, world)
        tcr = self._calibration(t_camera_radar) if augment is not None else None
        if self.clips is None:
            raise ValueError("DeviceSplit.epoch_clips: no clip ranges (build the split with from_dataset on a vodClipDataset)")
        L = int(mini_clip_len)
        first = mini_clip_starts(self.clips, L)
        if not first:
            return
        first = self._ids_to_device(first)[self._order(len(first), seed, epoch)]
        G, at = world * batch_size, rank * batch_size
        steps = first.numel() // G if world > 1 else -(-first.numel() // G)
        for step in range(steps):
            f0 = first[step * G + at:step * G + at + batch_size]
            yield [self.draw(f0 + j, npoints, seed, (epoch * steps + step) * L + j, at, augment, epoch * steps + step, tcr) for j in range(L)]

    def _ids_to_device(self, ids):
        """A host list of frame ids as an int32 device tensor: one asynchronous copy from pinned memory (the host does not wait)."""
        ids = torch.tensor(ids, dtype=torch.int32)
        return ids.pin_memory().to(self.device, non_blocking=True) if self.tab1.is_cuda else ids.to(self.device)

    # ---- every frame in index order, resampled: the validation iterators (main.py:206-208) ------------------------------------------
    def sweep_resampled(self, batch_size, npoints, seed, epoch=0, rank=0, world=1):
        """The reference's validation loader (main.py:206-208: the training-mode dataset on 'val', ``val_batch_size`` frames per batch,
        shuffle off, drop_last off): frames 0 .. F-1 in index order, every one resampled to ``npoints`` by ``draw``; the short last
        batch is kept.  Yields the dict of ``draw`` plus ``frames`` ((B,) int32 on the device), the frame of every row.
        ``sweep_shares`` does the bookkeeping: global batch b of ``G = world * batch_size`` frames is drawn with
        ``draw = epoch * nbatches + b`` and rank ``rank`` draws its rows ``b * G + rank * batch_size ..`` with
        ``slot0 = rank * batch_size`` -- the ranks' batches concatenated are, bit for bit, the batches of
        ``sweep_resampled(G, ...)`` in one process.  No collective belongs to a step, so the ranks may take different numbers of
        steps: a rank whose share of the last global batch is empty yields nothing for it.  Nothing is copied to or from the
        host."""
        rank, world = _rank_of("DeviceSplit.sweep_resampled", rank, world)
        self._need_gpu("sweep_resampled")
        nbatches, shares = sweep_shares(len(self), batch_size, rank, world)
        ids = torch.arange(len(self), dtype=torch.int32, device=self.device)
        for b, first, last in shares:
            batch = self.draw(ids[first:last], npoints, seed, int(epoch) * nbatches + b, rank * int(batch_size))
            batch["frames"] = ids[first:last]
            yield batch

    def sweep_clips(self, batch_size, mini_clip_len, npoints, seed, epoch=0, rank=0, world=1):
        """CMFlow-T's validation loader (vodClipDataset in training mode on 'val', shuffle off, drop_last off): the mini-clips of
        ``epoch_clips`` (``mini_clip_starts``) in order, ``batch_size`` per step, the short last step kept.  Every step yields a list
        of L batch dicts -- frame j of every mini-clip of the step, each as ``sweep_resampled`` yields them; frame j of
        global step s is drawn with ``draw = (epoch * steps + s) * L + j``.  ``rank`` / ``world`` as in ``sweep_resampled``, over
        mini-clips.  The starts go to the device in one asynchronous copy before the first step."""
        rank, world = _rank_of("DeviceSplit.sweep_clips", rank, world)
        if self.clips is None:
            raise ValueError("DeviceSplit.sweep_clips: no clip ranges (build the split with from_dataset on a vodClipDataset)")
        self._need_gpu("sweep_clips")
        L = int(mini_clip_len)
        starts = mini_clip_starts(self.clips, L)
        steps, shares = sweep_shares(len(starts), batch_size, rank, world)
        if not shares:
            return
        starts = self._ids_to_device(starts)
        for s, first, last in shares:
            step = []
            for j in range(L):
                frames = starts[first:last] + j
                step.append(self.draw(frames, npoints, seed, (int(epoch) * steps + s) * L + j, rank * int(batch_size)))
                step[-1]["frames"] = frames
            yield step

    # ---- one file per split ---------------------------------------------------------------------------------------------------------
    def save(self, path):
        """The packed split in one ``torch.save`` file (tensors on the CPU): a run, or a resumed one, need not decode a split's JSON
        files again.  Written to a temporary name and renamed, so a killed process leaves no half file under ``path``."""
        rec = {"format": "cmflow_amd.DeviceSplit", "version": SPLIT_FORMAT_VERSION, "max_points": self.max_points,
               "clips": None if self.clips is None else [(int(a), int(b)) for a, b in self.clips]}
        for k in ("tab1", "tab2", "off1", "off2", "trans", "interval"):
            rec[k] = getattr(self, k).detach().cpu()
        tmp = "%s.tmp%d" % (path, os.getpid())
        torch.save(rec, tmp)
        os.replace(tmp, path)

    @classmethod
    def load(cls, path, device):
        """The split ``save`` wrote, on ``device``.  A file of another format version (or not of this format) raises ValueError."""
        rec = torch.load(path, map_location="cpu")
        if not isinstance(rec, dict) or rec.get("format") != "cmflow_amd.DeviceSplit" or rec.get("version") != SPLIT_FORMAT_VERSION:
            raise ValueError("DeviceSplit.load: %s is not a DeviceSplit file of format version %d (found %r)"
                             % (path, SPLIT_FORMAT_VERSION, rec.get("version") if isinstance(rec, dict) else type(rec).__name__))
        clips = None if rec["clips"] is None else [tuple(c) for c in rec["clips"]]
        return cls(*(rec[k].to(device) for k in ("tab1", "tab2", "off1", "off2", "trans", "interval")), rec["max_points"], clips)

    # ---- whole frames as ragged batches (cmf_draw_frames) ---------------------------------------------------------------------------
    def _need_gpu(self, what):
        if not self.tab1.is_cuda:
            raise RuntimeError("DeviceSplit.%s: the split is on %s; batches are drawn on the GPU only (no CPU fallback)" % (what, self.device))

    def draw_frames(self, frames, nmax1=None, nmax2=None, augment=None, seed=None, aug_draw=None, slot0=0, t_camera_radar=None):
        """One ragged batch of WHOLE frames: slot s holds frame ``frames[s]``, cloud 1 (and everything indexed by its points) padded
        to ``nmax1``, cloud 2 to ``nmax2`` with the frame's first point -- bit for bit what
        as_batch_dict_ragged(extract_data_info_ragged(collate_ragged(items))) gives for the same frames when the two sizes are the
        batch maxima.  ``frames`` on the host (a sequence of ids): the sizes default to the batch maxima (from counts_host) and a
        given size smaller than one of the frames raises ValueError.  ``frames`` a device tensor: nothing is read back (but
        counts_host, once per split, when a size is left out); the sizes default to the split-wide maxima per cloud, and a frame
        larger than a given size is truncated (``n1`` / ``n2`` say so).  Ids outside the split are clamped to its first / last frame.
        ``augment`` (a ``dataset.Augment``; None: off, nothing more is launched): the batch goes through
        ``augment_batch(batch, augment, seed, aug_draw, slot0, t_camera_radar)`` -- nothing is sampled here, so ``seed`` and ``aug_draw``
        must then be given (ValueError) -- and gains ``aug`` and ``t_camera_radar``.
        -> the dict of as_batch_dict_ragged plus ``frames`` (B,) int32 on the device, the (clamped) frame of every slot."""
        from . import _lib
        self._need_gpu("draw_frames")
        if augment is not None and (seed is None or aug_draw is None):
            raise ValueError("DeviceSplit.draw_frames: augment needs seed and aug_draw (whole frames are not sampled: there is no draw id)")
        on_device = torch.is_tensor(frames) and frames.is_cuda
        # Errors: a size given on the host that is too small for a frame known on the host is this function's ValueError; B = 0
        # and a size outside [1, CMF_DRAW_MAX_NPOINTS] are left to the entry point (its argument error -> RuntimeError), so that
        # both kinds of id argument fail the same way.
        if on_device:
            if nmax1 is None or nmax2 is None:
                c1, c2 = self.counts_host
                nmax1, nmax2 = (int(c1.max()) if nmax1 is None else nmax1), (int(c2.max()) if nmax2 is None else nmax2)
        else:
            ids = np.clip(np.asarray(frames, dtype=np.int64).reshape(-1), 0, len(self) - 1)
            if ids.size:                                            # an empty batch: any size will do, the entry point refuses B = 0
                c1, c2 = self.counts_host
                m1, m2 = int(c1[ids].max()), int(c2[ids].max())
                for given, need in ((nmax1, m1), (nmax2, m2)):
                    if given is not None and 1 <= int(given) < need:
                        raise ValueError("DeviceSplit.draw_frames: nmax1 = %s, nmax2 = %s, but the batch has frames of %d / %d points"
                                         % (nmax1, nmax2, m1, m2))
            else:
                m1 = m2 = 1
            nmax1, nmax2 = (m1 if nmax1 is None else nmax1), (m2 if nmax2 is None else nmax2)
        frames = torch.as_tensor(frames, dtype=torch.int32, device=self.device).reshape(-1).clamp(0, len(self) - 1)
        B, N1, N2 = int(frames.numel()), int(nmax1), int(nmax2)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        out = dict(zip(self.KEYS, (f32(B, 3, N1), f32(B, 3, N2), f32(B, 3, N1), f32(B, 3, N2), f32(B, 4, 4), f32(B, N1, 3), f32(B, N1),
                                   f32(B), f32(B, N1), f32(B, N1), f32(B, N1, 2))))
        out["n1"] = torch.empty(B, dtype=torch.int32, device=self.device)
        out["n2"] = torch.empty(B, dtype=torch.int32, device=self.device)
        out["frames"] = frames
        fp, ip = (lambda t: _lib.dev_ptr(t, torch.float32)), (lambda t: _lib.dev_ptr(t, torch.int32))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().cmf_draw_frames(
                B, N1, N2, len(self), fp(self.tab1), fp(self.tab2), ip(self.off1), ip(self.off2), fp(self.trans), fp(self.interval),
                ip(frames), *(fp(out[k]) for k in self.KEYS), ip(out["n1"]), ip(out["n2"]), _lib.stream_ptr()), "cmf_draw_frames")
        if augment is not None:
            augment_batch(out, augment, seed, aug_draw, slot0, t_camera_radar)
        return out

    def draw_frame_batches(self, batches, augment=None, seed=None, aug_draw0=0, slot0=None, t_camera_radar=None):
        """``draw_frames`` for a list of frame-id lists known in advance (an epoch, a sweep, a schedule): all ids go to the device
        here, in ONE asynchronous copy from pinned memory; every batch is then a slice of that tensor with its sizes -- the batch
        maxima -- taken from counts_host, so a step costs launches only and the host never waits for the stream.  An iterator of
        the batch dicts of ``draw_frames``, bit for bit what ``draw_frames(batch)`` returns for each list.
        ``augment`` (with ``seed``): batch k is augmented with ``aug_draw = aug_draw0 + k`` and ``slot0[k]`` (a list; None: zeros)."""
        self._need_gpu("draw_frame_batches")
        if augment is not None and seed is None:
            raise ValueError("DeviceSplit.draw_frame_batches: augment needs a seed")
        batches = [[int(f) for f in b] for b in batches]
        flat = np.clip(np.array([f for b in batches for f in b], dtype=np.int64), 0, len(self) - 1)
        ids = torch.from_numpy(flat.astype(np.int32)).pin_memory().to(self.device, non_blocking=True) if flat.size else None
        tcr = self._calibration(t_camera_radar) if augment is not None else None
        return self._draw_frame_batches(batches, flat, ids, (augment, seed, int(aug_draw0), slot0, tcr))

    def _draw_frame_batches(self, batches, flat, ids, aug):
        c1, c2 = self.counts_host
        augment, seed, aug_draw0, slot0, tcr = aug
        first = 0
        for k, b in enumerate(batches):
            own = flat[first:first + len(b)]
            if len(b):
                yield self.draw_frames(ids[first:first + len(b)], int(c1[own].max()), int(c2[own].max()), augment, seed, aug_draw0 + k,
                                       0 if slot0 is None else int(slot0[k]), tcr)
            else:
                yield self.draw_frames(b)                              # the entry point's argument error
            first += len(b)

    def epoch_ragged(self, batch_size, seed, epoch, bucket=1, drop_last=True, rank=0, world=1, augment=None, t_camera_radar=None):
        """One pass over the whole frames in the shuffled order of ``epoch`` (``_order``, seeded by (seed, epoch); brought to the host
        once), cut by ``ragged_batches`` (``bucket`` > 1: size bucketing inside windows of bucket * batch_size frames) and sent back
        once (``draw_frame_batches``): an iterator of the batch dicts of ``draw_frames``, which TrainStep.step_ragged takes as they
        are.  After the first batch nothing moves between host and device but launches.
        Data parallel (``rank`` of ``world``, ``batch_size`` per rank): ``ragged_batches`` cuts GLOBAL batches of
        ``world * batch_size`` frames from the order every rank shares, and rank r takes its contiguous slice of each
        (``shard_batches``); ``drop_last=False`` is refused at world > 1 as in ``epoch``.  ``bucket`` > 1 sorts a window by size before
        it is cut, which narrows the size band of a global batch, so the ranks' ``Nmax`` -- and with them their step times --
        are close; nothing else balances the ranks.
        ``augment`` / ``t_camera_radar`` as in ``epoch``: step k of the epoch's ``steps`` global batches is augmented with
        ``aug_draw = epoch * steps + k`` -- the step's draw id -- and ``slot0`` = the position of the rank's slice in the global batch."""
        rank, world = self._equal_steps("DeviceSplit.epoch_ragged", rank, world, drop_last)
        self._need_gpu("epoch_ragged")
        whole = ragged_batches(self.counts_host[0], self._order(len(self), seed, epoch).tolist(), world * batch_size, bucket, drop_last)
        slot0 = [rank * (len(b) // world) + min(rank, len(b) % world) for b in whole]       # shard_batches' first row
        return self.draw_frame_batches(shard_batches(whole, rank, world), augment, seed, int(epoch) * len(whole), slot0, t_camera_radar)

    def sweep(self, batch_size, sort_by_size=False, rank=0, world=1):
        """Every frame once, no randomness -- the evaluation iterator: in frame order, or sorted by (n1, frame id) so that a batch
        holds frames of similar size, cut into consecutive batches (the last one may be short).  An iterator of the batch dicts of
        ``draw_frames`` (through ``draw_frame_batches``: one copy of the ids per sweep); ``batch["frames"]`` says which frames a
        batch holds.
        Data parallel (``rank`` of ``world``, ``batch_size`` per rank): the list is cut into global batches of
        ``world * batch_size`` frames and rank r takes its slice of each (``shard_batches``); an empty share -- a last global batch
        shorter than ``world`` -- is skipped, so the ranks may take different numbers of steps (an evaluation loop holds no
        collective) and together visit every frame once."""
        rank, world = _rank_of("DeviceSplit.sweep", rank, world)
        self._need_gpu("sweep")
        n1 = self.counts_host[0]
        order = sorted(range(len(self)), key=lambda f: (int(n1[f]), f)) if sort_by_size else range(len(self))
        return self.draw_frame_batches([b for b in shard_batches(ragged_batches(n1, order, world * batch_size), rank, world) if b])


def write_sample(path, pc1, pc2, gt_labels, pse_labels, gt_mask, pse_mask, trans, opt_flow=None, radar_u=None, radar_v=None):
    """Write one sample file in the format above (pc1, pc2: (n,5) arrays x,y,z,RCS,v_r)."""
    ls = lambda a: np.asarray(a).tolist()
    data = {"pc1": ls(pc1), "pc2": ls(pc2), "gt_labels": ls(gt_labels), "pse_labels": ls(pse_labels),
            "gt_mask": ls(gt_mask), "pse_mask": ls(pse_mask), "trans": ls(trans)}
    if opt_flow is not None:
        data["opt_info"] = {"opt_flow": ls(opt_flow), "radar_u": ls(radar_u), "radar_v": ls(radar_v)}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f)


def write_synthetic_split(root, seed=0, clips=(("train", "delft_1", (180, 256, 400)), ("train", "delft_12", (300,)),
                                               ("test", "delft_2", (210, 330)))):
    """A few synthetic samples with ragged point counts in the reference's directory layout (for tests and
    dry runs).  Returns the relative file names written."""
    names = []
    for ci, (part, clip, sizes) in enumerate(clips):
        for k, n in enumerate(sizes):
            b = synth.make_batch(1, N=n + 37, seed=seed + 100 * ci + k, train_extras=True)
            n2 = n + 37 - 11 * k
            xyz1, xyz2 = b["pc1"][0].t().numpy()[:n], b["pc2"][0].t().numpy()[:n2]
            f1, f2 = b["ft1"][0].t().numpy()[:n], b["ft2"][0].t().numpy()[:n2]
            pc1 = np.concatenate([xyz1, f1[:, 1:2], f1[:, 0:1]], axis=1)          # x, y, z, RCS, v_r
            pc2 = np.concatenate([xyz2, f2[:, 1:2], f2[:, 0:1]], axis=1)
            lab = b["flow_label"][0].numpy()[:n]
            rng = np.random.default_rng(seed + k)
            pse = lab + rng.normal(0, 0.02, lab.shape)
            mask = b["fg_mask"][0].numpy()[:n]
            rel = os.path.join(part, clip, "%d_%s.json" % (k + 5 * ci, clip))
            write_sample(os.path.join(root, rel), pc1, pc2, lab, pse, mask, (rng.random(n) < 0.8).astype(np.float64),
                         np.linalg.inv(b["gt_trans"][0].numpy().astype(np.float64)), b["opt_flow"][0].numpy()[:n],
                         b["radar_u"][0].numpy()[:n], b["radar_v"][0].numpy()[:n])
            names.append(rel)
    return names
