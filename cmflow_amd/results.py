"""What a test epoch leaves behind, kept on the device -- the reference's ``--eval --save_res`` run (main_util.py:149-168,
clip_util.py:238-257) without its per-frame copies to the host.

The reference writes, frame by frame, ``pred_f[0].cpu()``, ``pred_m[0].cpu()`` and ``pred_t[0].cpu()`` into one JSON file per
frame: three waits for the device in every step of a loop that ``evaluate.eval_split`` runs without any.  Here a
``ResultCollector`` is handed to ``eval_split`` / ``eval_split_clips`` as their ``on_batch`` hook; per batch it only launches --
``cmf_pack_results`` (csrc/results.hip) copies the valid rows of the network's outputs into a ``SplitResults`` store packed like the
split itself, ``cmf_eval_metrics_frames`` (csrc/eval.hip) writes the 14 metrics of every frame to the frame's row -- and the
store is read, chained (``cmf_pose_chain``: the odometry result of the paper, the per-frame transforms accumulated along a clip),
ranked, merged, saved or written out in the reference's JSON layout AFTER the epoch.  ``evaluate.test_split`` and
``evaluate.test_split_clips`` wrap this up.  DESIGN.md section 17 states the layout and the chain's arithmetic.
"""
import json
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from . import eval_util as E

METRIC_KEYS = E.SF_KEYS + E.SEG_KEYS + E.POSE_KEYS
RESULTS_FORMAT_VERSION = 1
_FIELDS = ("off1", "flow", "score", "mask", "pred_trans", "gt_trans", "metrics", "done")


def _affine_inverse(T):
    """inv of (...,4,4) affine matrices in their own dtype: the 3x3 block by its adjugate (rows of the inverse's transpose are cross
    products of the block's rows), translation -R^-1 t, bottom row (0,0,0,1).  Elementwise ops only: nothing that could wait for
    the device."""
    R, t = T[..., :3, :3], T[..., :3, 3]
    r0, r1, r2 = R[..., 0, :], R[..., 1, :], R[..., 2, :]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    det = (r0 * c0).sum(-1)
    Ri = torch.stack((c0, c1, c2), dim=-1) / det[..., None, None]
    out = torch.zeros_like(T)
    out[..., :3, :3] = Ri
    out[..., :3, 3] = -(Ri @ t[..., None])[..., 0]
    out[..., 3, 3] = 1
    return out


class SplitResults:
    """The per-frame results of one split of F frames, packed like the split's cloud-1 table:

      ``off1`` (F+1) int32        the split's own offsets: frame f owns rows off1[f] .. off1[f+1]-1
      ``flow`` (sum n1, 3) f32    predicted scene flow per point (``pred_f``, point-major)
      ``score`` (sum n1) f32      the static-class score per point (``stat_cls``)
      ``mask`` (sum n1) uint8     the predicted static mask per point (``pred_m``)
      ``pred_trans``, ``gt_trans`` (F,4,4) f32
      ``metrics`` (F,14) f64      columns ``METRIC_KEYS``; NaN until the frame has been evaluated
      ``done`` (F) uint8          1 once the frame's rows have been written
      ``clips``                   the split's [first, last) clip ranges, or None

    Everything but ``metrics`` starts as zeros, so stores of disjoint frame sets add up exactly (``all_reduce``).  The tensors may
    live on any device; filling the store (``ResultCollector``) and ``trajectories`` / ``odometry_metrics`` run on the GPU only."""

    def __init__(self, off1, flow, score, mask, pred_trans, gt_trans, metrics, done, clips=None):
        self.off1, self.flow, self.score, self.mask = off1, flow, score, mask
        self.pred_trans, self.gt_trans, self.metrics, self.done = pred_trans, gt_trans, metrics, done
        self.clips = None if clips is None else [(int(a), int(b)) for a, b in clips]
        self.device = flow.device
        self._off_host = None
        self._clip_tensor = None

    @classmethod
    def empty(cls, split):
        """The unwritten store of a DeviceSplit, on the split's device."""
        F, dev, total = len(split), split.device, split.tab1.shape[0]
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        return cls(split.off1, z((total, 3), torch.float32), z((total,), torch.float32), z((total,), torch.uint8),
                   z((F, 4, 4), torch.float32), z((F, 4, 4), torch.float32),
                   torch.full((F, len(METRIC_KEYS)), float("nan"), dtype=torch.float64, device=dev), z((F,), torch.uint8), split.clips)

    def __len__(self):
        return self.off1.numel() - 1

    def to(self, device):
        return SplitResults(*(getattr(self, k).to(device) for k in _FIELDS), self.clips)

    @property
    def offsets_host(self):
        """off1 as a numpy array, brought to the host on first use (one copy per store) and kept."""
        if self._off_host is None:
            self._off_host = self.off1.cpu().numpy()
        return self._off_host

    # ---- reading ----------------------------------------------------------------------------------------------------------------------
    def frame(self, i):
        """Views of frame ``i``: flow (n1,3), score (n1), mask (n1), pred_trans, gt_trans (4,4), metrics (14), done (0-d)."""
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError("SplitResults.frame: frame %d of %d" % (i, len(self)))
        a, b = int(self.offsets_host[i]), int(self.offsets_host[i + 1])
        return {"flow": self.flow[a:b], "score": self.score[a:b], "mask": self.mask[a:b], "pred_trans": self.pred_trans[i],
                "gt_trans": self.gt_trans[i], "metrics": self.metrics[i], "done": self.done[i]}

    def per_frame(self, key):
        """(F,) float64: metric ``key`` (one of METRIC_KEYS) of every frame, a view of ``metrics``."""
        if key not in METRIC_KEYS:
            raise KeyError("SplitResults.per_frame: %r is not one of %s" % (key, ", ".join(METRIC_KEYS)))
        return self.metrics[:, METRIC_KEYS.index(key)]

    def worst(self, key, k, largest=True):
        """The ``k`` frames with the largest (``largest=False``: smallest) value of metric ``key`` -> (values (k,), frame ids (k,)
        int64), on the store's device, nothing read back.  Frames whose value is NaN (not evaluated, or a NaN metric) come last."""
        v = self.per_frame(key)
        k = int(k)
        if not 0 <= k <= v.numel():
            raise ValueError("SplitResults.worst: k = %d of %d frames" % (k, v.numel()))
        ranked = torch.where(torch.isnan(v), torch.full_like(v, float("-inf") if largest else float("inf")), v)
        idx = torch.topk(ranked, k, largest=largest).indices
        return v[idx], idx

    # ---- combining --------------------------------------------------------------------------------------------------------------------
    def _same_split(self, other, what):
        if not isinstance(other, SplitResults) or other.off1.shape != self.off1.shape or other.flow.shape != self.flow.shape \
                or other.clips != self.clips or other.device != self.device:
            raise ValueError("SplitResults.%s: the two stores are not of the same split on the same device" % what)

    def merge(self, other):
        """A new store with the frames of both: every frame ``done`` in exactly one of the two (or in none).  A frame done in both
        raises ValueError (one comparison is read back; this is not for the inside of an epoch)."""
        self._same_split(other, "merge")
        if not torch.equal(self.off1, other.off1):
            raise ValueError("SplitResults.merge: the two stores have different offsets")
        both = (self.done != 0) & (other.done != 0)
        if bool(both.any()):
            raise ValueError("SplitResults.merge: frames %s are done in both stores" % both.nonzero().flatten().tolist()[:8])
        take = other.done != 0
        counts = (self.off1[1:] - self.off1[:-1]).long()
        rows = torch.repeat_interleave(take, counts, output_size=self.flow.shape[0])
        pick = lambda m, a, b: torch.where(m.reshape((-1,) + (1,) * (a.dim() - 1)), b, a)
        return SplitResults(self.off1, pick(rows, self.flow, other.flow), pick(rows, self.score, other.score),
                            pick(rows, self.mask, other.mask), pick(take, self.pred_trans, other.pred_trans),
                            pick(take, self.gt_trans, other.gt_trans), pick(take, self.metrics, other.metrics),
                            pick(take, self.done, other.done), self.clips)

    def all_reduce(self, group=None):
        """The ranks' parts into the whole, in place and on every rank: one all_reduce(SUM) per tensor.  Exact, because a row is
        written by the one rank that evaluated its frame and is zero elsewhere (a stored -0.0 comes back as +0.0); ``metrics`` is
        NaN where nothing was written, so its rows that are not ``done`` are summed as zeros and set back to NaN where no rank has
        the frame -- a NaN metric of an evaluated frame stays NaN.  A frame evaluated by two ranks is the caller's error."""
        own = (self.done != 0)[:, None]
        self.metrics.copy_(torch.where(own, self.metrics, torch.zeros_like(self.metrics)))
        for t in (self.flow, self.score, self.mask, self.pred_trans, self.gt_trans, self.metrics, self.done):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self.metrics.copy_(torch.where((self.done != 0)[:, None], self.metrics, torch.full_like(self.metrics, float("nan"))))
        return self

    # ---- one file per store -----------------------------------------------------------------------------------------------------------
    def save(self, path):
        """The store in one ``torch.save`` file (tensors on the CPU), written to a temporary name and renamed, as DeviceSplit.save."""
        rec = {"format": "cmflow_amd.SplitResults", "version": RESULTS_FORMAT_VERSION, "clips": self.clips}
        for k in _FIELDS:
            rec[k] = getattr(self, k).detach().cpu()
        tmp = "%s.tmp%d" % (path, os.getpid())
        torch.save(rec, tmp)
        os.replace(tmp, path)

    @classmethod
    def load(cls, path, device):
        """The store ``save`` wrote, on ``device``.  A file of another format (version) raises ValueError."""
        rec = torch.load(path, map_location="cpu")
        if not isinstance(rec, dict) or rec.get("format") != "cmflow_amd.SplitResults" or rec.get("version") != RESULTS_FORMAT_VERSION:
            raise ValueError("SplitResults.load: %s is not a SplitResults file of format version %d (found %r)"
                             % (path, RESULTS_FORMAT_VERSION, rec.get("version") if isinstance(rec, dict) else type(rec).__name__))
        return cls(*(rec[k].to(device) for k in _FIELDS), rec["clips"])

    # ---- the reference's files --------------------------------------------------------------------------------------------------------
    def _clip_ranges(self):
        return self.clips if self.clips else [(0, len(self))]

    def write_json(self, directory, split, clip_names=None):
        """The reference's ``save_res`` files (main_util.py:149-168): ``directory/<clip name>/<global frame index>.json`` with the keys
        pc1, pc2 (3 x n nested lists, from ``split``, the DeviceSplit the store was filled from), pred_f (3 x n1), pred_m (n1 floats),
        pred_t (4 x 4), written with the stdlib json module.  The folder is chosen as the reference chooses it: it starts with the
        first clip and moves on to the next clip -- one step -- at a frame whose index has reached the current clip's end.  Without
        clip ranges everything goes to one folder.  ``clip_names``: one name per clip (default clip_0, clip_1, ...).
        ONE device-to-host copy brings over everything the files need.  Every frame must be ``done``, else ValueError (before
        anything is written).  -> the list of paths written, in frame order."""
        clips = self._clip_ranges()
        names = ["clip_%d" % c for c in range(len(clips))] if clip_names is None else [str(n) for n in clip_names]
        if len(names) != len(clips):
            raise ValueError("SplitResults.write_json: %d clip names for %d clips" % (len(names), len(clips)))
        F = len(self)
        if len(split) != F or split.tab1.shape[0] != self.flow.shape[0]:
            raise ValueError("SplitResults.write_json: the split is not the one these results belong to")
        parts = [self.off1, split.off2, self.flow, self.pred_trans, split.tab1[:, :3], split.tab2[:, :3], self.mask, self.done]
        flat = torch.cat([p.detach().to(self.device).contiguous().reshape(-1).view(torch.uint8) for p in parts]).cpu().numpy()
        host, at = [], 0
        for p in parts:
            nbytes = p.numel() * p.element_size()
            host.append(np.frombuffer(flat[at:at + nbytes].tobytes(), dtype={torch.int32: np.int32, torch.float32: np.float32,
                                                                                torch.uint8: np.uint8}[p.dtype]).reshape(tuple(p.shape)))
            at += nbytes
        off1, off2, flow, trans, pc1, pc2, mask, done = host
        if not done.all():
            raise ValueError("SplitResults.write_json: %d of %d frames have no results" % (int((done == 0).sum()), F))
        paths, num_seq = [], 0
        for i in range(F):
            if i >= clips[num_seq][1] and num_seq < len(clips) - 1:      # main_util.py:158-166: one step, at the current clip's end
                num_seq += 1
            folder = os.path.join(directory, names[num_seq])
            os.makedirs(folder, exist_ok=True)
            a, b, c, d = int(off1[i]), int(off1[i + 1]), int(off2[i]), int(off2[i + 1])
            res = {"pc1": pc1[a:b].T.tolist(), "pc2": pc2[c:d].T.tolist(), "pred_f": flow[a:b].T.tolist(),
                   "pred_m": mask[a:b].astype(float).tolist(), "pred_t": trans[i].astype(float).tolist()}
            paths.append(os.path.join(folder, "%d.json" % i))
            with open(paths[-1], "w") as fh:
                json.dump(res, fh)
        return paths

    def write_vis(self, directory, split, layers=("flow", "seg_gt"), frames=None, view=None, chunk=64):
        """The reference's ``--vis`` pictures (main_util.py:170-172): ``directory/<layer>/<global frame index>.png`` for every selected
        frame and every layer of ``layers`` (``vis.LAYERS``), as ``args.vis_path_flow/{num_pcs}.png`` and
        ``args.vis_path_seg/{num_pcs}.png`` -- the two default layers are the two pictures the reference writes (its "seg" figure is
        coloured by the ground-truth mask).  ``frames``: None (all), a list or an int64 tensor (``worst(...)``'s); ``view``: a
        ``vis.BevView``.  ``vis.render`` draws ``chunk`` frames at a time, ONE device-to-host copy per chunk and layer, so memory stays
        bounded (2.16 MB per default picture).  Every selected frame must be ``done``, else ValueError (before anything is written).
        -> the list of paths written: layer by layer, in the order of ``frames``."""
        from . import vis
        layers = [layers] if isinstance(layers, str) else list(layers)
        for layer in layers:
            vis._layer_id(layer, "SplitResults.write_vis")
        vis.check_store(self, split, "SplitResults.write_vis")
        chunk = int(chunk)
        if not 1 <= chunk <= vis.MAX_FRAMES:
            raise ValueError("SplitResults.write_vis: chunk = %d" % chunk)
        F = len(self)
        ids = np.arange(F, dtype=np.int64) if frames is None else \
            (frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(list(frames))).astype(np.int64).reshape(-1)
        if ids.size and not (0 <= ids.min() and ids.max() < F):
            raise ValueError("SplitResults.write_vis: frames outside 0 .. %d" % (F - 1))
        done = self.done.cpu().numpy()
        if not done[ids].all():
            raise ValueError("SplitResults.write_vis: %d of the %d selected frames have no results" % (int((done[ids] == 0).sum()), ids.size))
        paths = []
        for layer in layers:
            folder = os.path.join(directory, layer)
            os.makedirs(folder, exist_ok=True)
            for a in range(0, ids.size, chunk):
                part = ids[a:a + chunk]
                images = vis.render(self, split, layer, None if frames is None and chunk >= F else torch.from_numpy(part), view).cpu().numpy()
                for f, image in zip(part.tolist(), images):
                    paths.append(os.path.join(folder, "%d.png" % f))
                    with open(paths[-1], "wb") as fh:
                        fh.write(vis.encode_png(image))
        return paths

    def accumulate(self, split, window=8, which="pred", dynamic="keep", frames=None):
        """``accumulate.accumulate(split, self, ...)``: the clouds of ``frames`` accumulated over ``window`` frames of their clip."""
        from . import accumulate as A
        return A.accumulate(split, self, window=window, which=which, dynamic=dynamic, frames=frames)

    def instances(self, split, **kw):
        """``instances.cluster(split, self, ...)``: the moving points of every selected frame grouped into instances (``which``,
        ``eps``, ``min_points``, ``flow_weight``, ``frames`` as there)."""
        from . import instances as I
        return I.cluster(split, self, **kw)

    def tracks(self, split, inst=None, gate=2.0, max_gap=2, **cluster_kw):
        """``tracks.track(inst, split, self, gate, max_gap)``: the instances associated from frame to frame inside every clip.  ``inst``:
        an ``instances`` result of this split, or None -- then ``self.instances(split, **cluster_kw)`` is formed first."""
        from . import tracks as K
        if inst is None:
            inst = self.instances(split, **cluster_kw)
        return K.track(inst, split, self, gate=gate, max_gap=max_gap)

    def objects(self, split, trk=None, **kw):
        """``objects.estimate(trk, split, self, ...)``: per match of every track the smoothed position and velocity, a heading and an
        oriented box (``sigma_pos``, ``sigma_disp``, ``sigma_acc``, ``min_disp`` as there).  ``trk``: a ``tracks`` result of this
        split, or None -- then ``self.tracks(split, ...)`` is formed first from the remaining keywords."""
        from . import objects as O
        own = {k: kw.pop(k) for k in ("sigma_pos", "sigma_disp", "sigma_acc", "min_disp") if k in kw}
        if trk is None:
            trk = self.tracks(split, **kw)
        elif kw:
            raise ValueError("SplitResults.objects: %s belong to the tracks, which were given" % ", ".join(sorted(kw)))
        return O.estimate(trk, split, self, **own)

    def score_tracks(self, split, iou=0.5, pred=None, gt=None, **kw):
        """``score.score(pred, gt, split, iou)``: the predicted chain's tracks and objects scored against the labels'.  ``pred`` /
        ``gt``: ``objects`` results of this split, or None -- then ``self.objects(split, which='pred' / 'gt', ...)`` is formed first
        from the remaining keywords, both sides with the same options (``'gt'`` reads no store).  (Not ``score``: that is the store's
        per-point classification score.)"""
        from . import score as S
        S.check_iou(iou)                                                    # before the chains launch anything
        if "which" in kw:
            raise ValueError("SplitResults.score_tracks: which = %r -- the two sides are 'pred' and 'gt'; pass pred= / gt= for others" % (kw["which"],))
        if pred is not None and gt is not None and kw:
            raise ValueError("SplitResults.score_tracks: %s belong to the object states, which were given" % ", ".join(sorted(kw)))
        if pred is None:
            pred = self.objects(split, which="pred", **kw)
        if gt is None:
            gt = self.objects(split, which="gt", **kw)
        return S.score(pred, gt, split, iou=iou)

    # ---- odometry ---------------------------------------------------------------------------------------------------------------------
    def trajectories(self, which="pred"):
        """(F,4,4) float64: the sensor's pose at every frame relative to its clip's first scan, ``cmf_pose_chain`` over ``pred_trans``
        (``which="pred"``) or ``gt_trans`` (``"gt"``): per clip P = I, then P = P . inv(T_k), poses[k] = P -- T_k maps static
        points from scan 1 to scan 2, so the pose accumulates its rigid inverse (R^T, -R^T t).  Float64 from the float32 entries in a
        fixed operation order (include/cmflow_hip.h).  A store without clip ranges is one clip [0, F); frames outside every clip
        are NaN.  GPU only."""
        if which not in ("pred", "gt"):
            raise ValueError("SplitResults.trajectories: which is 'pred' or 'gt'")
        T = (self.pred_trans if which == "pred" else self.gt_trans).reshape(-1, 16)
        ptr = _lib.dev_ptr(T, torch.float32)
        if self._clip_tensor is None:
            self._clip_tensor = torch.tensor(self._clip_ranges(), dtype=torch.int32, device=self.device).reshape(-1, 2)
        F, C = len(self), self._clip_tensor.shape[0]
        poses = torch.full((F, 4, 4), float("nan"), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().cmf_pose_chain(F, C, ptr, _lib.dev_ptr(self._clip_tensor, torch.int32), poses.data_ptr(),
                                                 _lib.stream_ptr()), "cmf_pose_chain")
        return poses

    def odometry_metrics(self, deltas=(1, 10)):
        """The chained ego-motion against the chained ground truth, per clip and overall, as float64 device tensors (batched torch
        ops on the two ``trajectories``; no loop over frames on the host, nothing read back):

          end_error      translation error at the clip's last frame
          ate_rmse       sqrt(mean_k |t_pred,k - t_gt,k|^2) -- no alignment: both chains start at I
          path_length    the ground truth's path from the clip's first scan (the origin) through every pose
          rpe_trans_D, rpe_rot_D   for every D in ``deltas``: the mean over k (k and k+D in the clip) of the translation norm and the
                         rotation angle (degrees; atan2(|axial vector|, trace - 1), as the RAE of csrc/eval.hip) of
                         E = (G_k^-1 G_k+D)^-1 (P_k^-1 P_k+D).  NaN for a clip of at most D frames.

        -> {"clips": {key: (C,) tensor}, "overall": {key: 0-d tensor}}; overall pools the frames (pairs) of all clips, its end_error is
        the mean over the non-empty clips."""
        return _odometry(self.trajectories("pred"), self.trajectories("gt"), self._clip_ranges(), deltas)


def _odometry(P, G, clips, deltas):
    """odometry_metrics from the two chains (F,4,4) float64, on their device."""
    dev, f64 = P.device, torch.float64
    zero = torch.zeros((), dtype=f64, device=dev)
    keys = ["end_error", "ate_rmse", "path_length"] + [k % int(d) for d in deltas for k in ("rpe_trans_%d", "rpe_rot_%d")]
    per = {k: [] for k in keys}
    sums = {k: [zero, 0] for k in keys}
    for a, b in clips:
        a, b = max(int(a), 0), min(int(b), P.shape[0])
        n = max(b - a, 0)
        tp, tg = P[a:b, :3, 3], G[a:b, :3, 3]
        if n:
            sq = ((tp - tg) ** 2).sum(-1)
            steps = torch.cat((tg[:1], tg[1:] - tg[:-1])).norm(dim=-1)
            vals = {"end_error": (sq[-1].sqrt(), 1, None), "ate_rmse": (sq.sum(), n, torch.sqrt), "path_length": (steps.sum(), None, None)}
        else:
            vals = {"end_error": (zero, 0, None), "ate_rmse": (zero, 0, torch.sqrt), "path_length": (zero, None, None)}
        for d in deltas:
            d = int(d)
            m = max(n - d, 0)
            if m:
                Pa, Pb, Ga, Gb = P[a:b - d], P[a + d:b], G[a:b - d], G[a + d:b]
                Em = _affine_inverse(_affine_inverse(Ga) @ Gb) @ (_affine_inverse(Pa) @ Pb)
                ax = torch.stack((Em[:, 2, 1] - Em[:, 1, 2], Em[:, 0, 2] - Em[:, 2, 0], Em[:, 1, 0] - Em[:, 0, 1]), dim=-1)
                ang = torch.atan2(ax.norm(dim=-1), Em[:, 0, 0] + Em[:, 1, 1] + Em[:, 2, 2] - 1.0).abs() * (180.0 / np.pi)
                vals["rpe_trans_%d" % d] = (Em[:, :3, 3].norm(dim=-1).sum(), m, None)
                vals["rpe_rot_%d" % d] = (ang.sum(), m, None)
            else:
                vals["rpe_trans_%d" % d] = (zero, 0, None)
                vals["rpe_rot_%d" % d] = (zero, 0, None)
        for k, (s, cnt, fin) in vals.items():
            v = s if cnt is None else s / cnt if cnt else s + float("nan")
            per[k].append(fin(v) if fin else v)
            sums[k] = [sums[k][0] + s, sums[k][1] + (cnt or 0)]
    out = {"clips": {k: torch.stack(v) for k, v in per.items()}, "overall": {}}
    for k, (s, cnt) in sums.items():
        v = s if k == "path_length" else s / cnt if cnt else s + float("nan")
        out["overall"][k] = torch.sqrt(v) if k == "ate_rmse" else v
    return out


class ResultCollector:
    """``on_batch`` hook of ``evaluate.eval_split`` / ``eval_split_clips`` that keeps every frame's outputs: called with the batch
    dict of ``draw_frames`` and the tuple ``forward_ragged`` returned (CMFlow's four outputs or CMFlow-T's five), it packs flow, score,
    mask and both transforms into ``self.results`` (``cmf_pack_results``) and writes the frames' metrics to their rows
    (``cmf_eval_metrics_frames`` on the inputs ``eval_batch_ragged`` gets).  Launches only: nothing is read back, and the three scratch
    buffers (the point-major flow, the mask as floats, the kernels' partial sums) are kept and only grow.  ``args.radar_res`` as in
    eval_util."""

    def __init__(self, split, args=None):
        split._need_gpu("ResultCollector")
        self.split, self.args = split, args
        self.results = SplitResults.empty(split)
        self._pred = self._pm = self._ws = None

    def _scratch(self, B, N):
        dev = self.split.device
        if self._pred is None or self._pred.numel() < B * N * 3:
            self._pred = torch.empty(B * N * 3, dtype=torch.float32, device=dev)
            self._pm = torch.empty(B * N, dtype=torch.float32, device=dev)
        if self._ws is None or self._ws.numel() < 16 * B:
            self._ws = torch.empty(16 * B, dtype=torch.float64, device=dev)
        return self._pred[:B * N * 3].view(B, N, 3), self._pm[:B * N].view(B, N), self._ws

    def __call__(self, batch, outputs):
        if len(outputs) not in (4, 5):
            raise ValueError("ResultCollector: outputs are forward_ragged's (sf, stat_cls, pre_trans, mask[, gfeat])")
        sf, stat_cls, pre_trans, mask = (t.detach().contiguous() for t in outputs[:4])
        r, sp = self.results, self.split
        B, _, N = sf.shape
        if batch["pc1"].shape != sf.shape or stat_cls.numel() != B * N or mask.shape != (B, N) or batch["frames"].numel() != B:
            raise ValueError("ResultCollector: the outputs are not those of this batch")
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        fp, ip = (lambda t: _lib.dev_ptr(t, f32)), (lambda t: _lib.dev_ptr(t, i32))
        mask8 = mask.view(u8) if mask.dtype == torch.bool else mask
        gt_trans, frames, n1 = batch["gt_trans"].contiguous(), batch["frames"].contiguous(), batch["n1"].contiguous()
        pred, pm, ws = self._scratch(B, N)
        res = getattr(self.args, "radar_res", None) or E.VOD_RADAR_RES
        with torch.cuda.device(sp.device):
            _lib.check(_lib.lib().cmf_pack_results(
                B, N, len(sp), ip(frames), ip(n1), ip(r.off1), r.flow.shape[0], fp(sf), fp(stat_cls), _lib.dev_ptr(mask8, u8),
                fp(pre_trans), fp(gt_trans), fp(r.flow), fp(r.score), _lib.dev_ptr(r.mask, u8), fp(r.pred_trans), fp(r.gt_trans),
                _lib.dev_ptr(r.done, u8), _lib.stream_ptr()), "cmf_pack_results")
            pred.copy_(sf.transpose(1, 2))
            pm.copy_(mask)
            _lib.check(_lib.lib().cmf_eval_metrics_frames(
                B, N, ip(n1), fp(batch["pc1"]), fp(pred), fp(batch["flow_label"]), fp(batch["fg_mask"]), fp(pm), fp(gt_trans),
                fp(pre_trans), res['r_res'], res['theta_res'], res['phi_res'], len(sp), ip(frames), r.metrics.data_ptr(),
                ws.data_ptr(), _lib.stream_ptr()), "cmf_eval_metrics_frames")
