"""A test run's tracks and objects scored against the labels', on the device -- what ``tracks.track`` and ``objects.estimate`` stop
short of: how many labelled objects the predicted chain finds, how often an object changes its id, and how far the smoothed
positions, velocities and boxes are from those the labels give.

Everything this needs lies on the device already, and one property of the chain makes it cheap and exact: on both sides the
instances of a frame partition THE SAME points (``inst.label`` lives in the split's cloud-1 row space), so two instances that share
more than half of their union can only be matched to each other -- the argument of MOTS: an overlap above one half fixes the
correspondence, without an assignment problem and without a greedy order.  ``score`` is ONE launch of ``cmf_score_tracks``
(csrc/score.hip), one workgroup per clip walking the clip's frames in order: per frame the overlaps counted from the labels and
the pairs with ``c / (|G| + |P| - c) > iou`` matched, per gt track the walk over its matches that counts id switches and
fragmentations.  A definition in integers with one float64 division per pair, stated in include/cmflow_hip.h and DESIGN.md section
25 and restated in numpy, bit for bit, by tests/score_ref.py.

What this is NOT: a score against ground-truth identities -- the split has none; the ``'gt'`` side is the SAME chain run on the
labelled moving points, so the numbers measure what the predicted flow, mask and ego-motion cost the chain, not the rules of the
tracker (a tracker that is wrong in the same way on both sides scores perfectly); IoU thresholds below 0.5 are not offered (the
match would need an assignment); there is no IDF1 and no HOTA (both need a global assignment over the whole clip); and nothing is
claimed about real data (the reference's twelve saved frames hold no labels; the tests score two settings of them).
"""
import numpy as np
import torch

from . import _frames, _lib
from .objects import TrackObjects

IOU_UNIT = 2 ** 30                                          # an IoU is summed in whole units of 2^-30, as ``instances.agreement`` does
PER_PRED = ("match", "iou")
PER_GT = ("match_gt", "switch", "frag")
PER_FRAME = ("frame_tp", "frame_fp", "frame_fn")
PER_TRACK = ("seen", "covered", "last_partner")
PER_CLIP = ("tp", "fp", "fn", "ids", "frags", "gt_total", "iou_units")
KEYS = ("match", "match_gt", "iou", "switch", "frag") + PER_FRAME + PER_TRACK + PER_CLIP      # the entry point's order
STATE_KEYS = ("pos", "vel", "box_size")


class TrackScore:
    """The score of a ``pred`` side against a ``gt`` side (two ``TrackObjects`` of one split), on the device.

    In the instances' row space (instance c of frame f is row off[f] + c), on the PRED side's rows:
      ``match`` (sum n1) int32         the row of the gt instance it matched, or -1
      ``iou`` (sum n1) float64         the overlap of that match, c / (|G| + |P| - c); 0 where unmatched
    on the GT side's rows:
      ``match_gt`` (sum n1) int32      the row of the predicted instance it matched, or -1
      ``switch`` (sum n1) int32        1: the track's match before this one was with another predicted track (an id switch)
      ``frag`` (sum n1) int32          1: the track was matched before, but its instance directly before this one was not
    per frame:
      ``frame_tp``, ``frame_fp``, ``frame_fn`` (F) int32   the matched pairs, predicted and gt instances without a match
    per gt track, in the clip's row space (track u of the clip [a, b) is row off[a] + u):
      ``seen``, ``covered`` (sum n1) int32   its instances, and those that matched
      ``last_partner`` (sum n1) int32        the predicted track of its latest match, or -1
    per clip:
      ``tp``, ``fp``, ``fn``, ``ids``, ``frags``, ``gt_total`` (C) int32 and ``iou_units`` (C) int64, the sum over the matches of
      floor(iou * 2^30).

    ``pred``, ``gt``: the two sides; ``iou_min``: the threshold as given to ``score``; ``clips`` / ``clips_host`` the clips."""

    def __init__(self, pred, gt, iou_min, arrays, clip_of_row=None):
        self.pred, self.gt, self.iou_min = pred, gt, float(iou_min)
        for k, t in zip(KEYS, arrays):
            setattr(self, k, t)
        self.off, self.offsets_host = pred.off, pred.offsets_host
        self.clips, self.clips_host = pred.clips, pred.clips_host
        self.device = self.match.device
        self._clip_of_row = clip_of_row

    def __len__(self):
        return self.clips_host.shape[0]

    @property
    def clip_of_row(self):
        """(sum n1) int64: the clip of every row, what the per-clip sums of ``summary`` and ``state_errors`` index by -- host
        arithmetic and a pinned upload on first use (no wait), kept."""
        if self._clip_of_row is None:
            self._clip_of_row = _frames.to_device(clip_of_rows(self.offsets_host, self.clips_host, self.match.shape[0]), torch.int64, self.device)
        return self._clip_of_row

    def frame(self, i):
        """Views of frame ``i`` of the split: match and iou (the first K_pred rows), match_gt, switch and frag (the first K_gt rows)
        and tp, fp, fn (0-d).  The K come from the instances' host copies of ``count``, made on first use and kept (the one wait,
        as ``TrackObjects.frame``)."""
        Kp, Kg = self.pred.inst.frame(i)["centroid"].shape[0], self.gt.inst.frame(i)["centroid"].shape[0]
        a = int(self.offsets_host[int(i)])
        out = {k: getattr(self, k)[a:a + Kp] for k in PER_PRED}
        out.update({k: getattr(self, k)[a:a + Kg] for k in PER_GT})
        out.update({k[6:]: getattr(self, k)[int(i)] for k in PER_FRAME})
        return out

    def worst(self, k):
        """The ``k`` frames with the most ``fp + fn`` (the lowest frame first among equals) -> (frames (k) int64, their fp + fn (k)
        int64), on the device, nothing read back."""
        F = self.frame_fp.numel()
        k = _frames.whole("worst", "k", k, 0)
        missed = self.frame_fp.long() + self.frame_fn.long()
        key = missed * F + (F - 1 - torch.arange(F, device=self.device))
        top = torch.topk(key, min(k, F)).indices
        return top, missed[top]

    def summary(self):
        """The CLEAR-MOT numbers of MOTS per clip, and over all clips under ``"all"`` -- torch ops on the device in float64, nothing
        read back; a convenience outside the bit-exact contract (as ``TrackObjects.yaw``).  -> dict of (C) float64 tensors, and
        ``"all"``: the same names as 0-d tensors from the sums over the clips.
          MOTSA = (tp - fp - ids) / gt_total          sMOTSA = (iou_sum - fp - ids) / gt_total, iou_sum = iou_units / 2^30
          MOTSP = iou_sum / tp                        recall = tp / (tp + fn)        precision = tp / (tp + fp)
          tracks, mostly_tracked, mostly_lost         the gt tracks, those with 5 covered >= 4 seen, those with 5 covered < seen
        A zero denominator gives NaN."""
        f64 = torch.float64
        C = len(self)
        track = self.seen > 0
        per_clip = lambda flag: torch.zeros(C, dtype=torch.int64, device=self.device).index_add_(0, self.clip_of_row, (track & flag).long())
        counts = {k: getattr(self, k).to(f64) for k in ("tp", "fp", "fn", "ids", "frags", "gt_total")}
        counts["iou_sum"] = self.iou_units.to(f64) / float(IOU_UNIT)
        counts["tracks"] = per_clip(track).to(f64)
        counts["mostly_tracked"] = per_clip(5 * self.covered >= 4 * self.seen).to(f64)
        counts["mostly_lost"] = per_clip(5 * self.covered < self.seen).to(f64)

        def derive(c):
            out = dict(c)
            out["MOTSA"] = (c["tp"] - c["fp"] - c["ids"]) / c["gt_total"]
            out["sMOTSA"] = (c["iou_sum"] - c["fp"] - c["ids"]) / c["gt_total"]
            out["MOTSP"] = c["iou_sum"] / c["tp"]
            out["recall"] = c["tp"] / (c["tp"] + c["fn"])
            out["precision"] = c["tp"] / (c["tp"] + c["fp"])
            return out

        out = derive(counts)
        out["all"] = derive({k: v.sum() for k, v in counts.items()})
        return out

    def state_errors(self):
        """How far the two sides' object states are apart, over the matches (the gt side gathered through ``match``) -- torch ops on
        the device in float64, nothing read back; a convenience outside the bit-exact contract.  -> dict: ``count`` (C) int64 the
        matches of every clip, ``heading_count`` (C) those where both sides have a heading from the velocity (``heading_src`` 1), and
        for ``pos``, ``vel``, ``box_size`` (the Euclidean norm of the difference, metres; ``vel`` metres per frame) and ``heading``
        (the angle between the two unit vectors, radians) a dict of ``mean`` and ``max`` (C) float64; NaN for a clip without one."""
        f64 = torch.float64
        C = len(self)
        held = self.match >= 0
        g = self.match.clamp(min=0).long()
        both = held & (self.pred.heading_src == 1) & (self.gt.heading_src[g] == 1)

        def per_clip(value, mask):
            count = torch.zeros(C, dtype=torch.int64, device=self.device).index_add_(0, self.clip_of_row, mask.long())
            total = torch.zeros(C, dtype=f64, device=self.device).index_add_(0, self.clip_of_row, torch.where(mask, value, torch.zeros_like(value)))
            most = torch.full((C,), float("-inf"), dtype=f64, device=self.device)
            most.scatter_reduce_(0, self.clip_of_row, torch.where(mask, value, torch.full_like(value, float("-inf"))), "amax", include_self=True)
            nan = torch.full_like(total, float("nan"))
            return count, {"mean": torch.where(count > 0, total / count.to(f64), nan), "max": torch.where(count > 0, most, nan)}

        out = {}
        for k in STATE_KEYS:
            d = getattr(self.pred, k).to(f64) - getattr(self.gt, k)[g].to(f64)
            out["count"], out[k] = per_clip(torch.sqrt((d * d).sum(dim=1)), held)
        hp, hg = self.pred.heading.to(f64), self.gt.heading[g].to(f64)
        angle = torch.atan2((hp[:, 0] * hg[:, 1] - hp[:, 1] * hg[:, 0]).abs(), hp[:, 0] * hg[:, 0] + hp[:, 1] * hg[:, 1])
        out["heading_count"], out["heading"] = per_clip(angle, both)
        return out


def clip_of_rows(offsets_host, clips_host, total):
    """Host arithmetic of ``TrackScore.clip_of_row``: per row of the split's row space the clip whose frames hold it (a row outside every clip: the
    clip of the frames before it, nothing is ever summed there) -> (total) int64 numpy."""
    out = np.zeros(total, dtype=np.int64)
    for c, (a, b) in enumerate(clips_host):
        out[int(offsets_host[int(a)]):int(offsets_host[int(b)])] = c
    return out


def check_iou(iou):
    return _frames.within("score", "iou", iou, 0.5, 1.0, "a finite number in [0.5, 1): below one half a match would need an assignment")


def score(pred, gt, split, iou=0.5):
    """The object states ``pred`` scored against ``gt`` (two ``objects.estimate`` results of ``split``) -> ``TrackScore``.

    Usually ``pred`` is the chain with ``which='pred'`` and ``gt`` the one with ``which='gt'``; any two results of the split are
    allowed (two parameter settings, say) as long as they were tracked over the same clips.  The frames selected when clustering
    may differ: a frame one side did not select has no instances there.  In every frame a gt and a predicted instance match iff
    they share a point and ``c / (|G| + |P| - c) > iou`` (c the points they share; the sizes counted from the labels) -- with
    ``iou >= 0.5`` at most one partner passes for either.  A gt track's matches are then walked in frame order: a match whose
    partner belongs to another predicted track than the track's match before is an id switch, one whose instance directly before
    was not matched a fragmentation.
    The outputs are filled once, then there is ONE launch -- one workgroup per clip; nothing waits for the device.
    ValueError, before any launch, for a ``pred`` or ``gt`` that is no ``TrackObjects``, a split they do not belong to, sides with
    different offsets, clips or devices, ``iou`` not finite or outside [0.5, 1); RuntimeError when the split or the tables are not
    on the GPU (no CPU fallback)."""
    for name, side in (("pred", pred), ("gt", gt)):
        if not isinstance(side, TrackObjects):
            raise ValueError("score: %s is an estimate() result, not %s" % (name, type(side).__name__))
    _frames.check_sides(split, pred, gt, "score", "object states")
    iou = check_iou(iou)
    tensors = [("%s %s" % (name, k), t) for name, side in (("pred", pred), ("gt", gt))
               for k, t in (("instances", side.inst.label), ("counts", side.inst.count), ("tracks", side.trk.track), ("states", side.pos))]
    _frames.on_device(split, tensors, "score", "scores")
    dev = split.device
    F, total, C = len(split), split.tab1.shape[0], pred.clips_host.shape[0]
    i32 = torch.int32
    # the int32 outputs are slices of ONE buffer, zero-filled; the three that start at -1 are filled again: 6 fills, not 18
    sizes = [total if k in PER_PRED + PER_GT + PER_TRACK else F if k in PER_FRAME else C for k in KEYS]
    ints = torch.zeros(sum(n for k, n in zip(KEYS, sizes) if k not in ("iou", "iou_units")), dtype=i32, device=dev)
    arrays, at = [], 0
    for k, n in zip(KEYS, sizes):
        if k == "iou":
            arrays.append(torch.zeros(n, dtype=torch.float64, device=dev))
        elif k == "iou_units":
            arrays.append(torch.zeros(n, dtype=torch.int64, device=dev))
        else:
            arrays.append(ints[at:at + n])
            at += n
            if k in ("match", "match_gt", "last_partner"):
                arrays[-1].fill_(-1)
    out = TrackScore(pred, gt, iou, arrays)
    if C == 0:
        return out
    p = _lib.dev_ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cmf_score_tracks(
            C, F, p(pred.clips, i32), p(split.off1, i32), total, iou,
            p(gt.inst.count, i32), p(gt.inst.label, i32), p(gt.trk.track, i32), p(gt.trk.prev_row, i32),
            p(pred.inst.count, i32), p(pred.inst.label, i32), p(pred.trk.track, i32),
            *(p(t, t.dtype) for t in arrays), _lib.stream_ptr()), "cmf_score_tracks")
    return out
