"""GPU: a test run's tracks and objects scored against the labels' (cmflow_amd/score.py) -- cmf_score_tracks bit for bit against its
numpy restatement (tests/score_ref.py) on a clustered, tracked and smoothed world for both pairings and two thresholds, the
hand-built clip that holds every case once, frames at the kernel's edges (0, 1, 63, 64, 65 and 1024 points, an empty clip, a
one-frame clip), the C entry point on corrupted tables with sentinel-filled and oversized buffers and its refusals, the store's
shorthand, the views and the derived numbers, and that none of it waits for the device.  Every comparison with the restatement is
exact: integers equal, ``iou`` as uint64."""
import numpy as np
import pytest
import torch

import instances_ref as iref
import objects_ref as oref
import score_ref as ref
from cmflow_amd import _lib
from cmflow_amd import dataset as D
from cmflow_amd import instances as I
from cmflow_amd import objects as O
from cmflow_amd import results as R
from cmflow_amd import score as S
from cmflow_amd import tracks as K

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TORCH = {np.int32: torch.int32, np.int64: torch.int64, f64: torch.float64}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """The world of objects_ref on the device with its two clips, the store filled from it, and both sides' object states."""
    frames, owners, truth = oref.build_world(flow_noise=0.01)
    split = D.DeviceSplit.from_items(iref.as_items(frames), dev, [tuple(c) for c in oref.WORLD_CLIPS])
    store = R.SplitResults.empty(split)
    store.flow.copy_(torch.from_numpy(np.concatenate([fr["flow"] for fr in frames])))
    store.mask.copy_(torch.from_numpy(np.concatenate([fr["mask"] for fr in frames])))
    store.pred_trans.copy_(torch.from_numpy(np.stack([fr["pred_t"] for fr in frames])))
    store.done.fill_(1)
    sides = {}
    for which in ("pred", "gt"):
        st = store if which == "pred" else None
        trk = K.track(I.cluster(split, st, which=which), split, st, gate=oref.GATE, max_gap=2)
        sides[which] = O.estimate(trk, split, st)
    return frames, split, store, sides


def _host(sc):
    return {k: getattr(sc, k).cpu().numpy() for k in ref.KEYS}


def _tables(obj):
    """What the call reads of a side, read back from the device."""
    return {"count": obj.inst.count.cpu().numpy(), "label": obj.inst.label.cpu().numpy(), "track": obj.trk.track.cpu().numpy(),
            "prev_row": obj.trk.prev_row.cpu().numpy()}


def _restated(pred, gt, iou):
    off1 = pred.off.cpu().numpy()
    return ref.score(off1, int(off1[-1]), pred.clips_host, iou, _tables(gt), _tables(pred))


# ---- 1. bit for bit on the world ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iou", [0.5, 0.75])
@pytest.mark.parametrize("pairing", [("pred", "gt"), ("gt", "gt")])
def test_score_is_the_restatement(world, pairing, iou):
    frames, split, store, sides = world
    pred, gt = sides[pairing[0]], sides[pairing[1]]
    sc = S.score(pred, gt, split, iou=iou)
    assert sc.match.is_cuda and sc.iou.dtype == torch.float64 and sc.iou_units.dtype == torch.int64 and len(sc) == 2 and sc.iou_min == iou
    got, want = _host(sc), _restated(pred, gt, iou)
    ref.same(got, want, (pairing, iou))
    assert want["tp"].sum() > 80 and (want["seen"] > 0).sum() == 11       # the world is what it is for: 11 gt tracks
    if pairing[0] == pairing[1]:
        assert not want["fp"].any() and not want["fn"].any() and not want["ids"].any() and (want["iou_units"] == want["tp"].astype(np.int64) * ref.IOU_UNIT).all()


# ---- tables of our own making through the public call ------------------------------------------------------------------------------------
class Rows:
    """What ``score`` asks of a split -- its frames, its rows, its offsets, its device -- for tables with an EMPTY frame, which a
    DeviceSplit refuses to hold (a frame without points is no sample)."""

    def __init__(self, off1, dev):
        self.off1 = torch.from_numpy(np.asarray(off1, dtype=np.int32)).to(dev)
        self.tab1 = torch.zeros((int(off1[-1]), 3), dtype=torch.float32, device=dev)
        self.device = dev

    def __len__(self):
        return self.off1.numel() - 1

    def _need_gpu(self, what):
        assert self.tab1.is_cuda


def _side(rows, off1, t, which, clips):
    """A TrackObjects on the device around the tables ``t`` (count, label, track, prev_row); everything the score does not read: zeros."""
    dev, total, F = rows.device, int(off1[-1]), len(off1) - 1
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
    fl, f8 = torch.float32, torch.float64
    interval = torch.full((F,), 0.1, device=dev)
    inst = I.FrameInstances(rows.off1, torch.arange(F, device=dev), up(t["label"]), z(total, dt=torch.uint8), up(t["count"]),
                            (z(total), z(total), z(total, 3, dt=fl), z(total, 3, dt=fl), z(total, 3, dt=fl), z(total, 3, dt=fl)), interval, which, 2.0, 2, 0.0,
                            np.asarray(off1, dtype=np.int64), np.arange(F))
    clips = np.asarray(clips, dtype=np.int32).reshape(-1, 2)
    arrays = (up(t["track"]), up(t["prev_row"]), z(total), z(total), z(total, 3, dt=fl), z(total) - 1, z(total) - 1, z(total) - 1, z(total))
    trk = K.InstanceTracks(inst, arrays, z(len(clips)), z(len(clips)), up(clips), clips, 2.0, 2)
    states = (z(total) - 1, z(total) - 1, z(total, 6, dt=f8), z(total, 3, dt=f8), z(total, 6, dt=f8), z(total, 3, dt=f8), z(total, 3, dt=fl), z(total, 3, dt=fl),
              z(total, 2, dt=fl), z(total) - 1, z(total, 3, dt=fl), z(total, 3, dt=fl))
    return O.TrackObjects(trk, states, z(F, 16, dt=f8), z(F, dt=torch.int64), interval, *oref.PARAMS)


def test_hand_built_clip_through_the_public_call(dev):
    off1, total, gt, pred, want = ref.hand_clip()
    F = len(off1) - 1
    rows = Rows(off1, dev)
    sides = _side(rows, off1, pred, "pred", [(0, F)]), _side(rows, off1, gt, "gt", [(0, F)])
    for iou in (0.5, 0.7):
        got = _host(S.score(*sides, rows, iou=iou))
        ref.same(got, ref.score(off1, total, [(0, F)], iou, gt, pred), iou)
    got = _host(S.score(*sides, rows))
    assert [tuple(int(got[k][f]) for k in ref.PER_FRAME) for f in range(F)] == want["frame"]
    assert np.flatnonzero(got["switch"]).tolist() == want["switch"] and np.flatnonzero(got["frag"]).tolist() == want["frag"]
    assert {k: int(got[k][0]) for k in want["clip"]} == want["clip"] and int(got["iou_units"][0]) == want["units"]
    assert tuple(int(_host(S.score(*sides, rows, iou=0.7))[k][1]) for k in ref.PER_FRAME) == want["iou_07"]


def test_sizes_at_the_kernels_edges(dev):
    off1, total, clips, gt, pred = ref.edge_tables()
    rows = Rows(off1, dev)
    sides = _side(rows, off1, pred, "pred", clips), _side(rows, off1, gt, "gt", clips)
    for iou in (0.5, 0.75):
        got = _host(S.score(*sides, rows, iou=iou))
        ref.same(got, ref.score(off1, total, clips, iou, gt, pred), iou)
    got = _host(S.score(*sides, rows))
    assert tuple(got[k][5] for k in ref.PER_FRAME) == (0, 512, 1) and tuple(got[k][6] for k in ref.PER_FRAME) == (0, 341, 341)
    assert got["tp"].tolist() == [45, 0, 2] and got["gt_total"].tolist() == [408, 0, 2]
    # the other way round, a side against itself: 1024 points in one instance, 512 matches in one frame
    ref.same(_host(S.score(sides[1], sides[0], rows)), ref.score(off1, total, clips, 0.5, pred, gt), "swapped")
    own = _host(S.score(sides[0], sides[0], rows))
    ref.same(own, ref.score(off1, total, clips, 0.5, pred, pred), "itself")
    assert own["frame_tp"][5] == 512 and own["frame_tp"][6] == 341 and not own["fp"].any()


# ---- 2. the C entry point on corrupted tables and sentinel-filled buffers ---------------------------------------------------------------
SENTINEL = {k: -90 - i for i, k in enumerate(ref.KEYS)}


def _call(dev, off1, total, clips, iou, gt, pred, rows):
    """cmf_score_tracks itself; outputs of ``rows`` rows (F + 64 frames, C + 64 clips), sentinel-filled."""
    i32 = torch.int32
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(i32).to(dev)
    F, C = len(off1) - 1, len(clips)
    clips_d, off_d = up(np.asarray(clips, dtype=np.int32).reshape(-1, 2)), up(off1)
    ins = [up(gt[k]) for k in ref.GT_TABLES] + [up(pred[k]) for k in ref.GT_TABLES[:3]]
    size = lambda k: rows if k in ref.PER_ROW else F + 64 if k in ref.PER_FRAME else C + 64
    out = {k: torch.full((size(k),), SENTINEL[k], dtype=TORCH[ref.dtype_of(k)], device=dev) for k in ref.KEYS}
    p = _lib.dev_ptr
    _lib.check(_lib.lib().cmf_score_tracks(C, F, p(clips_d, i32), p(off_d, i32), total, float(iou), *(p(t, i32) for t in ins),
                                           *(p(out[k], out[k].dtype) for k in ref.KEYS), _lib.stream_ptr()), "cmf_score_tracks")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sentinel_outputs(rows, F, C):
    return ref.outputs(rows, F + 64, C + 64, SENTINEL)


def test_entry_point_bounds_itself_on_corrupted_tables(dev):
    """Nothing here can fault: a label indexes a table only after it is clamped to the frame's K, a track only inside the clip's solid
    rows, prev_row only inside them before the frame (include/cmflow_hip.h), and tests/test_score_host.py takes the same tables
    through the restatement on the CPU."""
    frames, owners, sides = ref.tracking_world()
    off1, total, clips, gt, pred = ref.corrupt_tables(sides)
    F, C, rows = len(off1) - 1, len(clips), sides["gt"]["total"] + 64
    got = _call(dev, off1, total, clips, 0.5, gt, pred, rows)
    want = ref.score(off1, total, clips, 0.5, gt, pred, out=_sentinel_outputs(rows, F, C))
    ref.same(got, want, "corrupted")
    owned = ref.owned_rows(off1, total, clips, rows)
    for k in ref.PER_ROW:
        assert (got[k][~owned] == SENTINEL[k]).all() and (got[k][owned] != SENTINEL[k]).all(), k      # sentinels outside owned rows stay intact
    for k in ref.PER_FRAME:
        assert (got[k][F:] == SENTINEL[k]).all() and (got[k][:F] != SENTINEL[k]).all(), k
    for k in ref.PER_CLIP:
        assert (got[k][C:] == SENTINEL[k]).all() and (got[k][:C] != SENTINEL[k]).all(), k
    # the clean tables through the same call, sentinel-filled: the world's own clips, every frame owned
    clean_off, clean_total = sides["gt"]["off1"], sides["gt"]["total"]
    got = _call(dev, clean_off, clean_total, ref.tref.WORLD_CLIPS, 0.5, ref.side(sides["gt"]), ref.side(sides["pred"]), rows)
    want = ref.score(clean_off, clean_total, ref.tref.WORLD_CLIPS, 0.5, ref.side(sides["gt"]), ref.side(sides["pred"]), out=_sentinel_outputs(rows, F, 2))
    ref.same(got, want, "clean")
    assert all((got[k][clean_total:] == SENTINEL[k]).all() and (got[k][:clean_total] != SENTINEL[k]).all() for k in ref.PER_ROW)
    assert got["ids"][:2].tolist() == [1, 0] and got["frags"][:2].tolist() == [2, 0]
    # refusals of the entry point itself: nothing is launched
    z = torch.zeros(8, dtype=torch.int32, device=dev)
    zd, zl = torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
    i = _lib.dev_ptr(z, torch.int32)
    args = lambda iou, **null: [1, 1, i, i, 4, iou] + [i] * 7 + [None if null.get("match") else i, i, None if null.get("overlap") else zd.data_ptr()] + [i] * 14 \
        + [None if null.get("units") else zl.data_ptr(), _lib.stream_ptr()]
    entry = _lib.lib().cmf_score_tracks
    for iou in (float("nan"), 0.4999, 0.0, 1.0, 1.5, -1.0, float("inf")):
        assert entry(*args(iou)) != 0, iou
    for null in ("match", "overlap", "units"):
        assert entry(*args(0.5, **{null: True})) != 0, null
    bad = args(0.5)
    bad[2] = None                                                           # no clips
    assert entry(*bad) != 0
    bad = args(0.5)
    bad[4] = -1                                                             # total
    assert entry(*bad) != 0
    torch.cuda.synchronize()
    assert not z.any() and not zd.any() and not zl.any()


# ---- 3. the store's shorthand, the views and the derived numbers --------------------------------------------------------------------------
def test_store_shorthand_views_and_derived_numbers(world):
    frames, split, store, sides = world
    opts = dict(eps=1.5, min_points=3, gate=1.5, max_gap=1, sigma_pos=0.4)
    pred, gt = store.objects(split, which="pred", **opts), store.objects(split, which="gt", **opts)
    want = _host(S.score(pred, gt, split, iou=0.6))
    sc = store.score_tracks(split, iou=0.6, **opts)
    ref.same(_host(sc), want, "store.score_tracks")
    assert (sc.iou_min, sc.pred.which, sc.gt.which, sc.pred.sigma_pos, sc.gt.trk.max_gap) == (0.6, "pred", "gt", 0.4, 1)
    ref.same(_host(store.score_tracks(split, iou=0.6, pred=pred, gt=gt)), want, "given")
    ref.same(_host(store.score_tracks(split, iou=0.6, gt=gt, **opts)), want, "one given")
    ref.same(want, _restated(pred, gt, 0.6), "restated")
    # the views and the derived numbers against numpy
    out, off = want, pred.offsets_host
    for f in (0, 6, 12):
        a, Kp, Kg = int(off[f]), int(pred.inst.count[f]), int(gt.inst.count[f])
        view = sc.frame(f)
        assert view["match"].shape == (Kp,) and view["switch"].shape == (Kg,) and torch.equal(view["iou"], sc.iou[a:a + Kp])
        assert (int(view["tp"]), int(view["fp"]), int(view["fn"])) == tuple(int(out[k][f]) for k in ref.PER_FRAME)
    missed = out["frame_fp"].astype(np.int64) + out["frame_fn"]
    order = sorted(range(len(missed)), key=lambda f: (-missed[f], f))
    top, values = sc.worst(5)
    assert top.is_cuda and top.tolist() == order[:5] and values.tolist() == [int(missed[f]) for f in order[:5]]
    clip_of_row = sc.clip_of_row.cpu().numpy()
    got, numpy_says = sc.summary(), ref.summary_numpy(out, clip_of_row)
    for k, v in numpy_says.items():
        if k != "all":
            assert got[k].is_cuda and np.array_equal(got[k].cpu().numpy(), v, equal_nan=True), k
    for k, v in numpy_says["all"].items():
        assert np.array_equal(got["all"][k].cpu().numpy(), v, equal_nan=True), k
    errs = sc.state_errors()
    states = [{k: getattr(s, k).cpu().numpy() for k in oref.KEYS} for s in (pred, gt)]
    got = {k: {m: errs[k][m].cpu().numpy() for m in ("mean", "max")} for k in ref.STATE_KEYS + ("heading",)}
    ref.check_errors(got, ref.errors_numpy(out, *states, clip_of_row, 2), 2)
    assert errs["count"].tolist() == out["tp"].tolist() and 0 < got["pos"]["max"].max() < 0.5


# ---- 4. nothing waits for the device ----------------------------------------------------------------------------------------------------
def test_no_call_waits_for_the_device(world):
    frames, split, store, sides = world
    warm = S.score(sides["pred"], sides["gt"], split)                       # warm: library, allocator
    warm.summary(), warm.state_errors(), warm.worst(3)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sc = S.score(sides["pred"], sides["gt"], split, iou=0.75)
        summary, errors, worst = sc.summary(), sc.state_errors(), sc.worst(3)
        with pytest.raises(RuntimeError):
            split.off1.cpu()                                               # the control: a read-back IS caught in this mode
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    ref.same(_host(sc), _restated(sides["pred"], sides["gt"], 0.75), "no wait")
    assert summary["MOTSA"].shape == (2,) and errors["pos"]["mean"].shape == (2,) and worst[0].shape == (3,)
