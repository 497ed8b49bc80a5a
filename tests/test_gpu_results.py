"""GPU: a test run's per-frame results kept on the device (cmflow_amd/results.py) -- cmf_pack_results against packing by indexing,
cmf_eval_metrics_frames against eval_batch_ragged frame by frame and batch by batch, test_split / test_split_clips end to end under
torch's synchronisation check, cmf_pose_chain bit for bit against its numpy restatement (tests/results_ref.py) on the reference's
own saved transforms, and the odometry metrics against np.linalg."""
import json
import os

import numpy as np
import pytest
import torch

import results_ref as ref
from cmflow_amd import _lib
from cmflow_amd import dataset as D
from cmflow_amd import eval_util as E
from cmflow_amd import evaluate as EV
from cmflow_amd import results as R
from cmflow_amd import synth
from test_gpu_ragged import _check_against

pytestmark = pytest.mark.gpu
_i32, _i64, _f32, _u8 = torch.int32, torch.int64, torch.float32, torch.uint8
# cloud-1 counts around the wave / vector edge (64) and the pack kernel's chunk (256); cloud 2 differs everywhere
N1 = (1, 37, 63, 64, 65, 300, 8, 129, 256)
N2 = (20, 9, 64, 100, 33, 256, 300, 8, 65)
BATCHES = ([5, 0, 3], [8, 1], [2, 7, 4, 6])             # out of order, uneven: Nmax1 = 300, 256, 129
NO_STATIC, NO_MOVING = 1, 6                             # fg_mask: 1 = static
SENTINEL = 1e30


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _item(f, rng):
    n1, n2 = N1[f], N2[f]
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    mask = (np.arange(n1) % 2 == 0).astype(np.float32)                                  # deterministic: frame 0's one point is static
    if f == NO_STATIC:
        mask[:] = 0
    if f == NO_MOVING:
        mask[:] = 1
    trans = np.eye(4, dtype=np.float32)
    trans[:3] += 0.05 * r(3, 4)
    return (r(n1, 3) + 5, r(n2, 3) + 5, r(n1, 3), r(n2, 3), trans, 0.1 * r(n1, 3), mask, 0.1, r(n1), r(n1), r(n1, 2))


def _fake_outputs(batch, rng, dev):
    """What a network could have returned for ``batch``, with every padded slot holding a sentinel (1e30, mask byte 255)."""
    B, _, N = batch["pc1"].shape
    n1 = batch["n1"].tolist()
    sf = rng.standard_normal((B, 3, N)).astype(np.float32)
    cls = rng.random((B, 1, N)).astype(np.float32)
    mk = (cls[:, 0] > 0.5).astype(np.uint8)
    pt = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    pt[:, :3] += 0.05 * rng.standard_normal((B, 3, 4)).astype(np.float32)
    for s, n in enumerate(n1):
        sf[s, :, n:], cls[s, :, n:], mk[s, n:] = SENTINEL, SENTINEL, 255
    return tuple(torch.from_numpy(a).to(dev) for a in (sf, cls, pt, mk))


def _host_store(res):
    return {k: getattr(res, k).cpu().numpy().copy() for k in ("flow", "score", "mask", "pred_trans", "gt_trans", "done")}


def _nan_equal(a, b):
    """torch.equal with NaN equal to NaN (a frame without static points has NaN metrics, and NaN != NaN): same shape and dtype, NaN
    in the same places, every other value identical."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) \
        and torch.equal(a.nan_to_num(nan=-1.0e300), b.nan_to_num(nan=-1.0e300))


@pytest.fixture(scope="module")
def nine(dev):
    rng = np.random.default_rng(17)
    items = [_item(f, rng) for f in range(9)]
    return items, D.DeviceSplit.from_items(items, dev)


@pytest.fixture(scope="module")
def collected(nine, dev):
    """The three batches through a ResultCollector with sentinel-padded outputs, computed once: (collector, [(batch, outputs)])."""
    _, split = nine
    rng = np.random.default_rng(23)
    col = R.ResultCollector(split)
    seen = []
    for frames in BATCHES:
        batch = split.draw_frames(frames)
        out = _fake_outputs(batch, rng, dev)
        col(batch, out)
        seen.append((batch, out))
    torch.cuda.synchronize()
    return col, seen


# ---- cmf_pack_results ----------------------------------------------------------------------------------------------------------------
def test_pack_is_the_indexing_rule(nine, collected, dev):
    _, split = nine
    col, seen = collected
    res = col.results
    assert [b["pc1"].shape[2] for b, _ in seen] == [300, 256, 129]
    want = _host_store(R.SplitResults.empty(split))
    off1 = split.off1.cpu().numpy()
    for batch, (sf, cls, pt, mk) in seen:
        ref.pack(want, off1, batch["frames"].tolist(), batch["n1"].tolist(), sf.cpu().numpy(), cls[:, 0].cpu().numpy(), mk.cpu().numpy(),
                 pt.cpu().numpy(), batch["gt_trans"].cpu().numpy())
    assert res.flow.shape == (sum(N1), 3) and res.flow.dtype == _f32 and res.mask.dtype == _u8 and res.metrics.dtype == torch.float64
    for k, w in want.items():
        assert torch.equal(getattr(res, k), torch.from_numpy(w).to(dev)), k
    assert float(res.flow.abs().max()) < 1e3 and float(res.score.max()) <= 1.0 and int(res.mask.max()) <= 1        # no sentinel
    assert res.done.tolist() == [1] * 9
    assert torch.equal(res.gt_trans, split.trans.view(9, 4, 4))
    for f in range(9):
        fr = res.frame(f)
        assert fr["flow"].shape == (N1[f], 3) and fr["score"].shape == (N1[f],) and fr["mask"].shape == (N1[f],)


def test_pack_with_a_duplicate_and_an_out_of_range_id_and_without_scores(nine, dev):
    """frames = [3, 3, 11, -2]: the duplicate's two slots hold identical contents (allowed: identical writes), 11 and -2 are clamped to
    frames 8 and 0.  stat_cls = NULL leaves the store's scores as they are."""
    _, split = nine
    rng = np.random.default_rng(29)
    res = R.SplitResults.empty(split)
    res.score.fill_(5.0)
    frames = torch.tensor([3, 3, 11, -2], dtype=_i32, device=dev)
    n1 = torch.tensor([N1[3], N1[3], N1[8], N1[0]], dtype=_i32, device=dev)
    N = 256
    sf = rng.standard_normal((4, 3, N)).astype(np.float32)
    mk = (rng.random((4, N)) < 0.5).astype(np.uint8)
    pt, gt = rng.standard_normal((4, 4, 4)).astype(np.float32), rng.standard_normal((4, 4, 4)).astype(np.float32)
    for a in (sf, mk, pt, gt):
        a[1] = a[0]
    for s, n in enumerate(n1.tolist()):
        sf[s, :, n:], mk[s, n:] = SENTINEL, 255
    want = _host_store(res)
    ref.pack(want, split.off1.cpu().numpy(), frames.tolist(), n1.tolist(), sf, None, mk, pt, gt)
    t = [torch.from_numpy(a).to(dev) for a in (sf, mk, pt, gt)]
    fp, ip, bp = (lambda x: _lib.dev_ptr(x, _f32)), (lambda x: _lib.dev_ptr(x, _i32)), (lambda x: _lib.dev_ptr(x, _u8))
    _lib.check(_lib.lib().cmf_pack_results(4, N, 9, ip(frames), ip(n1), ip(res.off1), res.flow.shape[0], fp(t[0]), None, bp(t[1]), fp(t[2]),
                                           fp(t[3]), fp(res.flow), None, bp(res.mask), fp(res.pred_trans), fp(res.gt_trans), bp(res.done),
                                           _lib.stream_ptr()), "cmf_pack_results")
    for k, w in want.items():
        assert torch.equal(getattr(res, k), torch.from_numpy(w).to(dev)), k
    assert res.done.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 1] and float(res.flow.abs().max()) < 1e3 and int(res.mask.max()) <= 1
    assert bool((res.score == 5.0).all())
    # argument errors: B = 0, nmax = 0, no frame ids
    for args in ((0, N, 9, ip(frames)), (4, 0, 9, ip(frames)), (4, N, 9, None)):
        assert _lib.lib().cmf_pack_results(*args, ip(n1), ip(res.off1), res.flow.shape[0], fp(t[0]), None, bp(t[1]), fp(t[2]), fp(t[3]),
                                           fp(res.flow), None, bp(res.mask), fp(res.pred_trans), fp(res.gt_trans), bp(res.done),
                                           _lib.stream_ptr()) != 0
    # offsets that do not describe the store (total too small for frame 8): that frame is left alone, nothing is written outside
    small = R.SplitResults.empty(split)
    _lib.check(_lib.lib().cmf_pack_results(4, N, 9, ip(frames), ip(n1), ip(small.off1), int(sum(N1[:8])), fp(t[0]), None, bp(t[1]), fp(t[2]),
                                           fp(t[3]), fp(small.flow), None, bp(small.mask), fp(small.pred_trans), fp(small.gt_trans),
                                           bp(small.done), _lib.stream_ptr()), "cmf_pack_results")
    a8 = int(sum(N1[:8]))
    assert not small.flow[a8:].any() and torch.equal(small.flow[:a8], res.flow[:a8])


# ---- cmf_eval_metrics_frames ---------------------------------------------------------------------------------------------------------
def _vector(groups):
    return torch.stack([v for d in groups for v in d.values()])


def test_rows_are_the_frames_own_metrics_and_their_mean_is_the_batchs(nine, collected, dev):
    _, split = nine
    col, seen = collected
    table = col.results.metrics
    assert table.shape == (9, 14) and R.METRIC_KEYS == E.SF_KEYS + E.SEG_KEYS + E.POSE_KEYS
    for batch, (sf, cls, pt, mk) in seen:
        frames, n1 = batch["frames"].tolist(), batch["n1"].tolist()
        B = len(frames)
        whole = _vector(E.eval_batch_ragged(batch["pc1"], sf.transpose(1, 2).contiguous(), batch["flow_label"], batch["fg_mask"], mk.float(),
                                            batch["gt_trans"], pt, batch["n1"]))
        acc = torch.zeros(14, dtype=torch.float64, device=dev)
        for s, f in enumerate(frames):
            acc = acc + table[f]
            one = split.draw_frames([f])
            n = n1[s]
            assert one["pc1"].shape == (1, 3, n)
            alone = _vector(E.eval_batch_ragged(one["pc1"], sf[s:s + 1, :, :n].transpose(1, 2).contiguous(), one["flow_label"], one["fg_mask"],
                                                mk[s:s + 1, :n].float(), one["gt_trans"], pt[s:s + 1], one["n1"]))
            assert _nan_equal(table[f], alone), (f, table[f].tolist(), alone.tolist())
        mean = acc / torch.full((), B, dtype=torch.float64, device=dev)                # a true division (by a Python number torch multiplies by 1 / B)
        assert _nan_equal(mean, whole), (frames, mean.tolist(), whole.tolist())
    stat, fifty, mov = (table[:, R.METRIC_KEYS.index(k)] for k in ("stat_rne", "50-50 rne", "mov_rne"))
    assert torch.isnan(stat).tolist() == [f == NO_STATIC for f in range(9)] and torch.isnan(fifty).tolist() == [f == NO_STATIC for f in range(9)]
    assert float(mov[NO_MOVING]) == 0.0 and float(mov[0]) == 0.0 and bool((mov[[f for f in range(1, 9) if f != NO_MOVING]] > 0).all())
    others = [i for i, k in enumerate(R.METRIC_KEYS) if k not in ("stat_rne", "50-50 rne")]
    assert bool(torch.isfinite(table[:, others]).all())
    # worst: on the device, NaN rows last
    vals, idx = col.results.worst("stat_rne", 9)
    order = sorted((f for f in range(9) if f != NO_STATIC), key=lambda f: -float(stat[f]))
    assert idx.tolist() == order + [NO_STATIC] and idx.is_cuda and torch.isnan(vals[-1])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
class EvalArgs:
    num_points, eval, mini_clip_len, update_len = 256, True, 2, 2


CLIPS = (("test", "delft_2", (90, 140, 64)), ("test", "delft_5", (200, 65, 120, 257, 75, 100)))


def _net(manifest, golden_dir, args, dev, t=False):
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    net = (CMFlow_T if t else CMFlow)(args)
    net.load_state_dict(synth.synth_state_dict(manifest, seed=1234, calib=os.path.join(golden_dir, "bn_calib_cmflow_t.npz" if t else "bn_calib_cmflow.npz")))
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def clip_split(dev, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("results_clips"))
    D.write_synthetic_split(root, seed=9, clips=CLIPS)
    split = D.DeviceSplit.from_dataset(D.vodClipDataset(EvalArgs(), root, "test"), dev)
    assert split.clips == [(0, 3), (3, 9)] and split.counts_host[0].tolist() == [90, 140, 64, 200, 65, 120, 257, 75, 100]
    return split


def _same_five(a, b):
    return all(_nan_equal(x, y) for da, db in zip(a[:3], b[:3]) for x, y in zip(da.values(), db.values())) \
        and all(list(da) == list(db) for da, db in zip(a[:3], b[:3])) \
        and torch.equal(a[3].view(_i32), b[3].view(_i32)) and torch.equal(a[4].view(_i32), b[4].view(_i32))


def _same_store(a, b):
    return all(_nan_equal(getattr(a, k), getattr(b, k)) for k in R._FIELDS) and a.clips == b.clips


def _under_sync_check(split, run):
    """``run()`` with every host wait for the device an error, and the control: a read-back IS caught in that mode."""
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = run()
        with pytest.raises(RuntimeError):
            split.off1.cpu()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    return out


def test_test_split_keeps_every_frame_and_never_waits(clip_split, dev, manifest, golden_dir, args):
    split = clip_split
    net = _net(manifest, golden_dir, args, dev)
    plain = EV.eval_split(net, split, 4, sort_by_size=True)
    calls = []
    five, res = EV.test_split(net, split, 4, sort_by_size=True, on_batch=lambda b, o: calls.append(len(o)))
    assert calls == [4, 4, 4]                                                           # a user's own hook is still called
    assert isinstance(res, R.SplitResults) and res.clips == split.clips and res.done.tolist() == [1] * 9
    assert _same_five(five, plain)
    assert torch.equal(res.pred_trans.view(_i32), plain[4].view(_i32)) and torch.equal(res.gt_trans.view(_i32), plain[3].view(_i32))
    # the epoch's metrics are the mean of the rows (up to the order of the float64 sum: batches weigh in as B * mean)
    epoch = torch.stack([v for d in five[:3] for v in d.values()])
    np.testing.assert_allclose(res.metrics.mean(0).cpu().numpy(), epoch.cpu().numpy(), rtol=1e-13, atol=0)
    # frame(i) is the frame's own B = 1 forward, within the bounds test_gpu_ragged.py uses for that statement
    n1 = split.counts_host[0]
    with torch.no_grad():
        for f in range(9):
            one = split.draw_frames([f])
            want = net.forward_ragged(one["pc1"], one["pc2"], one["ft1"], one["ft2"], one["n1"], one["n2"])
            fr = res.frame(f)
            got = (fr["flow"].t()[None], fr["score"][None, None], fr["pred_trans"][None], fr["mask"].bool()[None])
            _check_against(got, 0, int(n1[f]), want, "frame(%d) vs its own B = 1 forward" % f)
    # warm, under the synchronisation check: collecting adds launches only
    five2, res2 = _under_sync_check(split, lambda: EV.test_split(net, split, 4, sort_by_size=True))
    assert _same_five(five2, plain) and _same_store(res2, res)

    # two ranks' collectors over their shares of the sweep, merged, are the single sweep
    def sweep(rank, world):
        col = R.ResultCollector(split)
        with torch.no_grad():
            for b in split.sweep(2, False, rank, world):
                col(b, net.forward_ragged(b["pc1"], b["pc2"], b["ft1"], b["ft2"], b["n1"], b["n2"]))
        return col.results
    parts, single = [sweep(0, 2), sweep(1, 2)], sweep(0, 1)
    assert parts[0].done.tolist() == [1, 1, 0, 0, 1, 1, 0, 0, 1] and parts[1].done.tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 0]
    assert _same_store(parts[0].merge(parts[1]), single) and single.done.tolist() == [1] * 9
    with pytest.raises(ValueError):
        single.merge(parts[0])


def test_test_split_clips_keeps_every_frame_and_never_waits(clip_split, dev, manifest_t, golden_dir, args):
    split = clip_split
    net = _net(manifest_t, golden_dir, args, dev, t=True)
    plain = EV.eval_split_clips(net, split, 3, 2)
    kept = {}

    def keep(b, o):
        assert len(o) == 5
        for s, f in enumerate(b["frames"].tolist()):
            n = int(b["n1"][s])
            kept[f] = (o[0][s, :, :n].t().clone(), o[1][s, 0, :n].clone(), o[2][s].clone(), o[3][s, :n].clone())
    five, res = EV.test_split_clips(net, split, 3, 2, on_batch=keep)
    assert _same_five(five, plain) and res.done.tolist() == [1] * 9 and sorted(kept) == list(range(9))
    for f, (sf, cls, pt, mk) in kept.items():
        fr = res.frame(f)
        assert torch.equal(fr["flow"], sf) and torch.equal(fr["score"], cls) and torch.equal(fr["pred_trans"], pt) and torch.equal(fr["mask"].bool(), mk), f
    five2, res2 = _under_sync_check(split, lambda: EV.test_split_clips(net, split, 3, 2))
    assert _same_five(five2, plain) and _same_store(res2, res)
    # the chained ego-motion of the run: every frame lies in a clip, so every pose is defined
    poses = res.trajectories("pred")
    assert poses.shape == (9, 4, 4) and poses.dtype == torch.float64 and bool(torch.isfinite(poses).all())
    assert np.array_equal(poses.cpu().numpy(), ref.pose_chain(res.pred_trans.cpu().numpy(), split.clips))


# ---- the pose chain and the odometry metrics -----------------------------------------------------------------------------------------
CHAIN_CLIPS = [(0, 1), (1, 3), (3, 3), (6, 71), (71, 408)]         # lengths 1, 2, 0, 65, 337; frames 3-5 lie in no clip
CHAIN_F = 408


def _rotation(axis, deg):
    a, (x, y, z) = np.radians(deg), np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


@pytest.fixture(scope="module")
def chain_store(dev, golden_dir):
    """Predicted transforms: the reference's 337 saved ``pred_t`` of delft_12 as the last clip, before it small random motions with
    rotations off orthonormal by about 3e-4 like the saved ones.  'Ground truth': every prediction followed by a fixed 1 degree /
    0.23 m error, so that the relative rotation error of any pair of frames D apart is about D degrees -- away from 0 and 180."""
    rng = np.random.default_rng(31)
    saved = np.load(os.path.join(golden_dir, "saved_pred_t_delft_12.npz"))["pred_t"]
    assert saved.shape == (337, 4, 4) and saved.dtype == np.float32
    T = np.tile(np.eye(4), (CHAIN_F, 1, 1))
    for k in range(71):
        T[k, :3, :3] = _rotation(rng.standard_normal(3), rng.uniform(0.2, 3.0)) + 3e-4 * rng.standard_normal((3, 3))
        T[k, :3, 3] = rng.standard_normal(3) * (0.5, 0.1, 0.02)
    T = T.astype(np.float32)
    T[71:] = saved
    err = np.eye(4)
    err[:3, :3], err[:3, 3] = _rotation((0.2, 0.1, 1.0), 1.0), (0.2, -0.1, 0.05)
    G = (err @ T.astype(np.float64)).astype(np.float32)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    res = R.SplitResults(torch.arange(CHAIN_F + 1, dtype=_i32, device=dev), z((CHAIN_F, 3), _f32), z((CHAIN_F,), _f32), z((CHAIN_F,), _u8),
                         torch.from_numpy(T).to(dev), torch.from_numpy(G).to(dev),
                         torch.full((CHAIN_F, 14), float("nan"), dtype=torch.float64, device=dev), z((CHAIN_F,), _u8), CHAIN_CLIPS)
    return res, T, G


def test_pose_chain_is_its_definition_bit_for_bit(chain_store, dev):
    res, T, G = chain_store
    R3 = T[71:, :3, :3].astype(np.float64)
    off = np.abs(R3 @ R3.transpose(0, 2, 1) - np.eye(3)).max()
    assert 1e-5 < off < 5e-3, off                                                       # the saved rotations are not orthonormal
    for which, src in (("pred", T), ("gt", G)):
        poses = res.trajectories(which)
        assert poses.shape == (CHAIN_F, 4, 4) and poses.dtype == torch.float64 and poses.device == res.device
        got, want = poses.cpu().numpy(), ref.pose_chain(src, CHAIN_CLIPS)
        inside = np.array([any(a <= k < b for a, b in CHAIN_CLIPS) for k in range(CHAIN_F)])
        assert inside.sum() == 405 and np.isnan(got[~inside]).all()                     # frames 3-5: still the caller's NaN
        assert np.array_equal(got[inside].view(np.int64), want[inside].view(np.int64)), np.abs(got[inside] - want[inside]).max()
        assert (got[inside][:, 3] == (0, 0, 0, 1)).all()
        assert np.array_equal(got[0, :3], ref.rigid_inverse(src[0])[:3])                # a clip's first pose: inv(T) itself
    # a store without clip ranges is one clip over all frames
    plain = R.SplitResults(*(getattr(res, k) for k in R._FIELDS), None)
    assert np.array_equal(plain.trajectories().cpu().numpy().view(np.int64), ref.pose_chain(T, [(0, CHAIN_F)]).view(np.int64))
    # clip ranges reaching outside the frames are clamped; no clips, no launch
    wide = torch.tensor([[-5, 2], [400, 500]], dtype=_i32, device=dev)
    poses = torch.full((CHAIN_F, 16), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().cmf_pose_chain(CHAIN_F, 2, _lib.dev_ptr(res.pred_trans.view(-1, 16), _f32), _lib.dev_ptr(wide, _i32), poses.data_ptr(),
                                         _lib.stream_ptr()), "cmf_pose_chain")
    want = ref.pose_chain(T, [(-5, 2), (400, 500)])
    assert np.array_equal(np.isnan(poses.cpu().numpy()).reshape(CHAIN_F, 4, 4), np.isnan(want))
    assert np.array_equal(poses.cpu().numpy().reshape(CHAIN_F, 4, 4)[400:].view(np.int64), want[400:].view(np.int64))
    assert _lib.lib().cmf_pose_chain(CHAIN_F, 0, None, None, None, _lib.stream_ptr()) == 0


def test_odometry_metrics_against_numpy(chain_store, dev):
    """Relative 1e-12: every number is a sum of at most 337 float64 terms of one sign (each term within a few ulp of numpy's), or a
    square root / quotient of one."""
    res, T, G = chain_store
    P64, G64 = ref.pose_chain(T, CHAIN_CLIPS), ref.pose_chain(G, CHAIN_CLIPS)
    want = ref.odometry_metrics(P64, G64, CHAIN_CLIPS, (1, 10))
    lo, hi = want["angle_range"]
    print("pair angles between %.4g and %.4g degrees" % (lo, hi))
    assert 0.5 <= lo and hi <= 30.0                                                     # away from 0 and 180, by construction
    mode = torch.cuda.get_sync_debug_mode()
    res.trajectories()                                                                  # the clip ranges go to the device once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = res.odometry_metrics()                                                    # default deltas (1, 10); nothing read back
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert list(got["clips"]) == list(want["clips"]) == list(got["overall"])
    for k, w in want["clips"].items():
        g = got["clips"][k]
        assert g.shape == (5,) and g.dtype == torch.float64 and g.is_cuda
        print(k, g.tolist(), w.tolist())
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
        o = got["overall"][k]
        assert o.dim() == 0 and o.dtype == torch.float64 and o.is_cuda
        np.testing.assert_allclose(float(o), want["overall"][k], rtol=1e-12, atol=0, err_msg="overall " + k)
    c = want["clips"]
    assert np.isnan(c["end_error"][2]) and c["path_length"][2] == 0 and np.isnan(c["rpe_trans_1"][0]) and np.isnan(c["rpe_trans_10"][1])
    assert np.isfinite(c["rpe_rot_10"][3:]).all() and np.isfinite(c["rpe_rot_1"][1])


def test_store_goes_through_rccl_unchanged(nine, collected, dev):
    """SplitResults.all_reduce over backend 'nccl' (= RCCL; world size 1 on a 1-GPU box): the byte and float64 tensors go through the
    collective, an evaluated frame's NaN metric and an unevaluated frame's NaN row both survive.  The two-rank rule itself is checked
    on the CPU (tests/test_results_host.py)."""
    import torch.distributed as dist
    _, split = nine
    res = collected[0].results
    part = R.SplitResults(*(getattr(res, k).clone() for k in R._FIELDS), res.clips)
    a, b = int(split.off1[4]), int(split.off1[5])
    part.flow[a:b], part.score[a:b], part.mask[a:b], part.pred_trans[4], part.gt_trans[4], part.done[4] = 0, 0, 0, 0, 0, 0
    part.metrics[4] = float("nan")                                                      # frame 4: nobody evaluated it
    want = R.SplitResults(*(getattr(part, k).clone() for k in R._FIELDS), res.clips)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        assert part.all_reduce() is part
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert _same_store(part, want)
    assert torch.isnan(part.metrics[4]).all() and torch.isnan(part.metrics[NO_STATIC, 3]) and part.done.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def test_save_load_and_write_json_of_a_gpu_store(nine, collected, dev, tmp_path):
    _, split = nine
    res = collected[0].results
    path = str(tmp_path / "results.pt")
    res.save(path)
    back = R.SplitResults.load(path, dev)
    assert _same_store(back, res) and back.device == res.device
    assert _same_store(R.SplitResults.load(path, "cpu").to(dev), res)
    paths = res.write_json(str(tmp_path / "json"), split)
    assert [os.path.relpath(p, str(tmp_path / "json")) for p in paths] == ["clip_0/%d.json" % f for f in range(9)]
    f32 = lambda v: torch.tensor(v, dtype=_f32, device=dev)
    for f, p in enumerate(paths):
        got, fr = json.load(open(p)), res.frame(f)
        assert list(got) == ["pc1", "pc2", "pred_f", "pred_m", "pred_t"]
        assert torch.equal(f32(got["pred_f"]).reshape(3, -1).t(), fr["flow"]) and torch.equal(f32(got["pred_m"]), fr["mask"].float())
        assert torch.equal(f32(got["pred_t"]), fr["pred_trans"])
        a, b, c, d = (int(x) for x in (split.off1[f], split.off1[f + 1], split.off2[f], split.off2[f + 1]))
        assert torch.equal(f32(got["pc1"]).reshape(3, -1).t(), split.tab1[a:b, :3]) and torch.equal(f32(got["pc2"]).reshape(3, -1).t(), split.tab2[c:d, :3])
    part = R.SplitResults.empty(split)
    with pytest.raises(ValueError):
        part.write_json(str(tmp_path / "none"), split)
