"""GPU: whole frames from a DeviceSplit -- cmf_draw_frames / draw_frames against the host assembly of the ORIGINAL items
(collate_ragged -> extract_data_info_ragged -> as_batch_dict_ragged), bit for bit; epoch_ragged feeding TrainStep.step_ragged; and the
evaluation epochs of cmflow_amd/evaluate.py against (a) the same protocol written out in the test on host-collated batches (bit-equal)
and (b) the reference's protocol itself: one frame per forward at B = 1 (dense forward / the CPU oracle's CMFlow_T)."""
import os

import numpy as np
import pytest
import torch

from cmflow_amd import dataset as D
from cmflow_amd import eval_util as E
from cmflow_amd import evaluate as EV
from cmflow_amd import synth
from oracle import cmflow_oracle as O

pytestmark = pytest.mark.gpu
_i32 = torch.int32
# the wave (64) and chunk (256) edges of cmf_draw_frames and the model's cap (1024)
N1 = [1, 7, 63, 64, 65, 255, 256, 257, 1000, 1024]
N2 = [257, 1024, 1, 256, 1000, 7, 65, 63, 255, 64]
FRAMES = list(range(10)) + [3, 3, 0, 9]               # B = 14: every frame, some repeated
CAP = D.DRAW_MAX_POINTS
KEYS = D.DeviceSplit.KEYS
RAGGED_KEYS = (*KEYS, "n1", "n2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float32), 0.1 + 0.01 * n1,
            r(n1), r(n1), r(n1, 2))


def host_batch(items, frames, dev):
    """The yardstick: the existing host path on the original items."""
    return D.as_batch_dict_ragged(D.extract_data_info_ragged(D.collate_ragged([items[f] for f in frames]), device=dev))


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(_i32), b.contiguous().view(_i32))


def _assert_is_host_batch(out, want, what=""):
    assert list(out) == [*want, "frames"], list(out)                                   # key order, frames last
    for k, w in want.items():
        assert out[k].shape == w.shape and out[k].dtype == w.dtype and out[k].device == w.device and out[k].is_contiguous(), (what, k)
        assert _bits_equal(out[k], w), (what, k)
    assert out["n1"].dtype == _i32 and out["n2"].dtype == _i32 and out["frames"].dtype == _i32


@pytest.fixture(scope="module")
def small(dev):
    rng = np.random.default_rng(7)
    items = [_item(a, b, rng) for a, b in zip(N1, N2)]
    return items, D.DeviceSplit.from_items(items, dev)


def test_frames_are_the_host_assembly_bit_for_bit(small, dev):
    items, gpu = small
    out = gpu.draw_frames(FRAMES)
    want = host_batch(items, FRAMES, dev)
    assert out["pc1"].shape == (14, 3, 1024) and out["pc2"].shape == (14, 3, 1024) and out["flow_label"].shape == (14, 1024, 3)
    _assert_is_host_batch(out, want)
    assert out["n1"].tolist() == [N1[f] for f in FRAMES] and out["n2"].tolist() == [N2[f] for f in FRAMES]
    assert out["frames"].tolist() == FRAMES
    for frames in ([0], [2, 0], [5, 6, 7], [4, 1, 3]):                                 # other maxima: 1/257, 63/257, 257/65, 65/1024
        _assert_is_host_batch(gpu.draw_frames(frames), host_batch(items, frames, dev), frames)
    assert gpu.draw_frames([5, 6, 7])["pc1"].shape == (3, 3, 257) and gpu.draw_frames([5, 6, 7])["pc2"].shape == (3, 3, 65)


def test_nmax_given_and_frames_on_the_device(small, dev):
    items, gpu = small
    frames = [5, 6, 7, 0]
    want = host_batch(items, frames, dev)                                              # maxima 257 / 257
    out = gpu.draw_frames(frames, nmax1=300, nmax2=513)
    assert out["pc1"].shape == (4, 3, 300) and out["pc2"].shape == (4, 3, 513) and out["opt_flow"].shape == (4, 300, 2)
    assert torch.equal(out["n1"], want["n1"]) and torch.equal(out["n2"], want["n2"])   # the counts do not change
    for k in ("pc1", "ft1", "pc2", "ft2"):
        m = want[k].shape[2]
        assert _bits_equal(out[k][:, :, :m], want[k]), k
        assert _bits_equal(out[k][:, :, m:], out[k][:, :, :1].expand(-1, -1, out[k].shape[2] - m)), k       # the extra slots: row 0
    for k in ("flow_label", "fg_mask", "radar_u", "radar_v", "opt_flow"):
        assert _bits_equal(out[k][:, :257], want[k]), k
        assert _bits_equal(out[k][:, 257:], out[k][:, :1].expand(-1, 43, *out[k].shape[2:])), k
    assert _bits_equal(out["gt_trans"], want["gt_trans"]) and _bits_equal(out["interval"], want["interval"])
    # frames on the device: nothing is read back, the sizes are the split's maxima per cloud
    c1, c2 = gpu.counts_host                                                           # the one copy of the split's lifetime
    on_dev = torch.tensor(frames, dtype=torch.int64, device=dev)
    wide = gpu.draw_frames(frames, nmax1=int(c1.max()), nmax2=int(c2.max()))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = gpu.draw_frames(on_dev)
        given = gpu.draw_frames(on_dev.to(_i32), nmax1=300, nmax2=513)
        with pytest.raises(RuntimeError):
            gpu.off1.cpu()                                                             # the control: a read-back is caught here
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert got["pc1"].shape == (4, 3, 1024) and got["pc2"].shape == (4, 3, 1024)
    assert all(_bits_equal(got[k], wide[k]) for k in wide) and all(_bits_equal(given[k], out[k]) for k in out)
    # a frame larger than a size given with device frames is truncated, and the counts say so
    cut = gpu.draw_frames(torch.tensor([8, 0], dtype=_i32, device=dev), nmax1=100, nmax2=50)
    assert cut["n1"].tolist() == [100, 1] and cut["n2"].tolist() == [50, 50]
    assert _bits_equal(cut["pc1"][0], torch.from_numpy(items[8][0][:100].T.copy()).to(dev))


def test_frames_at_the_cap(dev):
    """16384 and 16383 points: 64 chunks per cloud and slot, the last one a position short."""
    rng = np.random.default_rng(8)
    items = [_item(CAP, CAP - 1, rng), _item(CAP - 1, CAP, rng)]
    gpu = D.DeviceSplit.from_items(items, dev)
    _assert_is_host_batch(gpu.draw_frames([0, 1, 1]), host_batch(items, [0, 1, 1], dev))
    only = gpu.draw_frames([1, 1, 1])
    assert only["pc1"].shape == (3, 3, CAP - 1)
    _assert_is_host_batch(only, host_batch(items, [1, 1, 1], dev))


def test_output_offsets_past_2_to_the_31(dev):
    """3 * B * nmax1 > 2^31 elements in pc1 / ft1 / flow_label (and 2 * B * nmax1 close behind in opt_flow): the slots on both sides
    of element 2^31 and the last one hold their frames, as slot 0 / 1 do.  Nothing smaller reaches those offsets: nmax1 is at the
    entry point's limit (32768), so B = 21848 is the least batch that crosses, and one call writes all cloud-1 outputs, 14 floats
    per position -- about 40 GB of device memory, asked for up front."""
    free = torch.cuda.mem_get_info(dev)[0]
    assert free >= 44 * 2 ** 30, "this test needs 40 GB of free device memory (64-bit output offsets); %.1f GB are free" % (free / 2 ** 30)
    rng = np.random.default_rng(9)
    gpu = D.DeviceSplit.from_items([_item(700, 1, rng), _item(300, 2, rng)], dev)
    N = 32768
    cross = 2 ** 31 // (3 * N)                                                         # the slot element 2^31 falls into
    B = cross + 3
    frames = (torch.arange(B, device=dev) % 2).to(_i32)
    out = gpu.draw_frames(frames, nmax1=N, nmax2=2)
    assert out["pc1"].numel() > 2 ** 31 and out["pc1"].shape == (B, 3, N)
    small_ = gpu.draw_frames([0, 1], nmax1=N, nmax2=2)
    for s in (cross - 1, cross, cross + 1, B - 1):
        for k in RAGGED_KEYS:
            assert torch.equal(out[k][s], small_[k][s % 2]), (s, k)
    del out
    torch.cuda.empty_cache()


def test_a_slot_does_not_depend_on_the_batch(small):
    items, gpu = small
    mixed = [6, 9, 0, 4, 5, 1, 2, 3]
    a = gpu.draw_frames(mixed, nmax1=1024, nmax2=1024)
    for s, f in enumerate(mixed):
        b = gpu.draw_frames([f] * len(mixed), nmax1=1024, nmax2=1024)
        for k in RAGGED_KEYS:
            assert torch.equal(a[k][s], b[k][s]), (k, s)                               # the whole row, padding included
    lone = gpu.draw_frames([mixed[0]], nmax1=1024, nmax2=1024)
    assert all(torch.equal(lone[k][0], a[k][0]) for k in RAGGED_KEYS)


def test_bad_arguments_and_bad_frame_ids(small, dev):
    items, gpu = small
    with pytest.raises(RuntimeError):
        gpu.draw_frames([])                                                            # B >= 1
    with pytest.raises(RuntimeError):
        gpu.draw_frames(torch.zeros(0, dtype=_i32, device=dev), nmax1=4, nmax2=4)
    for kw in ({"nmax1": 0, "nmax2": 4}, {"nmax1": 4, "nmax2": 0}, {"nmax1": 32769, "nmax2": 4}):
        with pytest.raises(RuntimeError):
            gpu.draw_frames(torch.zeros(2, dtype=_i32, device=dev), **kw)              # 1 <= nmax <= CMF_DRAW_MAX_NPOINTS
    with pytest.raises(RuntimeError):
        gpu.draw_frames([0], nmax1=0)
    a = gpu.draw_frames([-5, 10 ** 6])                                                 # clamped to the first / last frame
    b = gpu.draw_frames([0, len(gpu) - 1])
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        gpu.draw_frames([8, 0], nmax1=999)                                             # frame 8 has 1000 points
    with pytest.raises(ValueError):
        gpu.draw_frames([8, 0], nmax2=254)                                             # ... and 255 in cloud 2
    assert gpu.draw_frames([8, 0], nmax1=1000, nmax2=257)["pc1"].shape == (2, 3, 1000)


def test_iterators_are_draw_frames_and_do_not_wait_for_the_device(small, dev):
    """sweep / epoch_ragged / draw_frame_batches: every batch is draw_frames of its id list bit for bit, and once the ids of the
    pass are on their way (one asynchronous copy, before the first batch) taking the batches synchronises nothing."""
    items, gpu = small
    lists = [[3, 9], [0], [8, 8, 1, 2]]
    n1 = gpu.counts_host[0]
    order = sorted(range(10), key=lambda f: (int(n1[f]), f))
    want_sweep = [order[0:4], order[4:8], order[8:10]]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = list(gpu.draw_frame_batches(lists))
        swept = list(gpu.sweep(4, sort_by_size=True))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for b, ids in zip(got + swept, lists + want_sweep, strict=True):
        alone = gpu.draw_frames(ids)
        assert list(b) == list(alone) and all(_bits_equal(b[k], alone[k]) for k in alone), ids
    shuffled = [b["frames"].tolist() for b in gpu.epoch_ragged(4, seed=3, epoch=2, bucket=2, drop_last=False)]
    assert shuffled == D.ragged_batches(n1, gpu._order(10, 3, 2).tolist(), 4, 2, False) and sorted(sum(shuffled, [])) == list(range(10))
    assert list(gpu.draw_frame_batches([])) == []
    with pytest.raises(RuntimeError):
        list(gpu.draw_frame_batches([[1], []]))                                        # B = 0: the entry point's argument error


# ---- model level ---------------------------------------------------------------------------------------------------------------------
class EvalArgs:
    num_points, eval, mini_clip_len, update_len = 256, True, 2, 3


def _weights(manifest, golden_dir, t=False):
    return synth.synth_state_dict(manifest, seed=1234, calib=os.path.join(golden_dir, "bn_calib_cmflow_t.npz" if t else "bn_calib_cmflow.npz"))


def _net(manifest, golden_dir, args, dev, t=False):
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    net = (CMFlow_T if t else CMFlow)(args)
    net.load_state_dict(_weights(manifest, golden_dir, t))
    return net.to(dev).eval()


def _oracle(manifest, golden_dir, args, t=False):
    ref = (O.CMFlow_T if t else O.CMFlow)(args)
    ref.load_state_dict(_weights(manifest, golden_dir, t))
    return ref.eval()


def _sample(item):
    """One whole-frame item as the (1,3,n) CPU tensors the models take."""
    cm = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32).T))[None]
    return cm(item[0]), cm(item[1]), cm(item[2]), cm(item[3])


def _vector(groups):
    return torch.stack([v for d in groups for v in d.values()])


def _numbers(result):
    return np.array([float(v) for d in result[:3] for v in d.values()])


def test_train_steps_on_whole_frames(dev, manifest, golden_dir, args, tmp_path):
    """epoch_ragged visits every frame once; two TrainStep.step_ragged steps under net.eval() on its batches: finite loss, every
    weight gradient written; the loss of a drawn batch equals, bit for bit, the loss of the same frames assembled on the host."""
    from cmflow_amd.train import TrainStep
    D.write_synthetic_split(str(tmp_path))
    ds = D.vodDataset(EvalArgs(), str(tmp_path), "train")
    items = [ds[i] for i in range(len(ds))]
    gpu = D.DeviceSplit.from_dataset(ds, dev)
    for bs, bucket, sizes in ((2, 1, [2, 2]), (3, 1, [3]), (2, 2, [2, 2])):
        batches = list(gpu.epoch_ragged(batch_size=bs, seed=11, epoch=1, bucket=bucket))
        assert [b["pc1"].shape[0] for b in batches] == sizes
        seen = sum((b["frames"].tolist() for b in batches), [])
        assert len(set(seen)) == len(seen) and (sorted(seen) == [0, 1, 2, 3] or bs == 3)
    assert [b["pc1"].shape[0] for b in gpu.epoch_ragged(3, 11, 1, drop_last=False)] == [3, 1]
    orders = [sum((b["frames"].tolist() for b in gpu.epoch_ragged(1, 11, e)), []) for e in range(6)]
    assert orders[1] == sum((b["frames"].tolist() for b in gpu.epoch_ragged(1, 11, 1)), []) and len({tuple(o) for o in orders}) > 1
    net = _net(manifest, golden_dir, args, dev)
    step = TrainStep(net, vr_thres=args.vr_thres)
    batches = list(gpu.epoch_ragged(batch_size=2, seed=11, epoch=0))
    names = {id(p): k for k, p in net.named_parameters()}
    for b in batches:
        loss, _, _, _ = step.step_ragged(b, validate=True)
        assert torch.isfinite(loss).item()
        assert torch.isfinite(step.bucket.flat).all()
        unwritten = [names[id(p)] for p in step.bucket.params if p.dim() >= 2 and not p.grad.any()]
        assert not unwritten, unwritten
    b = batches[0]
    host = host_batch(items, b["frames"].tolist(), dev)
    _assert_is_host_batch(b, host)
    drawn = step.forward_loss_ragged(b)[0].detach()
    again = step.forward_loss_ragged(host)[0].detach()
    assert torch.equal(drawn, again) and torch.isfinite(drawn).item()


@pytest.fixture(scope="module")
def six(dev, tmp_path_factory):
    """The default synthetic split, train + test: six whole frames."""
    root = str(tmp_path_factory.mktemp("six"))
    D.write_synthetic_split(root)
    items = []
    for part in ("train", "test"):
        d = D.vodDataset(EvalArgs(), root, part)
        items += [d[i] for i in range(len(d))]
    assert len(items) == 6
    return items, D.DeviceSplit.from_items(items, dev)


@pytest.mark.parametrize("sort_by_size", [False, True])
def test_eval_split_equals_the_existing_path(six, dev, manifest, golden_dir, args, sort_by_size):
    """The same epoch written out here on host-collated batches (collate_ragged -> forward_ragged -> eval_batch_ragged) for the
    frame groups sweep reports: all 14 metrics and both transform arrays bit-equal."""
    items, gpu = six
    net = _net(manifest, golden_dir, args, dev)
    groups = [b["frames"].tolist() for b in gpu.sweep(4, sort_by_size)]
    n1 = gpu.counts_host[0]
    order = sorted(range(6), key=lambda f: (n1[f], f)) if sort_by_size else list(range(6))
    assert groups == [order[:4], order[4:]]
    acc = torch.zeros(14, dtype=torch.float64, device=dev)
    gt_all, pre_all = torch.zeros(6, 4, 4, device=dev), torch.zeros(6, 4, 4, device=dev)
    with torch.no_grad():
        for g in groups:
            pc1, pc2, ft1, ft2, trans, gt, mask, _, _, _, _, c1, c2 = D.extract_data_info_ragged(D.collate_ragged([items[f] for f in g]), device=dev)
            sf, cls, pt, mk = net.forward_ragged(pc1, pc2, ft1, ft2, c1, c2, validate=True)
            acc = acc + len(g) * _vector(E.eval_batch_ragged(pc1, sf.transpose(1, 2).contiguous(), gt, mask, mk.float(), trans, pt, c1))
            gt_all[g], pre_all[g] = trans, pt
    want = (acc / 6).cpu().numpy()
    net.train()
    seen = []
    got = EV.eval_split(net, gpu, 4, sort_by_size=sort_by_size, on_batch=lambda b, o: seen.append((b["frames"].tolist(), len(o))))
    assert not net.training                                                            # net.eval(), not restored: the reference's switch
    assert seen == [(g, 4) for g in groups]
    assert list(got[0]) == list(E.SF_KEYS) and list(got[1]) == list(E.SEG_KEYS) and list(got[2]) == list(E.POSE_KEYS)
    assert all(v.dtype == torch.float64 and v.dim() == 0 and v.device == gt_all.device for d in got[:3] for v in d.values())
    print("eval_split", _numbers(got), "written out", want)
    assert np.array_equal(_numbers(got), want, equal_nan=True)
    assert np.isfinite(want[[4, 5, 6, 7, 8, 9, 10, 11, 12, 13]]).all()
    assert _bits_equal(got[3], gt_all) and _bits_equal(got[4], pre_all)
    # the epoch again, now warm, with every host wait for the device an error: the loop only enqueues
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = EV.eval_split(net, gpu, 4, sort_by_size=sort_by_size)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert np.array_equal(_numbers(again), want, equal_nan=True) and _bits_equal(again[4], pre_all)


def test_eval_split_is_the_references_protocol(six, dev, manifest, golden_dir, args):
    """Against the loop the reference runs (main.py:203: one frame per dense forward at B = 1, eval_batch, the sums divided by the
    frame count), with the assertions of test_gpu_ragged.py::test_collated_split_runs_end_to_end: zero mask flips first, then
    |d epe| <= sqrt(3) * 2e-4 * max(1, |flow|max), the segmentation metrics equal at rtol 1e-12.
    Zero flips is a property of the inputs: the CPU oracle's smallest |stat_cls - 0.5| over these six frames was measured at 2.19e-3
    (per frame 0.48, 2.19e-3, 9.6e-3, 1.1e-2, 5.9e-3, 8.4e-3), 10.9 x the 2e-4 score bound; the margin is asserted (>= 2e-3) so that a
    change of synth cannot erode it silently."""
    items, gpu = six
    net = _net(manifest, golden_dir, args, dev)
    ref = _oracle(manifest, golden_dir, args)
    masks = {}

    def keep(b, o):
        for s, f in enumerate(b["frames"].tolist()):
            masks[f] = o[3][s, :int(b["n1"][s])].clone()
    got = _numbers(EV.eval_split(net, gpu, 4, on_batch=keep))
    acc, scale, flips, margins = None, 1.0, 0, []
    with torch.no_grad():
        for f, it in enumerate(items):
            smp = _sample(it)
            margins.append(float((ref(*smp, None, "test")[1] - 0.5).abs().min()))
            pc1, pc2, ft1, ft2 = (t.to(dev) for t in smp)
            fl = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))[None].to(dev)
            o = net(pc1, pc2, ft1, ft2, None, "test")
            w = E.eval_batch(pc1, o[0].transpose(1, 2).contiguous(), fl(it[5]), fl(it[6]), o[3].float(), fl(it[4]), o[2])
            v = np.array([float(x) for d in w for x in d.values()])
            acc = v if acc is None else acc + v
            scale = max(scale, float(o[0].abs().max()))
            flips += int((o[3][0] != masks[f]).sum())
    print("eval_split", got, "per-frame loop", acc / 6, "mask flips", flips, "oracle margins", margins)
    assert min(margins) >= 2e-3, margins
    assert flips == 0
    assert abs(got[6] - acc[6] / 6) <= 3 ** 0.5 * 2e-4 * scale
    np.testing.assert_allclose(got[9:12], acc[9:12] / 6, rtol=1e-12, atol=0)


CLIPS = (("test", "delft_2", (210, 330, 150, 260)), ("test", "delft_5", (97, 300, 190)), ("test", "delft_9", (128,)))


def test_eval_split_clips_carries_and_resets_state_like_the_reference(dev, manifest_t, golden_dir, args, tmp_path):
    """update_len = 3 on clips [0,4) [4,7) [7,8): the reference resets at 0, 3, 6, 7 (the clip start at 4 is missed), so the segments
    are [0-2] [3-5] [6] [7] and the second one crosses a clip boundary; batch_size = 3 runs the first three side by side.
    (a) every frame's stat_cls and gfeat (both before the mask: no flip condition) against the oracle's CMFlow_T run frame by frame at
    B = 1 with the state reset exactly there, within 1e-4 (the bound of test_cmflow_t_forward_ragged_clip_matches_oracle);
    (b) metrics and transform arrays bit-equal to the schedule written out here on host-collated batches with gfeat[:active]."""
    D.write_synthetic_split(str(tmp_path), seed=5, clips=CLIPS)
    ds = D.vodClipDataset(EvalArgs(), str(tmp_path), "test")
    items = [ds[i] for i in range(len(ds))]
    gpu = D.DeviceSplit.from_dataset(ds, dev)
    assert gpu.clips == [(0, 4), (4, 7), (7, 8)] and gpu.counts_host[0].tolist() == [210, 330, 150, 260, 97, 300, 190, 128]
    resets = EV.clip_test_resets(gpu.clips, 8, 3)
    schedule = EV.clip_test_schedule(resets, 8, 3)
    assert resets == [0, 3, 6, 7] and schedule == [[[0, 3, 6], [1, 4], [2, 5]], [[7]]]
    net = _net(manifest_t, golden_dir, args, dev, t=True)
    per_frame, steps = {}, []

    def keep(b, o):
        frames = b["frames"].tolist()
        steps.append(frames)
        for s, f in enumerate(frames):
            per_frame[f] = (o[1][s, 0, :int(b["n1"][s])].cpu(), o[4][s].cpu())
    got = EV.eval_split_clips(net, gpu, 3, 3, on_batch=keep)
    assert steps == [s for g in schedule for s in g] and sorted(per_frame) == list(range(8))
    # (a) the oracle, frame by frame
    ref = _oracle(manifest_t, golden_dir, args, t=True)
    g = None
    with torch.no_grad():
        for f, it in enumerate(items):
            want = ref(*_sample(it), None, "test", None if f in resets else g)
            g = want[4]
            e_cls = float((per_frame[f][0] - want[1][0, 0]).abs().max())
            e_g = float((per_frame[f][1] - g[0]).abs().max())
            print("frame %d: |stat_cls err| %.3g, |gfeat err| %.3g, oracle margin %.3g" % (f, e_cls, e_g, float((want[1] - 0.5).abs().min())))
            assert e_cls <= 1e-4 and e_g <= 1e-4, (f, e_cls, e_g)
    # (b) the schedule on host-collated batches
    acc = torch.zeros(14, dtype=torch.float64, device=dev)
    gt_all, pre_all = torch.zeros(8, 4, 4, device=dev), torch.zeros(8, 4, 4, device=dev)
    with torch.no_grad():
        for group in schedule:
            gfeat = None
            for step in group:
                pc1, pc2, ft1, ft2, trans, gt, mask, _, _, _, _, c1, c2 = D.extract_data_info_ragged(D.collate_ragged([items[f] for f in step]), device=dev)
                sf, cls, pt, mk, gfeat = net.forward_ragged(pc1, pc2, ft1, ft2, c1, c2, None if gfeat is None else gfeat[:len(step)], validate=True)
                acc = acc + len(step) * _vector(E.eval_batch_ragged(pc1, sf.transpose(1, 2).contiguous(), gt, mask, mk.float(), trans, pt, c1))
                gt_all[step], pre_all[step] = trans, pt
    want = (acc / 8).cpu().numpy()
    print("eval_split_clips", _numbers(got), "written out", want)
    assert np.array_equal(_numbers(got), want, equal_nan=True)
    assert _bits_equal(got[3], gt_all) and _bits_equal(got[4], pre_all)
    plain = D.DeviceSplit.from_items(items, dev)
    with pytest.raises(ValueError):
        EV.eval_split_clips(net, plain, 3, 3)                                          # no clip ranges
    # the epoch again, warm, with every host wait for the device an error: ids sent once, the steps only enqueue
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = EV.eval_split_clips(net, gpu, 3, 3)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert np.array_equal(_numbers(again), want, equal_nan=True) and _bits_equal(again[4], pre_all)
