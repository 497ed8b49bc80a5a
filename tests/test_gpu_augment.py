"""GPU: label-consistent augmentation -- ``cmf_augment_batch`` against its numpy restatement bit for bit (tests/augment_ref.py), the
draw paths of ``DeviceSplit`` with ``augment=``, the loss's invariance against an independent float64 reference on the
UN-augmented batch (tests/augment_case.py, tests/loss_torch.py), the per-sample calibration of ``RadarFlowLoss`` alone, and a run
(``train.fit`` with resume; a CMFlow-T mini-clip).  Every test fails on the parent commit: the names do not exist there."""
import os

import numpy as np
import pytest
import torch

import augment_case as AC
import augment_ref as AR
import run_dp_worker as R
from cmflow_amd import dataset as D
from cmflow_amd import synth
from cmflow_amd import train as T
from cmflow_amd.losses import ITEM_KEYS, RadarFlowLoss, make_labels, make_labels_ragged

pytestmark = pytest.mark.gpu
TCR = np.array(synth.T_CAMERA_RADAR, dtype=np.float32)
CHANGED = ("pc1", "pc2", "flow_label", "gt_trans")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _same_batch(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        _same(a[k], b[k], (what, k))


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------
LAYOUTS = {"dense": (256, 256), "ragged": (70, 33), "one": (1, 1)}
_source = {}


def _host_batch(B, n1, n2):
    """B slots of n1 / n2 points cut from one seeded scene, computed once and never modified: numpy float32 arrays."""
    if (B, n1, n2) not in _source:
        b = synth.make_batch(B, max(n1, n2), seed=17, train_extras=True)
        _source[B, n1, n2] = {"pc1": b["pc1"][:, :, :n1].contiguous().numpy(), "pc2": b["pc2"][:, :, :n2].contiguous().numpy(),
                              "flow_label": b["flow_label"][:, :n1].contiguous().numpy(), "gt_trans": b["gt_trans"].numpy()}
    return _source[B, n1, n2]


def _device_batch(host, dev):
    return {k: torch.from_numpy(v.copy()).to(dev) for k, v in host.items()}


@pytest.mark.parametrize("yaw_deg", [0.0, 10.0, 179.0])
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("slot0", [0, 5])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_kernel_equals_the_restatement_bit_for_bit(dev, layout, slot0, mirror, yaw_deg):
    n1, n2 = LAYOUTS[layout]
    host = _host_batch(3, n1, n2)
    a = D.Augment(yaw_deg, mirror)
    want = AR.augment_ref(host, TCR, 77, 9, slot0, a.tan_half_max, mirror)
    batch = D.augment_batch(_device_batch(host, dev), a, 77, 9, slot0)
    for k in CHANGED:
        _same(batch[k], torch.from_numpy(want[k]), (k, layout, slot0, mirror, yaw_deg))
    _same(batch["aug"], torch.from_numpy(want["aug"]), "aug")
    _same(batch["t_camera_radar"], torch.from_numpy(want["calib"]), "calib")
    if yaw_deg > 0:
        assert not np.array_equal(want["pc1"], host["pc1"])                            # the case does something


def test_a_slot_depends_on_its_global_number_only(dev):
    """Row s of a B = 3 call with slot0 = 5 is row 5 + s of the B = 8 call, on the same slot contents."""
    a = D.Augment(179.0, True)
    big = _host_batch(8, 70, 33)
    part = {k: v[5:8] for k, v in big.items()}
    whole = D.augment_batch(_device_batch(big, dev), a, 3, 2 ** 40 + 1)
    share = D.augment_batch(_device_batch(part, dev), a, 3, 2 ** 40 + 1, slot0=5)
    for k in CHANGED + ("aug", "t_camera_radar"):
        _same(share[k], whole[k][5:8], k)
    other = D.augment_batch(_device_batch(part, dev), a, 3, 2 ** 40 + 2, slot0=5)      # another aug_draw, another transform
    assert not torch.equal(other["aug"], share["aug"])


def test_identity_setting_leaves_every_bit(dev):
    """yaw 0 without mirror: signed zeros, a NaN and an infinity survive; aug = I; calib = the shared matrix."""
    host = {k: v.copy() for k, v in _host_batch(3, 70, 33).items()}
    host["pc1"][0, 0, :4] = (-0.0, 0.0, np.nan, np.inf)
    host["pc2"][1, 1, :2] = (-0.0, 0.0)
    host["flow_label"][2, :2, :2] = ((-0.0, 0.0), (0.0, -0.0))
    host["gt_trans"][1, 0, 1] = -0.0
    batch = D.augment_batch(_device_batch(host, dev), D.Augment(0.0, False), 77, 9)
    for k in CHANGED:
        _same(batch[k], torch.from_numpy(host[k]), k)
    _same(batch["aug"], torch.eye(4).repeat(3, 1, 1), "aug")
    _same(batch["t_camera_radar"], torch.from_numpy(TCR).repeat(3, 1, 1), "calib")


def test_bad_sizes_are_argument_errors(dev):
    import ctypes
    from cmflow_amd import _lib
    call = _lib.lib().cmf_augment_batch
    buf = torch.zeros(64, device=dev)
    p = buf.data_ptr()
    ok = lambda **kw: dict(dict(slot0=0, B=1, n1=1, n2=1, thm=0.1), **kw)
    run = lambda c: call(c["slot0"], c["B"], c["n1"], c["n2"], 1, 2, ctypes.c_double(c["thm"]), 0, p, p, p, p, p, p, p, None)
    for bad in (ok(B=0), ok(B=65536), ok(n1=0), ok(n2=0), ok(n1=32769), ok(n2=32769), ok(slot0=-1), ok(slot0=2 ** 31 - 1),
                ok(thm=-0.1), ok(thm=float("nan")), ok(thm=float("inf"))):
        assert run(bad) != 0, bad
    assert call(0, 1, 1, 1, 1, 2, ctypes.c_double(0.1), 0, None, p, p, p, p, p, p, None) != 0
    torch.cuda.synchronize()


# ---- 2. the draw paths ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_split(dev):
    return R.train_split_of(dev)


@pytest.fixture(scope="module")
def clip_split(dev):
    return R.clip_split_of(dev)


AUG = D.Augment(10.0, True)


def test_draw_with_augment_is_draw_then_augment_batch(train_split):
    frames = [3, 0, 9, 9]
    got = train_split.draw(frames, 256, 11, 6, 4, augment=AUG)
    want = D.augment_batch(train_split.draw(frames, 256, 11, 6, 4), AUG, 11, 6, 4)
    _same_batch(got, want, "draw")
    plain = train_split.draw(frames, 256, 11, 6, 4)
    assert "aug" not in plain and not torch.equal(plain["pc1"], got["pc1"])
    for k in set(plain) - set(CHANGED):                                                # everything else is invariant
        _same(plain[k], got[k], k)
    got = train_split.draw_frames(frames, augment=AUG, seed=11, aug_draw=6, slot0=4)
    want = D.augment_batch(train_split.draw_frames(frames), AUG, 11, 6, 4)
    _same_batch(got, want, "draw_frames")
    pad = got["pc1"][1, :, int(got["n1"][1]):]                                         # frame 0 (180 points) padded to 300: copies of its first row
    assert pad.shape[1] > 0 and torch.equal(pad, got["pc1"][1, :, :1].expand_as(pad))
    with pytest.raises(ValueError):
        train_split.draw_frames(frames, augment=AUG)


def test_epoch_clips_keeps_one_transform_per_mini_clip(clip_split):
    steps = list(clip_split.epoch_clips(R.BATCH, R.MINI_CLIP_LEN, 256, R.SEED, 1, augment=AUG))
    assert len(steps) == 2 and all(len(s) == R.MINI_CLIP_LEN for s in steps)
    for step in steps:
        for frame in step[1:]:
            _same(frame["aug"], step[0]["aug"], "aug across a mini-clip")
            assert not torch.equal(frame["pc1"], step[0]["pc1"])
    assert not torch.equal(steps[0][0]["aug"][:1], steps[1][0]["aug"][:1])              # another step, another transform
    plain = list(clip_split.epoch_clips(R.BATCH, R.MINI_CLIP_LEN, 256, R.SEED, 1))
    _same(plain[0][0]["ft1"], steps[0][0]["ft1"], "the sampling is untouched")


def test_two_ranks_concatenate_to_the_single_process_batch(train_split):
    keys = CHANGED + ("aug", "t_camera_radar", "ft1", "idx1")
    whole = list(train_split.epoch(4, 256, R.SEED, 2, augment=AUG))
    ranks = [list(train_split.epoch(2, 256, R.SEED, 2, rank=r, world=2, augment=AUG)) for r in range(2)]
    assert len(whole) == 2 and all(len(r) == 2 for r in ranks)
    for s, want in enumerate(whole):
        for k in keys:
            _same(torch.cat([ranks[0][s][k], ranks[1][s][k]]), want[k], ("epoch", s, k))
    whole = list(train_split.epoch_ragged(4, R.SEED, 2, bucket=1, augment=AUG))
    ranks = [list(train_split.epoch_ragged(2, R.SEED, 2, bucket=1, rank=r, world=2, augment=AUG)) for r in range(2)]
    for s, want in enumerate(whole):
        _same(torch.cat([ranks[0][s]["aug"], ranks[1][s]["aug"]]), want["aug"], ("epoch_ragged aug", s))
        for r in range(2):                                                             # the ranks pad to their own maxima: compare the valid parts
            for i in range(2):
                n = int(ranks[r][s]["n1"][i])
                _same(ranks[r][s]["pc1"][i, :, :n], want["pc1"][2 * r + i, :, :n], ("epoch_ragged pc1", s, r, i))
    assert not torch.equal(whole[0]["aug"], whole[1]["aug"])


# ---- 3. the loss is invariant: GPU on the augmented batch against float64 on the original ----------------------------------------------
@pytest.fixture(scope="module")
def case():
    """The case, its conditions checked in float64 on the CPU, and the float64 references on the UN-augmented inputs with the shared
    calibration -- computed once, before the GPU is used, and left unchanged."""
    B, N, seed = AC.DENSE
    batch, outs = AC.make_case(B, N, seed)
    m = AC.margins(batch, outs)
    assert AC.conditions_hold(m), m
    samples = []
    for i, (n1, n2) in enumerate(AC.COUNTS):
        b, o = AC.sample(batch, outs, i, n1, n2)
        m = AC.margins(b, o)
        assert AC.conditions_hold(m), (i, m)
        samples.append((b, o, AC.reference(b, o)))
    return batch, outs, AC.reference(batch, outs), samples


def _augmented(batch, outs, dev, seed):
    """The batch through the KERNEL (179 degrees, mirror on) and the outputs through the transform it reports: A pred_f,
    A pre_trans A^T in float64 from the float32 ``aug``, rounded to float32 once."""
    b = D.augment_batch({k: v.clone().to(dev) for k, v in batch.items()}, D.Augment(179.0, True), seed, 0)
    A = b["aug"].double().cpu()
    o = {"pred_f": (A[:, :3, :3] @ outs["pred_f"].double()).float(), "pre_trans": (A @ outs["pre_trans"].double() @ A.transpose(2, 1)).float(),
         "mseg_pre": outs["mseg_pre"]}
    assert float((A - torch.eye(4, dtype=torch.float64)).abs().max()) > 0.1
    return b, {k: v.to(dev).requires_grad_(True) for k, v in o.items()}, A


def _check(got_items, got_grads, ref, A, scale_by=1.0):
    """Items within 1e-4 max(1, |ref|); every gradient element within 2e-3 |ref| + 2e-4 scale of the reference's gradient mapped
    into the augmented frame: d pred_f by A, d pre_trans by A G A^T, d mseg_pre unchanged."""
    items, grads, _ = ref
    for k in ("total",) + ITEM_KEYS:
        print("%-15s gpu %.9g  float64 %.9g" % (k, got_items[k], items[k]))
        assert abs(got_items[k] - items[k]) <= 1e-4 * max(1.0, abs(items[k])), (k, got_items[k], items[k])
    want = (A[:, :3, :3] @ grads[0], A @ grads[1] @ A.transpose(2, 1), grads[2])
    for name, g, w in zip(AC.KEYS, got_grads, want):
        g = g.double().cpu() * scale_by
        scale = float(w.abs().max())
        excess = (g - w).abs() - (2e-3 * w.abs() + 2e-4 * scale)
        print("d %-10s largest error %.3g of scale %.3g, elements over the bound %d" % (name, float((g - w).abs().max()), scale, int((excess > 0).sum())))
        assert scale > 0 and float(excess.max()) <= 0, name


def _dense_loss(crit, b, o):
    dyn, mseg = make_labels(b, AC.VR_THRES)
    total, items = crit(b["pc1"], b["pc2"], o["pred_f"], b["ft1"][:, 0], b["flow_label"].transpose(2, 1), o["pre_trans"], o["mseg_pre"],
                        b["gt_trans"], mseg, dyn, b["radar_u"], b["radar_v"], b["opt_flow"], t_camera_radar=b.get("t_camera_radar"))
    return total, items, (dyn, mseg)


@pytest.mark.parametrize("tiled", [False, True])
def test_dense_loss_is_invariant(dev, case, tiled):
    """B = 4, N = 100: the LDS form and the forced tiled form, with the calibration per sample the kernel wrote."""
    batch, outs, ref, _ = case
    b, o, A = _augmented(batch, outs, dev, 5)
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    crit.tiled = tiled
    total, items, labels = _dense_loss(crit, b, o)
    total.backward()
    plain = make_labels({k: v.to(dev) for k, v in batch.items()}, AC.VR_THRES)
    for x, y, r in zip(labels, plain, ref[2]):                                         # the pseudo labels: equal to the original's, exactly
        assert torch.equal(x, y) and torch.equal(x.cpu().double(), r)
    got = dict({k: v.item() for k, v in items.items()}, total=total.item())
    _check(got, [o[k].grad for k in AC.KEYS], ref, A)


def _padded(samples, n1max, n2max):
    """The truncated samples as one ragged batch: padding repeats the sample's first row (collate_ragged's rule)."""
    def pad(t, dim, n):
        first = t.narrow(dim, 0, 1)
        return torch.cat([t, first.expand(*[n - t.shape[dim] if d == dim else s for d, s in enumerate(t.shape)])], dim=dim)
    per_point = {"pc1": (2, n1max), "ft1": (2, n1max), "pc2": (2, n2max), "ft2": (2, n2max), "flow_label": (1, n1max), "fg_mask": (1, n1max),
                 "radar_u": (1, n1max), "radar_v": (1, n1max), "opt_flow": (1, n1max), "pred_f": (2, n1max), "mseg_pre": (2, n1max)}
    cat = lambda which: {k: torch.cat([pad(s[which][k], *per_point[k]) if k in per_point else s[which][k] for s in samples]).contiguous()
                         for k in samples[0][which]}
    b, o = cat(0), cat(1)
    b["n1"] = torch.tensor([s[0]["pc1"].shape[2] for s in samples], dtype=torch.int32)
    b["n2"] = torch.tensor([s[0]["pc2"].shape[2] for s in samples], dtype=torch.int32)
    return b, o


@pytest.mark.parametrize("tiled", [False, True])
def test_counted_loss_is_invariant_per_sample(dev, case, tiled):
    """n1 != n2 (70 / 33) next to 100 / 100, padded to (100, 100): every sample against the float64 reference at B = 1 on the truncated,
    un-augmented sample; the counted gradients are those of the mean over B samples."""
    samples = case[3]
    pb, po = _padded(samples, 100, 100)
    b, o, A = _augmented(pb, po, dev, 6)
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    crit.tiled = tiled
    dyn, mseg = make_labels_ragged(b, AC.VR_THRES)
    plain = make_labels_ragged({k: v.to(dev) for k, v in pb.items()}, AC.VR_THRES)
    assert torch.equal(dyn, plain[0]) and torch.equal(mseg, plain[1])
    total, items, per = crit.forward_ragged(b["pc1"], b["pc2"], o["pred_f"], b["ft1"][:, 0], b["n1"], b["n2"], b["flow_label"].transpose(2, 1),
                                            o["pre_trans"], o["mseg_pre"], b["gt_trans"], mseg, dyn, b["radar_u"], b["radar_v"],
                                            b["opt_flow"], validate=True, t_camera_radar=b["t_camera_radar"])
    total.backward()
    B = len(samples)
    for i, (sb, so, ref) in enumerate(samples):
        n1 = sb["pc1"].shape[2]
        assert torch.equal(dyn[i, :n1].cpu().double(), ref[2][0][0]) and torch.equal(mseg[i, :n1].cpu().double(), ref[2][1][0])
        got = dict(zip(("total",) + ITEM_KEYS, per[i].tolist()))
        grads = (o["pred_f"].grad[i:i + 1, :, :n1], o["pre_trans"].grad[i:i + 1], o["mseg_pre"].grad[i:i + 1, :, :n1])
        print("sample %d (%d / %d points)" % (i, n1, sb["pc2"].shape[2]))
        _check(got, grads, ref, A[i:i + 1], scale_by=float(B))


# ---- 4. the per-sample calibration alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "tiled", "counted"])
def test_equal_rows_are_the_shared_matrix_and_swapped_rows_move_the_optical_item_only(dev, case, form):
    batch, outs = case[0], case[1]
    b = {k: v.to(dev) for k, v in batch.items()}
    B, N = b["pc1"].shape[0], b["pc1"].shape[2]
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    crit.tiled = form == "tiled"
    n = torch.full((B,), N, dtype=torch.int32, device=dev)

    def run(calib):
        o = {k: v.clone().to(dev).requires_grad_(True) for k, v in outs.items()}
        if form == "counted":
            dyn, mseg = make_labels_ragged(dict(b, n1=n), AC.VR_THRES)
            total, items, per = crit.forward_ragged(b["pc1"], b["pc2"], o["pred_f"], b["ft1"][:, 0], n, n, b["flow_label"].transpose(2, 1),
                                                    o["pre_trans"], o["mseg_pre"], b["gt_trans"], mseg, dyn, b["radar_u"], b["radar_v"],
                                                    b["opt_flow"], t_camera_radar=calib)
        else:
            total, items, _ = _dense_loss(crit, dict(b, **({} if calib is None else {"t_camera_radar": calib})), o)
            per = total.reshape(1)
        total.backward()
        return total.detach(), {k: v.detach() for k, v in items.items()}, per.detach(), [o[k].grad for k in AC.KEYS]

    shared = run(None)
    rows = run(crit.t_camera_radar.repeat(B, 1, 1).contiguous())
    _same(rows[0], shared[0], "total")
    _same(rows[2], shared[2], "per sample")
    for k in ITEM_KEYS:
        _same(rows[1][k], shared[1][k], k)
    for x, y, k in zip(rows[3], shared[3], AC.KEYS):
        _same(x, y, "d " + k)
    calib = D.augment_batch({k: v.clone() for k, v in b.items()}, D.Augment(30.0, True), 1, 0)["t_camera_radar"]
    swapped = calib.clone()
    swapped[0], swapped[1] = calib[1], calib[0]
    one, two = run(calib), run(swapped)
    for k in ITEM_KEYS:
        assert torch.equal(one[1][k], two[1][k]) == (k != "opticalLoss"), k
    _same(one[3][1], two[3][1], "d pre_trans")                                         # the camera term does not reach pre_trans or the scores
    _same(one[3][2], two[3][2], "d mseg_pre")
    assert not torch.equal(one[3][0][:2], two[3][0][:2]) and torch.equal(one[3][0][2:], two[3][0][2:])
    with pytest.raises(ValueError):
        run(calib[:2].contiguous())


# ---- 5. a run ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def val_split(dev):
    return R.val_split_of(dev)


def _fit(net, train_split, val_split, epochs, **kw):
    return T.fit(net, train_split, val_split, epochs=epochs, batch_size=R.BATCH, val_batch_size=R.VAL_BATCH, num_points=R.NPOINTS,
                 seed=R.SEED, mini_clip_len=R.MINI_CLIP_LEN, **kw)


def _same_state(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        _same(a[k], b[k], (what, k))


def test_augmented_run_resumes_exactly(train_split, val_split, dev, tmp_path):
    whole, first, second = (str(tmp_path / d) for d in ("whole", "first", "second"))
    net = R.model("cmflow", dev)
    want = _fit(net, train_split, val_split, 2, augment=AUG, out_dir=whole)
    head = _fit(R.model("cmflow", dev), train_split, val_split, 1, augment=AUG, out_dir=first)
    assert head["train_loss"] == want["train_loss"][:1] and head["val_score"] == want["val_score"][:1]
    point = os.path.join(first, "last.pt")
    stored = torch.load(point)["settings"]
    assert stored["augment"] == (10.0, True) and type(stored["augment"]) is tuple
    for other in (None, D.Augment(10.0, False), D.Augment(11.0, True)):
        with pytest.raises(ValueError, match="augment"):
            _fit(R.model("cmflow", dev), train_split, val_split, 2, augment=other, resume=point)
    resumed = R.model("cmflow", dev)
    got = _fit(resumed, train_split, val_split, 2, augment=AUG, out_dir=second, resume=point)
    assert got["train_loss"] == want["train_loss"] and got["val_score"] == want["val_score"] and got["best"] == want["best"]
    _same_state(R.state_of(resumed), R.state_of(net), "parameters and buffers")
    a, b = torch.load(os.path.join(whole, "last.pt")), torch.load(os.path.join(second, "last.pt"))
    assert a["settings"] == b["settings"]
    _same_state({k: a["optimizer"]["flat"][k] for k in ("exp_avg", "exp_avg_sq")}, {k: b["optimizer"]["flat"][k] for k in ("exp_avg", "exp_avg_sq")},
                "Adam moments")


def test_identity_augmentation_trains_like_none_and_augmentation_trains_differently(train_split, val_split, dev, tmp_path):
    nets = [R.model("cmflow", dev) for _ in range(3)]
    off = _fit(nets[0], train_split, val_split, 2, out_dir=str(tmp_path / "off"))
    same = _fit(nets[1], train_split, val_split, 2, augment=D.Augment(0.0, False))
    moved = _fit(nets[2], train_split, val_split, 1, augment=AUG)
    assert "augment" not in torch.load(str(tmp_path / "off" / "last.pt"))["settings"]    # off: the settings keep their keys
    assert off["train_loss"] == same["train_loss"] and off["val_score"] == same["val_score"]
    _same_state(R.state_of(nets[1]), R.state_of(nets[0]), "Augment(0, False) against None")
    assert moved["train_loss"][0] != off["train_loss"][0] and np.isfinite(moved["train_loss"][0])
    with pytest.raises(ValueError, match="augment"):                                   # a point without the key counts as off
        _fit(R.model("cmflow", dev), train_split, val_split, 3, augment=D.Augment(0.0, False), resume=str(tmp_path / "off" / "last.pt"))


def test_augmented_mini_clip_step_of_cmflow_t(clip_split, dev):
    net = R.model("cmflow_t", dev).train()
    step = T.TrainStep(net)
    clip = next(iter(clip_split.epoch_clips(R.BATCH, R.MINI_CLIP_LEN, R.NPOINTS, R.SEED, 0, augment=AUG,
                                            t_camera_radar=step.loss_obj.t_camera_radar)))
    step.reset_clip()
    losses = []
    for frame in clip:
        _same(frame["aug"], clip[0]["aug"], "one transform per mini-clip")
        assert frame["t_camera_radar"].shape == (R.BATCH, 4, 4)
        losses.append(step(frame)[0])
    assert len(losses) == R.MINI_CLIP_LEN and all(torch.isfinite(l).item() for l in losses)
    total, items = T.train_epoch_clips(T.TrainStep(R.model("cmflow_t", dev)), clip_split, R.BATCH, R.MINI_CLIP_LEN, R.NPOINTS, R.SEED, 0,
                                       augment=AUG)
    assert torch.isfinite(total).item() and all(torch.isfinite(v).item() for v in items.values())
