"""CPU: the label-consistent augmentation (dataset.Augment / augment_batch, cmf_augment_batch) -- the host restatement of the
kernel's rule (tests/augment_ref.py), the mathematics of the transform family (the float64 loss is invariant under it), the settings
object, fit's resume comparison and the refusals.  The kernel itself runs in tests/test_gpu_augment.py."""
import math

import numpy as np
import pytest
import torch

import augment_case as AC
import augment_ref as AR
from cmflow_amd import dataset as D
from cmflow_amd import synth
from cmflow_amd import train as T

SWEEP = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1] + [int(v) for v in np.random.default_rng(5).integers(0, 2 ** 32, 200)]


@pytest.mark.parametrize("yaw_deg", [0.5, 10.0, 90.0, 179.0])
def test_restated_matrix_is_orthogonal_to_float32_rounding(yaw_deg):
    """|A^T A - I| <= 2^-22 over the sweep, both mirror signs: c^2 + s^2 = 1 up to float64 rounding, and each of cf, sf carries one
    float32 rounding (2^-24 relative), so cf^2 + sf^2 differs from 1 by at most about 2^-23; the mixed entries cancel exactly."""
    thm = D.Augment(yaw_deg).tan_half_max
    worst = 0.0
    for u in SWEEP:
        cf, sf = AR.angle(u, thm)
        assert abs(math.degrees(math.atan2(float(sf), float(cf)))) <= yaw_deg * (1 + 1e-6)
        for m in (1.0, -1.0):
            A = AR.matrix(cf, sf, np.float32(m)).astype(np.float64)
            worst = max(worst, float(np.abs(A.T @ A - np.eye(3)).max()))
            assert abs(np.linalg.det(A) - m) < 1e-6
    assert worst <= 2.0 ** -22, worst


def test_angle_endpoints_and_centre():
    thm = D.Augment(10.0).tan_half_max
    cf, sf = AR.angle(2 ** 31, thm)                            # r = 1/2: t = 0, the identity rotation
    assert cf == 1.0 and sf == 0.0
    lo, hi = AR.angle(0, thm), AR.angle(2 ** 32 - 1, thm)
    assert math.isclose(math.degrees(math.atan2(float(lo[1]), float(lo[0]))), -10.0, rel_tol=1e-6)
    assert math.isclose(math.degrees(math.atan2(float(hi[1]), float(hi[0]))), 10.0, rel_tol=1e-6)


def _arrays(B, n1, n2, seed):
    b = synth.make_batch(B, max(n1, n2), seed=seed, train_extras=True)
    return {"pc1": b["pc1"][:, :, :n1].contiguous().numpy(), "pc2": b["pc2"][:, :, :n2].contiguous().numpy(),
            "flow_label": b["flow_label"][:, :n1].contiguous().numpy(), "gt_trans": b["gt_trans"].numpy()}


def test_zero_yaw_without_mirror_is_the_exact_identity():
    """Every float keeps its bits -- signed zeros and a NaN included -- aug = I and calib = the shared matrix."""
    batch = _arrays(3, 40, 17, 3)
    batch["pc1"][0, 0, :3] = (-0.0, 0.0, np.nan)
    batch["flow_label"][1, :2, 1] = (-0.0, 0.0)
    tcr = np.array(synth.T_CAMERA_RADAR, dtype=np.float32)
    out = AR.augment_ref(batch, tcr, 7, 3, 0, D.Augment(0.0, False).tan_half_max, False)
    for k in batch:
        assert np.array_equal(out[k].view(np.int32), batch[k].view(np.int32)), k
    assert np.array_equal(out["aug"], np.broadcast_to(np.eye(4, dtype=np.float32), (3, 4, 4)))
    assert np.array_equal(out["calib"].view(np.int32), np.broadcast_to(tcr, (3, 4, 4)).view(np.int32))
    assert D.Augment(0.0, False).tan_half_max == 0.0
    mirrored = AR.augment_ref(batch, tcr, 7, 3, 0, 0.0, True)                          # zero yaw WITH the mirror is not the identity
    bits = [AR.slot_words(7, 3, s)[1] for s in range(3)]
    assert [float(mirrored["aug"][s, 1, 1]) for s in range(3)] == [-1.0 if b else 1.0 for b in bits] and any(bits)


def test_restated_point_rule_is_linear_up_to_float32_rounding():
    """A (p + f) against A p + A f, float32: each side carries a few roundings of numbers up to |p| + |f|."""
    batch = _arrays(4, 256, 256, 11)
    p, f = batch["pc1"], np.ascontiguousarray(batch["flow_label"].transpose(0, 2, 1))
    for s in range(4):
        cf, sf, m = AR.slot_params(21, 4, s, D.Augment(179.0).tan_half_max, True)
        px, py = AR.points(p[s, 0], p[s, 1], cf, sf, m)
        fx, fy = AR.points(f[s, 0], f[s, 1], cf, sf, m)
        wx, wy = AR.points(p[s, 0] + f[s, 0], p[s, 1] + f[s, 1], cf, sf, m)
        scale = float(np.abs(p[s, :2]).max() + np.abs(f[s, :2]).max())
        assert max(float(np.abs(wx - (px + fx)).max()), float(np.abs(wy - (py + fy)).max())) <= 8 * 2.0 ** -24 * scale


def test_restated_transforms_follow_the_float64_matrices():
    """gt' = A gt A^T and calib = Tcr A^T against numpy's float64 products of the same float32 matrices: one float32 rounding apart."""
    batch = _arrays(5, 20, 20, 2)
    tcr = np.array(synth.T_CAMERA_RADAR, dtype=np.float32)
    out = AR.augment_ref(batch, tcr, 99, 12, 3, D.Augment(60.0).tan_half_max, True)
    for s in range(5):
        A = out["aug"][s].astype(np.float64)
        assert np.array_equal(out["aug"][s, 3], (0, 0, 0, 1)) and not out["aug"][s, :3, 3].any()
        np.testing.assert_allclose(out["gt_trans"][s], A @ batch["gt_trans"][s].astype(np.float64) @ A.T, rtol=2.0 ** -23, atol=2.0 ** -24)
        np.testing.assert_allclose(out["calib"][s], tcr.astype(np.float64) @ A.T, rtol=2.0 ** -23, atol=2.0 ** -24)
        for k in ("gt_trans", "calib"):
            assert np.array_equal(out[k][s, 3], (0, 0, 0, 1))
    assert len({float(out["aug"][s, 0, 0]) for s in range(5)}) == 5                    # a transform per slot
    again = AR.augment_ref(batch, tcr, 99, 12, 0, D.Augment(60.0).tan_half_max, True)  # slot0 shifts the counter, nothing else
    assert np.array_equal(again["aug"][3:], out["aug"][:2])


def test_float64_loss_and_labels_are_invariant_under_the_family():
    """The evidence that the family is right: tests/loss_torch.py (all seven terms) and make_labels_torch in float64 on the case of
    the GPU test, sample by sample at B = 1 with the sample's own calibration Tcr A^-1, under an exact rotation (and mirror) of
    clouds, flow labels, predicted flow, gt_trans and pre_trans.  Items and gradients (mapped back) agree to rounding and the
    pseudo labels are equal.  Observed floor: 1.8e-14 relative over the items, 1.6e-14 of the gradients' scale (bound: 1e-11)."""
    B, N, seed = AC.DENSE
    batch, outs = AC.make_case(B, N, seed)
    floor_items = floor_grads = 0.0
    for i, (theta, mirror) in enumerate([(0.17, False), (-2.9, True), (1.3, True), (3.1, False)]):
        b, o = AC.sample(batch, outs, i)
        A = torch.from_numpy(AR.exact_matrix(theta, mirror)).unsqueeze(0)
        want, wg, wl = AC.reference(b, o)
        tb, to, calib = AC.transformed(AC.to64(b), AC.to64(o), A)
        got, gg, gl = AC.reference(tb, to, calib[0])
        assert torch.equal(wl[0], gl[0]) and torch.equal(wl[1], gl[1])
        for k in want:
            assert want[k] != 0.0, k                                           # every term is live on this case
            floor_items = max(floor_items, abs(got[k] - want[k]) / max(1.0, abs(want[k])))
        R = A[0, :3, :3]
        back = (R.T @ gg[0][0], A[0].T @ gg[1][0] @ A[0], gg[2][0])            # d pred_f by A^T, d pre_trans by A^T G A
        for x, y in zip(back, (wg[0][0], wg[1][0], wg[2][0])):
            floor_grads = max(floor_grads, float((x - y).abs().max() / y.abs().max()))
    print("float64 invariance floor: items %.3g, gradients %.3g" % (floor_items, floor_grads))
    assert floor_items < 1e-11 and floor_grads < 1e-11


def test_the_case_of_the_gpu_test_meets_its_conditions():
    """Every margin of tests/augment_case.py on the dense case and on the truncated samples of the counted one -- no case skipped."""
    B, N, seed = AC.DENSE
    batch, outs = AC.make_case(B, N, seed)
    cases = [(batch, outs)] + [AC.sample(batch, outs, i, n1, n2) for i, (n1, n2) in enumerate(AC.COUNTS)]
    for b, o in cases:
        m = AC.margins(b, o)
        assert AC.conditions_hold(m), m


def test_augment_settings_object():
    a = D.Augment(10, True)
    assert a == (10.0, True) and tuple(a) == (10.0, True) and type(tuple(a)) is tuple and a.yaw_deg == 10.0 and a.mirror is True
    assert D.Augment() == (0.0, False) and D.Augment(0.0, False).tan_half_max == 0.0
    assert math.isclose(a.tan_half_max, math.tan(math.radians(5.0)))
    assert hash(a) == hash((10.0, True)) and D.Augment(10.0, 1) == a
    with pytest.raises(AttributeError):
        a.yaw_deg = 20.0
    with pytest.raises(AttributeError):
        a.other = 1
    for bad in (-1.0, -0.001, 180.0, 360.0, float("nan"), float("inf"), "wide", None):
        with pytest.raises(ValueError):
            D.Augment(bad)
    import pickle
    assert pickle.loads(pickle.dumps(a)) == a and isinstance(pickle.loads(pickle.dumps(a)), D.Augment)


def test_fit_refuses_a_resume_point_whose_augment_differs():
    """``check_resume_settings`` is the comparison ``fit`` runs on a resume point; a point without the key compares as off."""
    base = {"model": "CMFlow", "batch_size": 4, "seed": 1}
    on = dict(base, augment=tuple(D.Augment(10, True)))
    T.check_resume_settings(base, base)
    T.check_resume_settings(on, dict(base, augment=tuple(D.Augment(10.0, True))))
    for stored, given in ((base, on), (on, base), (on, dict(base, augment=tuple(D.Augment(10, False)))),
                          (on, dict(base, augment=tuple(D.Augment(20, True)))), (base, dict(base, augment=tuple(D.Augment(0, False))))):
        with pytest.raises(ValueError, match="augment"):
            T.check_resume_settings(stored, given)
    with pytest.raises(ValueError, match="ema_decay"):                          # the options fit already had go through the same comparison
        T.check_resume_settings(base, dict(base, ema_decay=0.9))
    with pytest.raises(TypeError):
        T.fit(torch.nn.Linear(3, 3), None, None, epochs=1, batch_size=1, val_batch_size=1, num_points=8, augment=(10.0, True))


def test_cpu_tensors_raise():
    b = synth.make_batch(2, 32, seed=1, train_extras=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        D.augment_batch(b, D.Augment(10, True), 1, 0)
    with pytest.raises(TypeError):
        D.augment_batch(b, (10.0, True), 1, 0)
    items = [(np.zeros((5, 3), np.float32) + 1, np.zeros((4, 3), np.float32) + 1, np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float32),
              np.eye(4, dtype=np.float32), np.zeros((5, 3), np.float32), np.ones(5, np.float32), 0.1, np.zeros(5, np.float32),
              np.zeros(5, np.float32), np.zeros((5, 2), np.float32))]
    split = D.DeviceSplit.from_items(items, "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        split.draw([0], 8, 1, 0, augment=D.Augment(10, True))
    with pytest.raises(RuntimeError, match="GPU only"):
        split.draw_frames([0], augment=D.Augment(10, True), seed=1, aug_draw=0)
