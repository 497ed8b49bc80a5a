"""GPU: the whole-frame loss -- RadarFlowLoss.forward_ragged (cmf_radar_loss_counted) and make_labels_ragged
(cmf_pseudo_labels_counted) on padded batches with per-sample counts.

Yardsticks are never the counted path itself: the DENSE kernels at B = 1 on the truncated sample (bit-exact claims, n1 == n2) and the
CPU oracle at B = 1 on the truncated sample (every sample, N1 != N2 included) with the bounds of tests/test_gpu_loss.py.  Padded
slots hold +-1e4.  tests/test_ragged_loss_host.py shows on the CPU that the oracle is finite on every sample of these batches."""
import numpy as np
import pytest
import torch

import ragged_loss_case as RC
from cmflow_amd import synth
from cmflow_amd.losses import ITEM_KEYS, SELF_ITEM_KEYS, RadarFlowLoss, make_labels, make_labels_ragged
from oracle import train_oracle as TO
from test_gpu_loss import _gather_group, _stable_topk

pytestmark = pytest.mark.gpu
_i32 = torch.int32
CASES = [(RC.COUNTS6, RC.SEED6), (RC.COUNTS5, RC.SEED5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _run_ragged(crit, pb, po, dev, self_only=False, grad=True, labels=None):
    """-> total, items, per_sample, (pf, pt, pm) leaves, (dyn, mseg)"""
    b = _to(pb, dev)
    dyn, mseg = labels if labels is not None else make_labels_ragged(b, 0.3)
    pf, pt, pm = (po[k].to(dev).requires_grad_(grad) for k in ("pred_f", "pre_trans", "mseg_pre"))
    if self_only:
        out = crit.forward_ragged(b["pc1"], b["pc2"], pf, b["ft1"][:, 0], b["n1"], b["n2"], validate=True)
    else:
        out = crit.forward_ragged(b["pc1"], b["pc2"], pf, b["ft1"][:, 0], b["n1"], b["n2"], b["flow_label"].transpose(2, 1), pt, pm,
                                  b["gt_trans"], mseg, dyn, b["radar_u"], b["radar_v"], b["opt_flow"], validate=True)
    return out[0], out[1], out[2], (pf, pt, pm), (dyn, mseg)


def _run_dense(crit, b, o, dev, self_only=False):
    """The dense loss at B = 1 on a truncated sample -> items (9,), gradients."""
    bd = _to(b, dev)
    dyn, mseg = make_labels(bd, 0.3)
    pf, pt, pm = (o[k].to(dev).requires_grad_(True) for k in ("pred_f", "pre_trans", "mseg_pre"))
    if self_only:
        total, items = crit(bd["pc1"], bd["pc2"], pf, bd["ft1"][:, 0])
        keys = SELF_ITEM_KEYS
    else:
        total, items = crit(bd["pc1"], bd["pc2"], pf, bd["ft1"][:, 0], bd["flow_label"].transpose(2, 1), pt, pm, bd["gt_trans"], mseg,
                            dyn, bd["radar_u"], bd["radar_v"], bd["opt_flow"])
        keys = ITEM_KEYS
    total.backward()
    vec = torch.zeros(9, device=dev)
    vec[0] = total.detach()
    for j, k in enumerate(keys):
        vec[1 + j] = items[k].detach()
    return vec, (pf.grad, None if self_only else pt.grad, None if self_only else pm.grad), (dyn, mseg)


def _slices(grads, i, n1):
    gf, gt, gm = grads
    return gf[i, :, :n1], (gt[i] if gt is not None else None), (gm[i, :, :n1] if gm is not None else None)


@pytest.mark.parametrize("counts,seed", CASES + [(RC.COUNTS4, RC.SEED4)])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("self_only", [False, True])
def test_counted_loss_equals_the_dense_kernel_bit_for_bit(dev, counts, seed, tiled, self_only):
    """Check 1: samples with n1 == n2 -- per_sample[i] == the dense loss at B = 1 on the truncated sample, bit for bit, both forms,
    full loss and self_only.  The kernel multiplies by 1/B last: B = 6 -> one rounding of 1/B and one of the product (rtol 2**-22
    on the gradient times B in float64); padded gradient slots are exactly 0.  COUNTS4, padded to (600, 600), is the LDS form
    above 512 points: pass 3 by the scan, not the inverse list."""
    B = len(counts)
    full, nmax1, nmax2 = (RC.FULL4, RC.FULL4, RC.FULL4) if counts is RC.COUNTS4 else (300, 300, 256)
    batch, outs = RC.make_case(counts, seed, full)
    pb, po = RC.padded(batch, outs, counts, nmax1, nmax2)
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    crit.tiled = tiled
    total, items, per, leaves, _ = _run_ragged(crit, pb, po, dev, self_only)
    assert type(total.grad_fn).__name__.startswith("RadarFlowLossRaggedFn")
    total.backward()
    grads = (leaves[0].grad, leaves[1].grad, leaves[2].grad)
    assert per.shape == (B, 9)
    done = 0
    for i, (n1, n2) in enumerate(counts):
        assert not grads[0][i, :, n1:].any(), i
        if not self_only:
            assert not grads[2][i, :, n1:].any(), i
        if n1 != n2:
            continue
        b, o = RC.sample(batch, outs, counts, i)
        want, wg, _ = _run_dense(crit, b, o, dev, self_only)
        print("sample %d (n = %d) tiled %s self_only %s: counted %s dense %s" % (i, n1, tiled, self_only, per[i].tolist(), want.tolist()))
        assert torch.equal(per[i].view(_i32), want.view(_i32)), (i, per[i], want)
        for g, w in zip(_slices(grads, i, n1), wg):
            if w is None:
                continue
            g64, w64 = g.double().cpu().numpy() * B, w[0].double().cpu().numpy()
            np.testing.assert_allclose(g64, w64, rtol=2.0 ** -22, atol=0)
        done += 1
    assert done >= 2


@pytest.mark.parametrize("tiled", [False, True])
def test_gradients_are_exact_when_b_is_a_power_of_two(dev, tiled):
    """1/B is exact for B = 4 and it is the last operation: gradient * B == the dense B = 1 gradient, bit for bit."""
    counts = ((130, 130), (211, 187), (256, 256), (33, 9))
    batch, outs = RC.make_case(counts, RC.SEED6)
    pb, po = RC.padded(batch, outs, counts, 300, 256)
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    crit.tiled = tiled
    total, _, per, leaves, _ = _run_ragged(crit, pb, po, dev)
    total.backward()
    for i in (0, 2):
        n1 = counts[i][0]
        want, wg, _ = _run_dense(crit, *RC.sample(batch, outs, counts, i), dev)
        assert torch.equal(per[i], want)
        for g, w in zip(_slices((leaves[0].grad, leaves[1].grad, leaves[2].grad), i, n1), wg):
            assert torch.equal(g * 4.0, w[0]), i


def _oracle(b, o, dtype, monkeypatch):
    monkeypatch.setattr(torch, "topk", _stable_topk)
    if dtype == torch.float64:
        monkeypatch.setattr(TO, "index_points_group", _gather_group)
    b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items()}
    dyn, mseg = TO.make_labels(b)
    P, Tcr = torch.as_tensor(synth.CAMERA_PROJECTION, dtype=dtype), torch.as_tensor(synth.T_CAMERA_RADAR, dtype=dtype)
    pf, pt, pm = (o[k].to(dtype).clone().requires_grad_(True) for k in ("pred_f", "pre_trans", "mseg_pre"))
    total, items = TO.radar_flow_loss(b, pf, pt, pm, mseg, dyn, P, Tcr)
    total.backward()
    return total.item(), items, (pf.grad, pt.grad, pm.grad)


def _check_items(got, ref_total, ref_items, what):
    assert abs(got[0] - ref_total) < 1e-4 * max(1.0, abs(ref_total)), (what, got[0], ref_total)
    for j, k in enumerate(ITEM_KEYS):
        assert abs(got[1 + j] - ref_items[k]) < 1e-4 * max(1.0, abs(ref_items[k])), (what, k, got[1 + j], ref_items[k])


@pytest.mark.parametrize("counts,seed", CASES)
@pytest.mark.parametrize("tiled", [False, True])
def test_counted_loss_matches_oracle_per_sample(dev, monkeypatch, counts, seed, tiled):
    """Check 2: every sample against the oracle at B = 1 on the truncated sample with the bounds of tests/test_gpu_loss.py: items
    1e-4 * max(1, |ref|); gradients (times B) against the oracle's fp32 and fp64 autograd with 2e-3 |r| + 2e-4 scale + 1e-9 per
    element, mismatch shares and maxima as that file allows.  Check 3: items_mean is the float64 mean of per_sample within 4 ulp."""
    B = len(counts)
    batch, outs = RC.make_case(counts, seed)
    pb, po = RC.padded(batch, outs, counts, 300, 256)
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    crit.tiled = tiled
    total, items, per, leaves, _ = _run_ragged(crit, pb, po, dev)
    total.backward()
    grads = tuple(x.grad.cpu() for x in leaves)
    per_c = per.cpu()
    for i, (n1, n2) in enumerate(counts):
        b, o = RC.sample(batch, outs, counts, i)
        ref_total, ref_items, ref_g32 = _oracle(b, o, torch.float32, monkeypatch)
        _, _, ref_g64 = _oracle(b, o, torch.float64, monkeypatch)
        print("sample %d (%d, %d): counted %s oracle %.7g %s" % (i, n1, n2, per_c[i].tolist(), ref_total, ref_items))
        _check_items(per_c[i].tolist(), ref_total, ref_items, i)
        for got, r32, r64, name in zip(_slices(grads, i, n1), ref_g32, ref_g64, ("pred_f", "pre_trans", "mseg_pre")):
            got, r32, r64 = got.numpy().reshape(r32.shape[1:]) * np.float32(B), r32[0].numpy(), r64[0].float().numpy()
            scale = float(np.abs(r64).max())
            bad32 = np.abs(got - r32) > 2e-3 * np.abs(r32) + 2e-4 * scale + 1e-9
            bad64 = np.abs(got - r64) > 2e-3 * np.abs(r64) + 2e-4 * scale + 1e-9
            print("  %s mismatch fraction vs fp32 oracle %.5f, vs fp64 %.5f, max abs %.3g (scale %.3g)" %
                  (name, bad32.mean(), bad64.mean(), float(np.abs(got - r64).max()), scale))
            assert bad32.mean() <= 0.002 and bad64.mean() <= 0.06, (i, name, float(bad32.mean()), float(bad64.mean()))
            assert float(np.abs(got - r32).max()) <= 0.02 * scale and float(np.abs(got - r64).max()) <= 0.5 * scale, (i, name)
    mean64 = per_c.double().mean(dim=0)
    vec = torch.stack([total.detach()] + [items[k] for k in ITEM_KEYS]).cpu()
    ulp = np.spacing(np.abs(mean64.numpy()).astype(np.float32)).astype(np.float64)
    print("items_mean", vec.tolist(), "float64 mean", mean64.tolist())
    assert (np.abs(vec.double().numpy() - mean64.numpy()) <= 4 * ulp).all()


def test_backward_twice_scales_by_each_incoming_gradient(dev):
    batch, outs = RC.make_case(RC.COUNTS6, RC.SEED6)
    pb, po = RC.padded(batch, outs, RC.COUNTS6, 300, 256)
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    total, _, _, leaves, _ = _run_ragged(crit, pb, po, dev)
    g1 = torch.autograd.grad(2.0 * total, leaves, retain_graph=True)
    g2 = torch.autograd.grad(3.0 * total, leaves)
    for x, y in zip(g1, g2):
        assert torch.equal(x * 1.5, y)


@pytest.mark.parametrize("tiled", [False, True])
def test_padding_and_batch_composition_do_not_leak(dev, tiled):
    """Check 4: the same samples padded to (300, 256) and to (384, 320) with different padding contents, a sample batched with others
    vs repeated B times, and two runs: bit-identical per-sample items and gradient slices; padded gradient slots exactly 0."""
    counts = RC.COUNTS6
    B = len(counts)
    batch, outs = RC.make_case(counts, RC.SEED6)
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    crit.tiled = tiled
    runs = []
    for nm1, nm2, fs in ((300, 256, 0), (384, 320, 1), (300, 256, 0)):
        pb, po = RC.padded(batch, outs, counts, nm1, nm2, fill_seed=fs)
        total, items, per, leaves, _ = _run_ragged(crit, pb, po, dev)
        total.backward()
        runs.append((total.detach(), per, tuple(x.grad for x in leaves)))
    a, b, a2 = runs
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1]) and all(torch.equal(x, y) for x, y in zip(a[2], a2[2]))
    assert torch.equal(a[1].view(_i32), b[1].view(_i32)) and torch.equal(a[0], b[0])
    for i, (n1, _) in enumerate(counts):
        for x, y in zip(_slices(a[2], i, n1), _slices(b[2], i, n1)):
            assert torch.equal(x.view(_i32), y.view(_i32)), i
        assert not b[2][0][i, :, n1:].any() and not b[2][2][i, :, n1:].any(), i
    pb, po = RC.padded(batch, outs, counts, 300, 256)
    for i in (1, 4, 5):
        rep_b = {k: v[i:i + 1].expand(B, *v.shape[1:]).contiguous() for k, v in pb.items()}
        rep_o = {k: v[i:i + 1].expand(B, *v.shape[1:]).contiguous() for k, v in po.items()}
        total, _, per, leaves, _ = _run_ragged(crit, rep_b, rep_o, dev)
        total.backward()
        n1 = counts[i][0]
        for j in (0, B - 1):
            assert torch.equal(per[j].view(_i32), a[1][i].view(_i32)), (i, j)
            for x, y in zip(_slices(tuple(t.grad for t in leaves), j, n1), _slices(a[2], i, n1)):
                assert torch.equal(x.view(_i32), y.view(_i32)), (i, j)


@pytest.mark.parametrize("counts,seed", CASES)
def test_make_labels_ragged_equals_make_labels_per_sample(dev, counts, seed):
    """Check 5: bit-equal to make_labels at B = 1 on the truncated sample, every sample; padded slots 0."""
    batch, outs = RC.make_case(counts, seed)
    pb, _ = RC.padded(batch, outs, counts, 300, 256)
    dyn, mseg = make_labels_ragged(_to(pb, dev), 0.3)
    assert dyn.shape == (len(counts), 300) and mseg.shape == (len(counts), 300)
    for i, (n1, _) in enumerate(counts):
        b, _ = RC.sample(batch, outs, counts, i)
        wd, wm = make_labels(_to(b, dev), 0.3)
        assert torch.equal(dyn[i, :n1], wd[0]) and torch.equal(mseg[i, :n1].view(_i32), wm[0].view(_i32)), i
        assert not dyn[i, n1:].any() and not mseg[i, n1:].any(), i
        od, om = TO.make_labels(b)
        assert torch.equal(dyn[i, :n1].cpu(), od[0]) and torch.equal(mseg[i, :n1].cpu(), om[0]), i


def test_collated_split_loss_end_to_end(dev, manifest, golden_dir, args, tmp_path, monkeypatch):
    """Check 6: collate_ragged -> forward_ragged -> make_labels_ragged -> RadarFlowLoss.forward_ragged (forward only, the model under
    no_grad) against the oracle's B = 1 forward + loss per frame: the flow within 1e-4 (the forward bound of tests/test_gpu_ragged.py's
    model tests is 2e-4 x max(1, |flow|max); the tighter figure is asserted here as the issue sets it), items within
    1e-4 * max(1, |ref|)."""
    from cmflow_amd import dataset as D
    from test_gpu_ragged import _nets
    ref, net = _nets(manifest, golden_dir, args, dev)
    D.write_synthetic_split(str(tmp_path))

    class DA:
        num_points, eval = 256, True
    items = []
    for part in ("train", "test"):
        d = D.vodDataset(DA(), str(tmp_path), part)
        items += [d[i] for i in range(len(d))]
    cpu = D.extract_data_info_ragged(D.collate_ragged(items), device="cpu")
    bd = D.as_batch_dict_ragged(tuple(t.to(dev) for t in cpu))
    crit = RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR).to(dev)
    with torch.no_grad():
        sf, cls, pt, mk = net.forward_ragged(bd["pc1"], bd["pc2"], bd["ft1"], bd["ft2"], bd["n1"], bd["n2"], validate=True)
        dyn, mseg = make_labels_ragged(bd, 0.3)
        total, it, per = crit.forward_ragged(bd["pc1"], bd["pc2"], sf, bd["ft1"][:, 0], bd["n1"], bd["n2"], bd["flow_label"].transpose(2, 1),
                                             pt, cls, bd["gt_trans"], mseg, dyn, bd["radar_u"], bd["radar_v"], bd["opt_flow"], validate=True)
    assert total.grad_fn is None
    cb = D.as_batch_dict_ragged(cpu)
    P, Tcr = torch.as_tensor(synth.CAMERA_PROJECTION), torch.as_tensor(synth.T_CAMERA_RADAR)
    monkeypatch.setattr(torch, "topk", _stable_topk)
    for i in range(len(items)):
        a, b = int(cb["n1"][i]), int(cb["n2"][i])
        s = {k: cb[k][i:i + 1] for k in ("gt_trans", "interval")}
        for k in ("pc1", "ft1"):
            s[k] = cb[k][i:i + 1, :, :a].contiguous()
        for k in ("pc2", "ft2"):
            s[k] = cb[k][i:i + 1, :, :b].contiguous()
        for k in RC.ROW_KEYS1:
            s[k] = cb[k][i:i + 1, :a].contiguous()
        with torch.no_grad():
            o = ref(s["pc1"], s["pc2"], s["ft1"], s["ft2"], None, "test")
            e_sf = float((sf[i:i + 1, :, :a].cpu() - o[0]).abs().max())
            od, om = TO.make_labels(s)
            ref_total, ref_items = TO.radar_flow_loss(s, o[0], o[2], o[1], om, od, P, Tcr)
        print("frame %d (%d, %d): |flow err| %.3g, counted %s oracle %.7g %s" % (i, a, b, e_sf, per[i].tolist(), float(ref_total), ref_items))
        assert e_sf <= 1e-4, (i, e_sf)
        _check_items(per[i].tolist(), float(ref_total), ref_items, i)
