"""CPU: the host side of the whole-frame loss (RadarFlowLoss.forward_ragged, make_labels_ragged, cmf_radar_loss_counted,
cmf_pseudo_labels_counted) -- the C-ABI mirrors, the argument checks that need no GPU, and the ORACLE side of
tests/test_gpu_ragged_loss.py, so the inputs of that test are known to be good before a GPU sees them."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import ragged_loss_case as RC
from cmflow_amd import synth
from oracle import train_oracle as TO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cmf_radar_loss_counted": 2, "cmf_radar_loss_counted_tiled": 2, "cmf_radar_loss_counted_workspace": 4,
       "cmf_radar_loss_counted_workspace_tiled": 4, "cmf_pseudo_labels_counted": 14}


def test_header_and_ctypes_agree_on_the_new_entry_points(tmp_path):
    from cmflow_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "cmflow_hip.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\b(long long|int)\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert len(m.group(2).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert (_lib.RESTYPES.get(name, ctypes.c_int) is ctypes.c_longlong) == (m.group(1) == "long long"), name
    assert _lib.SIGNATURES["cmf_pseudo_labels_counted"] == _lib.SIGNATURES["cmf_pseudo_labels"][:2] + [ctypes.c_void_p] + \
        _lib.SIGNATURES["cmf_pseudo_labels"][2:]
    # the descriptor filled in from Python has the C layout; the dense descriptor's layout did not move
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cmflow_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(cmf_radar_loss_counted_desc),'
                   ' offsetof(cmf_radar_loss_counted_desc, pc2), offsetof(cmf_radar_loss_counted_desc, items_mean),'
                   ' offsetof(cmf_radar_loss_counted_desc, workspace), sizeof(cmf_radar_loss_desc),'
                   ' offsetof(cmf_radar_loss_desc, workspace)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D, P = _lib.RadarLossCountedDesc, _lib.RadarLossDesc
    assert got == [ctypes.sizeof(D), D.pc2.offset, D.items_mean.offset, D.workspace.offset, ctypes.sizeof(P), P.workspace.offset]


def test_workspace_sizes_are_host_arithmetic():
    from cmflow_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in ("cmf_radar_loss_counted_workspace", "cmf_radar_loss_counted_workspace_tiled"):
        getattr(L, n).restype = ctypes.c_longlong
    assert L.cmf_radar_loss_counted_workspace(6, 300, 256, 8) == 6 * 12                   # the LDS form: counts and partials only
    assert L.cmf_radar_loss_counted_workspace(6, 300, 705, 8) == L.cmf_radar_loss_counted_workspace_tiled(6, 300, 705, 8)
    assert L.cmf_radar_loss_counted_workspace(6, 300, 256, 4) == L.cmf_radar_loss_counted_workspace_tiled(6, 300, 256, 4)
    # a sample's workspace is carved for max(N1max, N2max): the dense tiled size of that cloud
    L.cmf_radar_loss_workspace_tiled.restype = ctypes.c_longlong
    per = lambda n, nb: L.cmf_radar_loss_workspace_tiled(2, n, nb) - L.cmf_radar_loss_workspace_tiled(1, n, nb) - 8
    for n1, n2, nb in ((300, 256, 8), (100, 900, 16), (2000, 40, 4)):
        assert L.cmf_radar_loss_counted_workspace_tiled(3, n1, n2, nb) == 3 * 12 + 3 * per(max(n1, n2), nb)


def _crit():
    from cmflow_amd.losses import RadarFlowLoss
    return RadarFlowLoss(synth.CAMERA_PROJECTION, synth.T_CAMERA_RADAR)


def test_forward_ragged_argument_checks():
    crit = _crit()
    batch, outs = RC.make_case(RC.COUNTS6, RC.SEED6)
    pb, po = RC.padded(batch, outs, RC.COUNTS6, 300, 256)
    call = lambda n1, n2, **kw: crit.forward_ragged(pb["pc1"], pb["pc2"], po["pred_f"], pb["ft1"][:, 0], n1, n2, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):                # CPU tensors: no fallback
        call(pb["n1"], pb["n2"])
    with pytest.raises(RuntimeError, match="GPU only"):
        call(pb["n1"], pb["n2"], validate=True)                        # ... also when the counts are fine
    with pytest.raises(ValueError, match="int32"):
        call(pb["n1"].long(), pb["n2"])
    with pytest.raises(ValueError, match="int32"):
        call(pb["n1"], pb["n2"][:5])
    with pytest.raises(ValueError, match="int32"):
        call(pb["n1"], pb["n2"].to("meta"))                            # another device than the inputs'
    with pytest.raises(ValueError, match="int32"):
        call([256] * 6, pb["n2"])
    for k, bad in (("n1", 8), ("n1", 301), ("n2", 0), ("n2", 257)):     # 8 = num_nb: topk(num_nb + 1) needs one more
        n = {"n1": pb["n1"].clone(), "n2": pb["n2"].clone()}
        n[k][3] = bad
        with pytest.raises(ValueError, match="npoints%s must lie" % k[1]):
            call(n["n1"], n["n2"], validate=True)
        with pytest.raises(RuntimeError, match="GPU only"):            # not validated: trusted (the kernels clamp)
            call(n["n1"], n["n2"])
    with pytest.raises(ValueError):
        crit.forward_ragged(pb["pc1"], pb["pc2"], po["pred_f"][:, :, :299], pb["ft1"][:, 0], pb["n1"], pb["n2"])
    with pytest.raises(ValueError, match="num_nb"):
        crit.forward_ragged(pb["pc1"][:, :, :8], pb["pc2"], po["pred_f"][:, :, :8], pb["ft1"][:, 0, :8], pb["n1"], pb["n2"])


def test_make_labels_ragged_argument_checks():
    from cmflow_amd import dataset as D
    from cmflow_amd.losses import make_labels_ragged
    batch, outs = RC.make_case(RC.COUNTS6, RC.SEED6)
    pb, _ = RC.padded(batch, outs, RC.COUNTS6, 300, 256)
    with pytest.raises(RuntimeError, match="GPU only"):
        make_labels_ragged(pb, 0.3)
    for bad in (pb["n1"].long(), pb["n1"][:5], pb["n1"].to("meta")):
        with pytest.raises(ValueError, match="int32"):
            make_labels_ragged(dict(pb, n1=bad), 0.3)
    info = tuple(pb[k] for k in ("pc1", "pc2", "ft1", "ft2", "gt_trans", "flow_label", "fg_mask", "interval", "radar_u", "radar_v",
                                 "opt_flow", "n1", "n2"))
    d = D.as_batch_dict_ragged(info)
    assert set(d) == set(D.as_batch_dict(info[:11])) | {"n1", "n2"} and d["n1"] is pb["n1"] and d["n2"] is pb["n2"]


@pytest.mark.parametrize("counts,seed", [(RC.COUNTS6, RC.SEED6), (RC.COUNTS5, RC.SEED5)])
def test_oracle_is_finite_on_every_sample_of_the_gpu_tests_batches(counts, seed):
    """losses/radar_loss.py:185-205: the class-balanced BCE of an empty class is NaN, and the masked terms need a dynamic point to be
    worth testing -- every truncated sample holds both motion-seg classes and at least one dynamic point; the oracle at B = 1 gives
    finite items and gradients for every sample, N1 != N2 included.  Padding must not reach a valid slot."""
    assert sum(a == b for a, b in counts) >= 2                         # the bit-exact comparison with the dense kernel needs n1 == n2
    batch, outs = RC.make_case(counts, seed)
    pb, po = RC.padded(batch, outs, counts, 300, 256)
    P, Tcr = torch.as_tensor(synth.CAMERA_PROJECTION), torch.as_tensor(synth.T_CAMERA_RADAR)
    for i, (n1, n2) in enumerate(counts):
        b, o = RC.sample(batch, outs, counts, i)
        assert b["pc1"].shape == (1, 3, n1) and b["pc2"].shape == (1, 3, n2) and b["flow_label"].shape == (1, n1, 3)
        assert torch.equal(pb["pc1"][i, :, :n1], b["pc1"][0]) and torch.equal(pb["pc2"][i, :, :n2], b["pc2"][0])
        assert torch.equal(po["pred_f"][i, :, :n1], o["pred_f"][0]) and torch.equal(pb["opt_flow"][i, :n1], b["opt_flow"][0])
        if n1 < 300:
            assert float(pb["pc1"][i, :, n1:].abs().min()) == 1e4 and float(po["mseg_pre"][i, :, n1:].abs().min()) == 1e4
        dyn, mseg = TO.make_labels(b)
        assert int((mseg == 0).sum()) >= 1 and int((mseg == 1).sum()) >= 1, (i, n1)
        assert int((dyn == 0).sum()) >= 1, (i, n1)
        pf, pt, pm = (o[k].clone().requires_grad_(True) for k in ("pred_f", "pre_trans", "mseg_pre"))
        total, items = TO.radar_flow_loss(b, pf, pt, pm, mseg, dyn, P, Tcr)
        total.backward()
        assert torch.isfinite(total).item() and all(map(lambda v: v == v and abs(v) < 1e6, items.values())), (i, items)
        assert all(torch.isfinite(g).all().item() for g in (pf.grad, pt.grad, pm.grad)), i
        st, sitems = TO.self_supervised_loss(b, o["pred_f"])
        assert torch.isfinite(st).item(), i


def test_the_600_point_case_holds_both_classes_in_every_sample():
    """The same precondition for RC.COUNTS4, down to its sample of 9 points: no empty motion-seg class, a dynamic point."""
    assert sum(a == b for a, b in RC.COUNTS4) >= 2
    batch, outs = RC.make_case(RC.COUNTS4, RC.SEED4, RC.FULL4)
    for i in range(len(RC.COUNTS4)):
        dyn, mseg = TO.make_labels(RC.sample(batch, outs, RC.COUNTS4, i)[0])
        assert int((mseg == 0).sum()) >= 1 and int((mseg == 1).sum()) >= 1 and int((dyn == 0).sum()) >= 1, i
