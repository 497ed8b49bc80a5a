"""CPU: the host side of ragged batches -- dataset.collate_ragged on the ragged synthetic split, the argument checks of
forward_ragged that need no device, and the ISA rule of the neighbour search for the counted kernels."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cmflow_amd import dataset as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Args:
    num_points, eval, mini_clip_len, update_len = 256, True, 2, 1


def _items(root, cls=D.vodDataset):
    D.write_synthetic_split(root)
    items = []
    for part in ("train", "test"):
        ds = cls(_Args(), root, part)
        items += [ds[i] for i in range(len(ds))]
    return items


@pytest.mark.parametrize("cls", [D.vodDataset, D.vodClipDataset])
def test_collate_ragged_on_the_synthetic_split(tmp_path, cls):
    items = _items(str(tmp_path), cls)
    assert len(items) == 6
    n1 = [it[0].shape[0] for it in items]
    n2 = [it[1].shape[0] for it in items]
    assert len(set(n1)) > 1 and any(a != b for a, b in zip(n1, n2))          # ragged, and N1 != N2
    out = D.collate_ragged(items)
    assert len(out) == 13
    m1, m2, B = max(n1), max(n2), len(items)
    shapes = [(B, m1, 3), (B, m2, 3), (B, m1, 3), (B, m2, 3), (B, 4, 4), (B, m1, 3), (B, m1), (B,), (B, m1), (B, m1), (B, m1, 2), (B,), (B,)]
    assert [tuple(t.shape) for t in out] == shapes
    assert out[11].dtype == torch.int32 and out[12].dtype == torch.int32
    assert out[11].tolist() == n1 and out[12].tolist() == n2
    for k in range(11):
        assert out[k].dtype == torch.float32, k
    for i, it in enumerate(items):
        for k, n in ((0, n1[i]), (1, n2[i]), (2, n1[i]), (3, n2[i]), (5, n1[i]), (6, n1[i]), (8, n1[i]), (9, n1[i]), (10, n1[i])):
            a = np.asarray(it[k]).astype(np.float32)
            assert np.array_equal(out[k][i, :n].numpy(), a), (i, k)                      # valid slice == the item
            pad = out[k][i, n:].numpy()
            assert np.array_equal(pad, np.broadcast_to(a[:1], pad.shape)), (i, k)        # padding == the sample's first point
        assert np.array_equal(out[4][i].numpy(), it[4]) and float(out[7][i]) == np.float32(it[7])


def test_extract_data_info_ragged_layout(tmp_path):
    data = D.collate_ragged(_items(str(tmp_path)))
    info = D.extract_data_info_ragged(data, device="cpu")
    dense = D.extract_data_info(data[:11], device="cpu")
    assert len(info) == 13
    for a, b in zip(info[:11], dense):
        assert torch.equal(a, b)
    assert info[0].shape[1] == 3 and info[0].shape[2] == data[0].shape[1] and info[1].shape[2] == data[1].shape[1]
    assert info[11].dtype == torch.int32 and torch.equal(info[11], data[11]) and torch.equal(info[12], data[12])


def test_collate_ragged_refuses_empty_input():
    with pytest.raises(ValueError):
        D.collate_ragged([])


def test_forward_ragged_is_a_new_method_with_the_documented_signature():
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    from cmflow_amd.raflow import RaFlow
    assert list(inspect.signature(CMFlow.forward_ragged).parameters) == \
        ["self", "pc1", "pc2", "feature1", "feature2", "npoints1", "npoints2", "validate"]
    assert list(inspect.signature(CMFlow_T.forward_ragged).parameters) == \
        ["self", "pc1", "pc2", "feature1", "feature2", "npoints1", "npoints2", "gfeat", "validate"]
    assert inspect.signature(CMFlow.forward_ragged).parameters["validate"].default is False
    with pytest.raises(NotImplementedError):
        RaFlow.forward_ragged(None)


def test_forward_ragged_refuses_training_and_autograd_before_touching_the_device():
    from cmflow_amd.cmflow import CMFlow

    class A:
        num_points, stat_thres = 256, 0.5
    net = CMFlow(A())
    x = torch.zeros(2, 3, 16)
    n = torch.full((2,), 16, dtype=torch.int32)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="eval"):
            net.forward_ragged(x, x, x, x, n, n)
    net.eval()
    with pytest.raises(RuntimeError, match="no_grad"):
        net.forward_ragged(x, x, x, x, n, n)
    with torch.no_grad():
        with pytest.raises(ValueError):
            net.forward_ragged(x, x, x, x, n.long(), n)                                   # counts are int32
        with pytest.raises(ValueError, match="1024"):
            big = torch.zeros(2, 3, 1025)
            net.forward_ragged(big, big, big, big, n, n)
        with pytest.raises(ValueError, match="npoints2"):
            net.forward_ragged(x, x, x, x, n, torch.tensor([16, 7], dtype=torch.int32), validate=True)
        with pytest.raises(ValueError, match="npoints1"):
            net.forward_ragged(x, x, x, x, torch.tensor([17, 16], dtype=torch.int32), n, validate=True)
        with pytest.raises(RuntimeError):                                                 # no CPU fallback behind the checks
            net.forward_ragged(x, x, x, x, n, n, validate=True)


def test_counted_neighbour_kernels_follow_the_isa_rule():
    """The counted ball query keeps the canonical distance (three products, two adds, no contraction); the counted kNN keeps the
    k-ordered FMA chain of the dense kNN -- the rule tests/test_build.py checks on the dense kernels."""
    src = os.path.join(REPO, "cmflow_amd", "csrc", "neighbor.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                          "--cuda-device-only", "-o", "-", src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    asm = out.stdout
    for sym in ("_Z30ball_query_multi_ballot_kernelILi1ELb1E", "_Z30ball_query_multi_ballot_kernelILi2ELb1E",
                "_Z30ball_query_multi_ballot_kernelILi4ELb1E"):
        start = asm.index(sym + "Ev")
        body = asm[start:asm.index("s_endpgm", start)]
        assert not re.search(r"v_(fma|fmac|mad|pk_fma)_f32", body), sym
    knn = asm[asm.index("_Z10knn_kernelILi8ELb0ELb1EEv"):]
    knn = knn[:knn.index("s_endpgm")]
    assert re.search(r"v_(fma|fmac)_f32", knn)
