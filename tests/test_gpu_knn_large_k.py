"""GPU: knn_wrapper / pointnet2_utils.knn over the upper part of the reference's range, 64 < k <= 200 (the wave-per-query kernel
knn_wave_kernel of csrc/neighbor.hip), against the C oracle's knn_wrapper on the CPU: indices bit-exact (strict '<', the
first-seen point wins ties), distances to rtol 1e-6 after the square root -- the bound test_knn_and_three_nn uses for the same op.
The oracle is the yardstick for m >= k only: behind the cloud it writes +inf where the kernels write index 0 / distance 0."""
import numpy as np
import pytest
import torch

from cmflow_amd import synth
from knn_large_k_case import grid_cloud, ordered_clouds
from oracle import ops as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _clouds(B, N, M, seed):
    b = synth.make_batch(B, N=max(N, M), seed=seed)
    return b["pc1"].permute(0, 2, 1)[:, :N].contiguous(), b["pc2"].permute(0, 2, 1)[:, :M].contiguous()


def _oracle(k, unknown, known):
    B, N, M = unknown.shape[0], unknown.shape[1], known.shape[1]
    d2, i = torch.empty(B, N, k), torch.empty(B, N, k, dtype=torch.int32)
    orc.knn_wrapper(B, N, M, k, unknown, known, d2, i)
    return d2, i


def _wrapper(dev, k, unknown, known):
    """knn_wrapper as a caller of the extension uses it: buffers of its own, squared distances back."""
    from cmflow_amd.pointnet2_utils import knn_wrapper
    B, N, M = unknown.shape[0], unknown.shape[1], known.shape[1]
    d2 = torch.full((B, N, k), -1.0, device=dev)
    i = torch.full((B, N, k), -1, dtype=torch.int32, device=dev)
    knn_wrapper(B, N, M, k, unknown.to(dev), known.to(dev), d2, i)
    return d2.cpu(), i.cpu()


def _check(dev, k, unknown, known):
    from cmflow_amd.pointnet2_utils import knn
    d_ref, i_ref = _oracle(k, unknown, known)
    d, i = knn(k, unknown.to(dev), known.to(dev))
    assert torch.equal(i.cpu(), i_ref)
    np.testing.assert_allclose(d.cpu().numpy(), np.sqrt(d_ref.numpy()), rtol=1e-6, atol=0)
    return i_ref


@pytest.mark.parametrize("B,N,M,k", [(1, 70, 200, 65),      # first k past the old limit; a partial last workgroup of queries
                                     (2, 130, 257, 128),    # two samples, M one past a multiple of 64
                                     (1, 64, 1025, 200),    # the largest k; M one past the LDS tile: the list crosses a tile boundary
                                     (1, 37, 200, 200),     # m == k: every point is in every list
                                     (1, 1, 300, 129)])     # a single query
def test_range_from_the_oracle(dev, B, N, M, k):
    unknown, known = _clouds(B, N, M, seed=N + M + k)
    _check(dev, k, unknown, known)


@pytest.mark.parametrize("k", [65, 200])
def test_ties_keep_the_first_seen_point(dev, k):
    unknown, known = grid_cloud(70, 300, seed=11)
    _check(dev, k, unknown, known)


def test_identical_points_are_listed_in_index_order(dev):
    k, M = 200, 300
    unknown, _ = grid_cloud(5, M, seed=3)
    known = torch.full((1, M, 3), 2.0)
    i_ref = _check(dev, k, unknown, known)
    assert torch.equal(i_ref, torch.arange(k, dtype=torch.int32).expand(1, 5, k))


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_order_of_arrival(dev, order):
    """Descending: every point enters at the head of the list; ascending: nothing enters after the first k."""
    known = ordered_clouds(400, seed=5)[order]
    _check(dev, 128, torch.zeros(1, 2, 3), known)


def test_fewer_points_than_slots(dev):
    B, N, M, k = 1, 5, 100, 150
    unknown, known = _clouds(B, N, M, seed=17)
    d_ref, i_ref = _oracle(k, unknown, known)
    d2, i = _wrapper(dev, k, unknown, known)
    assert torch.equal(i[..., :M], i_ref[..., :M])
    np.testing.assert_allclose(np.sqrt(d2[..., :M].numpy()), np.sqrt(d_ref[..., :M].numpy()), rtol=1e-6, atol=0)
    assert torch.equal(i[..., M:], torch.zeros(B, N, k - M, dtype=torch.int32))
    assert torch.equal(d2[..., M:], torch.zeros(B, N, k - M))


def test_empty_cloud(dev):
    unknown, _ = _clouds(1, 5, 5, seed=2)
    d2, i = _wrapper(dev, 70, unknown, torch.empty(1, 0, 3))
    assert torch.equal(i, torch.zeros(1, 5, 70, dtype=torch.int32))
    assert torch.equal(d2, torch.zeros(1, 5, 70))


def test_agreement_across_the_seam(dev):
    """The first 64 columns of the wave kernel's lists are the register kernel's k = 64 lists, bit for bit."""
    unknown, known = _clouds(2, 100, 500, seed=23)
    d64, i64 = _wrapper(dev, 64, unknown, known)
    for k in (65, 200):
        d2, i = _wrapper(dev, k, unknown, known)
        assert torch.equal(i[..., :64], i64)
        assert torch.equal(d2[..., :64], d64)


@pytest.mark.parametrize("k", [201, 0])
def test_k_outside_the_range_is_refused(dev, k):
    unknown, known = _clouds(1, 8, 300, seed=4)
    with pytest.raises(RuntimeError, match="cmf_knn_points failed"):
        _wrapper(dev, k, unknown, known)


@pytest.mark.parametrize("k", [64, 40])
def test_k_up_to_64_is_unchanged(dev, k):
    unknown, known = _clouds(1, 128, 500, seed=128 + 500 + k)
    _check(dev, k, unknown, known)


def test_through_the_public_function(dev):
    from cmflow_amd.pointnet2_utils import knn
    k = 100
    unknown, known = _clouds(2, 50, 300, seed=31)
    d2, i_w = _wrapper(dev, k, unknown, known)
    d, i = knn(k, unknown.to(dev).requires_grad_(), known.to(dev))
    assert i.dtype == torch.int32 and not i.requires_grad and i.shape == (2, 50, k)
    assert torch.equal(i.cpu(), i_w)
    assert torch.equal(d.detach(), torch.sqrt(d2.to(dev)))              # the same square root on the same device: bit for bit
