"""CPU: the yardstick of tests/test_gpu_knn_large_k.py at the sizes that file uses it at.  orc.knn_wrapper at k = 200 on the
tie-heavy grid cloud must be a stable sort of the fp32 direct-form distances, cut at k -- so that a failing tie test on the GPU
points at the kernel and not at the oracle."""
import numpy as np
import torch

from knn_large_k_case import grid_cloud, stable_knn
from oracle import ops as orc


def test_oracle_knn_at_k_200_is_a_stable_sort_of_the_direct_form_distances():
    N, M, k = 70, 300, 200
    unknown, known = grid_cloud(N, M, seed=11)
    d_ref, i_ref = torch.empty(1, N, k), torch.empty(1, N, k, dtype=torch.int32)
    orc.knn_wrapper(1, N, M, k, unknown, known, d_ref, i_ref)
    d, i = stable_knn(unknown[0].numpy(), known[0].numpy(), k)
    assert len(np.unique(known[0].numpy(), axis=0)) <= 64                # the cloud really is full of duplicates
    assert (d[:, 1:] == d[:, :-1]).sum() > 50 * N                       # ... and every list of exact ties
    assert np.array_equal(i_ref[0].numpy(), i)
    assert np.array_equal(d_ref[0].numpy(), d)
