"""CPU: pins tests/gemm_ref.py, the fp64 statement of cmf_gemm that tests/test_gpu_gemm_matrix.py judges the HIP kernel by, against
torch.nn.functional and autograd in float64 (agreement ~1e-12), so the reference does not lean on the kernel it judges."""
import torch
import torch.nn.functional as F

from gemm_ref import gemm_ref, grid

D = torch.float64
TOL = 1e-12


def _close(a, b, tol=TOL):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def _rand(*s, g):
    return torch.randn(*s, generator=g, dtype=D)


def test_forward_with_prologue_bias_and_each_activation_equals_functional():
    g = torch.Generator().manual_seed(0)
    M, N, K = 37, 11, 23
    A, W, b = _rand(M, K, g=g), _rand(N, K, g=g), _rand(N, g=g)
    pa, pc = torch.rand(K, generator=g, dtype=D) + 0.5, _rand(K, g=g)
    acts = {0: lambda x: x, 1: F.relu, 2: lambda x: F.leaky_relu(x, 0.1), 3: torch.sigmoid}
    for act, fn in acts.items():
        r = gemm_ref(A, W.t(), pro=(pa, pc), bias=b, act=act)
        want = fn(F.linear(F.relu(pa * A + pc), W, b))
        _close(r.C, want)
        _close(r.P, F.relu(pa * A + pc).abs() @ W.t().abs())
        # the two statistics sums give the batch mean and biased variance F.batch_norm(training=True) normalises with
        s1, s2 = r.terms[0].sum(0), r.terms[1].sum(0)
        mean, var = s1 / M, s2 / M - (s1 / M) ** 2
        eps = 1e-5
        _close((want - mean) / torch.sqrt(var + eps), F.batch_norm(want, None, None, training=True, eps=eps), 1e-10)
    # no prologue, no bias: the plain product, factor 1
    r = gemm_ref(A, W.t())
    _close(r.C, A @ W.t())
    assert bool((r.factor == 1).all())
    # accumulate
    prior = _rand(M, N, g=g)
    _close(gemm_ref(A, W.t(), prior=prior).C, prior + A @ W.t())
    _close(gemm_ref(A, W.t(), prior=prior).P, prior.abs() + A.abs() @ W.t().abs())


def test_b_prologue_equals_functional():
    g = torch.Generator().manual_seed(1)
    rows, cout, cin = 41, 7, 13
    dZ, X = _rand(rows, cout, g=g), _rand(rows, cin, g=g)
    qa, qc = torch.rand(cin, generator=g, dtype=D) + 0.5, _rand(cin, g=g)
    r = gemm_ref(dZ.t(), X, prob=(qa, qc))                           # the weight gradient: contraction over the rows
    _close(r.C, dZ.t() @ F.relu(qa * X + qc))


def test_mode_1_equals_autograd_through_batchnorm_relu_linear():
    g = torch.Generator().manual_seed(2)
    M, N, Kout = 53, 9, 17
    Z = _rand(M, N, g=g).requires_grad_(True)
    gamma = (torch.rand(N, generator=g, dtype=D) + 0.5).requires_grad_(True)
    beta = _rand(N, g=g).requires_grad_(True)
    W, dZout = _rand(Kout, N, g=g), _rand(M, Kout, g=g)
    eps = 1e-5
    bn = F.batch_norm(Z, None, None, gamma, beta, training=True, eps=eps)
    bn.retain_grad()
    F.linear(F.relu(bn), W).backward(dZout)
    mean = Z.detach().mean(0)
    invstd = 1.0 / torch.sqrt(Z.detach().var(0, unbiased=False) + eps)
    ea = gamma.detach() * invstd
    ec = beta.detach() - mean * ea
    d4 = _rand(M, 4, g=g)
    r = gemm_ref(dZout, W, bwd=(1, Z.detach(), ea, ec, mean, invstd), dxyz=d4)
    _close(r.C, bn.grad)                                             # the gradient at the BN output, after the ReLU mask
    _close(r.terms[0].sum(0), beta.grad)
    _close(r.terms[1].sum(0), gamma.grad)
    assert bool((r.factor == (bn.detach() > 0)).all())
    for k in range(3):
        _close(r.terms[2 + k].sum(0), torch.einsum("mn,mk->kn", r.C, d4[:, :3])[k])
    assert len(r.terms) == 5 and len(gemm_ref(dZout, W, bwd=(1, Z.detach(), ea, ec, mean, invstd)).terms) == 2


def test_modes_2_and_3_equal_autograd_through_leaky_relu_and_relu():
    g = torch.Generator().manual_seed(3)
    M, N, Kout = 29, 10, 6
    W, dZout, d4 = _rand(Kout, N, g=g), _rand(M, Kout, g=g), _rand(M, 4, g=g)
    for mode, fn in ((2, lambda x: F.leaky_relu(x, 0.1)), (3, F.relu)):
        Z = _rand(M, N, g=g).requires_grad_(True)                    # no exact zeros: the subgradient there is torch's choice
        assert bool((Z != 0).all())
        F.linear(fn(Z), W).backward(dZout)
        r = gemm_ref(dZout, W, bwd=(mode, Z.detach()), dxyz=d4)
        _close(r.C, Z.grad)
        _close(r.terms[0].sum(0), Z.grad.sum(0))
        assert r.terms[1] is None                                    # the header gives row 1 no meaning in these modes
        _close(torch.stack([t.sum(0) for t in r.terms[2:]]), torch.einsum("mn,mk->kn", r.C, d4[:, :3]))


def test_exact_zeros_take_the_strict_side_of_each_mask():
    Z = torch.tensor([[0.0, 1.0, -1.0]], dtype=D)
    A, B = torch.ones(1, 1, dtype=D), torch.ones(1, 3, dtype=D)
    one, zero = torch.ones(3, dtype=D), torch.zeros(3, dtype=D)
    assert gemm_ref(A, B, bwd=(1, Z, one, zero, zero, one)).C.tolist() == [[0.0, 1.0, 0.0]]
    assert gemm_ref(A, B, bwd=(2, Z)).C.tolist() == [[0.1, 1.0, 0.1]]
    assert gemm_ref(A, B, bwd=(3, Z)).C.tolist() == [[0.0, 1.0, 0.0]]


def test_grid_values_have_exact_zeros_and_survive_fp32():
    g = torch.Generator().manual_seed(4)
    M, N = 257, 40
    Z = grid((M, N), -2, 2, g)
    a, c = grid((N,), 0.5, 2, g), grid((N,), -2, 2, g)
    assert Z.dtype == torch.float32 and bool(((Z * 4) == (Z * 4).round()).all())
    assert float(a.min()) >= 0.5 and float(a.max()) <= 2 and float(Z.min()) >= -2 and float(Z.max()) <= 2
    v64 = a.double() * Z.double() + c.double()
    assert bool((v64.float().double() == v64).all())                 # a * x + c is exact in fp32 ...
    assert bool(((a * Z + c).double() == v64).all())                 # ... rounded per operation
    assert bool((torch.addcmul(c.expand_as(Z), a.expand_as(Z), Z).double() == v64).all())
    assert int((v64 == 0).sum()) > 0 and int((Z == 0).sum()) > M * N // 40
    assert bool(((a * Z + c) > 0).eq(v64 > 0).all())
