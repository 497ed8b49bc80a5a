"""CPU: pins tests/kabsch_ref.py, the SVD-free fp64 reference tests/test_gpu_kabsch.py judges the HIP solve by, against three
independent yardsticks: the reference program's own output (golden), the fp64 SVD oracle where its autograd is usable, and central
finite differences where it is not."""
import os

import numpy as np
import torch

from oracle import cmflow_oracle as O
from kabsch_ref import NEWTON_STEPS, centroids_and_H, ego_refine_ref, kabsch_ref, polar_orthogonal


def _case(b, n, seed, planar=1.0, iso=False):
    """A cloud A (b,3,n), B = a rigid motion of it plus noise, positive normalised weights.  fp64."""
    g = torch.Generator().manual_seed(seed)
    ext = torch.tensor([1.0, 1.0, 1.0] if iso else [100.0, 60.0, 6.0 * planar], dtype=torch.float64).view(1, 3, 1)
    A = (torch.rand(b, 3, n, generator=g, dtype=torch.float64) - 0.5) * ext + torch.tensor([40.0, 5.0, 1.0], dtype=torch.float64).view(1, 3, 1)
    ax = torch.randn(b, 3, generator=g, dtype=torch.float64)
    ax = ax / ax.norm(dim=1, keepdim=True) * 0.3
    K = torch.zeros(b, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -ax[:, 2], ax[:, 1], -ax[:, 0]
    R = torch.linalg.matrix_exp(K - K.transpose(1, 2))
    B = R @ A + torch.randn(b, 3, 1, generator=g, dtype=torch.float64) + 0.05 * ext * torch.randn(b, 3, n, generator=g, dtype=torch.float64)
    W = torch.rand(b, n, generator=g, dtype=torch.float64) + 0.1
    return A, B, W / W.sum(dim=1, keepdim=True)


def test_newton_reference_reproduces_the_reference_programs_output(golden_dir):
    """tests/golden/kabsch_kat.npz is models/cmflow.py:WeightedKabsch run in fp32 (identity, equal weights, mirrored cloud = the
    reflection branch, noise, one-hot-ish weights).  Bounds = that golden's own fp32 accuracy, the ones test_gpu_ops.py::
    test_kabsch_kat_and_grad documents: R 1e-5; t 5e-5, because t = cB - R cA cancels centroids of ~50 m in fp32 (the golden's
    "identity" case returns t = 3.8e-6 where the exact answer is 0)."""
    with np.load(os.path.join(golden_dir, "kabsch_kat.npz")) as z:
        A, Bm, W, T = (torch.from_numpy(z[k]) for k in ("A", "B", "W", "trans"))
    got = kabsch_ref(A.double(), Bm.double(), W.double())
    np.testing.assert_allclose(got[:, :3, :3].numpy(), T[:, :3, :3].double().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(got[:, :, 3].numpy(), T[:, :, 3].double().numpy(), rtol=0, atol=5e-5)
    det = torch.linalg.det(got[:, :3, :3])
    np.testing.assert_allclose(det.numpy(), 1.0, atol=1e-12)                       # the mirrored case included
    assert float(torch.linalg.det(polar_orthogonal(centroids_and_H(A.double(), Bm.double(), W.double())[2].transpose(1, 2)))[2]) < 0
    np.testing.assert_allclose(got[0].numpy(), np.eye(4), atol=1e-12)              # identity: exact to fp64 rounding at 50 m
    assert torch.equal(got[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(5, 4))


def test_newton_reference_equals_the_fp64_svd_oracle_on_separated_spectra():
    """Values and autograd gradients against O.weighted_kabsch in fp64 on radar-like clouds (singular values of H ~ 2800 : 1000 : 10
    x N-independent factor: well separated, so torch.svd's autograd with its 1 / (s_i^2 - s_j^2) terms is accurate).  Both sides are
    fp64 with errors ~1e-16 x conditioning (s_1 / s_3 ~ 3e2, gap terms ~1e1): 1e-10 of each tensor's largest entry leaves three
    decades."""
    for b, n, seed, mirror in ((4, 256, 1, False), (3, 37, 2, False), (2, 200, 3, True)):
        A, B, W = _case(b, n, seed)
        if mirror:
            B = B * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64).view(1, 3, 1)
        s = torch.linalg.svdvals(centroids_and_H(A, B, W)[2])
        assert float((s[:, 1] / s[:, 0]).max()) < 0.9 and float((s[:, 2] / s[:, 1]).max()) < 0.9 and float((s[:, 2] / s[:, 0]).min()) > 1e-4
        G = torch.randn(b, 4, 4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        grads = []
        for fn in (kabsch_ref, O.weighted_kabsch):
            a, bb, w = (t.clone().requires_grad_(True) for t in (A, B, W))
            T = fn(a, bb, w)
            (T * G).sum().backward()
            grads.append((T.detach(), a.grad, bb.grad, w.grad))
        assert bool((torch.linalg.det(grads[0][0][:, :3, :3]) > 0).all())
        if mirror:
            assert bool((torch.linalg.det(polar_orthogonal(centroids_and_H(A, B, W)[2].transpose(1, 2))) < 0).all())
        for got, ref, name in zip(grads[0], grads[1], ("T", "gA", "gB", "gW")):
            assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), (name, b, n, float((got - ref).abs().max()), float(ref.abs().max()))


def test_newton_reference_gradient_on_an_isotropic_cloud_matches_finite_differences():
    """s_1 ~ s_2 ~ s_3 (a unit cube rotated rigidly: H ~ R^T / 12): the SVD autograd divides by s_i^2 - s_j^2 ~ 0 and is not usable;
    the Newton reference is checked against central differences of itself in fp64.  Step h = 1e-5 on inputs of O(1)-O(40):
    truncation ~ h^2 |f'''| ~ 1e-10, rounding ~ 1e-16 x 40 / h ~ 4e-10 per entry of T, summed over 12 entries with |G| ~ 1: the
    bound 2e-8 x the gradient's largest entry (>= 1e-1 here) leaves a decade."""
    g = torch.Generator().manual_seed(7)
    n = 12
    A = (torch.rand(1, 3, n, generator=g, dtype=torch.float64) - 0.5)
    A = A - A.mean(dim=2, keepdim=True)
    # exactly isotropic second moments: whiten the cloud, so that H = A W A^T R^T is a multiple of a rotation
    W = torch.full((1, n), 1.0 / n, dtype=torch.float64)
    C = (A * W.unsqueeze(1)) @ A.transpose(1, 2)
    evals, evecs = torch.linalg.eigh(C)
    A = (evecs @ torch.diag_embed(evals.rsqrt()) @ evecs.transpose(1, 2)) @ A + torch.tensor([3.0, -2.0, 1.0], dtype=torch.float64).view(1, 3, 1)
    ang = torch.tensor([[0.0, -0.3, 0.2], [0.3, 0.0, -0.1], [-0.2, 0.1, 0.0]], dtype=torch.float64)
    B = torch.linalg.matrix_exp(ang) @ A + torch.tensor([0.5, 0.2, -0.1], dtype=torch.float64).view(1, 3, 1)
    s = torch.linalg.svdvals(centroids_and_H(A, B, W)[2])[0]
    assert float((s[0] - s[2]) / s[0]) < 1e-12                                        # isotropic to rounding
    G = torch.randn(1, 4, 4, generator=g, dtype=torch.float64)

    def f(a, b, w):
        return float((kabsch_ref(a, b, w) * G).sum())

    a, b, w = (t.clone().requires_grad_(True) for t in (A, B, W))
    (kabsch_ref(a, b, w) * G).sum().backward()
    h = 1e-5
    for k, (x, gx) in enumerate(((A, a.grad), (B, b.grad), (W, w.grad))):
        fd = torch.zeros_like(x)
        flat, out = x.reshape(-1), fd.view(-1)
        for i in range(flat.numel()):
            xp, xm = flat.clone(), flat.clone()
            xp[i] += h
            xm[i] -= h
            args_p, args_m = [A, B, W], [A, B, W]
            args_p[k], args_m[k] = xp.view_as(x), xm.view_as(x)
            out[i] = (f(*args_p) - f(*args_m)) / (2 * h)
        scale = float(fd.abs().max())
        assert scale >= 1e-1
        assert float((gx - fd).abs().max()) <= 2e-8 * scale, (k, float((gx - fd).abs().max()), scale)


def test_newton_iteration_count_covers_the_admitted_conditioning():
    """The fixed count of kabsch_ref.py: at s_3 / s_1 = 1e-6 (a decade below anything the GPU tests admit) the iterate is orthogonal
    to fp64 rounding and four more steps move it by rounding only; the polar factor equals V U^T of an fp64 SVD to 1e-16 x s_1 / s_3
    with margin (1e-9)."""
    g = torch.Generator().manual_seed(11)
    Q1, _ = torch.linalg.qr(torch.randn(6, 3, 3, generator=g, dtype=torch.float64))
    Q2, _ = torch.linalg.qr(torch.randn(6, 3, 3, generator=g, dtype=torch.float64))
    S = torch.tensor([[1.0, 0.5, 1e-6], [1.0, 1e-3, 1e-6], [7.0, 7.0, 7.0], [1e3, 1.0, 1e-2], [1e-9, 1e-10, 1e-12], [2.0, 2.0, 1e-5]], dtype=torch.float64)
    M = Q1 @ torch.diag_embed(S) @ Q2.transpose(1, 2)
    Z = polar_orthogonal(M)
    I = torch.eye(3, dtype=torch.float64)
    assert float((Z.transpose(1, 2) @ Z - I).abs().max()) <= 1e-14
    assert float((polar_orthogonal(M, NEWTON_STEPS + 4) - Z).abs().max()) <= 1e-14
    assert float((Z - Q1 @ Q2.transpose(1, 2)).abs().max()) <= 1e-9


def test_ego_refine_ref_is_the_oracle_tail_in_fp64():
    """ego_refine_ref against the oracle's own lines (EgoMotionHead + refine_with_transform, cmflow_oracle.py:260-270) in fp64 on a
    separated spectrum: same bound and reasoning as the solve above; the mask is an integer decision on identical numbers."""
    A, B, _ = _case(3, 200, 5)
    g = torch.Generator().manual_seed(5)
    score = torch.rand(3, 200, generator=g, dtype=torch.float64)
    flow = B - A
    for eps, thres in ((1e-4, 0.5), (0.0, 0.3)):
        T, sf, m = ego_refine_ref(flow, A, score, eps, thres)
        e32, t32 = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(thres, dtype=torch.float32))
        sc = score + e32 if eps else score
        Tr = O.weighted_kabsch(A, A + flow, sc / sc.sum(dim=1).unsqueeze(1))
        mr = score > t32
        sfr = O.CMFlow.refine_with_transform(flow, A, Tr, mr)
        assert torch.equal(m, mr) and 0 < int(m.sum()) < m.numel()
        assert float((T - Tr).abs().max()) <= 1e-10 * float(Tr.abs().max())
        assert float((sf - sfr).abs().max()) <= 1e-10 * float(sfr.abs().max())
