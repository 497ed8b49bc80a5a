"""Test fixture: an fp64 reference of the ego-motion solve that contains no SVD.

kabsch_ref restates models/cmflow.py:128-169 (centroids and H exactly as oracle/cmflow_oracle.py:weighted_kabsch) but obtains the
orthogonal factor Z = V U^T of H = U S V^T as the polar factor of H^T by Higham's Newton iteration Z <- (Z + Z^-T) / 2 (N. J. Higham,
"Computing the polar decomposition -- with applications", SIAM J. Sci. Stat. Comput. 7, 1986).  Only torch.linalg.inv is differentiated,
so plain autograd carries no 1 / (s_i - s_j) term and the gradient stays valid for clouds with equal singular values, where the
autograd of torch.svd is not usable.  ego_refine_ref is cmflow.py:96-125 around it.  Everything runs in the dtype of its inputs;
the tests pass fp64 CPU tensors.  Nothing under cmflow_amd/ is imported here.

Iteration count.  Z_0 = H^T / ||H||_F has singular values sigma in (0, 1] with sigma_1 >= 3^-1/2.  One step maps sigma to
(sigma + 1/sigma) / 2: a sigma << 1 becomes ~1/(2 sigma), after which it halves per step until it is O(1) -- at most
log2(1 / sigma_min) + 1 steps -- and from sigma <= 2 the error e = sigma - 1 obeys e' = e^2 / (2 sigma) <= e^2 / 2: 1 -> 0.25 ->
0.025 -> 3e-4 -> 5e-8 -> 1e-15 -> 0, six steps.  The tests admit s_3 / s_1 >= 1e-6 at the very worst (the GPU families stay above
1e-4), i.e. sigma_min >= 5e-7: 22 + 6 = 28 steps.  NEWTON_STEPS = 40 leaves twelve spare; extra steps at the fixed point change nothing
(Z orthogonal => Z^-T = Z up to rounding).
"""
import torch

NEWTON_STEPS = 40


def polar_orthogonal(M, steps=NEWTON_STEPS):
    """(b,3,3) nonsingular M = Z P (Z orthogonal, P symmetric positive definite) -> Z, by Newton's iteration."""
    Z = M / torch.linalg.matrix_norm(M, keepdim=True)           # the polar factor does not depend on a positive scale
    for _ in range(steps):
        Z = 0.5 * (Z + torch.linalg.inv(Z).transpose(1, 2))
    return Z


def centroids_and_H(A, B, W):
    """The weighted centroids (b,3,1) and the covariance H (b,3,3), line for line as oracle/cmflow_oracle.py:weighted_kabsch."""
    b = A.size(0)
    W = W.unsqueeze(2)
    cA = torch.sum(A.transpose(2, 1).contiguous() * W, dim=1).reshape(b, 3, 1)
    cB = torch.sum(B.transpose(2, 1).contiguous() * W, dim=1).reshape(b, 3, 1)
    Am, Bm = A - cA, B - cB
    H = torch.matmul(Am, Bm.transpose(2, 1).contiguous() * W)
    return cA, cB, H


def kabsch_ref(A, B, W):
    """A, B (b,3,N), W (b,N) -> (b,4,4).  R = diag(1, 1, sign det Z) Z with Z = V U^T the polar factor of H^T = V S U^T = Z (U S U^T):
    the reference's "negate row 2 of V when det(V U^T) < 0" (cmflow.py:157-163).  The sign is piecewise constant (no gradient)."""
    b = A.size(0)
    cA, cB, H = centroids_and_H(A, B, W)
    Z = polar_orthogonal(H.transpose(1, 2))
    d = torch.where(torch.linalg.det(Z.detach()) < 0, -1.0, 1.0).to(A.dtype)
    D = torch.ones(b, 3, 1, dtype=A.dtype)
    D[:, 2, 0] = d
    R = D * Z
    t = torch.matmul(-R, cA) + cB
    last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=A.dtype).repeat(b, 1).view(b, 1, 4)
    return torch.cat((torch.cat((R, t), dim=2), last), dim=1)


def rigid_to_flow_ref(pc, trans):
    """models/cmflow.py:51-55: R pc + t - pc."""
    return torch.matmul(trans[:, :3, :3], pc) + trans[:, :3, 3:4] - pc


def ego_refine_ref(flow, pc1, score, eps, thres):
    """models/cmflow.py:96-125 end to end: flow, pc1 (b,3,N), score (b,N) -> (pre_trans (b,4,4), sf_agg (b,3,N), mask (b,N) bool).
    eps is added only when non-zero (cmflow_t.py:119 adds nothing); thres is compared as the fp32 number the kernel receives."""
    mask = score > float(torch.tensor(thres, dtype=torch.float32))
    sc = score + float(torch.tensor(eps, dtype=torch.float32)) if eps else score
    w = sc / sc.sum(dim=1).unsqueeze(1)
    T = kabsch_ref(pc1, pc1 + flow, w)
    return T, torch.where(mask.unsqueeze(1), rigid_to_flow_ref(pc1, T), flow), mask
