"""Test fixture: the set-conv block (utils/model_utils/radarflow_util.py:121-162, PointLocalFeature) with eval-mode BatchNorm in plain
torch, in any dtype, with the neighbour lists as an INPUT.  Written from the block's definition in the form the product evaluates it
(cmflow_amd/radarflow_util.py PointLocalFeature.forward_pm: the feature half of the first 1x1 conv applied per point beforehand, by
linearity), not from any kernel:

    z1[b,n,s,:] = y[b, idx[b,n,s], :] + Wx (xyz[b, idx[b,n,s]] - xyz[b,n])          first conv, hoisted
    x_l         = relu(a_l z_l + c_l),  a_l = gamma_l / sqrt(var_l + eps_l),  c_l = beta_l - mean_l a_l      (running statistics)
    z2 = x1 W2^T,  z3 = x2 W3^T,  pooled = max_s x3,  then (W4, W5, W6): three per-point linear + BN + ReLU layers (mlp2).

Nothing under cmflow_amd/ or oracle/ is imported here; tests/test_setconv_ref.py anchors it to oracle.cmflow_oracle.PointLocalFeature
and tests/test_gpu_setconv_chain.py judges the register-chain kernels (csrc/setconv_chain.hip) by it.  Gradients come from autograd.
"""
import math

import torch


class SetConvRef:
    """What set_conv_ref returns.  out (B,N,C6); y, params: the leaves (copies of the inputs in `dtype`) the gradients refer to;
    u: the six BatchNorm outputs (pre-ReLU), u[0..2] per neighbour slot (B,N,S,C), u[3..5] per point (B,N,C);
    argmax_src (B,N,C3): the SOURCE POINT of the slot torch's max selected (tied slots that repeat one point agree on it)."""

    def __init__(self, out, y, params, u, argmax_src):
        self.out, self.y, self.params, self.u, self.argmax_src = out, y, params, u, argmax_src

    def grads(self, dout):
        """One backward pass: -> [dy, then the 18 parameter gradients in the order of `params`]."""
        return list(torch.autograd.grad(self.out, [self.y] + self.params, dout.to(self.out.dtype)))

    def masks(self):
        return [t > 0 for t in self.u]


def set_conv_ref(xyz, y, idx, params, bn_buffers, dtype):
    """xyz (B,N,3); y (B,N,O1) (any strides); idx (B,N,S) integer source points inside the sample;
    params: wx (O1,3), g1, b1, w2, g2, b2, w3, g3, b3, w4, g4, b4, w5, g5, b5, w6, g6, b6 (weights as (out, in) matrices);
    bn_buffers: six (running_mean, running_var, eps).  Everything is evaluated in `dtype` on the CPU."""
    xyz = xyz.detach().cpu().to(dtype)
    y = y.detach().cpu().to(dtype).clone().requires_grad_(True)
    P = [p.detach().cpu().to(dtype).clone().requires_grad_(True) for p in params]
    idx = idx.detach().cpu().long()
    B, N, S = idx.shape
    bi = torch.arange(B).view(B, 1, 1)
    u = []

    def bn_relu(z, l):
        mean, var, eps = bn_buffers[l]
        a = P[3 * l + 1] / torch.sqrt(var.detach().cpu().to(dtype) + eps)
        c = P[3 * l + 2] - mean.detach().cpu().to(dtype) * a
        u.append(a * z + c)
        return torch.relu(u[-1])

    d = xyz[bi, idx] - xyz.unsqueeze(2)                               # (B,N,S,3)
    x = bn_relu(y[bi, idx] + d @ P[0].t(), 0)
    x = bn_relu(x @ P[3].t(), 1)
    x = bn_relu(x @ P[6].t(), 2)
    x, am = x.max(dim=2)                                              # (B,N,C3)
    src = torch.gather(idx, 2, am)
    for l in (3, 4, 5):
        x = bn_relu(x @ P[3 * l].t(), l)
    return SetConvRef(x, y, P, u, src)


def ulp32(v):
    """One fp32 unit in the last place of |v| (0 for 0)."""
    v = abs(float(v))
    return 0.0 if v == 0.0 else 2.0 ** (max(math.floor(math.log2(v)), -126) - 23)


def max_err(a, r):
    """Largest elementwise |a - r| (r: the fp64 reference)."""
    return float((a.detach().cpu().double() - r.detach().cpu().double()).abs().max())


def norm_err(a, r):
    """||a - r|| / ||r||"""
    r = r.detach().cpu().double()
    return float((a.detach().cpu().double() - r).norm() / r.norm())
