"""GPU: the ego-motion solve (csrc/kabsch.hip: cmf_weighted_kabsch, cmf_ego_refine, their backward and counted variants) against
tests/kabsch_ref.py, an fp64 reference that contains no SVD and nothing of the product (pinned on the CPU by tests/test_kabsch_ref.py).

Inputs are built on the CPU from seeded generators in fp64, rounded to fp32 ONCE, and those fp32 values go to the kernel and, as
.double(), to the reference.  Strict bounds where the mathematics is well posed (a, c, d); properties only where the rotation is
not unique (b).  Every bound is derived next to its constant; the measured figures are in DESIGN.md "Kabsch".
"""
import numpy as np
import pytest
import torch

from oracle import cmflow_oracle as O
from kabsch_ref import centroids_and_H, ego_refine_ref, kabsch_ref, polar_orthogonal

pytestmark = pytest.mark.gpu
_f32, _f64, _i32 = torch.float32, torch.float64, torch.int32

U32 = 2.0 ** -23          # one fp32 ulp relative to the binade's lower end: rounding once to fp32 errs by at most half of it
# (a) |got - ref| <= U32 |ref| + C_SOLVE * scale.  The kernel reads fp32, sums and solves in fp64 and rounds each output once: the
# first term (twice the half-ulp of that one rounding).  The second is the fp64 work of BOTH sides: unit roundoff 1.1e-16, grown to
# ~1e-15 by the sums over up to 4096 points and the Jacobi threshold (1e-15), times the conditioning of the polar factor,
# s_1 / (s_2 + s_3) <= 1e3 as admitted below: 1e-12 of the tensor's largest entry; two decades of margin for the gradient, which
# divides by s_i + s_j once more, and for t = cB - R cA, which multiplies R's error by a centroid of up to 5e3 m.
C_SOLVE = 1e-10
COND_MIN = 1e-3           # admitted (s_2 + s_3) / s_1: the issue's line between well-posed and degenerate
DET_MIN = 1e-4            # admitted s_3 / s_1 = |det H| / (s_1^2 s_2) scaled: the sign of det(V U^T) is then decided 12 decades above fp64 rounding
# angle of Rgot^T Rref: Rgot's entries (|.| <= 1) are rounded to fp32, each by <= 2^-24, so ||dR||_F <= 3 * 2^-24 and the rotation
# angle of (R + dR)^T R is ||skew part||_F / sqrt(2) <= ||dR||_F / sqrt(2) = 1.27e-7 rad; C_SOLVE for the fp64 solve behind it.
ANGLE_MAX = 3 * 2.0 ** -24 / np.sqrt(2.0) + C_SOLVE
EXTENT = (100.0, 60.0, 6.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


# ---- input builders (fp64 on the CPU; rounded to fp32 by the caller) -------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rot(axis, angle):
    """Rodrigues in fp64: axis (3,), angle in radians."""
    a = torch.tensor(axis, dtype=_f64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=_f64)
    return torch.eye(3, dtype=_f64) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _cloud(b, n, g, extent=EXTENT, centre=(40.0, 0.0, 0.0)):
    e = torch.tensor(extent, dtype=_f64).view(1, 3, 1)
    return (torch.rand(b, 3, n, generator=g, dtype=_f64) - 0.5) * e + torch.tensor(centre, dtype=_f64).view(1, 3, 1)


TETRA = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))


def _tetra(b, n, g, centre=(40.0, 0.0, 0.0)):
    """n points around the corners of a 60 x 40 x 20 m tetrahedron (corner i % 4) with +-5 m of jitter: a handful of points whose H
    keeps three comparable singular values (s_3 / s_1 ~ 0.1), which a handful of uniform points in a 6 m slab does not."""
    v = torch.tensor(TETRA, dtype=_f64).t()[:, torch.arange(n) % 4] * torch.tensor([30.0, 20.0, 10.0], dtype=_f64).view(3, 1)
    return v.unsqueeze(0) + (torch.rand(b, 3, n, generator=g, dtype=_f64) - 0.5) * 10.0 + torch.tensor(centre, dtype=_f64).view(1, 3, 1)


def _moved(A, g, angle=0.02, axis=(0.1, -0.2, 1.0), t=(1.0, 0.2, -0.05), noise=0.05):
    """B = R A + t + noise, about the origin (what an ego-motion does to a cloud)."""
    B = _rot(axis, angle) @ A + torch.tensor(t, dtype=_f64).view(1, 3, 1)
    return B + noise * torch.randn(A.shape, generator=g, dtype=_f64) if noise else B


def _uniform_w(b, n):
    return torch.full((b, n), 1.0 / n, dtype=_f64)


def _random_w(b, n, g):
    w = torch.rand(b, n, generator=g, dtype=_f64) + 0.05
    return w / w.sum(dim=1, keepdim=True)


def _sizes(b, n):
    g = _gen(1000 * b + n)
    A = _cloud(b, n, g) if n >= 16 else _tetra(b, n, g)
    return A, _moved(A, g), _random_w(b, n, g)


def _rotation(angle, axis):
    g = _gen(int(angle * 1e6) + 7)
    A = _cloud(3, 256, g)
    return A, _moved(A, g, angle=angle, axis=axis, noise=0.0), _random_w(3, 256, g)


def _offset(dist):
    """Weights 2^-8: they sum to 1 EXACTLY in fp32.  The reference's centroids are sum(W A), not sum(W A) / sum(W), so H and the
    gradients carry terms in (1 - sum W) cA cB^T: with weights that merely round to a sum of 1 +- 1e-8, the gradient's sensitivity to
    sum W is |cA| |cB| ||G_H|| ~ 1e9 at 5 km, and fp64 ITSELF (reference and kernel alike, 1e-16 on the sum) resolves it to ~1e-7 only
    -- a property of that formula, outside what C_SOLVE describes.  The (1 - sum W) terms are pinned at 40 m by w_sum0.5 / w_sum3."""
    g = _gen(int(dist))
    d = dist / np.sqrt(3.0)
    A = _cloud(3, 256, g, centre=(d, -d, d))
    return A, _moved(A, g, angle=0.01), _uniform_w(3, 256)


HOT = [3, 70, 131, 199]


def _weights(kind):
    b, n = 5, 200
    g = _gen(sum(map(ord, kind)))
    A = _cloud(b, n, g)
    if kind == "four_hot":
        A[:, :, HOT] = _tetra(b, 4, g)
    B = _moved(A, g)
    if kind == "uniform":
        W = _uniform_w(b, n)
    elif kind in ("sum0.5", "sum3"):
        W = _random_w(b, n, g) * float(kind[3:])
    elif kind == "half_zero":
        W = _random_w(b, n, g)
        W[:, n // 2:] = 0.0
        W = W / W.sum(dim=1, keepdim=True)
    elif kind == "span1e-8":
        W = 10.0 ** (-8.0 * torch.rand(b, n, generator=g, dtype=_f64))
        W[:, 0], W[:, 1] = 1.0, 1e-8
        W = W / W.sum(dim=1, keepdim=True)
    else:                                                           # nearly one-hot over four points
        W = torch.full((b, n), 1e-6, dtype=_f64)
        W[:, HOT] = 1.0
        W = W / W.sum(dim=1, keepdim=True)
    return A, B, W


def _isotropic():
    """s_1 ~ s_2 ~ s_3: a whitened cloud (weighted second moment = identity x 100 m^2), moved rigidly without noise."""
    g = _gen(31)
    b, n = 3, 200
    A = torch.randn(b, 3, n, generator=g, dtype=_f64)
    W = _uniform_w(b, n)
    A = A - (A * W.unsqueeze(1)).sum(dim=2, keepdim=True)
    ev, evec = torch.linalg.eigh((A * W.unsqueeze(1)) @ A.transpose(1, 2))
    A = 10.0 * (evec @ torch.diag_embed(ev.rsqrt()) @ evec.transpose(1, 2)) @ A + torch.tensor([20.0, -5.0, 1.0], dtype=_f64).view(1, 3, 1)
    return A, _moved(A, g, angle=0.3, axis=(1.0, 1.0, 0.5), noise=0.0), W


def _planar():
    g = _gen(32)
    A = _cloud(3, 256, g, extent=(100.0, 60.0, 4.5))                # s_3 / s_1 ~ (4.5 / 100)^2 = 2e-3
    return A, _moved(A, g, noise=0.02), _random_w(3, 256, g)


def _mirrored():
    g = _gen(33)
    A = _cloud(3, 256, g)
    return A, _moved(A, g) * torch.tensor([1.0, 1.0, -1.0], dtype=_f64).view(1, 3, 1), _random_w(3, 256, g)


WELL_POSED = {}
for _n in (4, 5, 63, 64, 65, 127, 128, 200, 256, 1000, 4096):
    WELL_POSED["size_B5_N%d" % _n] = (_sizes, (5, _n))
for _b, _n in ((1, 4), (1, 65), (1, 256), (64, 5), (64, 63), (64, 256)):
    WELL_POSED["size_B%d_N%d" % (_b, _n)] = (_sizes, (_b, _n))
for _a in (1e-6, 1e-4, 1e-2, 1.0, 3.0):
    WELL_POSED["yaw_%g" % _a] = (_rotation, (_a, (0.0, 0.0, 1.0)))
    WELL_POSED["axis_%g" % _a] = (_rotation, (_a, (0.5, -0.3, 0.8)))
for _d in (50.0, 500.0, 5000.0):
    WELL_POSED["offset_%g" % _d] = (_offset, (_d,))
for _k in ("uniform", "sum0.5", "sum3", "half_zero", "span1e-8", "four_hot"):
    WELL_POSED["w_" + _k] = (_weights, (_k,))
WELL_POSED["isotropic"] = (_isotropic, ())
WELL_POSED["planar"] = (_planar, ())
WELL_POSED["mirrored"] = (_mirrored, ())


def _within(got, ref, name, c=C_SOLVE):
    """|got - ref| <= U32 |ref| + c * (largest |ref| of the sample's tensor); got fp32 from the kernel, ref fp64."""
    got, ref = got.detach().cpu().double(), ref.detach()
    assert bool(torch.isfinite(got).all()), name
    scale = ref.abs().reshape(ref.shape[0], -1).amax(dim=1).view(-1, *([1] * (ref.dim() - 1)))
    excess = (got - ref).abs() - (U32 * ref.abs() + c * scale)
    worst = float(((got - ref).abs() / scale.clamp_min(1e-300)).max())
    print("%-24s max|err|/scale %.3e" % (name, worst))
    assert float(excess.max()) <= 0.0, (name, float(excess.max()), worst)


def _angle(Ra, Rb):
    """Rotation angle of Ra^T Rb in radians, fp64, accurate near 0: atan2(|vee(skew)|, (trace - 1) / 2)."""
    M = Ra.transpose(1, 2) @ Rb
    v = torch.stack((M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]), dim=1) / 2
    return torch.atan2(v.norm(dim=1), (M.diagonal(dim1=1, dim2=2).sum(dim=1) - 1) / 2)


# ---- (a) the solve, well-posed inputs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(WELL_POSED))
def test_weighted_kabsch_matches_fp64_reference(dev, case):
    """Forward and backward of cmf_weighted_kabsch on well-posed inputs, every entry within U32 |ref| + C_SOLVE scale of the fp64
    Newton reference; the rotation error asserted as an angle.  Gradients with all of A, B, W and with subsets (null output pointers)."""
    from cmflow_amd.radarflow_util import weighted_kabsch
    fn, args = WELL_POSED[case]
    A, B, W = (t.float() for t in fn(*args))
    b = A.shape[0]
    a64, b64, w64 = (t.double().requires_grad_(True) for t in (A, B, W))
    H = centroids_and_H(a64, b64, w64)[2].detach()
    s = torch.linalg.svdvals(H)
    cond, det = (s[:, 1] + s[:, 2]) / s[:, 0], s[:, 2] / s[:, 0]
    print("%s: (s2+s3)/s1 min %.3e, s3/s1 min %.3e, s2/s1 max %.4f" % (case, float(cond.min()), float(det.min()), float((s[:, 1] / s[:, 0]).max())))
    assert float(cond.min()) >= COND_MIN and float(det.min()) >= DET_MIN, "not a well-posed input: fix the case"
    if case == "isotropic":
        assert float(((s[:, 0] - s[:, 2]) / s[:, 0]).max()) <= 1e-3
    if case == "planar":
        assert 1e-3 <= float(det.min()) and float(det.max()) <= 1e-2
    negative = torch.linalg.det(polar_orthogonal(H.transpose(1, 2))) < 0
    assert bool(negative.all()) if case == "mirrored" else not bool(negative.any())      # the reflection branch, and only there

    G = torch.randn(b, 4, 4, generator=_gen(b + A.shape[2])).float()
    G[:, 3] = 0
    Tref = kabsch_ref(a64, b64, w64)
    (Tref * G.double()).sum().backward()
    a, bb, w = (t.clone().to(dev).requires_grad_(True) for t in (A, B, W))
    T = weighted_kabsch(a, bb, w)
    (T * G.to(dev)).sum().backward()
    _within(T, Tref, "T")
    assert torch.equal(T[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(b, 4))
    ang = _angle(T[:, :3, :3].detach().cpu().double(), Tref[:, :3, :3].detach())
    print("angle error max %.3e rad (reference angle %.3e rad)" % (float(ang.max()), float(_angle(torch.eye(3, dtype=_f64).expand(b, 3, 3), Tref[:, :3, :3].detach()).max())))
    assert float(ang.max()) <= ANGLE_MAX
    refs = {"A": a64.grad, "B": b64.grad, "W": w64.grad}
    for t, k in ((a, "A"), (bb, "B"), (w, "W")):
        _within(t.grad, refs[k], "g" + k)
    for subset in ("A", "BW", "W", "B"):                                                 # the others' output pointers are null
        leaves = {k: t.clone().to(dev).requires_grad_(k in subset) for k, t in (("A", A), ("B", B), ("W", W))}
        (weighted_kabsch(leaves["A"], leaves["B"], leaves["W"]) * G.to(dev)).sum().backward()
        for k, t in leaves.items():
            if k in subset:
                _within(t.grad, refs[k], "g%s of {%s}" % (k, subset))
            else:
                assert t.grad is None


# ---- (b) degenerate inputs: properties only -----------------------------------------------------------------------------------------

def _line(n, p0, d):
    """n points p0 + k d, k = 0..n-1 shuffled by a fixed stride: dyadic numbers, exactly representable (exactly collinear in fp32)."""
    k = (torch.arange(n, dtype=_f64) * 7) % n
    return (torch.tensor(p0, dtype=_f64).view(3, 1) + torch.tensor(d, dtype=_f64).view(3, 1) * k.view(1, n)).unsqueeze(0)


def _degenerate(kind):
    g = _gen(sum(map(ord, kind)))
    if kind in ("n1", "n2", "n3"):
        n = int(kind[1])
        A = _cloud(2, n, g)
        return A, _moved(A, g), _uniform_w(2, n)
    if kind == "identical":
        A = torch.tensor([12.5, -3.25, 0.75], dtype=_f64).view(1, 3, 1).expand(2, 3, 40).clone()
        return A, A + torch.tensor([0.5, 0.25, 0.0], dtype=_f64).view(1, 3, 1), _uniform_w(2, 40)
    if kind == "collinear":
        A = _line(40, (8.0, 4.0, 2.0), (0.5, 0.25, 0.125))
        B = _line(40, (8.5, 3.75, 2.0), (0.25, 0.5, -0.125))
        return A, B, _uniform_w(1, 40)
    if kind == "planar_z0":
        A = _cloud(2, 100, g)
        A[:, 2] = 0.0
        B = _moved(A, g, axis=(0.0, 0.0, 1.0), t=(1.0, 0.2, 0.0))
        B[:, 2] = 0.0
        return A, B, _random_w(2, 100, g)
    if kind == "zero_weights":
        A = _cloud(2, 100, g)
        return A, _moved(A, g), torch.zeros(2, 100, dtype=_f64)
    assert kind == "a_equals_b"
    A = _cloud(3, 200, g)
    return A, A.clone(), _random_w(3, 200, g)


@pytest.mark.parametrize("kind", ["n1", "n2", "n3", "identical", "collinear", "planar_z0", "zero_weights", "a_equals_b"])
def test_weighted_kabsch_degenerate_inputs_keep_the_contract(dev, kind):
    """Rank-deficient H (the completion branches of svd3, the zero-denominator guard of the backward): the rotation is not unique, so
    only the contract of include/cmflow_hip.h is asserted -- finite, orthogonal and proper to 1e-6 (fp32 entries: 3 * 2^-24 ~ 2e-7 of
    rounding in a row's products, five-fold margin), exact bottom row, t consistent with the returned R, finite gradients that carry
    nothing through a pair of undetermined directions.  A = B (full rank) must give the identity within the bound of (a)."""
    from cmflow_amd.radarflow_util import weighted_kabsch
    A, B, W = (t.float() for t in _degenerate(kind))
    b, _, n = A.shape
    G = torch.randn(b, 4, 4, generator=_gen(n)).float()
    a, bb, w = (t.clone().to(dev).requires_grad_(True) for t in (A, B, W))
    T = weighted_kabsch(a, bb, w)
    (T * G.to(dev)).sum().backward()
    T = T.detach().cpu()
    assert bool(torch.isfinite(T).all())
    R, t = T[:, :3, :3].double(), T[:, :3, 3].double()
    assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=_f64)).abs().max()) <= 1e-6
    assert float((torch.linalg.det(R) - 1.0).abs().max()) <= 1e-6
    assert torch.equal(T[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(b, 4))
    a64, b64, w64 = A.double(), B.double(), W.double()
    cA, cB, H = centroids_and_H(a64, b64, w64)
    # t = cB - R cA from the RETURNED (fp32) R: R's entries and t are each rounded once (2^-24 relative), so the difference is at
    # most one fp32 ulp (2^-23) of the sum of the magnitudes of the terms
    terms = cB.abs().squeeze(2) + (R.abs() @ cA.abs()).squeeze(2)
    assert bool(((t - (cB - R @ cA).squeeze(2)).abs() <= U32 * terms + 1e-300).all()), (t, (cB - R @ cA).squeeze(2))
    s = torch.linalg.svdvals(H)
    if kind == "a_equals_b":
        assert float(((s[:, 1] + s[:, 2]) / s[:, 0]).min()) >= COND_MIN
        eye = torch.eye(4, dtype=_f64).expand(b, 4, 4)
        _within(T, eye, "T (A = B)")
    else:
        assert float((s[:, 2] / s[:, 0].clamp_min(1e-300)).max()) <= 1e-12 or float(s[:, 0].max()) == 0.0      # really rank deficient
    # gradients: finite, and no larger than the polar derivative over the DETERMINED singular values allows.  With G_H = -U Y V^T,
    # Y_ij = (Q_ij - Q_ji) / (s_i + s_j) and Y_ij = 0 where both are null:  ||G_H||_F <= 2 ||G_Z||_F / s_min,  s_min the smallest
    # non-null singular value, ||G_Z||_F <= ||G_R||_F + |g_t| |cA|;  then per point  |g_B| <= w (||G_H|| |a - cA| + |g_cB|),
    # |g_cB| <= |g_t| + |1 - sum W| ||G_H|| |cA|  (kabsch.hip, backward) and likewise for A and W.  Dividing by the rounding residue of
    # a null direction instead (~1e-16 s_1) overshoots this ceiling by ten decades or more.
    G64 = G.double()
    gR, gt = G64[:, :3, :3].flatten(1).norm(dim=1), G64[:, :3, 3].norm(dim=1)
    nonnull = s > 1e-12 * s[:, :1]
    s_min = torch.where(nonnull, s, torch.full_like(s, float("inf"))).amin(dim=1)
    gH = 2.0 * (gR + gt * cA.flatten(1).norm(dim=1)) / s_min                               # 0 where H = 0
    da, db = (a64 - cA).norm(dim=1).amax(dim=1), (b64 - cB).norm(dim=1).amax(dim=1)
    cmax = torch.maximum(cA.flatten(1).norm(dim=1), cB.flatten(1).norm(dim=1))
    pmax = torch.maximum(a64.norm(dim=1).amax(dim=1), b64.norm(dim=1).amax(dim=1))
    gc = gt + (1.0 - w64.sum(dim=1)).abs() * gH * cmax
    ceil_pts = w64.amax(dim=1) * (gH * torch.maximum(da, db) + gc)
    ceil_w = da * gH * db + 2.0 * gc * pmax
    for leaf, ceil, name in ((a, ceil_pts, "gA"), (bb, ceil_pts, "gB"), (w, ceil_w, "gW")):
        gr = leaf.grad.cpu().double()
        assert bool(torch.isfinite(gr).all()), name
        got = gr.flatten(1).abs().amax(dim=1)
        print("%s %s: max |g| %s, ceiling %s" % (kind, name, got.tolist(), ceil.tolist()))
        assert bool((got <= 1.001 * ceil + 1e-30).all()), (name, got, ceil)


# ---- (c) ego_refine against ego_refine_ref ------------------------------------------------------------------------------------------

THRES = 0.5                                                          # exactly representable: "score == thres" is unambiguous


def _ego_inputs(n, kind, seed, b=3):
    g = _gen(seed)
    pc1 = _cloud(b, n, g).float()
    flow = (_moved(pc1.double(), g, noise=0.3) - pc1.double()).float()
    score = torch.rand(b, n, generator=g).float()
    if kind == "labels":
        score = (score > 0.6).float()
    elif kind == "all_above":
        score = 0.5 + 2.0 ** -10 + 0.4 * score
    elif kind == "all_below":
        score = 0.01 + 0.48 * score
    elif kind == "at_thres":
        score[:, [0, 1, n // 2, n - 2, n - 1]] = THRES
        score[:, 2] = float(np.nextafter(np.float32(THRES), np.float32(1)))
        score[:, 3] = float(np.nextafter(np.float32(THRES), np.float32(0)))
    Gt = torch.randn(b, 4, 4, generator=g).float()
    Gt[:, 3] = 0
    return pc1, flow, score, Gt, torch.randn(b, 3, n, generator=g).float()


def _oracle32(flow, pc1, score, eps, thres):
    """The reference's own arithmetic: cmflow.py:96-125 as the oracle states it, in fp32 on the CPU."""
    mask = score > thres
    sc = score + eps if eps else score
    w = sc / sc.sum(dim=1).unsqueeze(1)
    T = O.weighted_kabsch(pc1, pc1 + flow, w)
    return T, torch.where(mask.unsqueeze(1), O.rigid_to_flow(pc1, T), flow), mask


def _run(fn, flow, pc1, score, Gt, Gs, score_grad, dtype, device="cpu"):
    f = flow.detach().clone().to(dtype).to(device).requires_grad_(True)
    s = score.detach().clone().to(dtype).to(device).requires_grad_(score_grad)
    T, sf, m = fn(f, pc1.to(dtype).to(device), s)
    loss = 0
    if Gt is not None:
        loss = loss + (T * Gt.to(dtype).to(device)).sum()
    if Gs is not None:
        loss = loss + (sf * Gs.to(dtype).to(device)).sum()
    loss.backward()
    out = {"R": T[:, :3, :3], "t": T[:, :3, 3], "sf": sf, "g_flow": f.grad}
    if score_grad:
        out["g_score"] = s.grad
    return {k: v.detach().cpu().double() for k, v in out.items()}, m.cpu(), T.detach().cpu()


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


def _check_ego(got, ref, o32, label):
    """Each quantity within max(2 x the fp32 oracle's own error, 4 fp32 ulps at the quantity's largest magnitude) of the fp64
    reference: the kernel mirrors the reference's fp32 steps (fp32 total, weights, B = pc1 + flow, sf from the fp32 transform), so its
    error is measured against the same steps done by torch in fp32; 2 for an equally valid rounding order, the ulp floor so that a
    lucky oracle error cannot make the bound vacuous."""
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), (label, k)
        e_hip, e_o32 = float((got[k] - ref[k]).abs().max()), float((o32[k] - ref[k]).abs().max())
        bound = max(2.0 * e_o32, 4.0 * _ulp32(float(ref[k].abs().max())))
        print("EGO %-40s %-8s hip %.3e  oracle32 %.3e  bound %.3e" % (label, k, e_hip, e_o32, bound))
        assert e_hip <= bound, (label, k, e_hip, e_o32, bound)


EGO_CASES = [(n, eps, kind) for n in (65, 200, 256, 1000) for eps in (1e-4, 0.0)
             for kind in ("random", "labels", "all_above", "all_below", "at_thres") if not (kind == "labels" and eps == 0.0)]
BACKWARDS = (("both", True, True, True), ("sf_only", False, True, True), ("trans_only", True, False, True), ("no_score_grad", True, True, False))


@pytest.mark.parametrize("n,eps,kind", EGO_CASES)
def test_ego_refine_matches_fp64_reference(dev, n, eps, kind):
    """cmf_ego_refine and its backward against ego_refine_ref (fp64, Newton polar factor): independent of the HIP solve."""
    from cmflow_amd.radarflow_util import ego_refine
    pc1, flow, score, Gt, Gs = _ego_inputs(n, kind, seed=n + len(kind))
    for name, use_t, use_s, sg in BACKWARDS:
        gt, gs = (Gt if use_t else None), (Gs if use_s else None)
        ref, m_ref, _ = _run(lambda f, p, s: ego_refine_ref(f, p, s, eps, THRES), flow, pc1, score, gt, gs, sg, _f64)
        o32, m_o32, _ = _run(lambda f, p, s: _oracle32(f, p, s, eps, THRES), flow, pc1, score, gt, gs, sg, _f32)
        got, m, _ = _run(lambda f, p, s: ego_refine(f, p, s, eps, THRES), flow, pc1, score, gt, gs, sg, _f32, dev)
        assert torch.equal(m, m_ref) and torch.equal(m_o32, m_ref)
        assert torch.equal(m, score > THRES)
        if kind == "at_thres":                                       # strict >: a score equal to the threshold is NOT refined
            idx = [0, 1, n // 2, n - 2, n - 1]
            assert not bool(m[:, idx].any()) and bool(m[:, 2].all()) and not bool(m[:, 3].any())
            assert torch.equal(got["sf"][:, :, idx], flow[:, :, idx].double())
        if kind == "all_above":
            assert bool(m.all())
        if kind == "all_below":
            assert not bool(m.any()) and torch.equal(got["sf"], flow.double())
        if kind in ("random", "labels", "at_thres"):
            assert 0 < int(m.sum()) < m.numel()
        assert ("g_score" in got) == sg
        _check_ego(got, ref, o32, "N%d eps%g %s %s" % (n, eps, kind, name))


def _raw_forward(dev, pc1, flow, score, eps, thres, counts=None, sentinel=7.0):
    """cmf_ego_refine / cmf_ego_refine_counted called directly: every output buffer, pre-filled with a sentinel."""
    from cmflow_amd import _lib
    b, _, n = pc1.shape
    pc1, flow, score = pc1.to(dev).contiguous(), flow.to(dev).contiguous(), score.to(dev).contiguous()
    o = {"W": torch.full((b, n), sentinel, dtype=_f32, device=dev), "Bm": torch.full((b, 3, n), sentinel, dtype=_f32, device=dev),
         "trans": torch.full((b, 4, 4), sentinel, dtype=_f32, device=dev), "aux": torch.zeros(b, 32, dtype=_f64, device=dev),
         "sf": torch.full((b, 3, n), sentinel, dtype=_f32, device=dev), "mask": torch.full((b, n), 9, dtype=torch.uint8, device=dev),
         "stat": torch.full((b, n), sentinel, dtype=_f32, device=dev)}
    p = _lib.dev_ptr
    if counts is None:
        err = _lib.lib().cmf_ego_refine(b, n, float(eps), float(thres), p(pc1, _f32), p(flow, _f32), p(score, _f32), p(o["W"], _f32), p(o["Bm"], _f32),
                                        p(o["trans"], _f32), p(o["aux"], _f64), p(o["sf"], _f32), o["mask"].data_ptr(), _lib.stream_ptr())
    else:
        cnt = torch.tensor(counts, dtype=_i32).to(dev)
        err = _lib.lib().cmf_ego_refine_counted(b, n, float(eps), float(thres), p(pc1, _f32), p(flow, _f32), p(score, _f32), p(cnt, _i32),
                                                p(o["W"], _f32), p(o["Bm"], _f32), p(o["trans"], _f32), p(o["aux"], _f64), p(o["sf"], _f32),
                                                o["mask"].data_ptr(), p(o["stat"], _f32), _lib.stream_ptr())
    _lib.check(err, "cmf_ego_refine")
    o.update(pc1=pc1, score=score)
    return o


def test_ego_refine_grad_with_null_pointers(dev):
    """The autograd wrapper materialises an absent transform gradient as zeros, so the NULL g_trans / g_score arguments of
    cmf_ego_refine_grad are reached through the C entry point itself: g_flow within the (c) bound of the fp64 reference."""
    from cmflow_amd import _lib
    n, eps = 200, 1e-4
    pc1, flow, score, _, Gs = _ego_inputs(n, "random", seed=5)
    o = _raw_forward(dev, pc1, flow, score, eps, THRES)
    gs = Gs.to(dev)
    g_flow, g_w = torch.full_like(o["Bm"], 7.0), torch.full_like(o["W"], 7.0)
    p = _lib.dev_ptr
    _lib.check(_lib.lib().cmf_ego_refine_grad(3, n, eps, p(o["pc1"], _f32), p(o["score"], _f32), p(o["W"], _f32), p(o["Bm"], _f32), o["mask"].data_ptr(),
                                              p(o["aux"], _f64), p(gs, _f32), None, p(g_flow, _f32), p(g_w, _f32), None, _lib.stream_ptr()),
               "cmf_ego_refine_grad")
    ref, m_ref, _ = _run(lambda f, p_, s: ego_refine_ref(f, p_, s, eps, THRES), flow, pc1, score, None, Gs, False, _f64)
    o32, _, _ = _run(lambda f, p_, s: _oracle32(f, p_, s, eps, THRES), flow, pc1, score, None, Gs, False, _f32)
    assert torch.equal(o["mask"].cpu().bool(), m_ref)
    T = o["trans"].cpu().double()
    got = {"R": T[:, :3, :3], "t": T[:, :3, 3], "sf": o["sf"].cpu().double(), "g_flow": g_flow.cpu().double()}
    _check_ego(got, ref, o32, "N200 direct call, null g_trans/g_score")


# ---- (d) ego_refine_counted against ego_refine_ref per truncated sample --------------------------------------------------------------

COUNTS = (1, 3, 63, 64, 65, 300)
NMAX = 300


@pytest.mark.parametrize("fill", [float("nan"), 1e30])
@pytest.mark.parametrize("eps", [1e-4, 0.0])
def test_ego_refine_counted_matches_fp64_reference(dev, fill, eps):
    """One ragged batch, padding filled with NaN or 1e30 (tests/test_gpu_ragged.py fills with +-1e4 and copies): every valid slice
    against ego_refine_ref on the truncated sample within the bounds of (c); padded slots zero / False; counts beyond ld clamp.
    Counts 1 and 3 leave H with rank 0 and 2: the rotation is a completion there (b), but the refined flow of the sample's own
    points is still determined -- R (a - cA) = V_k U_k^T (a - cA) over the k determined singular pairs, the points spanning exactly
    that subspace -- so sf is compared with that expression in fp64, within 4 fp32 ulps at max(|a|, |t|) (the kernel forms
    R a + t - a in fp32 from the fp32 transform: three roundings of R a, one of t, the two sums)."""
    pc1, flow, score, _, _ = _ego_inputs(NMAX, "random", seed=77, b=len(COUNTS))
    for t in (pc1, flow, score):
        for i, c in enumerate(COUNTS):
            t[i, ..., c:] = fill
    o = _raw_forward(dev, pc1, flow, score, eps, THRES, counts=COUNTS)
    over = _raw_forward(dev, pc1, flow, score, eps, THRES, counts=COUNTS[:-1] + (NMAX + 100,))
    for k in ("W", "Bm", "trans", "sf", "mask", "stat"):
        assert torch.equal(o[k].view(torch.uint8), over[k].view(torch.uint8)), k          # a count beyond ld is clamped to ld
    o = {k: v.cpu() for k, v in o.items()}
    for i, n in enumerate(COUNTS):
        p, f, s = pc1[i:i + 1, :, :n], flow[i:i + 1, :, :n], score[i:i + 1, :n]
        for k in ("sf", "Bm"):
            assert not o[k][i, :, n:].any(), (k, i)                                         # exact zeros, not NaN, not the sentinel
        assert not o["W"][i, n:].any() and not o["stat"][i, n:].any() and not o["mask"][i, n:].any()
        assert torch.equal(o["stat"][i, :n], s[0]) and torch.equal(o["Bm"][i, :, :n], (p + f)[0])
        assert torch.equal(o["mask"][i, :n].bool(), s[0] > THRES)
        T = o["trans"][i:i + 1].double()
        assert bool(torch.isfinite(T).all())
        R = T[:, :3, :3]
        assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=_f64)).abs().max()) <= 1e-6 and abs(float(torch.linalg.det(R)) - 1.0) <= 1e-6
        got = {"R": R, "t": T[:, :3, 3], "sf": o["sf"][i:i + 1, :, :n].double()}
        if n >= 63:
            Tr, sfr, _ = ego_refine_ref(f.double(), p.double(), s.double(), eps, THRES)
            T32, sf32, _ = _oracle32(f, p, s, eps, THRES)
            ref = {"R": Tr[:, :3, :3], "t": Tr[:, :3, 3], "sf": sfr}
            o32 = {"R": T32[:, :3, :3].double(), "t": T32[:, :3, 3].double(), "sf": sf32.double()}
            _check_ego(got, ref, o32, "counted n%d eps%g fill%g" % (n, eps, fill))
        else:
            p64, b64 = p.double(), (p + f).double()
            sc = s.double() + float(torch.tensor(eps, dtype=_f32)) if eps else s.double()
            cA, cB, H = centroids_and_H(p64, b64, sc / sc.sum(dim=1, keepdim=True))
            U, S, Vh = torch.linalg.svd(H)
            k = {1: 0, 3: 2}[n]
            assert k == 0 or float(S[0, k - 1] / S[0, 0]) >= COND_MIN
            Zk = Vh[:, :k].transpose(1, 2) @ U[:, :, :k].transpose(1, 2)
            rigid = Zk @ (p64 - cA) + cB - p64
            want = torch.where((s > THRES).unsqueeze(1), rigid, f.double())
            tol = 4.0 * _ulp32(max(float(p64.abs().max()), float(T[:, :3, 3].abs().max())))
            err = float((got["sf"] - want).abs().max())
            print("EGO counted n%d eps%g fill%g sf: hip %.3e  bound %.3e" % (n, eps, fill, err, tol))
            assert err <= tol, (n, err, tol)
