"""Host restatement of ``cmf_augment_batch``'s rule (include/cmflow_hip.h), numpy only, written from the header's text and not from
the kernel's code: the generator (Philox4x32-10 of tests/draw_ref.py), the angle without trigonometry in float64, the float32 point
rule and the float64 transform rule.  Python floats are IEEE doubles and numpy float32 scalars round every operation on its own, so
every line below is one rounded operation, in the header's order.

``exact_*``: the same transform family in exact-as-float64 form (a true rotation from cos / sin), for the mathematics -- the loss is
invariant under it -- where the bit pattern does not matter."""
import math

import numpy as np

import draw_ref as DR

F32 = np.float32


def slot_words(seed, aug_draw, slot):
    """(u32, mirror bit) of a slot: words 0 and 1 of counter (slot, 2, 0, 0) under the key of (seed, aug_draw)."""
    w = DR.philox4x32_10((int(slot), 2, 0, 0), DR.draw_key(seed, aug_draw))
    return int(w[0]), int(w[1]) >> 31


def angle(u32, tan_half_max):
    """-> (cf, sf) float32 from the 32-bit word, float64 operations rounded one by one."""
    r = float(u32) * 2.0 ** -32
    t = ((2.0 * r) - 1.0) * float(tan_half_max)
    q = t * t
    d = 1.0 + q
    c = (1.0 - q) / d
    s = (2.0 * t) / d
    return F32(c), F32(s)


def slot_params(seed, aug_draw, slot, tan_half_max, mirror):
    u32, bit = slot_words(seed, aug_draw, slot)
    cf, sf = angle(u32, tan_half_max)
    m = F32(-1.0) if (mirror and bit) else F32(1.0)
    return cf, sf, m


def is_identity(cf, sf, m):
    return cf == F32(1.0) and sf == F32(0.0) and m == F32(1.0)


def matrix(cf, sf, m):
    """A (3,3) float32: [cf, -m sf, 0; sf, m cf, 0; 0, 0, 1]."""
    return np.array([[cf, -(m * sf), 0.0], [sf, m * cf, 0.0], [0.0, 0.0, 1.0]], dtype=F32)


def points(x, y, cf, sf, m):
    """x, y float32 arrays -> (x', y'), every float32 operation rounded on its own; the exact identity copies."""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    if is_identity(cf, sf, m):
        return x.copy(), y.copy()
    ym = m * y
    return (cf * x) - (sf * ym), (sf * x) + (cf * ym)


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def transforms(gt, tcr, cf, sf, m):
    """gt (4,4), tcr (4,4) float32 -> (gt', aug, calib) float32 (4,4), float64 from the float32 entries, one rounding to float32."""
    gt, tcr = np.asarray(gt, dtype=F32), np.asarray(tcr, dtype=F32)
    aug, calib = np.zeros((4, 4), dtype=F32), np.zeros((4, 4), dtype=F32)
    aug[3, 3] = calib[3, 3] = 1.0
    if is_identity(cf, sf, m):
        aug[:3, :3] = np.eye(3, dtype=F32)
        calib[:3] = tcr[:3]
        return gt.copy(), aug, calib
    Af = matrix(cf, sf, m)
    aug[:3, :3] = Af
    A = [[float(Af[i, j]) for j in range(3)] for i in range(3)]
    R = [[float(gt[i, j]) for j in range(3)] for i in range(3)]
    t = [float(gt[i, 3]) for i in range(3)]
    C = [[float(tcr[i, j]) for j in range(3)] for i in range(3)]
    H = [[_dot3(R[i][0], A[j][0], R[i][1], A[j][1], R[i][2], A[j][2]) for j in range(3)] for i in range(3)]
    out = np.zeros((4, 4), dtype=F32)
    out[3, 3] = 1.0
    for i in range(3):
        for j in range(3):
            out[i, j] = F32(_dot3(A[i][0], H[0][j], A[i][1], H[1][j], A[i][2], H[2][j]))
            calib[i, j] = F32(_dot3(C[i][0], A[j][0], C[i][1], A[j][1], C[i][2], A[j][2]))
        out[i, 3] = F32(_dot3(A[i][0], t[0], A[i][1], t[1], A[i][2], t[2]))
        calib[i, 3] = tcr[i, 3]
    return out, aug, calib


def augment_ref(batch, tcr, seed, aug_draw, slot0, tan_half_max, mirror):
    """batch: numpy float32 arrays pc1 (B,3,n1), pc2 (B,3,n2), flow_label (B,n1,3), gt_trans (B,4,4); tcr (4,4) -> a dict with the
    four transformed arrays plus aug, calib (B,4,4).  The inputs are left alone."""
    B = batch["pc1"].shape[0]
    out = {k: np.array(batch[k], dtype=F32, copy=True) for k in ("pc1", "pc2", "flow_label", "gt_trans")}
    out["aug"], out["calib"] = np.zeros((B, 4, 4), dtype=F32), np.zeros((B, 4, 4), dtype=F32)
    for s in range(B):
        cf, sf, m = slot_params(seed, aug_draw, slot0 + s, tan_half_max, mirror)
        for k in ("pc1", "pc2"):
            out[k][s, 0], out[k][s, 1] = points(batch[k][s, 0], batch[k][s, 1], cf, sf, m)
        out["flow_label"][s, :, 0], out["flow_label"][s, :, 1] = points(batch["flow_label"][s, :, 0], batch["flow_label"][s, :, 1], cf, sf, m)
        out["gt_trans"][s], out["aug"][s], out["calib"][s] = transforms(batch["gt_trans"][s], tcr, cf, sf, m)
    return out


# ---- the family itself, in float64 with a true rotation ------------------------------------------------------------------------------
def exact_matrix(theta, mirror):
    """Rz(theta) diag(1, m, 1) as a (4,4) float64 with zero translation; orthogonal to float64 rounding."""
    c, s, m = math.cos(theta), math.sin(theta), (-1.0 if mirror else 1.0)
    A = np.eye(4)
    A[:3, :3] = np.array([[c, -m * s, 0.0], [s, m * c, 0.0], [0.0, 0.0, 1.0]])
    return A
