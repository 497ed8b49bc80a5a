"""numpy restatements of cmflow_amd/csrc/vis.hip (tests/test_vis_host.py, tests/test_gpu_vis.py): the point colours in float64 and the
rasteriser in float32, each with the operation order of include/cmflow_hip.h written out so that every operation is rounded on its
own, plus the builder of the case both GPU tests share."""
import numpy as np

f32 = np.float32
LAYERS = ("flow", "flow_gt", "seg", "seg_gt")
TOMATO, ROYAL_BLUE, BACKGROUND, WHITE = (255, 99, 71), (65, 105, 225), (80, 80, 80), (255, 255, 255)
SEGMENTS = (15, 6, 4, 11, 13, 6)                            # RY, YG, GC, CB, BM, MR

# the table of csrc/vis.hip, copied
WHEEL = np.array([
    (255, 0, 0), (255, 17, 0), (255, 34, 0), (255, 51, 0), (255, 68, 0), (255, 85, 0), (255, 102, 0), (255, 119, 0), (255, 136, 0),
    (255, 153, 0), (255, 170, 0), (255, 187, 0), (255, 204, 0), (255, 221, 0), (255, 238, 0),
    (255, 255, 0), (213, 255, 0), (170, 255, 0), (128, 255, 0), (85, 255, 0), (43, 255, 0),
    (0, 255, 0), (0, 255, 63), (0, 255, 127), (0, 255, 191),
    (0, 255, 255), (0, 232, 255), (0, 209, 255), (0, 186, 255), (0, 163, 255), (0, 140, 255), (0, 116, 255), (0, 93, 255), (0, 70, 255),
    (0, 47, 255), (0, 24, 255),
    (0, 0, 255), (19, 0, 255), (39, 0, 255), (58, 0, 255), (78, 0, 255), (98, 0, 255), (117, 0, 255), (137, 0, 255), (156, 0, 255),
    (176, 0, 255), (196, 0, 255), (215, 0, 255), (235, 0, 255),
    (255, 0, 255), (255, 0, 213), (255, 0, 170), (255, 0, 128), (255, 0, 85), (255, 0, 43)], dtype=np.float64)

# (tan, sqrt(1 + tan^2)) of the bearing lines at 0, +-5, +-10, +-15 degrees: the float literals of csrc/vis.hip, copied
BEARING = np.array([(0.0, 1.0), (0.0874886662, 1.00381982), (-0.0874886662, 1.00381982), (0.176326975, 1.01542664),
                    (-0.176326975, 1.01542664), (0.267949194, 1.03527617), (-0.267949194, 1.03527617)]).astype(f32)


def wheel_from_rule():
    """The 55 entries from the rule: inside a segment of length L the moving channel is floor(255 k / L) or 255 minus it."""
    rows = []
    # (fixed channel at 255, moving channel, rising?) per segment: R->Y, Y->G, G->C, C->B, B->M, M->R
    plan = ((0, 1, True), (1, 0, False), (1, 2, True), (2, 1, False), (2, 0, True), (0, 2, False))
    for L, (fixed, moving, rising) in zip(SEGMENTS, plan):
        for k in range(L):
            step = (255 * k) // L
            row = [0, 0, 0]
            row[fixed] = 255
            row[moving] = step if rising else 255 - step
            rows.append(row)
    return np.array(rows, dtype=np.float64)


# ---- colours: float64 -------------------------------------------------------------------------------------------------------------------
def _wheel_cols(u, v):
    """(255 * col) of flow_xy_to_colors before the floor, (n, 3) float64, for float64 u, v."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        rad = np.sqrt(u * u + v * v)
        a = np.arctan2(-v, -u) / np.pi
        fk = (a + 1.0) / 2.0 * 54.0
        fl = np.floor(fk)
        k0 = np.where((fl >= 0.0) & (fl <= 54.0), fl, 0.0).astype(np.int64)
        k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
        f = fk - k0.astype(np.float64)
        out = np.empty(u.shape + (3,), dtype=np.float64)
        for ch in range(3):
            col0, col1 = WHEEL[k0, ch] / 255.0, WHEEL[k1, ch] / 255.0
            col = (1.0 - f) * col0 + f * col1
            col = np.where(rad <= 1.0, 1.0 - rad * (1.0 - col), col * 0.75)
            out[..., ch] = 255.0 * col
    return out


def _levels(x255):
    with np.errstate(all="ignore"):
        q = np.floor(x255)
        return np.where((q >= 0.0) & (q <= 255.0), q, 0.0).astype(np.uint8)


def wheel_colors(u, v):
    """vis_ops.flow_xy_to_colors(u, v) restated: (n, 3) uint8."""
    return _levels(_wheel_cols(u, v))


def wheel_margin(u, v):
    """The smallest distance of a NON-integer 255 * col to an integer (inf when all are integers)."""
    x = _wheel_cols(u, v)
    x = x[np.isfinite(x)]
    d = np.abs(x - np.rint(x))
    d = d[d > 0]
    return float(d.min()) if d.size else float("inf")


def _normalised(flow, by):
    """(u, v) of vis_util.py:32-42,63 for one frame: ``flow`` (n, >=2) float32 normalised by the largest radius of ``by``."""
    flow, by = np.asarray(flow, dtype=f32).astype(np.float64), np.asarray(by, dtype=f32).astype(np.float64)
    with np.errstate(all="ignore"):
        rad_max = np.max(np.sqrt(by[:, 0] * by[:, 0] + by[:, 1] * by[:, 1]))
        d = rad_max + 1e-5
        return flow[:, 0] / d, -(flow[:, 1] / d)


def frame_colors(layer, flow, label, mask, gt_mask):
    """cmf_vis_point_colors for one frame -> (colors (n,3) uint8, drawn (n) uint8).  flow, label (n,3) float32; mask (n) uint8: the
    predicted one; gt_mask (n) float32: the split's column."""
    n = flow.shape[0]
    drawn = np.ones(n, dtype=np.uint8)
    if layer == "flow":
        return wheel_colors(*_normalised(flow, flow)), drawn
    if layer == "flow_gt":
        return wheel_colors(*_normalised(label, flow)), drawn
    col = np.zeros((n, 3), dtype=np.uint8)
    if layer == "seg":
        col[:] = TOMATO
        col[np.asarray(mask) != 0] = ROYAL_BLUE
        return col, drawn
    assert layer == "seg_gt", layer
    gt_mask = np.asarray(gt_mask, dtype=f32)
    col[gt_mask == 0] = TOMATO
    col[gt_mask == 1] = ROYAL_BLUE
    return col, ((gt_mask == 0) | (gt_mask == 1)).astype(np.uint8)


def frame_margin(layer, flow, label):
    return wheel_margin(*_normalised(flow if layer == "flow" else label, flow))


# ---- raster: float32, + - * and compares ------------------------------------------------------------------------------------------------
def guide_mask(W, H, p):
    """(H, W) bool: the pixels whose centre lies on a range ring or a bearing line.  ``p``: BevView.kernel_params()."""
    cx, cy = (np.arange(W, dtype=f32) + f32(0.5))[None, :], (np.arange(H, dtype=f32) + f32(0.5))[:, None]
    x = (p["x0"] + cx * p["s"]) + np.zeros((H, 1), dtype=f32)
    y = (p["y1"] - cy * p["s"]) + np.zeros((1, W), dtype=f32)
    h = p["half"]
    q, ay = x * x + y * y, np.abs(y)
    on = np.zeros((H, W), dtype=bool)
    for k in range(1, 6):
        r = f32(10.0) * f32(k)
        lo, hi = r - h, r + h
        on |= (x >= 0) & (ay <= f32(10.0 if k == 1 else 12.5)) & (lo * lo <= q) & (q <= hi * hi)
    for t, kt in BEARING:
        on |= (x >= 0) & (x <= f32(60.0)) & (np.abs(y - t * x) <= h * kt)
    assert x.dtype == f32 and y.dtype == f32 and q.dtype == f32
    return on


def render_frame(xy, colors, drawn, W, H, p, guides):
    """cmf_vis_render_bev for one frame -> (H, W, 3) uint8.  xy (n, >=2) float32; p: BevView.kernel_params()."""
    xy = np.asarray(xy, dtype=f32)
    cx, cy = (np.arange(W, dtype=f32) + f32(0.5))[None, :], (np.arange(H, dtype=f32) + f32(0.5))[:, None]
    img = np.empty((H, W, 3), dtype=np.uint8)
    img[:] = BACKGROUND
    with np.errstate(all="ignore"):
        pu, pv = (xy[:, 0] - p["x0"]) * p["inv_s"], (p["y1"] - xy[:, 1]) * p["inv_s"]
        assert pu.dtype == f32 and pv.dtype == f32
        for i in range(xy.shape[0]):                                        # in index order: a later point paints over an earlier one
            if not drawn[i]:
                continue
            dx, dy = cx - pu[i], cy - pv[i]
            cover = dx * dx + dy * dy <= p["r2"]
            assert cover.dtype == bool and (dx * dx).dtype == f32
            img[cover] = colors[i]
    if guides:
        img[guide_mask(W, H, p)] = WHITE
    return img


def render(case_frames, layer, view, frames=None):
    """The pictures of ``frames`` (default all) of a case (``build_case``'s list of per-frame dicts) -> (len, H, W, 3) uint8."""
    p = view.kernel_params()
    out = []
    for f in (range(len(case_frames)) if frames is None else frames):
        fr = case_frames[f]
        col, drawn = frame_colors(layer, fr["flow"], fr["label"], fr["mask"], fr["gt_mask"])
        out.append(render_frame(fr["pos1"], col, drawn, view.width, view.height, p, view.guides))
    return np.stack(out)


# ---- the shared case --------------------------------------------------------------------------------------------------------------------
# A float32 flow (fx, fy) whose float64 radius r satisfies r + 1e-5 == 1.0 exactly: with it as a frame's largest flow, u = fx, v = -fy
UNIT_FLOW = (float.fromhex("0x1.912a64p-12"), float.fromhex("0x1.fffeaep-1"))
COUNTS = (1, 63, 64, 65, 130, 65, 16, 64)                   # the lane-stride edges of a 64-wide wave, then the special frames
F_TRIPLE, F_ZERO, F_AXES, F_NAN = 3, 5, 6, 7               # label = 3 x prediction | all-zero flow | axis and diagonal flows | one NaN flow
# the two views of the raster test, both at 0.25 m per pixel: 64 x 32 over 16 m x 8 m, 50 x 30 over 12.5 m x 7.5 m (no tile multiple)
VIEWS = ((64, 32, (0.0, 16.0), (-4.0, 4.0)), (50, 30, (0.0, 12.5), (-3.75, 3.75)))
# positions at 0.25 m per pixel: on the tile border at pixel (16, 16) of the first view, the four canvas corners, centres half outside
# the canvas, well outside, three coincident points (COINCIDENT: their labels are made 0, 1 and 0.4 -- the last is not drawn in seg_gt and
# must not hide the second), and one exactly on a pixel centre
SPECIAL_XY = ((4.0, 0.0), (0.0, 4.0), (16.0, -4.0), (0.0, -4.0), (16.0, 4.0), (-0.125, 1.0), (8.0, 4.125), (12.5, -3.75), (16.125, 0.3),
              (-3.0, 0.0), (30.0, 9.0), (6.1, 1.3), (6.1, 1.3), (6.1, 1.3), (2.125, 2.125), (8.0, 0.0), (3.9375, 0.0625))
COINCIDENT = (11, 12, 13)
AXIS_FLOWS = ((1.0, 0.0), (1.0, -0.0), (-1.0, 0.0), (-1.0, -0.0), (0.0, 1.0), (0.0, -1.0), (-0.0, 1.0), (-0.0, -1.0), (0.0, 0.0),
              (-0.0, -0.0), (0.5, 0.5), (-0.5, 0.5), (0.5, -0.5), (-0.5, -0.5), (0.25, 0.25), (2.0, 0.0))


def _draw_frame(f, n, rng):
    r = lambda *s: rng.standard_normal(s).astype(f32)
    pos1 = np.stack([rng.uniform(-1.0, 17.0, n), rng.uniform(-5.0, 5.0, n), rng.uniform(-1.0, 1.0, n)], axis=1).astype(f32)
    k = min(n, len(SPECIAL_XY))
    if n == 1:
        pos1[0, :2] = SPECIAL_XY[0]
    elif f in (4, F_TRIPLE):
        pos1[n - k:, :2] = SPECIAL_XY[:k]                                   # last, so that they lie on top
    flow = (0.3 * r(n, 3)).astype(f32)
    label = (0.3 * r(n, 3)).astype(f32)                                     # radii on both sides of the prediction's largest
    if f == F_TRIPLE:
        label = (f32(3.0) * flow).astype(f32)
    if f == F_ZERO:
        flow[:] = 0
    if f == F_AXES:
        flow[:, :2] = AXIS_FLOWS[:n]
        label[:, :2] = np.asarray(AXIS_FLOWS[:n], dtype=f32)[::-1]
    if f == F_NAN:
        flow[n // 2, 0] = np.nan
        pos1[3, 0] = np.nan                                                 # and a NaN coordinate: covers nothing
    gt_mask = rng.choice(np.array([0.0, 1.0, 0.4], dtype=f32), n)
    mask = rng.integers(0, 2, n).astype(np.uint8)
    if n > 1 and f in (4, F_TRIPLE):
        rows = [n - k + j for j in COINCIDENT]
        gt_mask[rows] = (0.0, 1.0, 0.4)
        mask[rows] = (0, 1, 0)
    return {"pos1": pos1, "flow": flow, "label": label, "mask": mask, "gt_mask": gt_mask}


def build_case(seed=41):
    """The frames of the GPU tests: a list of dicts pos1 (n,3), flow (n,3), label (n,3) float32, mask (n) uint8 (predicted), gt_mask (n)
    float32 in {0, 1, 0.4}.  No non-integer 255 * col of any flow layer lies within 1e-9 of an integer (asserted here, on the host;
    the random part is redrawn with the next seed otherwise), so a device atan2 a few ulp from numpy's cannot change a level."""
    for attempt in range(8):
        rng = np.random.default_rng(seed + attempt)
        frames = [_draw_frame(f, n, rng) for f, n in enumerate(COUNTS)]
        margin = min(frame_margin(layer, fr["flow"], fr["label"]) for layer in ("flow", "flow_gt")
                     for f, fr in enumerate(frames) if f != F_NAN)
        if margin >= 1e-9:
            return frames
    raise AssertionError("vis_ref.build_case: no seed with a 1e-9 margin")


def as_items(frames, n2=8):
    """The case as the whole-frame 11-tuples of DeviceSplit.from_items (cloud 2 and the unused columns: zeros)."""
    items = []
    for fr in frames:
        n = fr["pos1"].shape[0]
        z = lambda *s: np.zeros(s, dtype=f32)
        items.append((fr["pos1"], z(n2, 3) + 1, z(n, 3), z(n2, 3), np.eye(4, dtype=f32), fr["label"], fr["gt_mask"], 0.1, z(n), z(n), z(n, 2)))
    return items
