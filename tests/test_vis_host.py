"""CPU: the host side of cmflow_amd/vis.py -- the numpy restatement of the colour kernel (tests/vis_ref.py) against the reference's
own colours (tests/golden/vis_colors_kat.npz), the wheel and bearing tables of csrc/vis.hip against the rule and the restatement,
the PNG writer, BevView's and write_vis's refusals, and the restated rasteriser on cases small enough to count by hand."""
import os
import re

import numpy as np
import pytest
import torch

import vis_ref as ref
from cmflow_amd import dataset as D
from cmflow_amd import results as R
from cmflow_amd import vis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- colours ----------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_colours(golden_dir):
    g = np.load(os.path.join(golden_dir, "vis_colors_kat.npz"))
    u, v, want = g["u"], g["v"], g["colors"]
    assert u.dtype == np.float64 and want.dtype == np.uint8 and want.shape == (u.size, 3) and u.size >= 2048 + 32
    assert np.array_equal(u.astype(f32).astype(np.float64), u) and np.array_equal(v.astype(f32).astype(np.float64), v)
    rad = np.sqrt(u * u + v * v)
    assert (rad > 1).sum() > 500 and (rad <= 1).sum() > 500
    # the cases the fixture must hold: v = +0 and v = -0 on both half axes, u = 0, u = v = 0, the diagonals
    for su in (1, -1):
        assert ((np.sign(u) == su) & (v == 0) & ~np.signbit(v)).any() and ((np.sign(u) == su) & (v == 0) & np.signbit(v)).any()
        assert ((u == 0) & (np.sign(v) == su)).any() and ((np.abs(u) == np.abs(v)) & (np.sign(u) == su) & (v > 0)).any()
    assert ((u == 0) & (v == 0)).sum() >= 4
    assert ref.wheel_margin(u, v) >= 1e-9
    exact = ref._wheel_cols(u, v) % 1 == 0
    assert 0.3 < exact.mean() < 0.4                                        # saturated channels and col == 1: they must come out exact
    assert np.array_equal(ref.wheel_colors(u, v), want)


def _table(name):
    text = open(os.path.join(REPO, "cmflow_amd", "csrc", "vis.hip")).read()
    body = re.search(r"\b%s\[[^=]*=\s*\{(.*?)\};" % name, text, flags=re.S).group(1)
    return [[float(x.rstrip("fu")) for x in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", body)]


def test_tables_of_the_kernel_file():
    wheel = ref.wheel_from_rule()
    assert wheel.shape == (55, 3) and np.array_equal(wheel, ref.WHEEL)
    assert np.array_equal(np.array(_table("WHEEL")), wheel)
    bearing = np.array(_table("BEARING")).astype(f32)
    assert np.array_equal(bearing, ref.BEARING)
    t = np.tan(np.radians([0, 5, -5, 10, -10, 15, -15]))
    assert np.array_equal(bearing[:, 0], t.astype(f32)) and np.array_equal(bearing[:, 1], np.sqrt(1 + bearing[:, 0].astype(np.float64) ** 2).astype(f32))


def test_shared_case_has_its_margin():
    frames = ref.build_case()
    assert [fr["pos1"].shape[0] for fr in frames] == list(ref.COUNTS)
    lab, flo = frames[ref.F_TRIPLE]["label"], frames[ref.F_TRIPLE]["flow"]
    u, v = ref._normalised(lab, flo)
    assert (np.sqrt(u * u + v * v) > 1).any()                              # the rad > 1 branch occurs in flow_gt
    assert np.isnan(frames[ref.F_NAN]["flow"]).sum() == 1 and not frames[ref.F_ZERO]["flow"].any()
    fx, fy = (np.float64(f32(c)) for c in ref.UNIT_FLOW)
    assert f32(fx) == fx and np.sqrt(fx * fx + fy * fy) + 1e-5 == 1.0


# ---- PNG --------------------------------------------------------------------------------------------------------------------------------
def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 3), (7, 5, 3), (30, 50, 3)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        data = vis.encode_png(img)
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data.count(b"IDAT") == 1
        assert np.array_equal(vis.decode_png(data), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        path = str(tmp_path / "a.png")
        open(path, "wb").write(data)
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)
    with pytest.raises(ValueError):
        vis.encode_png(img[:, :, 0])
    with pytest.raises(ValueError):
        vis.encode_png(img.astype(np.float32))
    with pytest.raises(ValueError):
        vis.decode_png(b"not a png")
    broken = bytearray(data)
    broken[40] ^= 1
    with pytest.raises(ValueError):
        vis.decode_png(bytes(broken))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bev_view_refusals():
    v = vis.BevView()
    assert (v.width, v.height, v.x_range, v.y_range, v.radius_px, v.guides) == (1200, 600, (0.0, 60.0), (-15.0, 15.0), 3.5, True)
    p = v.kernel_params()
    assert all(isinstance(x, np.float32) for x in p.values())
    assert p["s"] == f32(0.05) and p["inv_s"] == f32(20.0) and p["half"] == f32(0.025) and p["r2"] == f32(12.25) and p["y1"] == f32(15.0)
    for w, h, xr, yr in ref.VIEWS:
        assert vis.BevView(w, h, xr, yr).scale == 0.25
    for bad in (dict(width=1200, height=500), dict(x_range=(5.0, 5.0)), dict(y_range=(3.0, -3.0)), dict(radius_px=0.0), dict(radius_px=-1.0),
                dict(width=4112, height=2056), dict(width=0), dict(width=8192, height=4096), dict(radius_px=float("nan"))):
        with pytest.raises(ValueError):
            vis.BevView(**bad)


def test_cpu_tensors_and_foreign_stores_are_refused(tmp_path):
    frames = ref.build_case()
    split = D.DeviceSplit.from_items(ref.as_items(frames), "cpu")
    other = D.DeviceSplit.from_items(ref.as_items(frames[:-1]), "cpu")
    store = R.SplitResults.empty(split)
    store.done.fill_(1)
    out = str(tmp_path / "vis")
    with pytest.raises(ValueError):
        store.write_vis(out, other)                                        # not this split's store
    with pytest.raises(ValueError):
        store.write_vis(out, split, layers=("flow", "depth"))              # unknown layer
    with pytest.raises(ValueError):
        vis.render(store, split, "error")
    with pytest.raises(ValueError):
        vis.point_colors(store, other, "flow")
    for call in (lambda: store.write_vis(out, split), lambda: vis.render(store, split, "flow"), lambda: vis.point_colors(store, split, "seg")):
        with pytest.raises(RuntimeError):
            call()                                                         # CPU tensors: no fallback
    assert not os.path.exists(out)


# ---- the restated rasteriser, by hand ---------------------------------------------------------------------------------------------------
def _view(radius, guides=False):
    return vis.BevView(64, 32, (0.0, 16.0), (-4.0, 4.0), radius_px=radius, guides=guides)


def _centre(c, r):
    """The position in metres of the centre of pixel (row r, col c) of ``_view``."""
    return ((c + 0.5) * 0.25, 4.0 - (r + 0.5) * 0.25)


RED, GREEN = (200, 10, 10), (10, 200, 10)


def _paint(view, xy, colors, drawn=None):
    xy = np.asarray(xy, dtype=f32).reshape(-1, 2)
    drawn = np.ones(len(xy), dtype=np.uint8) if drawn is None else np.asarray(drawn, dtype=np.uint8)
    return ref.render_frame(xy, np.asarray(colors, dtype=np.uint8).reshape(-1, 3), drawn, view.width, view.height, view.kernel_params(), view.guides)


def _count(img, color):
    return int((img == np.array(color, dtype=np.uint8)).all(-1).sum())


def test_one_disc_covers_1_5_and_37_pixels():
    for radius, want in ((0.5, 1), (1.0, 5), (3.5, 37)):
        img = _paint(_view(radius), [_centre(20, 10)], [RED])
        assert _count(img, RED) == want and _count(img, ref.BACKGROUND) == 64 * 32 - want, radius
        assert tuple(img[10, 20]) == RED
    # a sub-pixel disc between four centres covers none of them
    x, y = _centre(20, 10)
    assert _count(_paint(_view(0.5), [(x + 0.125, y - 0.125)], [RED]), RED) == 0
    # clipped at the canvas corner: a quarter of the 37-pixel disc (the centre pixel's quadrant, 3 + 3 + 2 + 1 and the axes)
    img = _paint(_view(3.5), [_centre(0, 0)], [RED])
    assert _count(img, RED) == 13 and tuple(img[0, 0]) == RED
    # outside the view and NaN: nothing
    assert _count(_paint(_view(3.5), [(-3.0, 0.0), (float("nan"), 0.0), (1.0, float("nan"))], [RED] * 3), ref.BACKGROUND) == 64 * 32


def test_the_higher_index_wins_and_an_undrawn_point_hides_nothing():
    p = _centre(30, 16)
    assert _count(_paint(_view(1.0), [p, p], [RED, GREEN]), GREEN) == 5
    assert _count(_paint(_view(1.0), [p, p], [GREEN, RED]), GREEN) == 0
    # a seg_gt point with mask 0.4 is not drawn: the lower-indexed point under it stays
    col, drawn = ref.frame_colors("seg_gt", np.zeros((3, 3), f32), np.zeros((3, 3), f32), np.zeros(3, np.uint8), np.array([0.0, 0.4, 1.0], f32))
    assert drawn.tolist() == [1, 0, 1] and col.tolist() == [list(ref.TOMATO), [0, 0, 0], list(ref.ROYAL_BLUE)]
    img = _paint(_view(1.0), [p, p, _centre(5, 5)], col, drawn)
    assert _count(img, ref.TOMATO) == 5 and _count(img, ref.ROYAL_BLUE) == 5 and _count(img, (0, 0, 0)) == 0


def test_guides_lie_over_points():
    view = _view(3.5, guides=True)
    on = ref.guide_mask(64, 32, view.kernel_params())
    assert on[15, :].all() or on[16, :].all() or (on[15, :] | on[16, :]).all()          # the 0 degree line runs along y = 0
    ring = (39, 16)                                                         # x = 9.875 m, y = -0.125 m: on the 10 m ring
    assert on[ring[1], ring[0]] and not on[2, 2]
    img = _paint(view, [_centre(*ring)], [RED])
    assert tuple(img[ring[1], ring[0]]) == ref.WHITE and 0 < _count(img, RED) < 37
    assert np.array_equal((img == 255).all(-1), on)
    plain = _paint(_view(3.5), [_centre(*ring)], [RED])
    assert _count(plain, RED) == 37 and np.array_equal(img[~on], plain[~on])
