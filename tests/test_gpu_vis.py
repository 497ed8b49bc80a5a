"""GPU: a test run's results as bird's-eye-view images (cmflow_amd/vis.py) -- cmf_vis_point_colors and cmf_vis_render_bev bit for bit
against their numpy restatements (tests/vis_ref.py), the colours also against the reference's own (tests/golden/vis_colors_kat.npz),
frame selection without a wait for the device, and test_split -> write_vis end to end."""
import os

import numpy as np
import pytest
import torch

import vis_ref as ref
from cmflow_amd import dataset as D
from cmflow_amd import evaluate as EV
from cmflow_amd import results as R
from cmflow_amd import synth
from cmflow_amd import vis

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _filled(frames, dev):
    """(split, store) of a list of per-frame dicts: the store filled by hand, every frame done."""
    split = D.DeviceSplit.from_items(ref.as_items(frames), dev)
    store = R.SplitResults.empty(split)
    store.flow.copy_(torch.from_numpy(np.concatenate([fr["flow"] for fr in frames])))
    store.mask.copy_(torch.from_numpy(np.concatenate([fr["mask"] for fr in frames])))
    store.done.fill_(1)
    return split, store


@pytest.fixture(scope="module")
def case(dev):
    frames = ref.build_case()                                               # asserts the 1e-9 margin on the host
    split, store = _filled(frames, dev)
    assert split.counts_host[0].tolist() == list(ref.COUNTS)
    return frames, split, store


def _views(radius, guides):
    return [vis.BevView(w, h, xr, yr, radius_px=radius, guides=guides) for w, h, xr, yr in ref.VIEWS]


@pytest.fixture(scope="module")
def full(case):
    """The device's pictures of all frames in layer seg_gt, first view, radius 3.5, guides on: computed once."""
    _, split, store = case
    view = _views(3.5, True)[0]
    return view, vis.render(store, split, "seg_gt", None, view)


# ---- 1. colours against the restatement -------------------------------------------------------------------------------------------------
def test_point_colors_are_the_restatement(case):
    frames, split, store = case
    off = split.off1.cpu().numpy()
    for layer in ref.LAYERS:
        colors, drawn = vis.point_colors(store, split, layer)
        assert colors.shape == (off[-1], 3) and colors.dtype == torch.uint8 and drawn.shape == (off[-1],) and colors.is_cuda
        colors, drawn = colors.cpu().numpy(), drawn.cpu().numpy()
        for f, fr in enumerate(frames):
            if f == ref.F_NAN and layer in ("flow", "flow_gt"):
                continue                                                    # a NaN flow: the frame only has to return
            want_c, want_d = ref.frame_colors(layer, fr["flow"], fr["label"], fr["mask"], fr["gt_mask"])
            a, b = off[f], off[f + 1]
            bad = np.argwhere(colors[a:b] != want_c)
            assert bad.size == 0, (layer, f, bad[:4].tolist(), colors[a:b][bad[:4, 0]].tolist(), want_c[bad[:4, 0]].tolist())
            assert np.array_equal(drawn[a:b], want_d), (layer, f)
    zero, _ = vis.point_colors(store, split, "flow", [ref.F_ZERO])
    zero = zero.cpu().numpy()
    assert (zero[off[ref.F_ZERO]:off[ref.F_ZERO + 1]] == 255).all()         # rad_max = 0: every point white
    assert not zero[:off[ref.F_ZERO]].any() and not zero[off[ref.F_ZERO + 1]:].any()     # rows of frames not selected stay zero


# ---- 2. golden colours ------------------------------------------------------------------------------------------------------------------
def test_point_colors_are_the_references(golden_dir, dev):
    g = np.load(os.path.join(golden_dir, "vis_colors_kat.npz"))
    u, v, want = g["u"], g["v"], g["colors"]
    n = u.size + 1
    flow, label = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    flow[0, :2] = ref.UNIT_FLOW                                             # the predicted flow's largest radius + 1e-5 is exactly 1 ...
    label[1:, 0], label[1:, 1] = u, -v                                      # ... so the label flow goes through as (u, v) itself
    assert np.array_equal(label[1:, 0].astype(np.float64), u) and np.array_equal(-label[1:, 1].astype(np.float64), v)
    fr = {"pos1": np.zeros((n, 3), f32), "flow": flow, "label": label, "mask": np.zeros(n, np.uint8), "gt_mask": np.zeros(n, f32)}
    un, vn = ref._normalised(label, flow)
    assert np.array_equal(un[1:], u) and np.array_equal(vn[1:], v) and np.array_equal(np.signbit(vn[1:]), np.signbit(v))
    split, store = _filled([fr], dev)
    colors, drawn = vis.point_colors(store, split, "flow_gt")
    got = colors.cpu().numpy()[1:]
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), u[bad[:4, 0]].tolist(), v[bad[:4, 0]].tolist(), got[bad[:4, 0]].tolist(), want[bad[:4, 0]].tolist())
    assert bool(drawn.all())


# ---- 3. raster against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.5, 1.0, 3.5])
def test_render_is_the_restatement(case, radius):
    frames, split, store = case
    sane = [f for f in range(len(frames)) if f != ref.F_NAN]
    for guides in (False, True):
        for view in _views(radius, guides):
            for layer, sel in (("seg_gt", None), ("flow_gt", sane), ("flow", sane), ("seg", None)) if guides else (("seg_gt", None), ("flow", sane)):
                got = vis.render(store, split, layer, sel, view)
                want = ref.render(frames, layer, view, sel)
                assert got.shape == want.shape and got.dtype == torch.uint8 and got.is_cuda
                got = got.cpu().numpy()
                bad = np.argwhere((got != want).any(-1))
                assert bad.size == 0, (radius, guides, view.width, layer, len(bad), bad[:6].tolist())
    # the pictures are not empty: points, both segmentation colours, background and guides all occur
    pic = got[4]
    for color in (ref.TOMATO, ref.ROYAL_BLUE, ref.BACKGROUND, ref.WHITE):
        assert (pic == np.array(color, dtype=np.uint8)).all(-1).any(), color


# ---- 4. frame selection -----------------------------------------------------------------------------------------------------------------
def test_selections_are_rows_of_the_full_render(case, full, dev):
    frames, split, store = case
    view, whole = full
    assert whole.shape == (len(frames), 32, 64, 3)
    store.metrics[:, R.METRIC_KEYS.index("epe")] = torch.tensor([3.0, 1.0, 7.0, 2.0, 9.0, 0.5, 4.0, 6.0], dtype=torch.float64, device=dev)
    vis.render(store, split, "seg_gt", [0], view)                          # warm: the library is loaded, the pinned pool exists
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        subset = vis.render(store, split, "seg_gt", [6, 1, 4], view)
        twice = vis.render(store, split, "seg_gt", torch.tensor([2, 5, 2], dtype=torch.int64), view)
        worst = store.worst("epe", 3)[1]
        ranked = vis.render(store, split, "seg_gt", worst, view)
        with pytest.raises(RuntimeError):
            split.off1.cpu()                                               # the control: a read-back IS caught in this mode
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert worst.is_cuda and worst.tolist() == [4, 2, 7]
    assert torch.equal(subset, whole[[6, 1, 4]]) and torch.equal(twice, whole[[2, 5, 2]]) and torch.equal(ranked, whole[[4, 2, 7]])
    assert vis.render(store, split, "seg_gt", [], view).shape == (0, 32, 64, 3)
    with pytest.raises(ValueError):
        vis.render(store, split, "seg_gt", torch.tensor([1, 2], dtype=torch.int32, device=dev), view)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
class EvalArgs:
    num_points, eval, mini_clip_len, update_len = 256, True, 2, 2


CLIPS = (("test", "delft_2", (90, 140, 64)), ("test", "delft_5", (200, 65, 120)))


def test_test_split_to_png_files(dev, tmp_path, manifest, golden_dir, args):
    from cmflow_amd.cmflow import CMFlow
    root = str(tmp_path / "split")
    D.write_synthetic_split(root, seed=9, clips=CLIPS)
    split = D.DeviceSplit.from_dataset(D.vodClipDataset(EvalArgs(), root, "test"), dev)
    assert len(split) == 6
    net = CMFlow(args)
    net.load_state_dict(synth.synth_state_dict(manifest, seed=1234, calib=os.path.join(golden_dir, "bn_calib_cmflow.npz")))
    _, store = EV.test_split(net.to(dev).eval(), split, 4, sort_by_size=True)
    assert store.done.tolist() == [1] * 6
    view = vis.BevView(400, 200, radius_px=2.0)
    out = str(tmp_path / "vis")
    paths = store.write_vis(out, split, view=view, chunk=4)                # two chunks per layer
    assert [os.path.relpath(p, out) for p in paths] == ["%s/%d.png" % (layer, f) for layer in ("flow", "seg_gt") for f in range(6)]
    for layer in ("flow", "seg_gt"):
        want = vis.render(store, split, layer, None, view).cpu().numpy()
        assert (want != np.array(ref.BACKGROUND, dtype=np.uint8)).any()
        for f in range(6):
            got = vis.decode_png(open(os.path.join(out, layer, "%d.png" % f), "rb").read())
            assert got.shape == (200, 400, 3) and np.array_equal(got, want[f]), (layer, f)
    # a selection: only those files, named by their global frame index
    some = store.write_vis(str(tmp_path / "some"), split, layers="seg", frames=store.worst("epe", 2)[1], view=view)
    assert sorted(os.listdir(str(tmp_path / "some" / "seg"))) == sorted(os.path.basename(p) for p in some) and len(some) == 2
    # one frame without results: ValueError, and nothing is written
    store.done[3] = 0
    with pytest.raises(ValueError):
        store.write_vis(str(tmp_path / "none"), split, view=view)
    assert not os.path.exists(str(tmp_path / "none"))
    assert len(store.write_vis(str(tmp_path / "rest"), split, layers=("flow",), frames=[0, 5], view=view)) == 2
