"""A test run's results as bird's-eye-view images, rendered on the device -- the reference's ``--vis`` branch (main_util.py:170-172:
utils/vis_util.py ``visulize_result_2D_pre`` and ``visulize_result_2D_seg_pre``) without its three ``.cpu()`` copies and two
matplotlib figures per frame.

A ``results.SplitResults`` store holds what a picture needs, packed like the split.  ``render`` turns any selection of its frames
into ``(frames, H, W, 3)`` uint8 images with two launches and no wait for the device: ``cmf_vis_point_colors`` (one RGB triple per
point: the Middlebury flow wheel of utils/vis_ops.py in float64, or the two segmentation colours) and ``cmf_vis_render_bev`` (hard
discs painted in index order, the range rings and bearing lines over them; float32, ``+ - *`` and compares only).  Both are
definitions, stated in include/cmflow_hip.h and DESIGN.md section 20 and restated in numpy, bit for bit, by tests/vis_ref.py.
``SplitResults.write_vis`` writes the pictures as PNG files where the reference puts them; ``encode_png`` needs the stdlib only.

What differs from matplotlib: no antialiasing (a pixel is covered or not), no text (the reference's "10" .. "50" labels along the
rings are not drawn -- there is no font here), hard discs of ``radius_px`` instead of markers of ``s=6`` points^2, and the angle of
the flow wheel taken in float64 where the reference takes it in float32 (one colour level on about 1e-4 of the values).
"""
import struct
import zlib

import numpy as np
import torch

from . import _frames, _lib

LAYERS = ("flow", "flow_gt", "seg", "seg_gt")               # CMF_VIS_FLOW .. CMF_VIS_SEG_GT of include/cmflow_hip.h
MAX_SIDE = 4096                                             # CMF_VIS_MAX_SIDE
MAX_FRAMES = 65535                                          # frames of one render call: the launch grid's z extent


class BevView:
    """The canvas of a picture: ``width`` x ``height`` pixels over ``x_range`` x ``y_range`` metres (x to the right, y up: row 0 is
    the largest y), discs of ``radius_px`` pixels, ``guides``: the range rings and bearing lines.  The defaults are the reference's
    limits and aspect (vis_util.py:86-88: x 0 .. 60, y -15 .. 15, box aspect 0.5); 3.5 pixels is about its ``s=6`` marker at dpi 200.
    Pixels must be square.  ValueError for non-square pixels, an empty range, ``radius_px <= 0`` or a side above 4096."""

    def __init__(self, width=1200, height=600, x_range=(0.0, 60.0), y_range=(-15.0, 15.0), radius_px=3.5, guides=True):
        self.width, self.height = int(width), int(height)
        self.x_range, self.y_range = (float(x_range[0]), float(x_range[1])), (float(y_range[0]), float(y_range[1]))
        self.radius_px, self.guides = float(radius_px), bool(guides)
        if not (1 <= self.width <= MAX_SIDE and 1 <= self.height <= MAX_SIDE) or self.width != width or self.height != height:
            raise ValueError("BevView: a canvas of %r x %r pixels (whole numbers from 1 to %d a side)" % (width, height, MAX_SIDE))
        if not (self.x_range[1] > self.x_range[0] and self.y_range[1] > self.y_range[0]):
            raise ValueError("BevView: empty range x %r, y %r" % (x_range, y_range))
        if not (0.0 < self.radius_px <= MAX_SIDE):
            raise ValueError("BevView: radius_px = %r" % (radius_px,))
        sx, sy = (self.x_range[1] - self.x_range[0]) / self.width, (self.y_range[1] - self.y_range[0]) / self.height
        if not (abs(sx - sy) <= 1e-9 * sx and np.isfinite(sx)):
            raise ValueError("BevView: pixels are not square (%.9g m wide, %.9g m high)" % (sx, sy))
        self.scale = sx                                                      # metres per pixel

    def kernel_params(self):
        """The float32 numbers ``cmf_vis_render_bev`` gets, formed here in float64 and rounded once each: x0, y1 (the canvas's top
        left corner in metres), s (metres per pixel), inv_s = 1/s, half = s/2, radius, r2 = radius^2."""
        f = np.float32
        return {"x0": f(self.x_range[0]), "y1": f(self.y_range[1]), "s": f(self.scale), "inv_s": f(1.0 / self.scale),
                "half": f(self.scale / 2.0), "radius": f(self.radius_px), "r2": f(self.radius_px * self.radius_px)}


def _layer_id(layer, what):
    if layer not in LAYERS:
        raise ValueError("%s: layer %r is not one of %s" % (what, layer, ", ".join(LAYERS)))
    return LAYERS.index(layer)


def check_store(store, split, what):
    """ValueError unless ``store`` is a store of ``split`` (the two comparisons of ``SplitResults.write_json``); RuntimeError unless
    both are on one GPU."""
    _frames.belongs(split, store, what)
    if not (store.flow.is_cuda and split.tab1.is_cuda and store.flow.device == split.tab1.device):
        raise RuntimeError("%s: store on %s, split on %s; pictures are rendered on the GPU only (no CPU fallback)"
                           % (what, store.flow.device, split.tab1.device))


def _selection(store, frames, what):
    """-> (int64 device tensor or None for all frames, how many).  A list or a CPU tensor goes to the device through pinned memory
    (no wait); a device tensor is taken as it is."""
    if frames is None:
        return None, len(store)
    if not torch.is_tensor(frames):
        frames = torch.tensor([int(f) for f in frames], dtype=torch.int64)
    _frames.check_frames_tensor(frames, what)
    if not frames.is_cuda:
        frames = _frames.pinned(frames, store.device)
    elif frames.device != store.device:
        raise RuntimeError("%s: frames on %s, the store on %s" % (what, frames.device, store.device))
    return frames.contiguous(), int(frames.numel())


def _launch_colors(store, split, layer_id, sel, nsel, colors, drawn):
    u8 = torch.uint8
    with torch.cuda.device(store.device):
        _lib.check(_lib.lib().cmf_vis_point_colors(
            nsel, len(store), None if sel is None else _lib.dev_ptr(sel, torch.int64), _lib.dev_ptr(store.off1, torch.int32),
            store.flow.shape[0], layer_id, _lib.dev_ptr(store.flow, torch.float32), _lib.dev_ptr(split.tab1, torch.float32),
            split.tab1.shape[1], _lib.dev_ptr(store.mask, u8), _lib.dev_ptr(colors, u8), _lib.dev_ptr(drawn, u8), _lib.stream_ptr()),
            "cmf_vis_point_colors")


def point_colors(store, split, layer, frames=None):
    """The colour of every point of the selected frames in ``layer`` (one of ``LAYERS``): ``flow`` / ``flow_gt`` the predicted / the
    label flow on the Middlebury wheel, both normalised by the predicted flow's largest radius in the frame (vis_util.py:32-42,63);
    ``seg`` / ``seg_gt`` tomato for a moving and royal blue for a static point of the predicted mask / the split's mask column
    (vis_util.py:139-140), where a label that is neither 0 nor 1 is not drawn.
    -> (colors (sum n1, 3) uint8, drawn (sum n1) uint8) on the device, packed like the store: a selected frame's rows hold its
    points' colours, every other row is zero.  ``frames``: None (all), a list, or an int64 tensor -- a device tensor such as
    ``store.worst("epe", 50)[1]`` is used without a read-back.  The two zero fills and one launch; the host does not wait."""
    layer_id = _layer_id(layer, "vis.point_colors")
    check_store(store, split, "vis.point_colors")
    sel, nsel = _selection(store, frames, "vis.point_colors")
    total = store.flow.shape[0]
    colors = torch.zeros((total, 3), dtype=torch.uint8, device=store.device)
    drawn = torch.zeros((total,), dtype=torch.uint8, device=store.device)
    _launch_colors(store, split, layer_id, sel, nsel, colors, drawn)
    return colors, drawn


def render(store, split, layer, frames=None, view=None):
    """Bird's-eye-view pictures of the selected frames -> (len(frames), H, W, 3) uint8 on the device.  Arguments as ``point_colors``;
    ``view``: a ``BevView`` (default: the reference's 60 m x 30 m at 1200 x 600).  A pixel has the colour of the highest-indexed drawn
    point whose disc covers its centre, else the background (80, 80, 80); the guides lie over the points (DESIGN.md section 20 has
    the definition).  The reference's text labels ("10" .. "50") are not drawn: there is no font here.
    Two launches -- ``cmf_vis_point_colors``, ``cmf_vis_render_bev`` -- are the only device work, and the host never waits."""
    layer_id = _layer_id(layer, "vis.render")
    check_store(store, split, "vis.render")
    view = BevView() if view is None else view
    sel, nsel = _selection(store, frames, "vis.render")
    if nsel > MAX_FRAMES:
        raise ValueError("vis.render: %d frames in one call (at most %d: render in chunks, as write_vis does)" % (nsel, MAX_FRAMES))
    total, u8 = store.flow.shape[0], torch.uint8
    out = torch.empty((nsel, view.height, view.width, 3), dtype=u8, device=store.device)
    if nsel == 0:
        return out
    colors = torch.empty((total, 3), dtype=u8, device=store.device)        # only the selected frames' rows are written -- and read
    drawn = torch.empty((total,), dtype=u8, device=store.device)
    _launch_colors(store, split, layer_id, sel, nsel, colors, drawn)
    p = {k: float(v) for k, v in view.kernel_params().items()}              # exact: every float32 is a double
    with torch.cuda.device(store.device):
        _lib.check(_lib.lib().cmf_vis_render_bev(
            nsel, len(store), None if sel is None else _lib.dev_ptr(sel, torch.int64), _lib.dev_ptr(store.off1, torch.int32), total,
            _lib.dev_ptr(split.tab1, torch.float32), split.tab1.shape[1], _lib.dev_ptr(colors, u8), _lib.dev_ptr(drawn, u8),
            view.width, view.height, p["x0"], p["y1"], p["s"], p["inv_s"], p["half"], p["radius"], p["r2"], int(view.guides),
            _lib.dev_ptr(out, u8), _lib.stream_ptr()), "cmf_vis_render_bev")
    return out


AGE_LAYER = "age"                                           # render_accumulated only: royal blue fading into the background with age
_ROYAL_BLUE, _BACKGROUND = (65, 105, 225), (80, 80, 80)


def age_colors(age, window):
    """The colours of the ``'age'`` layer, (n, 3) uint8 from ages (n) uint8 on any device: channel c of a point of age g is
    (blue_c * (window - g) + background_c * g) // window in whole numbers -- royal blue (65, 105, 225) for the current scan, one
    step short of the background (80, 80, 80) for the oldest age a full window has.  Ages from ``window`` on give the background."""
    window = int(window)
    g = age.to(torch.int32).clamp(max=window)
    channels = [torch.div(blue * (window - g) + back * g, window, rounding_mode="floor") for blue, back in zip(_ROYAL_BLUE, _BACKGROUND)]
    return torch.stack(channels, dim=1).to(torch.uint8)


def render_accumulated(acc, store, split, layer, view=None):
    """Bird's-eye-view pictures of accumulated clouds (``accumulate.accumulate``) -> (len(acc), H, W, 3) uint8 on the device, one
    picture per target frame.  ``layer``: one of ``LAYERS`` -- every point keeps the colour ``point_colors(store, split, layer)``
    gives it in its own source frame (the flow wheel is normalised per source frame), gathered by ``acc.src`` -- or ``'age'``
    (``age_colors``; ``store`` is not read and may be None).  A row behind a target's count (``src < 0``) is not drawn.  Rows run
    oldest first, so the newest scan is painted on top.  ``view`` as ``render``.  The colour launch, a few gathers and ONE call of the
    rasteriser ``render`` uses (``cmf_vis_render_bev`` over ``acc.off`` / ``acc.xyz``); the host never waits."""
    if layer != AGE_LAYER:
        _layer_id(layer, "vis.render_accumulated")
        check_store(store, split, "vis.render_accumulated")
    if not (acc.xyz.is_cuda and acc.xyz.device == split.tab1.device):
        raise RuntimeError("vis.render_accumulated: clouds on %s, split on %s; pictures are rendered on the GPU only" % (acc.xyz.device, split.tab1.device))
    view = BevView() if view is None else view
    nsel, R, u8 = len(acc), acc.xyz.shape[0], torch.uint8
    if nsel > MAX_FRAMES:
        raise ValueError("vis.render_accumulated: %d targets in one call (at most %d)" % (nsel, MAX_FRAMES))
    out = torch.empty((nsel, view.height, view.width, 3), dtype=u8, device=acc.device)
    if nsel == 0:
        return out
    held = acc.src >= 0
    if layer == AGE_LAYER:
        colors, drawn = age_colors(acc.age, acc.window), held.to(u8)
    else:
        all_colors, all_drawn = point_colors(store, split, layer)
        row = acc.src.clamp(min=0).long()
        colors, drawn = all_colors[row], all_drawn[row] * held.to(u8)
    colors, drawn = colors.contiguous(), drawn.contiguous()
    p = {k: float(v) for k, v in view.kernel_params().items()}
    with torch.cuda.device(acc.device):
        _lib.check(_lib.lib().cmf_vis_render_bev(
            nsel, nsel, None, _lib.dev_ptr(acc.off, torch.int32), R, _lib.dev_ptr(acc.xyz, torch.float32), 3,
            _lib.dev_ptr(colors, u8), _lib.dev_ptr(drawn, u8), view.width, view.height,
            p["x0"], p["y1"], p["s"], p["inv_s"], p["half"], p["radius"], p["r2"], int(view.guides),
            _lib.dev_ptr(out, u8), _lib.stream_ptr()), "cmf_vis_render_bev")
    return out


# the instances of ``instances.cluster``: twelve colours by label % 12, light grey for noise, dim grey for a point that is no candidate
INSTANCE_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
                    (70, 240, 240), (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (170, 110, 40))
INSTANCE_NOISE, INSTANCE_STATIC = (200, 200, 200), (120, 120, 120)


def instance_colors(label, kind):
    """The colours of ``render_instances``, (n, 3) uint8 from ``label`` (n) int32 and ``kind`` (n) uint8 on any device, in whole
    numbers: a core or border point (kind >= 2) gets entry ``label % 12`` of ``INSTANCE_PALETTE``, a noise point (kind 1) light grey
    (200, 200, 200), every other point dim grey (120, 120, 120)."""
    slot = torch.remainder(label.to(torch.int32), len(INSTANCE_PALETTE))
    member, noise = kind >= 2, kind == 1
    channels = []
    for ch in range(3):
        col = torch.full_like(slot, INSTANCE_STATIC[ch])
        col = torch.where(noise, torch.full_like(slot, INSTANCE_NOISE[ch]), col)
        for k, rgb in enumerate(INSTANCE_PALETTE):
            col = torch.where(member & (slot == k), torch.full_like(slot, rgb[ch]), col)
        channels.append(col)
    return torch.stack(channels, dim=1).to(torch.uint8)


def render_instances(inst, split, frames=None, view=None):
    """Bird's-eye-view pictures of clustered frames (``instances.cluster``) -> (frames, H, W, 3) uint8 on the device.  ``frames``:
    None (the frames ``inst`` was computed for), a list, or an int64 tensor; a frame ``inst`` does not hold is drawn dim grey.  Every
    point of a selected frame is drawn in its ``instance_colors``, in index order.  ``view`` as ``render``.  A few whole-number torch
    ops and ONE call of the rasteriser ``render`` uses (``cmf_vis_render_bev``); the host never waits."""
    return _render_labelled(inst.label, inst, split, frames, view, "vis.render_instances")


def render_tracks(tracks, inst, split, frames=None, view=None):
    """Bird's-eye-view pictures of tracked frames (``tracks.track``) -> (frames, H, W, 3) uint8 on the device: ``render_instances``
    with every member point coloured by its TRACK -- ``instance_colors(tracks.point_track, inst.kind)``, entry ``track % 12`` of the
    palette -- so an object keeps its colour from frame to frame inside a clip (track ids restart with every clip).  ``inst``: the
    instances ``tracks`` was formed from.  ``frames`` and ``view`` as there; the same ONE call of the rasteriser, the host never waits."""
    if tracks.point_track.shape != inst.label.shape or tracks.point_track.device != inst.label.device:
        raise ValueError("vis.render_tracks: the tracks are not the ones of these instances")
    return _render_labelled(tracks.point_track, inst, split, frames, view, "vis.render_tracks")


def _render_labelled(label, inst, split, frames, view, what):
    if len(split) != inst.off.numel() - 1 or split.tab1.shape[0] != inst.label.shape[0]:
        raise ValueError("%s: the split is not the one these instances belong to" % what)
    if not (inst.label.is_cuda and split.tab1.is_cuda and inst.label.device == split.tab1.device):
        raise RuntimeError("%s: instances on %s, split on %s; pictures are rendered on the GPU only (no CPU fallback)"
                           % (what, inst.label.device, split.tab1.device))
    view = BevView() if view is None else view
    if frames is None:
        sel, nsel = (None, len(split)) if inst.frames_host.size == len(split) and bool((inst.frames_host == np.arange(len(split))).all()) \
            else (inst.frames, len(inst))
    else:
        sel, nsel = _selection(split, frames, what)
    if nsel > MAX_FRAMES:
        raise ValueError("%s: %d frames in one call (at most %d)" % (what, nsel, MAX_FRAMES))
    total, u8 = inst.label.shape[0], torch.uint8
    out = torch.empty((nsel, view.height, view.width, 3), dtype=u8, device=inst.device)
    if nsel == 0:
        return out
    colors = instance_colors(label, inst.kind).contiguous()
    drawn = torch.ones((total,), dtype=u8, device=inst.device)
    p = {k: float(v) for k, v in view.kernel_params().items()}
    with torch.cuda.device(inst.device):
        _lib.check(_lib.lib().cmf_vis_render_bev(
            nsel, len(split), None if sel is None else _lib.dev_ptr(sel, torch.int64), _lib.dev_ptr(split.off1, torch.int32), total,
            _lib.dev_ptr(split.tab1, torch.float32), split.tab1.shape[1], _lib.dev_ptr(colors, u8), _lib.dev_ptr(drawn, u8),
            view.width, view.height, p["x0"], p["y1"], p["s"], p["inv_s"], p["half"], p["radius"], p["r2"], int(view.guides),
            _lib.dev_ptr(out, u8), _lib.stream_ptr()), "cmf_vis_render_bev")
    return out


# ---- PNG, with the stdlib only ----------------------------------------------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(image):
    """An (H, W, 3) uint8 numpy array as the bytes of a PNG file: 8-bit RGB, every row with filter type 0, one IDAT chunk.
    Only ``zlib`` and ``struct`` are used."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("encode_png: an (H, W, 3) uint8 array, not %s of shape %s" % (image.dtype, image.shape))
    h, w = image.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)                        # column 0: the filter type of the row, 0 = none
    rows[:, 1:] = image.reshape(h, 3 * w)
    return _PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) \
        + _chunk(b"IDAT", zlib.compress(rows.tobytes())) + _chunk(b"IEND", b"")


def decode_png(data):
    """The (H, W, 3) uint8 array of a PNG file as ``encode_png`` writes them: 8-bit RGB, not interlaced, filter type 0 in every row
    (any number of IDAT chunks).  Anything else, or a chunk whose CRC does not match, raises ValueError."""
    if data[:8] != _PNG_MAGIC:
        raise ValueError("decode_png: not a PNG file")
    at, header, body = 8, None, []
    while at < len(data):
        (n,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        payload = data[at + 8:at + 8 + n]
        if len(payload) != n or struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(kind + payload) & 0xFFFFFFFF):
            raise ValueError("decode_png: chunk %r is damaged" % kind)
        at += 12 + n
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", payload)
        elif kind == b"IDAT":
            body.append(payload)
        elif kind == b"IEND":
            break
    if header is None or header[2:] != (8, 2, 0, 0, 0):
        raise ValueError("decode_png: only 8-bit RGB without interlace is read (IHDR %r)" % (header,))
    w, h = header[:2]
    raw = np.frombuffer(zlib.decompress(b"".join(body)), dtype=np.uint8)
    if raw.size != h * (1 + 3 * w):
        raise ValueError("decode_png: %d bytes of image data for %d x %d pixels" % (raw.size, w, h))
    rows = raw.reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError("decode_png: only rows of filter type 0 are read")
    return rows[:, 1:].reshape(h, w, 3).copy()
