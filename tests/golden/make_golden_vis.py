#!/usr/bin/env python3
"""Golden vectors for the flow colour wheel, produced by the REFERENCE's own utils/vis_ops.py (flow_xy_to_colors :54-91 with
make_colorwheel :3-50) on float64 inputs -- the reference's `--vis` branch takes the angle in float32 and the rest in float64;
cmf_vis_point_colors takes everything in float64, and on float64 inputs the two agree exactly.
Build container only.

    python tests/golden/make_golden_vis.py      ->  tests/golden/vis_colors_kat.npz   (u, v float64; colors uint8)

The inputs are float32-representable (the GPU test pushes them through a float32 store whose normaliser is exactly 1):
2048 random flows with radii on both sides of 1; the axis cases v = +0.0, v = -0.0, u = 0, u = v = 0, where atan2's signed-zero rules
and the wrap k1 == 55 -> 0 decide; the exact diagonals.  No non-integer 255 * col lies within 1e-9 of an integer (asserted on the
float64 restatement of tests/vis_ref.py; the random part is redrawn with the next seed otherwise).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_shims  # noqa: E402
import vis_ref  # noqa: E402


def inputs(seed):
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(-np.pi, np.pi, 2048), rng.uniform(0.0, 2.0, 2048)
    u, v = [rad * np.cos(ang)], [rad * np.sin(ang)]
    z = 0.0
    # magnitudes that are no multiples of a power of two: on an axis 255 * col = 255 - m * (255 - w) is then no integer in exact
    # arithmetic either (at m = 0.25 it is 202 for w = 43, and the float64 result is one ulp off that integer)
    for m in (0.3, 0.7, 0.9, 1.3, 1.7):
        u += [[m, m, -m, -m, z, z, -z, -z]]                                 # v = +-0 on both half axes, u = +-0 on both
        v += [[z, -z, z, -z, m, -m, m, -m]]
        u += [[m, -m, m, -m]]                                               # the exact diagonals
        v += [[m, m, -m, -m]]
    u += [[z, z, -z, -z]]                                                   # u = v = 0 with every pair of signs
    v += [[z, -z, z, -z]]
    f = lambda parts: np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]).astype(np.float32).astype(np.float64)
    u, v = f(u), f(v)
    # beyond rad = 1 the colour is 0.75 * col whatever the magnitude: on the half axis u = 0, v < 0 (fk = 40.5) the red channel is
    # 0.75 * 88 = 66 and on the diagonal u = -v > 0 (fk = 47.25) it is 0.75 * 220 = 165 in exact arithmetic, integers the float64
    # operations miss by an ulp -- these two directions stay inside rad <= 1
    rad = np.sqrt(u * u + v * v)
    keep = ~((rad > 1) & (((u == 0) & (v < 0)) | ((u == -v) & (u > 0))))
    return u[keep], v[keep]


def main():
    install_shims()
    from utils import vis_ops                                # the reference
    for seed in range(7, 64):
        u, v = inputs(seed)
        if vis_ref.wheel_margin(u, v) >= 1e-9:
            break
    else:
        raise SystemExit("no seed with a 1e-9 margin")
    colors = vis_ops.flow_xy_to_colors(u, v)
    assert colors.dtype == np.uint8 and colors.shape == (u.size, 3)
    rad = np.sqrt(u * u + v * v)
    print("seed %d: %d flows, %d with rad > 1, margin %.3g, %d of %d values are exact integers" % (
        seed, u.size, int((rad > 1).sum()), vis_ref.wheel_margin(u, v), int((vis_ref._wheel_cols(u, v) % 1 == 0).sum()), 3 * u.size))
    print("restatement equals the reference:", bool(np.array_equal(vis_ref.wheel_colors(u, v), colors)))
    np.savez_compressed(os.path.join(HERE, "vis_colors_kat.npz"), u=u, v=v, colors=colors)


if __name__ == "__main__":
    main()
