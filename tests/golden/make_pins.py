#!/usr/bin/env python3
"""An INDEPENDENT, exact rasteriser for the real mh5l mesh, in Python integers — a second implementation of DESIGN.md §3's
rendering rules that shares no code and no arithmetic style with oracle/rope_oracle.c or the HIP kernels:

  * vertex shading: the float32 operations of the specification (four fused multiply-add chains, one reciprocal, the viewport
    fused multiply-adds, the snap to 1/256 pixel) evaluated EXACTLY as rationals over big integers and rounded once per operation
    to float32 by hand (round to nearest, ties to even) — no hardware float32, no libm, no double rounding;
  * coverage: per triangle, brute force over every pixel of its bounding box with the three edge functions in Python's unbounded
    integers, OpenGL's top-left rule (y up), back faces culled, pixel centres at 256 p + 128;
  * visibility: the window depth at a sample centre by exact barycentric interpolation (a Fraction), nearest wins, ties to the lower
    link id.  The oracle evaluates a float32 plane and quantises to 24 bits; the two may disagree on WHICH link wins only where two
    links' surfaces are within a few 2^-24 of each other, and those pixels are listed instead of compared.

Inputs taken from the oracle: the six float32 link matrices P·V·T of a pose (forward kinematics and the matrix product are pinned
separately by closed forms, tests/test_oracle_pins.py).  Output: tests/golden/pins_raster_160x120.npz — per pose the coverage mask,
the link-id image, the exact depth quantised to 24 bits, and the mask of near-tie pixels; and pins_bound_160x120.npz — per pose and
pixel the bound B of DESIGN.md §6 on how far a float32 depth plane may land from the exact 24-bit depth.  tests/test_oracle_pins.py holds the
oracle (CPU suite) and tests/test_golden.py the engine (GPU suite) to these.

    python tests/golden/make_pins.py [out.npz [bound.npz]]     # minutes: a million exact float32 operations per pose in pure Python
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, os.pardir, os.pardir))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from raster_ref import render_exact          # the rasteriser itself: tests/raster_ref.py, which holds it for any mesh and any matrices

POSES = [[0.4, 0.3, 0.8, 0, 0, 0], [-0.6, 1.2, -0.3, 0.5, -0.7, 1.0], [1.3, -0.8, 2.1, -1.0, 0.9, 0.2]]


def render(o, rb, q, W, H, stats=None):
    """-> link ids, exact depth in 24 bits, and the near-tie list: pixels where another link's surface lies within 8 * 2^-24 of
    the winner's.  stats: see render_exact (its 'bound' is the per-pixel B of DESIGN.md §6)."""
    ids, d24, gap = render_exact(rb.verts, rb.faces, rb.vtx_off, rb.tri_off, o.mvp(q, 6), W, H, 6, stats=stats)
    return ids, d24, gap < 8.0 / (1 << 24)


if __name__ == '__main__':
    import helpers
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=4)
    o = helpers.make_oracle(rb, intr, PV)
    out = {'poses': np.array(POSES)}
    bounds = {'poses': np.array(POSES)}                 # a file of its own: the pins themselves stay byte for byte what they were
    for k, q in enumerate(POSES):
        st = {}
        ids, d24, near = render(o, rb, q, intr.width, intr.height, st)
        out[f'ids{k}'], out[f'd24_{k}'], out[f'near{k}'] = ids, d24, near
        assert st['bound'].max() < 65536
        bounds[f'bound{k}'] = st['bound'].astype(np.uint16)
        key = o.raster_key(q, 6)
        o_ids = np.where(key == 0xFFFFFFFF, 255, key & 0xFF).astype(np.uint8)
        print(f"pose {k}: {int((ids != 255).sum())} covered pixels; coverage equal to the oracle's: {np.array_equal(ids != 255, o_ids != 255)}; "
              f"ids differ on {int((ids != o_ids).sum())} pixels ({int(((ids != o_ids) & ~near).sum())} outside the near-tie list of {int(near.sum())}); "
              f"max |d24 - oracle| = {int(np.abs(d24.astype(np.int64) - (key >> 8).astype(np.int64))[ids != 255].max())}")
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'pins_raster_160x120.npz'), **out)
    np.savez_compressed(sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'pins_bound_160x120.npz'), **bounds)
    print('written')
