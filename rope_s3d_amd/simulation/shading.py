"""What turns a render into a photograph: the per-frame records rope_shade_frames takes (csrc/rope_shade.hip: light, surface
colours, white balance, sensor noise, background) and the procedural backgrounds it composes over.  Everything is drawn from seeds
on the host; the pixels are made on the GPU (Engine.shade_frames, Renderer.render_photo_batch_device).  The reference has no such
stage: its synthetic pictures are the flat link colours, its 'real' mode pyrender's shader.  The ranges are constants.py's."""
import numpy as np

from ..constants import (SHADE_ALBEDO, SHADE_ALBEDO_JITTER, SHADE_AMBIENT, SHADE_AMBIENT_RANGE, SHADE_BG_DEPTH_RANGE, SHADE_GAIN_RANGE,
                         SHADE_LIGHT_CONE_DEG, SHADE_NOISE_Q_RANGE, SHADE_PALETTE)
from ..engine import SHADE_DTYPE

ShadeParams = SHADE_DTYPE             # one record per frame: rope_shade_params of include/rope_s3d.h
_STREAM = 0x5AADE                     # second word of the generators' seeds: apart from the poses' default_rng(seed + frame)


def unit_light(direction) -> np.ndarray:
    """A direction the light travels in (camera axes: x right, y down, z forward), normalised in float64 and then rounded to the
    float32 the kernel takes as it is."""
    d = np.asarray(direction, np.float64).reshape(3)
    return (d / np.linalg.norm(d)).astype(np.float32)


def default_params(n: int, n_links: int = 6) -> np.ndarray:
    """n records of shade_depth's scene: head-on light, ambient 0.12, every link 200 grey, gain 1, no noise, flat black background,
    no background depth."""
    p = np.zeros(int(n), ShadeParams)
    p['light'] = unit_light([0, 0, 1])
    p['ambient'] = SHADE_AMBIENT
    p['gain'] = 1.0
    p['albedo'][:, :n_links] = SHADE_ALBEDO
    p['bg_index'] = -1
    return p


def draw_params(seed: int, frame_indices, n_links: int = 6, n_bg: int = 0) -> np.ndarray:
    """One record per frame index, frame f from default_rng((seed, 0x5AADE, f)) alone, so a frame's record does not depend on which
    other frames are asked for: a light within SHADE_LIGHT_CONE_DEG of the view axis (uniform in solid angle), an ambient level, per
    link a palette colour jittered per channel, a gain per channel, noise_q, a background picture (n_bg > 0) or a flat colour, and
    a background depth behind the robot."""
    frames = np.asarray(frame_indices, np.int64).reshape(-1)
    p = np.zeros(len(frames), ShadeParams)
    palette = np.asarray(SHADE_PALETTE, np.int64)
    cos_min = np.cos(np.radians(SHADE_LIGHT_CONE_DEG))
    for k, f in enumerate(frames):
        rng = np.random.default_rng((int(seed), _STREAM, int(f)))
        c, phi = rng.uniform(cos_min, 1.0), rng.uniform(0.0, 2 * np.pi)
        s = np.sqrt(1.0 - c * c)
        p['light'][k] = unit_light([s * np.cos(phi), s * np.sin(phi), c])
        p['ambient'][k] = rng.uniform(*SHADE_AMBIENT_RANGE)
        base = palette[rng.integers(0, len(palette), n_links)]
        jitter = rng.integers(-SHADE_ALBEDO_JITTER, SHADE_ALBEDO_JITTER + 1, (n_links, 3))
        p['albedo'][k, :n_links] = np.clip(base + jitter, 0, 255)
        p['gain'][k] = rng.uniform(*SHADE_GAIN_RANGE, 3)
        p['noise_q'][k] = rng.integers(SHADE_NOISE_Q_RANGE[0], SHADE_NOISE_Q_RANGE[1] + 1)
        p['bg_index'][k] = rng.integers(0, n_bg) if n_bg > 0 else -1
        p['bg_colour'][k] = rng.integers(20, 236, 3)
        p['bg_depth'][k] = rng.uniform(*SHADE_BG_DEPTH_RANGE)
    return p


def _value_noise(rng, H: int, W: int, cell: int) -> np.ndarray:
    """(H, W) float64 in [0, 1]: a coarse random lattice, bilinearly interpolated."""
    gh, gw = H // cell + 2, W // cell + 2
    lat = rng.random((gh, gw))
    y, x = np.arange(H) / cell, np.arange(W) / cell
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    a, b = lat[y0][:, x0], lat[y0][:, x0 + 1]
    c, d = lat[y0 + 1][:, x0], lat[y0 + 1][:, x0 + 1]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


def make_backgrounds(seed: int, n_bg: int, H: int, W: int) -> np.ndarray:
    """n_bg procedural pictures (n_bg, H, W, 3) uint8 BGR, picture b from default_rng((seed, 0x5AADE, 1 << 40 | b)): a two-colour
    gradient along a random direction, a few filled rectangles (shelves, panels), stripes over a band, and value noise on top.  No
    image files: a workshop wall is not a photograph, but it is not black either."""
    out = np.empty((int(n_bg), H, W, 3), np.uint8)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    for b in range(int(n_bg)):
        rng = np.random.default_rng((int(seed), _STREAM, (1 << 40) | b))
        c0, c1 = rng.uniform(30, 225, 3), rng.uniform(30, 225, 3)
        th = rng.uniform(0, 2 * np.pi)
        t = xx * np.cos(th) / max(W - 1, 1) + yy * np.sin(th) / max(H - 1, 1)
        t = (t - t.min()) / max(t.max() - t.min(), 1e-9)
        img = c0 + (c1 - c0) * t[..., None]
        for _ in range(int(rng.integers(2, 7))):
            h, w = int(rng.integers(1, max(H // 2, 2))), int(rng.integers(1, max(W // 2, 2)))
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            img[y:y + h, x:x + w] = rng.uniform(20, 235, 3)
        period, y, h = int(rng.integers(4, 33)), int(rng.integers(0, H)), int(rng.integers(1, max(H // 3, 2)))
        stripe = ((np.arange(W) // period) % 2).astype(np.float64) * rng.uniform(-40, 40)
        img[y:y + h] += stripe[None, :, None]
        img += (_value_noise(rng, H, W, int(rng.integers(8, 65)))[..., None] - .5) * rng.uniform(20, 70)
        out[b] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return out
