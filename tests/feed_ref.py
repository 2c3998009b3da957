"""Plain reference of the depth conditioning (include/rope_s3d.h, rope_depth_*; csrc/rope_feed.hip): Python loops over numpy
arrays, float32 and float64 scalars exactly as the header writes the steps, nothing clever.  Planes are uint16 sensor units,
0 = no data.  tests/test_feed_refs.py pins it by cases worked by hand; the GPU must equal it word for word."""
import math

import numpy as np

PERSISTENCE = [(0, 0), (8, 8), (2, 3), (2, 4), (2, 8), (1, 2), (1, 5), (1, 8), (0, 8)]      # (need, window); window 0 = never
MAX_FOOTPRINT = 16
F32 = np.float32


def decimated_shape(H, W, k):
    return ((H // k) // 4) * 4, ((W // k) // 4) * 4


def decimate(raw, k):
    """(n, H, W) -> (n, h, w)."""
    n, H, W = raw.shape
    h, w = decimated_shape(H, W, k)
    assert 2 <= k <= 8 and h > 0 and w > 0
    out = np.zeros((n, h, w), np.uint16)
    for f in range(n):
        for r in range(h):
            for c in range(w):
                valid = sorted(int(v) for v in raw[f, r * k:r * k + k, c * k:c * k + k].ravel() if v != 0)
                m = len(valid)
                if m:
                    out[f, r, c] = valid[(m - 1) // 2] if k <= 3 else sum(valid) // m
    return out


def _spatial_step(a, b, alpha, delta):
    a, b = int(a), int(b)
    if a != 0 and b != 0 and 1 <= abs(b - a) <= delta:
        v = F32(b) * alpha
        u = F32(a) * (F32(1.0) - alpha)
        return int(v + u + F32(0.5))                 # (v + u) rounds, then + 0.5 rounds; int() truncates
    return b


def spatial_pass(line, alpha, delta, backward=False):
    """One pass over a 1-D line, in place."""
    alpha = F32(alpha)
    L = len(line)
    order = range(L - 2, -1, -1) if backward else range(1, L)
    for i in order:
        line[i] = _spatial_step(line[i + 1 if backward else i - 1], line[i], alpha, delta)
    return line


def spatial_sweep(line, alpha, delta):
    spatial_pass(line, alpha, delta)
    spatial_pass(line, alpha, delta, backward=True)
    return line


def spatial(planes, alpha, delta, iterations):
    """(n, h, w) -> a filtered copy."""
    x = planes.copy()
    n, h, w = x.shape
    for f in range(n):
        for _ in range(iterations):
            for r in range(h):
                spatial_sweep(x[f, r, :], alpha, delta)
            for c in range(w):
                spatial_sweep(x[f, :, c], alpha, delta)
    return x


def temporal(planes, alpha, delta, persistence, last, history):
    """(n, h, w) consecutive frames -> a filtered copy; `last` (uint16) and `history` (uint8) are updated in place."""
    alpha = F32(alpha)
    beta = F32(1.0) - alpha
    need, window = PERSISTENCE[persistence]
    x = planes.copy()
    n, h, w = x.shape
    for f in range(n):
        for r in range(h):
            for q in range(w):
                c, p, hist = int(x[f, r, q]), int(last[r, q]), int(history[r, q])
                if c != 0:
                    if p != 0 and abs(c - p) <= delta:
                        v = int(alpha * F32(c) + beta * F32(p) + F32(0.5))
                        x[f, r, q] = v
                        last[r, q] = v
                    else:
                        last[r, q] = c
                elif p != 0 and window != 0 and bin(hist & ((1 << window) - 1)).count('1') >= need:
                    x[f, r, q] = p
                history[r, q] = ((hist << 1) | (c != 0)) & 0xFF
    return x


def _corner(u, v, Z, d, c, R, t):
    X = (u - d[2]) / d[0] * Z
    Y = (v - d[3]) / d[1] * Z
    X2 = R[0] * X + R[1] * Y + R[2] * Z + t[0]
    Y2 = R[3] * X + R[4] * Y + R[5] * Z + t[1]
    Z2 = R[6] * X + R[7] * Y + R[8] * Z + t[2]
    if not Z2 > 0.0:
        return None
    return X2 / Z2 * c[0] + c[2], Y2 / Z2 * c[1] + c[3]


def align(planes, depth_intrin, color_intrin, extrin, depth_scale, Hc, Wc, stats=None):
    """(n, h, w) depth planes seen from the colour sensor -> (n, Hc, Wc).  Intrinsics {fx, fy, cx, cy}; extrin = row-major R, then t.
    stats, a dict, receives how many contributing pixels fell outside and how many colour pixels had more than one contributor
    of different depth."""
    d = [float(v) for v in depth_intrin]
    c = [float(v) for v in color_intrin]
    e = [float(v) for v in extrin]
    R, t = e[:9], e[9:]
    scale = float(depth_scale)
    n, h, w = planes.shape
    best = np.full((n, Hc, Wc), 0xFFFFFFFF, np.uint32)
    outside = collided = 0
    for f in range(n):
        for y in range(h):
            for x in range(w):
                z = int(planes[f, y, x])
                if z == 0:
                    continue
                Z = float(z) * scale
                p0 = _corner(x - 0.5, y - 0.5, Z, d, c, R, t)
                p1 = _corner(x + 0.5, y + 0.5, Z, d, c, R, t)
                if p0 is None or p1 is None:
                    continue
                fl = [math.floor(v + 0.5) if math.isfinite(v) else -1 for v in (p0[0], p0[1], p1[0], p1[1])]
                x0, x1 = min(fl[0], fl[2]), max(fl[0], fl[2])
                y0, y1 = min(fl[1], fl[3]), max(fl[1], fl[3])
                if x0 < 0 or x1 >= Wc or y0 < 0 or y1 >= Hc:
                    outside += 1
                    continue
                if x1 - x0 + 1 > MAX_FOOTPRINT or y1 - y0 + 1 > MAX_FOOTPRINT:
                    continue
                for yy in range(y0, y1 + 1):
                    for xx in range(x0, x1 + 1):
                        if best[f, yy, xx] != 0xFFFFFFFF and best[f, yy, xx] != z:
                            collided += 1
                        if z < best[f, yy, xx]:
                            best[f, yy, xx] = z
    if stats is not None:
        stats.update(outside=outside, collided=collided)
    return np.where(best == 0xFFFFFFFF, 0, best).astype(np.uint16)


def scaled_intrinsics(intrin, k):
    """What the conditioner hands the alignment after a decimation by k: every term divided by k."""
    return [float(v) / k for v in intrin]


class Chain:
    """The whole chain with its state: DepthConditioner's counterpart (defaults: the reference's LiveCamera settings)."""

    def __init__(self, depth_intrin, color_intrin, extrin, depth_scale, color_shape, decimation=2, spatial=(2, 0.5, 20),
                 temporal=(0.5, 20, 3)):
        self.d, self.c, self.e, self.scale, self.color_shape = depth_intrin, color_intrin, extrin, depth_scale, color_shape
        self.decimation, self.spatial, self.temporal = decimation, spatial, temporal
        self.last = self.history = None

    def reset(self):
        self.last = self.history = None

    def process_many(self, raw):
        x = decimate(raw, self.decimation) if self.decimation else raw.copy()
        if self.spatial:
            x = spatial(x, self.spatial[1], self.spatial[2], self.spatial[0])
        if self.temporal:
            if self.last is None:
                self.last, self.history = np.zeros(x.shape[1:], np.uint16), np.zeros(x.shape[1:], np.uint8)
            x = temporal(x, self.temporal[0], self.temporal[1], self.temporal[2], self.last, self.history)
        d = scaled_intrinsics(self.d, self.decimation) if self.decimation else self.d
        return align(x, d, self.c, self.e, self.scale, *self.color_shape)

    def process(self, raw):
        return self.process_many(raw[None])[0]

    def metres(self, plane):
        return np.array(plane, dtype=float) * self.scale

    def average(self, raws):
        planes = self.process_many(raws)
        return planes.astype(np.uint32).sum(axis=0, dtype=np.uint32).astype(np.float64) * self.scale / len(raws)
