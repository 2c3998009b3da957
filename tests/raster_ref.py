"""An exact rasteriser in integers and scenes built for the edges of the raster kernels ("What the rasteriser is
held to").

The exact rasteriser is the independent implementation that tests/golden/make_pins.py introduced, for any vertex / face / link
arrays and any float32 link matrices:

  * vertex shading: every float32 operation of DESIGN.md §3 step 2 evaluated as a rational over Python integers and rounded once,
    by hand (round to nearest, ties to even);
  * coverage: brute force over every sample of a triangle's box, the three edge functions as integers, OpenGL's top-left rule
    (y up), back faces culled, sample centres at 256 p + 128.  The edge functions are numpy int64: the guard in render_exact
    holds every coordinate below 2^29, so every product stays below 2^60 and every edge function below 2^61;
  * depth: exact barycentric interpolation of the float32 vertex depths in Python integers (numpy object arrays), GL_LESS against
    1.0, nearest wins, ties to the lower link.  A depth is kept as floor(d * 2^SH) with SH large enough that the floor preserves
    both the order and the equality of any two depths that can occur (see _shift).

It calls neither the C oracle nor the engine.  `wrong=` selects one deliberately wrong rule, for the tests that show the scenes
tell the right rules from the wrong ones.

The scene builders put vertices on exact multiples of 1/256 px through an affine camera (see SceneBuilder) and decide themselves
which triangles share a meshlet and in what order.
"""
from types import SimpleNamespace

import numpy as np

S = 149                      # every finite float32 is an integer multiple of 2^-149
D24 = (1 << 24) - 1
TILE_W, TILE_H = 128, 96
SMALL_COLS = SMALL_ROWS = 4
EDGE_COEF_LIMIT = 1 << 22
EDGE_K_LIMIT = 1 << 30
COMPACT_PX = 60
MAX_MESHLETS = 2048
WRONG = ('topleft_inverted', 'owns_dy_positive', 'centre_256p', 'lequal', 'tie_high', 'front_cw', 'box_no_offset', 'snap_trunc')


# ------------------------------------------------------------------ float32 by hand
def f32_to_int(x) -> int:
    """float32 -> the integer I with x = I * 2^-149 (exact)."""
    b = int(np.float32(x).view(np.uint32))
    sign, e, m = b >> 31, (b >> 23) & 0xFF, b & 0x7FFFFF
    assert e != 0xFF, "non-finite"
    v = (m | 0x800000) << (e - 1) if e else m
    return -v if sign else v


def round_to_f32(num: int, den: int = 1) -> int:
    """The float32 nearest to num / (den * 2^149) (ties to even), returned as its own integer (multiple of 2^-149 units).
    num, den: Python ints, den > 0."""
    if num == 0:
        return 0
    sign = -1 if num < 0 else 1
    n = abs(num)
    # value v = n / den (in units of 2^-149).  Want m = round(v / 2^k) with k >= 0 chosen so that m has at most 24 bits.
    q = n // den
    L = q.bit_length()                                   # v in [2^(L-1), 2^L) when q > 0
    k = max(L - 24, 0)                                   # subnormal / small values: k = 0, ulp = one unit
    scale = den << k
    m, r = divmod(n, scale)
    twice = 2 * r
    if twice > scale or (twice == scale and (m & 1)):
        m += 1
    if m.bit_length() > 24:                              # the rounding carried into the next binade
        m >>= 1
        k += 1
    assert (m << k).bit_length() <= 128 + S + 24, "overflow"
    return sign * (m << k)


def fma(a: int, b: int, c: int) -> int:                  # fmaf(a, b, c): a*b is in units of 2^-298
    return round_to_f32(a * b + (c << S), 1 << S)


def mul(a: int, b: int) -> int:
    return round_to_f32(a * b, 1 << S)


def add(a: int, b: int) -> int:
    return round_to_f32(a + b)


def rcp(a: int) -> int:                                  # 1.0f / a
    sign = -1 if a < 0 else 1
    return sign * round_to_f32(1 << (2 * S), abs(a))


HALF = f32_to_int(np.float32(0.5))


def shade(m, x, y, z, hw, hh, trunc=False):
    """DESIGN.md §3 step 2 -> (X, Y, d in units of 2^-149) or None when the vertex has no window position."""
    cx = fma(m[0], x, fma(m[1], y, fma(m[2], z, m[3])))
    cy = fma(m[4], x, fma(m[5], y, fma(m[6], z, m[7])))
    cz = fma(m[8], x, fma(m[9], y, fma(m[10], z, m[11])))
    cw = fma(m[12], x, fma(m[13], y, fma(m[14], z, m[15])))
    if not (cw > 0 and -cw <= cz <= cw):
        return None
    rw = rcp(cw)
    sx = fma(mul(cx, rw), hw, hw)
    sy = fma(mul(cy, rw), hh, hh)
    d = fma(mul(cz, rw), HALF, HALF)
    lim = 10 ** 6 << S
    if not (abs(sx) < lim and abs(sy) < lim):
        return None

    def snap(s):                                         # rint(256 * s): 256 * s is exact in float32 here (|s| < 1e6), ties to even
        n, den = s * 256, 1 << S
        q, r = divmod(n, den)
        if trunc:                                        # the wrong rule: towards zero
            return q + 1 if (n < 0 and r) else q
        if 2 * r > den or (2 * r == den and (q & 1)):
            q += 1
        return q
    return snap(sx), snap(sy), d


def owns(ax, ay, bx, by):
    dy, dx = by - ay, bx - ax
    return dy < 0 or (dy == 0 and dx < 0)


def edge_class(ax, ay, bx, by) -> str:
    """Which side of a counter-clockwise (y up) triangle the edge a->b is."""
    dy, dx = by - ay, bx - ax
    if dx == 0:
        return 'left' if dy < 0 else 'right'
    if dy == 0:
        return 'top' if dx < 0 else 'bottom'
    return ('down' if dy < 0 else 'up') + ('_leftwards' if dx < 0 else '_rightwards')


def _shift(unit_bits: int) -> int:
    """A depth is n / (area2 * 2^unit_bits) with area2 < 2^61: two different depths differ by more than 2^-(2 * (61 + unit_bits)),
    so floor(d * 2^SH) with SH eight bits above that keeps order and equality."""
    return 2 * (61 + unit_bits) + 8


def shade_links(verts, vtx_off, mats, W, H, n_links, trunc=False):
    hw, hh = f32_to_int(np.float32(0.5) * np.float32(W)), f32_to_int(np.float32(0.5) * np.float32(H))
    out = []
    for l in range(n_links):
        m = [f32_to_int(v) for v in np.asarray(mats[l], np.float32).reshape(16)]
        out.append([shade(m, f32_to_int(v[0]), f32_to_int(v[1]), f32_to_int(v[2]), hw, hh, trunc)
                    for v in verts[vtx_off[l]:vtx_off[l + 1]]])
    return out


def render_exact(verts, faces, vtx_off, tri_off, mats, W, H, n_links=6, wrong=None, stats=None):
    """-> ids (H, W) uint8 (255 = nothing), d24 (H, W) uint32, gap (H, W) float64: the distance in window depth from the winner to
    the nearest surface of ANOTHER link on that pixel (inf where there is none; 0.0 exactly where two links tie).

    stats (a dict, optional) receives: 'count' (H, W) how many triangles drew each pixel (before the depth test), 'zero' a dict
    edge class -> number of samples whose edge function on an edge of that class is exactly 0, 'tri' per front-facing triangle whose box
    holds a sample its (link, face index, window vertices), 'bound' (H, W) the per-pixel bound B of DESIGN.md §6 on |d24_oracle - d24_exact|."""
    assert wrong is None or wrong in WRONG, wrong
    sv = shade_links(verts, vtx_off, mats, W, H, n_links, trunc=(wrong == 'snap_trunc'))
    ds = [v[2] for link in sv for v in link if v is not None and v[2] != 0]
    tz = min(((d & -d).bit_length() - 1 for d in ds), default=S)
    unit = S - tz                                        # depths are integers in units of 2^-unit
    SH = _shift(unit)
    INF = 1 << (SH + 2)
    keys = np.empty((n_links, H, W), object)
    keys.fill(INF)
    d24s = np.zeros((n_links, H, W), np.int64)
    if stats is not None:
        stats['count'] = np.zeros((H, W), np.int32)
        stats['zero'] = {}
        stats['tri'] = []
        stats['bound'] = np.zeros((H, W), np.float64)
    off = 0 if wrong == 'centre_256p' else 128
    for l in range(n_links):
        F = faces[tri_off[l]:tri_off[l + 1]]
        for fi, tri in enumerate(F):
            a, b, c = sv[l][tri[0]], sv[l][tri[1]], sv[l][tri[2]]
            if a is None or b is None or c is None:
                continue
            if wrong == 'front_cw':
                b, c = c, b
            (ax, ay, da), (bx, by, db), (cx, cy, dc) = a, b, c
            assert max(abs(ax), abs(ay), abs(bx), abs(by), abs(cx), abs(cy)) < 1 << 29 and max(W, H) <= 1 << 14, "int64 guard"
            area2 = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay)
            if area2 <= 0:                               # GL_BACK culled: counter-clockwise (y up) is the front
                continue
            if wrong == 'box_no_offset':
                x0, x1 = -((-min(ax, bx, cx)) >> 8), max(ax, bx, cx) >> 8
                y0, y1 = -((-min(ay, by, cy)) >> 8), max(ay, by, cy) >> 8
            elif wrong == 'centre_256p':
                x0, x1 = (min(ax, bx, cx) >> 8) - 1, (max(ax, bx, cx) >> 8) + 1
                y0, y1 = (min(ay, by, cy) >> 8) - 1, (max(ay, by, cy) >> 8) + 1
            else:
                x0, x1 = -((-(min(ax, bx, cx) - 128)) >> 8), (max(ax, bx, cx) - 128) >> 8
                y0, y1 = -((-(min(ay, by, cy) - 128)) >> 8), (max(ay, by, cy) - 128) >> 8
            x0, x1, y0, y1 = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            fx = (256 * np.arange(x0, x1 + 1, dtype=np.int64) + off)[None, :]
            fy = (256 * np.arange(y0, y1 + 1, dtype=np.int64) + off)[:, None]
            E, inside = [], True
            for (px_, py_, qx, qy) in ((ax, ay, bx, by), (bx, by, cx, cy), (cx, cy, ax, ay)):
                e = (qx - px_) * (fy - py_) - (qy - py_) * (fx - px_)
                o = owns(px_, py_, qx, qy)
                if wrong == 'topleft_inverted':
                    o = not o
                elif wrong == 'owns_dy_positive':
                    dy, dx = qy - py_, qx - px_
                    o = dy > 0 or (dy == 0 and dx < 0)
                inside = inside & (e + (0 if o else -1) >= 0)
                E.append(e)
            if stats is not None:                        # samples exactly on an edge (and not outside the other two), per edge class
                for k, (px_, py_, qx, qy) in enumerate(((ax, ay, bx, by), (bx, by, cx, cy), (cx, cy, ax, ay))):
                    on = (E[k] == 0) & (E[(k + 1) % 3] >= 0) & (E[(k + 2) % 3] >= 0)
                    kc = edge_class(px_, py_, qx, qy)
                    stats['zero'][kc] = stats['zero'].get(kc, 0) + int(on.sum())
            if stats is not None:                        # every front-facing triangle whose box holds a sample, drawn or not
                stats['tri'].append((l, fi, (ax, ay, to_float(da)), (bx, by, to_float(db)), (cx, cy, to_float(dc))))
            if not inside.any():
                continue
            iy, ix = np.nonzero(inside)
            e01, e12, e20 = (E[k][iy, ix].astype(object) for k in range(3))
            num = e12 * (da >> tz) + e20 * (db >> tz) + e01 * (dc >> tz)          # depth = num / den, exactly
            den = area2 << unit
            draw = np.asarray(num <= den if wrong == 'lequal' else num < den, bool)   # GL_LESS against the cleared 1.0
            rows, cols = H - 1 - (y0 + iy), x0 + ix                                  # image rows top-down
            if stats is not None:
                stats['count'][rows[draw], cols[draw]] += 1
                bnd = d24_bound(a, b, c, area2, x0 + ix, y0 + iy, num, den)
                np.maximum.at(stats['bound'], (rows[draw], cols[draw]), bnd[draw])
            if not draw.any():
                continue
            num, rows, cols = num[draw], rows[draw], cols[draw]
            key = (num << SH) // den
            n2 = num * D24
            q = n2 // den
            r2 = (n2 - q * den) * 2
            up = np.asarray(r2 > den, bool) | (np.asarray(r2 == den, bool) & np.asarray(q % 2 == 1, bool))   # round half to even
            q = (q + up.astype(object)).astype(np.int64)
            cur = keys[l][rows, cols]
            better = np.asarray(key < cur, bool)
            keys[l][rows[better], cols[better]] = key[better]
            d24s[l][rows[better], cols[better]] = q[better]
    # nearest link per pixel, ties to the lower link (the wrong rule: to the higher)
    order = range(n_links - 1, -1, -1) if wrong == 'tie_high' else range(n_links)
    best = np.empty((H, W), object)
    best.fill(INF)
    ids = np.full((H, W), 255, np.uint8)
    d24 = np.zeros((H, W), np.uint32)
    for l in order:
        take = np.asarray(keys[l] < best, bool)
        best[take] = keys[l][take]
        ids[take] = l
        d24[take] = d24s[l][take]
    gap = np.full((H, W), np.inf)
    for l in range(n_links):
        other = np.asarray(keys[l] < INF, bool) & (ids != l) & (ids != 255)
        if other.any():
            g = np.array([float(v) for v in ((keys[l][other] - best[other]) >> (SH - 64))]) / 2.0 ** 64
            gap[other] = np.minimum(gap[other], g)
    return ids, d24, gap


def to_float(i: int) -> float:
    return i / 2.0 ** S


def d24_bound(a, b, c, area2, px, py, num, den):
    """B of DESIGN.md §6 per sample: how far the oracle's 24-bit depth (a float32 plane, two fmaf, one product, one rint) may lie
    from rint(exact depth * (2^24 - 1)).  First order in u = 2^-24:
        |d_f32 - d| <= u (8 Gx|dx| + 9 Gy|dy| + 10 Dc)  <=  11 u M,   M = Gx|dx| + Gy|dy| + Dc
    with Gx = 256 (|e1 A20| + |e2 A01|) / area2, Gy alike with B20, B01, Dc = |d_a| + (|e1 E20a| + |e2 E01a|) / area2 (the
    magnitudes BEFORE cancellation, which is what the roundings scale with), dx, dy the sample's distance from the anchor pixel;
    the 11th u covers the second-order terms.  The product with 2^24 - 1 adds u |d| 2^24 <= |d|, and two values less than t apart
    round to integers at most floor(t + 1) apart."""
    (ax, ay, da), (bx, by, db), (cx, cy, dc) = a, b, c
    u = 2.0 ** -24
    fa, fb, fc = to_float(da), to_float(db), to_float(dc)
    e1, e2 = abs(fb - fa), abs(fc - fa)
    ar = float(area2)
    Gx = 256.0 * (e1 * abs(ay - cy) + e2 * abs(by - ay)) / ar
    Gy = 256.0 * (e1 * abs(ax - cx) + e2 * abs(bx - ax)) / ar
    pxa, pya = ax >> 8, ay >> 8
    fxa, fya = 256 * pxa + 128, 256 * pya + 128
    E20a = (ax - cx) * (fya - cy) - (ay - cy) * (fxa - cx)
    E01a = (bx - ax) * (fya - ay) - (by - ay) * (fxa - ax)
    Dc = abs(fa) + (e1 * abs(E20a) + e2 * abs(E01a)) / ar
    M = Gx * np.abs(px - pxa) + Gy * np.abs(py - pya) + Dc
    d = np.abs(np.array([float(n) for n in num]) / float(den)) if len(num) else np.zeros(0)
    return np.floor(11 * u * M * D24 + d + 1.0)


# ------------------------------------------------------------------ the kernel's own decisions, restated
def tile_frames(W, H):
    """Every tile as (col0, vy0, wx0, wx1, wy0, wy1): the window rectangle (y up, inclusive) and the origin of (u, v)."""
    out = []
    for ty in range((H + TILE_H - 1) // TILE_H):
        for tx in range((W + TILE_W - 1) // TILE_W):
            col0, row0 = tx * TILE_W, ty * TILE_H
            out.append((col0, H - row0 - TILE_H, col0, min(col0 + TILE_W, W) - 1, max(H - row0 - TILE_H, 0), H - 1 - row0))
    return out


def classify(tri, W, H):
    """How raster_tile walks a front-facing window triangle ((X, Y), ...) in every tile its box meets:
    -> list of (tile index, walk, w, h, items) with walk in 'exact' | 'small' | 'rows' | 'cols'."""
    (ax, ay), (bx, by), (cx, cy) = [(v[0], v[1]) for v in tri]
    big = max(abs(bx - ax), abs(by - ay), abs(cx - bx), abs(cy - by), abs(ax - cx), abs(ay - cy))
    out = []
    for t, (col0, vy0, wx0, wx1, wy0, wy1) in enumerate(tile_frames(W, H)):
        x0, x1 = max(-((-(min(ax, bx, cx) - 128)) >> 8), wx0), min((max(ax, bx, cx) - 128) >> 8, wx1)
        y0, y1 = max(-((-(min(ay, by, cy) - 128)) >> 8), wy0), min((max(ay, by, cy) - 128) >> 8, wy1)
        if x0 > x1 or y0 > y1:
            continue
        w, h = x1 - x0 + 1, y1 - y0 + 1
        if big >= EDGE_COEF_LIMIT:
            out.append((t, 'exact', w, h, 0))
        elif w <= SMALL_COLS and h <= SMALL_ROWS:
            out.append((t, 'small', w, h, 0))
        else:
            out.append((t, 'cols', w, h, w) if h > w else (t, 'rows', w, h, h))
    return out


def edge_K(ax, ay, bx, by, col0, vy0):
    """make_edge's K before the clamp to +-EDGE_K_LIMIT, and the coefficients A, B."""
    A, B = -(by - ay), bx - ax
    Cc = 128 * (A + B) - A * ax - B * ay + (0 if owns(ax, ay, bx, by) else -1)
    return A, B, -(Cc >> 8) - A * col0 - B * vy0


def span_cases(tri, W, H):
    """Which of clip_span's cases the row (or column) items of a window triangle meet, over every tile where it takes the row or
    the column walk: 'A0_n_pos' / 'A0_n_nonpos' (A == 0 with n > 0: an empty line; with n <= 0: no limit), 'A1' (|A| == 1),
    'cut_hi' / 'cut_lo' (the exact quotient lies beyond the clamp of floor_div_pos to [-3, TILE_W + 2]), 'K_clamped'."""
    (ax, ay), (bx, by), (cx, cy) = [(v[0], v[1]) for v in tri]
    out = set()
    for (t, walk, w, h, items) in classify(tri, W, H):
        if walk not in ('rows', 'cols'):
            continue
        col0, vy0, wx0, wx1, wy0, wy1 = tile_frames(W, H)[t]
        x0, y0 = max(-((-(min(ax, bx, cx) - 128)) >> 8), wx0), max(-((-(min(ay, by, cy) - 128)) >> 8), wy0)
        for (p, q) in (((ax, ay), (bx, by)), ((bx, by), (cx, cy)), ((cx, cy), (ax, ay))):
            A, B, K = edge_K(p[0], p[1], q[0], q[1], col0, vy0)
            if abs(K) > EDGE_K_LIMIT:
                out.add('K_clamped')
            K = max(min(K, EDGE_K_LIMIT), -EDGE_K_LIMIT)
            if walk == 'cols':
                A, B = B, A
            first = (x0 - col0) if walk == 'cols' else (y0 - vy0)
            for c in range(first, first + items):
                n = K - B * c
                if A == 0:
                    out.add('A0_n_pos' if n > 0 else 'A0_n_nonpos')
                    continue
                if abs(A) == 1:
                    out.add('A1')
                quo = (-n) // (-A) if A < 0 else (n + A - 1) // A
                if quo > TILE_W + 2:
                    out.add('cut_hi')
                if quo < -3:
                    out.add('cut_lo')
    return out


def meshlet_extent_px(pts, PV, W, H):
    """The screen extent (x, y) of a meshlet as meshlet_box works it out: the float32 box rope_set_robot builds around the
    vertices (centre and half extent, rounded outwards), its eight corners through float32(PV), max - min in float32."""
    p = np.asarray(pts, np.float64)
    lo, hi = p.min(0), p.max(0)
    ctr = ((lo + hi) * 0.5).astype(np.float32)
    ext = (np.maximum(hi - ctr.astype(np.float64), ctr.astype(np.float64) - lo) * (1.0 + 1e-6) + 1e-7).astype(np.float32)
    m = [f32_to_int(v) for v in np.asarray(PV, np.float64).astype(np.float32).reshape(16)]
    hw, hh = f32_to_int(np.float32(0.5) * np.float32(W)), f32_to_int(np.float32(0.5) * np.float32(H))
    sx, sy = [], []
    for k in range(8):
        x, y, z = (add(f32_to_int(ctr[i]), f32_to_int(ext[i]) * (1 if (k >> i) & 1 else -1)) for i in range(3))
        cx = fma(m[0], x, fma(m[1], y, fma(m[2], z, m[3])))
        cy = fma(m[4], x, fma(m[5], y, fma(m[6], z, m[7])))
        cw = fma(m[12], x, fma(m[13], y, fma(m[14], z, m[15])))
        rw = rcp(cw)
        sx.append(fma(mul(cx, rw), hw, hw))
        sy.append(fma(mul(cy, rw), hh, hh))
    return to_float(add(max(sx), -min(sx))), to_float(add(max(sy), -min(sy)))


# ------------------------------------------------------------------ scenes
SC = 1 << 14            # model units: one is 16384 px, so that even the 16384 px triangles stay within a reach of a few units


class SceneBuilder:
    """Vertices are given in window coordinates: (X, Y) integers in 1/256 px and a window depth d (a float32 value).  The camera
    is affine — PV = [[SC/hw, 0, 0, -1], [0, SC/hh, 0, -1], [0, 0, k10, k11], [0, 0, 0, 1]] — every joint is the identity at
    q = 0, so every link matrix is float32(PV) and the model vertex (X / 2^22, Y / 2^22, (2 d - 1 - k11) / k10) lands on
    (X, Y, d): exactly on a power-of-two image, and after the snap to 1/256 px on any other.  finish() proves it through the
    exact `shade`.  depth='mid' keeps d in [1/4, 3/4] and the near plane out of the robot's reach (the kernels without the
    clipping code run); depth='full' maps z to d = z in [0, 1] (the clipping kernels run, and d = 0 takes the cutting pass)."""

    def __init__(self, name, W, H, depth='mid', PV=None):
        self.name, self.W, self.H = name, W, H
        self.k10, self.k11 = (0.125, 0.0) if depth == 'mid' else (2.0, -1.0)
        self.PV = np.array([[SC / (0.5 * W), 0, 0, -1], [0, SC / (0.5 * H), 0, -1], [0, 0, self.k10, self.k11], [0, 0, 0, 1]], np.float64)
        self.raw = PV is not None                        # a camera of the caller's: vertices are model coordinates (x, y, z) as they are
        if self.raw:
            self.PV = np.asarray(PV, np.float64)
        self.meshlets = [[] for _ in range(6)]          # per link: list of meshlets, each a list of triangles of (X, Y, d)
        self.edges = {}                                  # what the builder claims to reach, checked by the CPU tests

    def meshlet(self, link, tris):
        if self.raw:
            tris = [tuple(tuple(float(np.float32(c)) for c in v) for v in t) for t in tris]
        else:
            tris = [tuple((int(v[0]), int(v[1]), float(np.float32(v[2]))) for v in t) for t in tris]
        assert 1 <= len(tris) <= 128
        self.meshlets[link].append(tris)
        return self

    def quad(self, x0, y0, x1, y1, d00, d10, d01, d11=None):
        """Two counter-clockwise triangles over the rectangle [x0, x1] x [y0, y1] (1/256 px), split along the diagonal from
        (x1, y0) to (x0, y1); depths at (x0,y0), (x1,y0), (x0,y1), (x1,y1) (the last defaults to the plane of the others)."""
        if d11 is None:
            d11 = d10 + d01 - d00
        return [((x0, y0, d00), (x1, y0, d10), (x0, y1, d01)), ((x1, y0, d10), (x1, y1, d11), (x0, y1, d01))]

    def model_vertex(self, v):
        if self.raw:
            return v
        return (v[0] / 2.0 ** 22, v[1] / 2.0 ** 22, (2.0 * v[2] - 1.0 - self.k11) / self.k10)

    def finish(self, rows=None):
        for l in range(6):
            assert self.meshlets[l] or not self.raw
            if not self.meshlets[l]:                     # a link with nothing to show: one triangle far off screen
                x = -(3000 << 8) - (l << 12)
                self.meshlet(l, [((x, x, 0.5), (x + 512, x, 0.5), (x, x + 512, 0.5))])
        verts, faces, vtx_off, tri_off = [], [], [0], [0]
        hdr, mverts, mtris, link_first = [], [], [], [0]
        for l in range(6):
            base = len(verts)
            for tris in self.meshlets[l]:
                local, idx = {}, []
                for t in tris:
                    idx.append([local.setdefault(v, len(local)) for v in t])
                assert len(local) <= 64, "a meshlet holds at most 64 vertices"
                pts = np.array([self.model_vertex(v) for v in local], np.float32)
                v0 = len(verts)
                verts.extend(pts.tolist())
                faces.extend([[v0 - base + i for i in t] for t in idx])
                c = (pts.astype(np.float64).min(0) + pts.astype(np.float64).max(0)) * 0.5
                rad = float(np.sqrt(((pts - c) ** 2).sum(1).max())) * (1.0 + 1e-5) + 1e-7
                h = np.zeros(8, np.uint32)
                h[0:4] = np.array([c[0], c[1], c[2], rad], np.float32).view(np.uint32)
                h[4], h[5], h[6], h[7] = len(mverts), len(mtris), len(local) | (len(tris) << 16), l
                hdr.append(h)
                mverts.extend(pts.tolist())
                mtris.extend([t[0] | (t[1] << 8) | (t[2] << 16) for t in idx])
            vtx_off.append(len(verts))
            tri_off.append(len(faces))
            link_first.append(len(hdr))
        assert len(hdr) <= MAX_MESHLETS
        jf = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64), (6, 1))
        ja = np.tile(np.array([0.0, 0.0, 1.0]), (6, 1))
        ml = SimpleNamespace(header=np.stack(hdr), verts=np.array(mverts, np.float32), tris=np.array(mtris, np.uint32),
                             link_first=np.array(link_first, np.int32))
        model = SimpleNamespace(verts=np.array(verts, np.float32), faces=np.array(faces, np.int32), vtx_off=np.array(vtx_off, np.int32),
                                tri_off=np.array(tri_off, np.int32), joint_fixed=jf, joint_axes=ja, meshlets=ml, n_links=6)
        sc = SimpleNamespace(name=self.name, W=self.W, H=self.H, PV=self.PV, znear=0.05, zfar=100.0, model=model,
                             rows=np.zeros((1, 6)) if rows is None else np.asarray(rows, np.float64), edges=self.edges,
                             meshlet_tris=self.meshlets, mats=np.tile(self.PV.astype(np.float32).reshape(1, 16), (6, 1)))
        if self.raw:
            return sc
        # every vertex landed where the builder put it
        sv = shade_links(model.verts, model.vtx_off, sc.mats, sc.W, sc.H, 6)
        k = 0
        for l in range(6):
            want = [v for tris in self.meshlets[l] for v in dict.fromkeys(v for t in tris for v in t)]
            assert len(want) == len(sv[l])
            for w, got in zip(want, sv[l]):
                far = abs(w[0]) >= 10 ** 6 * 256 or abs(w[1]) >= 10 ** 6 * 256 or not (0.0 <= w[2] <= 1.0)
                assert (got is None) if far else (got == (w[0], w[1], f32_to_int(w[2]))), (self.name, l, w, got)
                k += 1
        return sc


def px(v):
    """Pixels (multiples of 1/256) -> 1/256 px."""
    r = v * 256
    assert r == int(r), v
    return int(r)


def many_rows(n):
    """Candidate rows beyond a scene's own: row 0 is the scene (q = 0), the others small rotations about the joints' z axes —
    a few distinct (q0, q1) prefixes, so that the shared layers have something to share."""
    i = np.arange(n)
    q = np.zeros((n, 6))
    q[:, 0], q[:, 1], q[:, 2], q[:, 5] = (i % 4) * 0.01, (i % 3) * 0.005, (i % 5) * 0.005, (i % 2) * 0.005
    return q


TARGET_ROW = np.array([0.004, 0.002, 0.003, 0.0, 0.0, 0.001])      # the pose the targets are rendered at: none of many_rows


def plane(x, y):
    """The tilted plane most scenes put their triangles on: dyadic, within [1/4, 3/4] over a 256 x 256 image."""
    return 0.3 + (x + 2 * y) / (256.0 * 2048.0)


def scene_boxes():
    """(a) Boxes of every size from 1x1 to 6x6 samples inside a tile (the one-lane walk up to 4x4, rows, columns when taller than
    wide, h == w), and the same sizes across the seams at column 127|128 and rows 160|159, 64|63 (y up) of a 256x256 image,
    where the tile cuts the box down to every smaller size; each box is a rectangle of two triangles on two links."""
    b = SceneBuilder('boxes', 256, 256)
    per_link = [[] for _ in range(6)]

    def box(X, Y, w, h, k):
        x0, y0, x1, y1 = px(X + 0.25), px(Y + 0.25), px(X + w - 0.25), px(Y + h - 0.25)
        t = b.quad(x0, y0, x1, y1, plane(x0, y0), plane(x1, y0), plane(x0, y1))
        per_link[k % 6].append(t[0])
        per_link[(k + 1) % 6].append(t[1])
    k = 0
    for w in range(1, 7):
        for h in range(1, 7):
            box(8 * w, 168 + 8 * h, w, h, k)                      # inside tile (0, 0)
            box(136 + 8 * w, 8 * h, w, h, k + 3)                  # inside the partial last tile row
            k += 1
    j = 0
    for w in range(2, 7):
        for s in range(1, w):                                     # s columns left of the seam at 128, every height in turn
            box(128 - s, 168 + 7 * j if j < 12 else 70 + 8 * (j - 12), w, 1 + k % 6, k)
            k, j = k + 1, j + 1
    for h in range(2, 7):
        for s in range(1, h):                                     # s rows below the seams at y = 160 and y = 64
            box(8 * k % 248, 160 - s, 1 + k % 6, h, k)
            box(8 * (k + 7) % 248, 64 - s, 1 + (k + 3) % 6, h, k + 1)
            k += 1
    box(125, 157, 6, 6, k)                                        # across both seams at once
    box(126, 62, 5, 5, k + 1)
    box(0, 0, 5, 3, k + 2)                                        # the image's corners
    box(251, 253, 5, 3, k + 3)
    for l in range(6):
        T = per_link[l]
        for i in range(0, len(T), 21):                            # 21 triangles: 63 vertices, one short of a meshlet's 64
            b.meshlet(l, T[i:i + 21])
    return b.finish()


def scene_corners():
    """(a) A box of 6x6 samples at every position relative to a tile corner: the 25 ways the seams can split it (1..5 columns left
    of the seam, 1..5 rows below it), one at each of the 25 interior tile corners of a 768x576 image, so that none hides another;
    each a rectangle of two triangles on two links."""
    b = SceneBuilder('corners', 768, 576)
    per_link = [[] for _ in range(6)]
    k = 0
    for j in range(1, 6):
        for i in range(1, 6):
            X, Y = TILE_W * i - i, 576 - TILE_H * j - j          # i columns left of the seam, j rows below it
            x0, y0, x1, y1 = px(X + 0.25), px(Y + 0.25), px(X + 5.75), px(Y + 5.75)
            d = lambda x, y: 0.3 + (x + 2 * y) / (256.0 * 8192.0)
            t = b.quad(x0, y0, x1, y1, d(x0, y0), d(x1, y0), d(x0, y1))
            per_link[k % 6].append(t[0])
            per_link[(k + 1) % 6].append(t[1])
            k += 1
    for l in range(6):
        b.meshlet(l, per_link[l])
    return b.finish()


def scene_edges():
    """(c) Edges with A == 0, B == 0 and |A| == 1 through sample centres in boxes large enough for clip_span; coefficients of
    2^22 - 1 (the fast walk's last) and 2^22 (raster_exact's first) on triangles that cross the tiles; K beyond the clamp on
    edges wholly on the covered and wholly on the uncovered side."""
    b = SceneBuilder('edges', 256, 256)
    c = lambda x, y: (px(x), px(y), plane(px(x) % 65536, px(y) % 65536))
    # axis-aligned through sample centres: a bottom edge that does not own its row (A == 0, n > 0), a top edge that does
    b.meshlet(0, [(c(10.5, 170.5), c(40.5, 170.5), c(10.5, 200.5)), (c(50.5, 200.5), c(20.5, 200.5), c(50.5, 170.5))])
    # |A| == 1: one sub-pixel of rise over 90 px, once each way
    b.meshlet(1, [((px(10.5), px(100.5), 0.4), (px(100.5), px(100.5) + 1, 0.4), (px(10.5), px(120.5), 0.45)),
                  ((px(10.5), px(140.5) + 1, 0.4), (px(100.5), px(140.5), 0.4), (px(100.5), px(150.5), 0.45))])
    # an extent of 16383 + 255/256 px (coefficient 2^22 - 1) and of 16384 px (2^22), both ways, crossing the tiles
    L = 1 << 22
    far = lambda x, y, ex, ey, d: [((px(x), px(y), d), (px(x) + ex, px(y) + ey + px(20), d + 0.01), (px(x), px(y) + px(40), d))]
    b.meshlet(2, far(5.5, 60.5, L - 1, 0, 0.50))
    b.meshlet(3, far(5.5, 110.5, L, 0, 0.52))
    tall = lambda x, y, e, d: [((px(x), px(y), d), (px(x) + px(30), px(y), d), (px(x) + px(15), px(y) + e, d + 0.01))]
    b.meshlet(4, tall(130.5, 20.5, L - 1, 0.54))
    b.meshlet(5, tall(180.5, 20.5, L, 0.56))
    # K beyond +-2^30: a triangle 16000 px across that covers the image from far away (its far edges wholly on the covered
    # side), and one whose box meets the image while all of it lies 4000 px outside (an edge wholly on the uncovered side)
    b.meshlet(0, [((px(-8000), px(-7000), 0.70), (px(8000), px(-7500), 0.70), (px(100), px(8000), 0.72))])
    b.meshlet(1, [((px(-6000), px(300), 0.6), (px(-5000), px(-5000), 0.6), (px(300), px(-6000), 0.6))])
    return b.finish()


def scene_queue(n_tri):
    """(d) One meshlet whose n_tri triangles all survive the cull and each cover the whole 128x96 tile: 96 row items each, so
    64 of them fill the row-item queue to its last chunk (6144 items, 96 chunks of 64); 63 leave the batch one short, 65 start
    a second one.  24 shared vertices (8 depths at each of three places) give every triangle a plane of its own."""
    b = SceneBuilder(f'queue{n_tri}', 128, 96)
    A = [(px(-64), px(-64), 0.30 + 0.02 * i) for i in range(8)]
    B = [(px(448), px(-64), 0.70 - 0.045 * i) for i in range(8)]
    C = [(px(-64), px(448), 0.25 + 0.055 * i) for i in range(8)]
    tris = [(A[k % 8], B[(k // 8 + k) % 8], C[(k // 8) % 8 if k < 64 else 7]) for k in range(n_tri)]
    assert len(set(tris)) == n_tri
    b.meshlet(2, tris)
    return b.finish()


def scene_shared():
    """(e) Fans and a strip whose interior samples all lie on a shared edge or a shared vertex; neighbouring triangles are on
    different links, so a sample drawn twice or not at all shows in the link image."""
    b = SceneBuilder('shared', 256, 256)
    k = 0
    for (X, Y, r) in ((60.5, 200.5, 2), (127.5, 160.5, 3), (128.5, 63.5, 2), (200.5, 30.5, 5)):      # two of them on tile corners
        ring = [(r, 0), (r, r), (0, r), (-r, r), (-r, 0), (-r, -r), (0, -r), (r, -r)]
        ctr = (px(X), px(Y), plane(px(X), px(Y)))
        for i in range(8):
            p, q = ring[i], ring[(i + 1) % 8]
            P, Q = (px(X + p[0]), px(Y + p[1])), (px(X + q[0]), px(Y + q[1]))
            b.meshlet(k % 6, [(ctr, P + (plane(*P),), Q + (plane(*Q),))])
            k += 1
        k += 1                                           # 8 triangles over 6 links: shift, so that the last and the first differ
    for i in range(40):                                  # a strip one pixel high, every sample a shared vertex
        x0, x1, y0, y1 = px(20.5 + i), px(21.5 + i), px(100.5), px(101.5)
        t = b.quad(x0, y0, x1, y1, plane(x0, y0), plane(x1, y0), plane(x0, y1))
        b.meshlet((2 * i) % 6, [t[0]])
        b.meshlet((2 * i + 1) % 6, [t[1]])
    # back-facing and degenerate triangles over the same samples: they draw nothing
    b.meshlet(0, [((px(20.5), px(100.5), 0.26), (px(20.5), px(140.5), 0.26), (px(60.5), px(100.5), 0.26)),
                  ((px(20.5), px(100.5), 0.26), (px(40.5), px(120.5), 0.26), (px(60.5), px(140.5), 0.26))])
    return b.finish()


def scene_depth():
    """(f) Depth: planes at d24 = 0 (d = 0, on the near plane: the cutting pass draws it), D24_MAX - 1 (d = 1 - 2^-24) and D24_MAX
    (d = 1: GL_LESS against the cleared 1.0 draws nothing); a sliver 0.3 px wide whose depth runs across it; two links on
    bit-identical vertices (the lower one wins); a stack of overlapping rectangles, each in a meshlet of its own, the later
    meshlets nearer."""
    b = SceneBuilder('depth', 256, 256, depth='full')
    flat = lambda X, Y, d: b.quad(px(X), px(Y), px(X + 20), px(Y + 12), d, d, d)
    b.meshlet(0, flat(4.25, 4.25, 0.0))
    b.meshlet(1, flat(30.25, 4.25, 1.0 - 2.0 ** -24))
    b.meshlet(2, flat(56.25, 4.25, 1.0))
    b.meshlet(3, flat(82.25, 4.25, 1.0 - 2.0 ** -24) + flat(82.25, 10.25, 1.0))           # the drawable plane under the undrawable one
    b.meshlet(4, [((px(150.375), px(10.5), 0.125), (px(150.6875), px(10.5), 0.875), (px(150.53125), px(60.5), 0.5))])
    same = b.quad(px(120.25), px(150.25), px(140.75), px(175.75), 0.375, 0.5, 0.4375)    # across the seams at 128 and 160
    b.meshlet(1, same)
    b.meshlet(3, same)
    b.meshlet(5, same)
    for i in range(18):                                  # later meshlets nearer, links in turn, 2^-6 apart
        b.meshlet(i % 6, b.quad(px(10.25 + 5 * i), px(80.25 + 3 * i), px(50.75 + 5 * i), px(120.75 + 3 * i),
                                0.75 - i / 64.0, 0.75 - i / 64.0 + 1 / 256.0, 0.75 - i / 64.0 + 1 / 512.0))
    return b.finish()


def scene_compact():
    """(b) The 32-bit set-up against the 64-bit one: the same cluster of small triangles in meshlets whose vertex extent is
    60 - 1/256 px (the largest that rope_set_robot's outward-rounded box still passes as compact) and 60 px (the next reachable
    extent: not compact), many of each listed by one tile so that a wave's batch of 64 mixes survivors of both kinds; and compact
    meshlets that reach 60 px beyond a tile's left and right edge (tile-relative coordinates at their largest, 48128 / 256 px)."""
    b = SceneBuilder('compact', 256, 256)
    b.edges['compact'], b.edges['loose'] = [], []

    def cluster(X, Y, ext, link):
        x, y = px(X), px(Y)
        d = lambda u, v: plane(x + u, y + v)
        v = lambda u, v_: (x + u, y + v_, d(u, v_))
        tris = [(v(0, 0), v(px(3.5), px(0.25)), v(px(0.5), px(2.75))), (v(px(3.5), px(0.25)), v(px(4), px(3)), v(px(0.5), px(2.75))),
                (v(0, 0), v(ext, 0), v(0, px(1.5)))]     # the last one stretches the meshlet to its extent (a sliver 1.5 px high)
        b.meshlet(link, tris)
        return tris
    for i in range(24):                                  # 48 meshlets in tile (0, 0), compact and not compact in turn
        X, Y = 2.25 + 62 * (i % 2), 162.25 + 3.75 * i
        (b.edges['compact'] if i % 2 == 0 else b.edges['loose']).append(cluster(X, Y, px(60) - (1 if i % 2 == 0 else 0), i % 3))
        X = 2.25 + 62 * ((i + 1) % 2)
        (b.edges['loose'] if i % 2 == 0 else b.edges['compact']).append(cluster(X, Y, px(60) - (0 if i % 2 == 0 else 1), 3 + i % 3))
    # compact meshlets hanging over the seam at column 127|128 from either side, and over the seam at y = 64 into the partial row
    b.edges['compact'].append(cluster(127.25, 100.25, px(60) - 1, 0))
    b.edges['compact'].append(cluster(68.5 + 1 / 256.0, 110.5, px(60) - 1, 4))
    b.edges['compact'].append(cluster(180.25, 62.25, px(60) - 1, 2))
    return b.finish()


def scene_limits(which):
    """(g) Meshlet limits.  'full': a meshlet of 128 triangles over 64 vertices (both steps of the cull loop full), one of 65
    (one lane of the second step), one of a single triangle, and a meshlet with a vertex beyond the far plane (no window
    position: its triangles are dropped, the others of the meshlet drawn).  'many': 2048 single-triangle meshlets all listed by
    the one tile of a 128x96 image — the capacity of the tile's meshlet list."""
    if which == 'many':
        b = SceneBuilder('limits_many', 128, 96)
        for i in range(MAX_MESHLETS):
            X, Y = 2 * (i % 64), 3 * (i // 64)
            x0, y0 = px(X + 0.25), px(Y + 0.25)
            b.meshlet(i * 6 // MAX_MESHLETS, [((x0, y0, plane(x0, y0)), (x0 + px(1.5), y0, plane(x0 + px(1.5), y0)), (x0, y0 + px(2.5), plane(x0, y0 + px(2.5))))])
        return b.finish()
    b = SceneBuilder('limits_full', 256, 256)

    def grid(X, Y, nx, ny, n_tri):
        # a lattice of nx x ny vertices 2.5 px apart on one plane: its cells split in two, then (a planar mesh of 64 vertices has
        # fewer than 128 triangles) the same plane again in triangles two cells wide
        P = [[(px(X + 2.5 * i), px(Y + 2.5 * j)) for i in range(nx)] for j in range(ny)]
        v = lambda i, j: P[j][i] + (plane(*P[j][i]),)
        T = []
        for s in (1, 2):
            for j in range(ny - s):
                for i in range(nx - s):
                    T += [(v(i, j), v(i + s, j), v(i, j + s)), (v(i + s, j), v(i + s, j + s), v(i, j + s))]
        assert len(T) >= n_tri
        return T[:n_tri]
    b.meshlet(1, grid(100.25, 155.25, 16, 4, 128))                    # 64 vertices, 128 triangles, across both seams
    b.meshlet(2, grid(10.25, 20.25, 12, 4, 65))
    b.meshlet(3, [((px(200.25), px(200.25), 0.4), (px(203.75), px(200.5), 0.4), (px(200.5), px(203), 0.41))])
    T = grid(60.25, 220.25, 5, 3, 16)
    bad = (px(70), px(240), 1.5)                                      # beyond the far plane: no window position
    b.meshlet(5, T[:6] + [(T[0][0], T[0][1], bad)] + T[6:])
    return b.finish()


def scene_sizes(W, H):
    """Tile geometry on an image narrower than a tile (100x37), lower than a tile, or of a width that is no multiple of 4 (131): a triangle
    that covers every tile, and rectangles that end on the image's last column and row and one sample short of them."""
    b = SceneBuilder(f'sizes_{W}x{H}', W, H)
    d = lambda x, y: 0.3 + (x + 2 * y) / (256.0 * 4096.0)
    b.meshlet(0, [((px(-20), px(-20), 0.70), (px(3 * W + 40), px(-20), 0.72), (px(-20), px(3 * H + 40), 0.71))])
    k = 1
    for (x0, y0, x1, y1) in ((W - 9.75, H - 6.75, W - 0.25, H - 0.25), (W - 9.75, 0.25, W - 1.25, 5.75), (0.25, H - 7.75, 6.75, H - 1.25),
                             (0.25, 0.25, 5.75, 3.75), (W / 2 - 10.75, H / 2 - 3.75, W / 2 + 10.25, H / 2 + 3.25)):
        t = b.quad(px(x0), px(y0), px(x1), px(y1), d(px(x0), px(y0)), d(px(x1), px(y0)), d(px(x0), px(y1)))
        b.meshlet(k % 6, [t[0]])
        b.meshlet((k + 1) % 6, [t[1]])
        k += 1
    return b.finish()


ZN, ZF = 0.05, 100.0
PERSPECTIVE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -(ZF + ZN) / (ZF - ZN), -2 * ZF * ZN / (ZF - ZN)], [0, 0, -1, 0]], np.float64)


def clip_class(v, PV=PERSPECTIVE):
    """A model vertex under float32(PV) as the cutting pass sees it: 'behind' the near plane (cz < -cw), 'bad' (in front of it but
    without a window position: beyond the far plane or w <= 0), or 'ok'; the clip coordinates in float32, one rounding a step."""
    m = [f32_to_int(x) for x in np.asarray(PV, np.float64).astype(np.float32).reshape(16)]
    x, y, z = (f32_to_int(np.float32(c)) for c in v)
    cz = fma(m[8], x, fma(m[9], y, fma(m[10], z, m[11])))
    cw = fma(m[12], x, fma(m[13], y, fma(m[14], z, m[15])))
    return 'behind' if cz < -cw else ('ok' if cw > 0 and cz <= cw else 'bad')


def cut_vertex_px(inside, outside, W, H, PV=PERSPECTIVE):
    """Where the edge from `inside` to `outside` (behind the near plane) meets that plane, in window pixels — clip_near's formula
    in float64, to show on which side of 10^6 px a cut vertex falls (it is asserted with a wide margin, not to the bit)."""
    a, b = PV @ np.append(np.asarray(inside, np.float64), 1.0), PV @ np.append(np.asarray(outside, np.float64), 1.0)
    bi, bo = a[2] + a[3], b[2] + b[3]
    c = a + bi / (bi - bo) * (b - a)
    return c[0] / c[3] * 0.5 * W + 0.5 * W, c[1] / c[3] * 0.5 * H + 0.5 * H


def scene_nearplane(only=None):
    """(h) Triangles cut at the near plane, under a perspective camera at the model's origin looking down -z (near 0.05, far 100;
    256x256, 90 degrees).  One vertex behind the plane in each of the three places of the vertex order (links 0, 1, 2), two
    behind with the one in front in each place (links 3, 4, 5), each beside an uncut triangle of the same meshlet; a triangle
    whose cut vertex falls beyond 10^6 px and one with a vertex beyond the far plane and one behind the near plane (both are
    dropped whole); and a rectangle three units away in a meshlet that never comes near the plane.  The exact rasteriser does not
    cut: this scene is held to the oracle only.  edges['classes']: per triangle (link, vertices behind, place of the odd vertex);
    edges['drops']: the two dropped triangles.  only='drops' keeps the two dropped triangles alone and only=i the i-th
    cut triangle alone (the other links hold a triangle off screen), for the tests that show what each of them draws."""
    b = SceneBuilder('nearplane', 256, 256, PV=PERSPECTIVE)
    b.edges['classes'], b.edges['drops'] = [], []
    rot = lambda t, k: tuple(t[(i + k) % 3] for i in range(3))
    for k in range(3):
        dx = -0.55 + 0.55 * k
        # q, p in front, r behind (the triangle runs down and out of the image): the odd one out comes to place 2, 1, 0 as the
        # order is rotated
        one = rot(((dx + 0.3, -0.3, -1.0), (dx - 0.3, -0.3, -1.0), (dx, -0.6, 0.2)), k)
        # p in front, q and r behind (it runs up and out): the odd one out (p) comes to place 0, 2, 1
        two = rot(((dx, 0.1, -1.0), (dx + 0.3, 0.5, 0.2), (dx - 0.3, 0.5, 0.2)), k)
        plain = lambda x: ((x, -0.12, -1.0), (x + 0.1, -0.12, -1.0), (x, 0.03, -1.0))
        if only is None:
            b.meshlet(k, [one, plain(dx - 0.15)])
            b.meshlet(3 + k, [plain(dx + 0.05), two])
        elif only in (2 * k, 2 * k + 1):
            b.meshlet(k if only == 2 * k else 3 + k, [one if only == 2 * k else two])
        b.edges['classes'] += [(k, 1, [clip_class(v) for v in one].index('behind')), (3 + k, 2, [clip_class(v) for v in two].index('ok'))]
    drop_far_px = ((0.0, 0.0, -1.0), (0.2, 0.0, -1.0), (1000.0, 0.3, 0.2))          # the cut on the way to x = 1000 lies 2 * 10^6 px out
    drop_far_plane = ((-0.2, 0.0, -1.0), (0.0, 0.0, -150.0), (-0.1, 0.3, 0.2))      # a vertex beyond the far plane, another behind the near
    b.edges['drops'] = [drop_far_px, drop_far_plane]
    if only is None or only == 'drops':
        b.meshlet(0, [drop_far_px])
        b.meshlet(1, [drop_far_plane])
    if only is not None:
        for l in range(6):
            if not b.meshlets[l]:
                b.meshlet(l, [((50.0 + l, 50.0, -1.0), (50.5 + l, 50.0, -1.0), (50.0 + l, 50.5, -1.0))])     # off screen
    else:
        b.meshlet(5, [((-2.5, -2.5, -3.0), (2.5, -2.5, -3.0), (-2.5, 2.5, -3.0)), ((2.5, -2.5, -3.0), (2.5, 2.5, -3.0), (-2.5, 2.5, -3.0))])
    return b.finish()


CUT_SCENES = {'nearplane'}        # held to the oracle only: the exact rasteriser does not cut triangles
SCENES = {
    'boxes': scene_boxes, 'compact': scene_compact, 'edges': scene_edges,
    'queue63': lambda: scene_queue(63), 'queue64': lambda: scene_queue(64), 'queue65': lambda: scene_queue(65),
    'shared': scene_shared, 'depth': scene_depth, 'limits_full': lambda: scene_limits('full'), 'limits_many': lambda: scene_limits('many'),
    'sizes_160x120': lambda: scene_sizes(160, 120), 'sizes_131x37': lambda: scene_sizes(131, 37), 'sizes_256x256': lambda: scene_sizes(256, 256), 'sizes_100x37': lambda: scene_sizes(100, 37),
    'corners': scene_corners, 'nearplane': scene_nearplane,
}
_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def make_oracle(sc):
    from oracle import oracle as orc
    m = sc.model
    return orc.Oracle(m.verts, m.faces, m.vtx_off, m.tri_off, m.joint_fixed, m.joint_axes, sc.PV, sc.W, sc.H, sc.znear, sc.zfar)
