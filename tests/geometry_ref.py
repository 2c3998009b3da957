"""Plain references and inputs for the first and the last kernels of an evaluation pass (rope_kernels.hip: meshlet_box through
fk_mvp / bounds / fk_bounds, finalize_one through finalize_only / finalize_frames / finalize_argmin).  numpy and Python only; no GPU.

box_exact      meshlet_box one float32 IEEE operation at a time (the library is built with -ffp-contract=off and writes fmaf where it
               fuses): boxes with both flag bits, both tile masks, both weight arrays.  The kernels must equal it bit for bit.
box_bounds64   the same eight corners projected in float64, in no particular order of operations, and what the design promises of a
               box: conservative, tight, the flag bits; check_boxes() holds any boxes (box_exact's or a kernel's) to it.
finalize_ref   finalize_one / mean_std_parts: Python integers modulo 2^64, numpy float64 in the kernel's order; argmin() its rule.
queue_ref      score_queue_kernel: the (row, tile) pairs of every weight class, their counts and the sums after the layer-only tiles,
               a loop over rows and tiles in Python integers; clear_pass_ref: clear_pass_kernel's zeros.

fmaf: a float32 fused multiply-add rounds ONCE.  float64 a * b + c rounds twice (the product of two float32 is exact in float64, the
sum is rounded to 53 bits and then to 24), and so would math.fma on doubles followed by a conversion — this Python (3.10) has no
math.fma anyway.  fmaf() therefore takes the exact product, the rounded sum and its exact error term (Knuth's TwoSum), forces the
53-bit sum to an odd last bit when it is inexact (rounding to odd, which a later rounding to <= 51 bits cannot be misled by) and
rounds that to float32 once; fmaf_fraction() is the definition with fractions.Fraction, and tests/test_geometry_refs.py holds the
fast one to it on random and adversarial operands.

The constants come out of the headers (constants()); tests/test_gpu_geometry_kernels.py checks them against what the shim exports."""
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
F32 = np.float32
U = 2.0 ** -24                                           # unit round-off of float32
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=1)
def constants():
    with open(os.path.join(ROOT, 'rope_s3d_amd', 'csrc', 'rope_kernels.h')) as f:
        text = f.read()
    with open(os.path.join(ROOT, 'include', 'rope_s3d.h')) as f:
        text += f.read()

    def num(name):
        m = re.search(r'\b%s\b\s*=?\s*(\d+)' % name, text)
        assert m, name
        return int(m.group(1))
    c = dict(TILE_W=num('ROPE_TILE_W'), TILE_H=num('ROPE_TILE_H'), MAX_MASK_WORDS=num('MAX_MASK_WORDS'),
             QUEUE_WEIGHT_TILES=num('QUEUE_WEIGHT_TILES'), QUEUE_COUNTERS=2 + num('ROPE_QUEUE_CLASSES'), COMPACT_PX=num('COMPACT_PX'),
             SUM_WORDS=num('ROPE_SUM_WORDS'), MAX_LINKS=num('ROPE_MAX_LINKS'), MAX_MESHLETS=num('MAX_MESHLETS'),
             QUEUE_CLASSES=num('ROPE_QUEUE_CLASSES'), QUEUE_TOP_LOG2=num('ROPE_QUEUE_TOP_LOG2'))
    for k, name in enumerate(('DEPTH', 'FULL', 'LOOKUP', 'TSWEEP')):
        c['LOSS_' + name] = num('ROPE_LOSS_' + name)
        assert c['LOSS_' + name] == k
    return c


SHIM_CONSTANTS = ('TILE_W', 'TILE_H', 'MAX_MASK_WORDS', 'QUEUE_WEIGHT_TILES', 'QUEUE_COUNTERS', 'COMPACT_PX', 'SUM_WORDS', 'MAX_LINKS',
                  'LOSS_DEPTH', 'LOSS_FULL', 'LOSS_LOOKUP', 'LOSS_TSWEEP', 'MAX_MESHLETS', 'QUEUE_CLASSES', 'QUEUE_TOP_LOG2')   # shim_constant(i), in this order
SUM_CNT, SUM_S1, SUM_AA, SUM_AB, SUM_BB, SUM_LINK0 = range(6)                                      # rope_kernels.h's enum
EMPTY_BOX = (1, 0, 1, 0)


# ------------------------------------------------------------------------------------------------ float32 arithmetic
def fmaf(a, b, c):
    """float32 fused multiply-add, correctly rounded, element-wise."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, F32).astype(np.float64) for v in (a, b, c)))
    p = a * b                                            # exact: 48 significant bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                        # s + e == p + c exactly
    s = np.ascontiguousarray(s)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0.0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
    return s.astype(F32)


def fmaf_fraction(a, b, c):
    """The definition: the exact value, rounded once (scalars)."""
    exact = Fraction(float(F32(a))) * Fraction(float(F32(b))) + Fraction(float(F32(c)))
    if exact == 0:
        return F32(float(F32(a)) * float(F32(b)) + float(F32(c)))                 # the sign of an exact zero
    sign, mag = (-1 if exact < 0 else 1), abs(exact)
    ex = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** ex > mag:
        ex -= 1                                          # 2^ex <= mag < 2^(ex + 1)
    q = max(ex, -126) - 23                               # the last place of a float32 of this size (subnormals: 2^-149)
    scaled = mag / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rest = scaled - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and (n & 1)):
        n += 1
    return F32(sign * math.ldexp(float(n), q))


# ------------------------------------------------------------------------------------------------ meshlet_box, exactly
def tiles_of(W, H):
    k = constants()
    return (W + k['TILE_W'] - 1) // k['TILE_W'], (H + k['TILE_H'] - 1) // k['TILE_H']


def frame(W, H):
    return (W, H) + tiles_of(W, H)


def mask_words_of(fp):
    return (fp[2] * fp[3] + 31) // 32


def box_exact(fp, header, aabb, mvp6, n_render, n_shared, lo_first=0, skip_shared=False, wrong=()):
    """meshlet_box for every meshlet of one candidate.  fp (W, H, tiles_x, tiles_y); header (M, 8) uint32; aabb (M, 8) float32; mvp6
    (6, 16) float32 (rows of links >= n_render are never read).  skip_shared: bounds_kernel's candidate that is not its layer's
    representative.  wrong: names of deliberate mistakes (WRONG_BOX), for tests/test_geometry_refs.py only.
    -> dict: boxes (M, 4) int16 {x0 | flags, x1, y0, y1}; mask_lo, mask_hi (mask_words,) uint32; tris, tris_lo (n_tiles,) uint32;
    and what was decided on the way, per meshlet: sxlo, sxhi, sylo, syhi (float32), behind, front, near, compact (bool)."""
    k = constants()
    W, H, tiles_x, tiles_y = fp
    header = np.asarray(header, np.uint32).reshape(-1, 8)
    aabb = np.asarray(aabb, F32).reshape(-1, 8)
    M = len(header)
    link = header[:, 7].astype(np.int64)
    ntri = (header[:, 6] >> 16).astype(np.int64)
    rendered = link < n_render
    mm = np.asarray(mvp6, F32).reshape(-1, 16)[np.where(rendered, link, 0)]
    hw, hh = F32(0.5) * F32(W), F32(0.5) * F32(H)
    big = F32(3.0e38)
    sxlo, sxhi, sylo, syhi = np.full(M, big), np.full(M, -big), np.full(M, big), np.full(M, -big)
    behind, front, near = np.zeros(M, bool), np.zeros(M, bool), np.zeros(M, bool)
    with np.errstate(all='ignore'):
        for c in range(8):
            x = aabb[:, 0] + (aabb[:, 4] if c & 1 else -aabb[:, 4])
            y = aabb[:, 1] + (aabb[:, 5] if c & 2 else -aabb[:, 5])
            z = aabb[:, 2] + (aabb[:, 6] if c & 4 else -aabb[:, 6])
            cx, cy, cz, cw = (fmaf(mm[:, 4 * r], x, fmaf(mm[:, 4 * r + 1], y, fmaf(mm[:, 4 * r + 2], z, mm[:, 4 * r + 3]))) for r in range(4))
            limit = F32(0.0) if 'near margin dropped' in wrong else fmaf(F32(1.0e-5), np.abs(cw), F32(1.0e-3))
            near |= (cz + cw) < limit
            back = cw <= F32(1e-4)
            behind |= back
            front |= ~back
            rw = F32(1.0) / np.where(back, F32(1.0), cw)
            sx, sy = fmaf(cx * rw, hw, hw), fmaf(cy * rw, hh, hh)
            assert not (np.isnan(sx) | np.isnan(sy))[~back & rendered].any(), "fminf / fmaxf drop a NaN, numpy does not"
            sxlo = np.where(back, sxlo, np.minimum(sxlo, sx)); sxhi = np.where(back, sxhi, np.maximum(sxhi, sx))
            sylo = np.where(back, sylo, np.minimum(sylo, sy)); syhi = np.where(back, syhi, np.maximum(syhi, sy))
        m_lo = F32(0.5) if 'margin 0.5' in wrong else F32(1.5)
        m_hi = m_lo - F32(1.0)
        full = behind | near
        fx0, fx1 = np.maximum(np.floor(sxlo - m_lo), F32(0.0)), np.minimum(np.ceil(sxhi + m_hi), F32(W - 1))
        fy0, fy1 = np.maximum(np.floor(sylo - m_lo), F32(0.0)), np.minimum(np.ceil(syhi + m_hi), F32(H - 1))
        assert (np.abs(np.stack([fx0, fx1, fy0, fy1]))[:, front & rendered & ~full] < 2.0 ** 31).all(), "beyond what (int) converts"
        x0, x1 = np.where(full, 0, fx0.astype(np.int64)), np.where(full, W - 1, fx1.astype(np.int64))
        y0, y1 = np.where(full, 0, fy0.astype(np.int64)), np.where(full, H - 1, fy1.astype(np.int64))
        px = F32(k['COMPACT_PX'])
        ex, ey = sxhi - sxlo, syhi - sylo
        compact = ~full & ((ex < px) & (ey < px) if 'compact <' in wrong else (ex <= px) & (ey <= px))
    live = rendered & front & (x0 <= x1) & (y0 <= y1)
    if skip_shared:
        live &= link >= n_shared
    compact &= live
    boxes = np.tile(np.array(EMPTY_BOX, np.int16), (M, 1))
    words, n_tiles = mask_words_of(fp), tiles_x * tiles_y
    masks = np.zeros((2, words), np.uint32)
    tris, tris_lo = np.zeros(n_tiles, np.uint32), np.zeros(n_tiles, np.uint32)
    seam = 1 if 'tile seam off by one' in wrong else 0
    TW, TH = k['TILE_W'], k['TILE_H']
    for m in np.flatnonzero(live).tolist():
        boxes[m] = (int(x0[m]) | (0x4000 if compact[m] else 0) | (0x2000 if near[m] else 0), x1[m], y0[m], y1[m])
        tx0, tx1 = int(x0[m] + seam) // TW, min(int(x1[m] + seam) // TW, tiles_x - 1)
        if 'no y flip' in wrong:
            ty0, ty1 = int(y0[m]) // TH, int(y1[m]) // TH
        else:
            ty0, ty1 = int(H - 1 - y1[m]) // TH, int(H - 1 - y0[m]) // TH
        l = int(link[m])
        which = 0 if l < n_shared else 1
        if 'masks swapped' in wrong:
            which ^= 1
        for ty in range(ty0, ty1 + 1):
            for tx in range(tx0, tx1 + 1):
                t = ty * tiles_x + tx
                masks[which, t >> 5] |= np.uint32(1 << (t & 31))
                if l >= n_shared:
                    tris[t] += np.uint32(ntri[m])
                elif l >= lo_first:
                    tris_lo[t] += np.uint32(ntri[m])
    return dict(boxes=boxes, mask_lo=masks[0], mask_hi=masks[1], tris=tris, tris_lo=tris_lo, sxlo=sxlo, sxhi=sxhi, sylo=sylo, syhi=syhi,
                behind=behind, front=front, near=near, compact=compact, live=live)


WRONG_BOX = ('margin 0.5', 'no y flip', 'masks swapped', 'tile seam off by one', 'compact <', 'near margin dropped')


def same_boxes(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ('boxes', 'mask_lo', 'mask_hi', 'tris', 'tris_lo'))


def unpack(box):
    """(x0, x1, y0, y1, compact, near) of a stored box."""
    x0 = int(box[0]) & 0xFFFF
    return x0 & 0x1FFF, int(box[1]), int(box[2]), int(box[3]), bool(x0 & 0x4000), bool(x0 & 0x2000)


# ------------------------------------------------------------------------------------------------ the promises, in float64
# How far a float32 evaluation of a screen coordinate can lie from the float64 one.  Both meshlet_box and the rasteriser's vertex
# shading form it from the same operations: a coordinate x = ctr +- ext (one rounding, relative error <= u = 2^-24; a vertex is given
# exactly), a clip row c = fma(m0, x, fma(m1, y, fma(m2, z, m3))) (three roundings, each of a partial sum no larger in magnitude
# than S = |m0 x| + |m1 y| + |m2 z| + |m3|, up to a factor (1 + u)^2), rw = 1 / cw, q = cx * rw, sx = fma(q, hw, hw) (one
# rounding each).  So, to first order in u and with every higher-order term covered by writing 5 for 4 and 3 for 2:
#   |c32 - c| <= E = 5 u S                                         for each of the rows cx, cy, cz, cw,
#   |cx32 / cw32 - cx / cw| <= (Ex + |q| Ew) / (cw - Ew),          q = cx / cw,
#   |q32 - q| <= dq = (Ex + |q| Ew) / (cw - Ew) + 3 u (|q| + the same),
#   |sx32 - sx| <= hw dq + u (|sx| + hw dq),
# and the box adds the rounding of sxlo - 1.5f / sxhi + 0.5f: u (|sx| + 1.5).  slack = the sum of the last two lines, per corner; a
# meshlet's slack is the largest of its corners'.  The comparisons cw <= 1e-4f and cz + cw < fma(1e-5f, |cw|, 1e-3f) are decided
# the same way in float32 and float64 when they are clear of their thresholds by Ew, resp. by
#   Ez + Ew + u (|cz + cw| + Ez + Ew) + 1e-5 Ew + 2 u (1e-3 + 1e-5 |cw|);
# a meshlet with a corner inside those margins is "unsure": it is held to the conservative inequality only.
def project64(fp, mm, pts):
    """pts (..., 3) float64 under the float32 rows mm (..., 16) -> sx, sy, cz, cw, slack_x, slack_y, Ez, Ew (float64)."""
    W, H = fp[0], fp[1]
    hw, hh = 0.5 * W, 0.5 * H
    mm = np.asarray(mm, np.float64)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    row = lambda r: ((mm[..., 4 * r] * x + mm[..., 4 * r + 1] * y) + mm[..., 4 * r + 2] * z) + mm[..., 4 * r + 3]
    mag = lambda r: 5.0 * U * (np.abs(mm[..., 4 * r] * x) + np.abs(mm[..., 4 * r + 1] * y) + np.abs(mm[..., 4 * r + 2] * z) + np.abs(mm[..., 4 * r + 3]))
    cx, cy, cz, cw = (row(r) for r in range(4))
    Ex, Ey, Ez, Ew = (mag(r) for r in range(4))
    with np.errstate(all='ignore'):
        out = []
        for cc, Ec, half in ((cx, Ex, hw), (cy, Ey, hh)):
            q = cc / cw
            s = q * half + half
            base = (Ec + np.abs(q) * Ew) / (cw - Ew)
            dq = base + 3.0 * U * (np.abs(q) + base)
            out += [s, half * dq + U * (np.abs(s) + half * dq) + U * (np.abs(s) + 1.5)]
    return out[0], out[2], cz, cw, out[1], out[3], Ez, Ew


EYE = float(F32(1e-4))


def box_bounds64(fp, header, aabb, mvp6, n_render):
    """Per meshlet, from the eight corners in float64: lo / hi of sx and sy over the corners in front, the slack, and the class —
    'unrendered' (link >= n_render), 'none in front' (every corner surely at w <= 1e-4), 'behind' (a corner surely at w <= 1e-4 and
    one surely in front), 'near' (all surely in front, one surely inside the near margin), 'plain' (all surely in front, all surely
    outside the margin), 'unsure' (a comparison within float32 rounding of its threshold)."""
    header = np.asarray(header, np.uint32).reshape(-1, 8)
    aabb = np.asarray(aabb, F32).reshape(-1, 8).astype(np.float64)
    M = len(header)
    link = header[:, 7].astype(np.int64)
    rendered = link < n_render
    mm = np.asarray(mvp6, F32).reshape(-1, 16)[np.where(rendered, link, 0)][:, None, :]
    sign = np.array([[(1 if c & 1 else -1), (1 if c & 2 else -1), (1 if c & 4 else -1)] for c in range(8)], np.float64)
    pts = aabb[:, None, 0:3] + sign[None] * aabb[:, None, 4:7]
    sx, sy, cz, cw, slx, sly, Ez, Ew = project64(fp, mm, pts)
    sure_front, sure_back = cw - Ew > EYE * (1 + U), cw + Ew < EYE * (1 - U)
    thr = 1.0e-3 + 1.0e-5 * np.abs(cw)
    marg = Ez + Ew + U * (np.abs(cz + cw) + Ez + Ew) + 1.0e-5 * Ew + 2 * U * thr + 1.0e-3 * 2 * U      # the last: 1e-3f and 1e-5f are not 1e-3, 1e-5
    sure_near, sure_far = (cz + cw) + marg < thr, (cz + cw) - marg > thr
    cls = np.full(M, 'unsure', object)
    cls[sure_back.all(1)] = 'none in front'
    cls[sure_back.any(1) & sure_front.any(1) & (sure_back | sure_front).all(1)] = 'behind'
    cls[sure_front.all(1) & sure_near.any(1)] = 'near'
    cls[sure_front.all(1) & sure_far.all(1)] = 'plain'
    cls[~rendered] = 'unrendered'
    with np.errstate(all='ignore'):
        f = sure_front
        lo_x, hi_x = np.where(f, sx, np.inf).min(1), np.where(f, sx, -np.inf).max(1)
        lo_y, hi_y = np.where(f, sy, np.inf).min(1), np.where(f, sy, -np.inf).max(1)
        slack = np.maximum(np.where(f, slx, 0.0).max(1), np.where(f, sly, 0.0).max(1))
    near = np.where(sure_near.any(1), 1, np.where(sure_far.all(1), 0, -1))               # every corner takes part, in front or not
    return dict(cls=cls, lo_x=lo_x, hi_x=hi_x, lo_y=lo_y, hi_y=hi_y, slack=slack, near=near)


SNAP = 1.0 / 512.0                                       # vertices are snapped to 1/256 px: half a step either way


def sample_range(lo, hi, slack, size):
    """The sample columns p a primitive between lo and hi (float64) can cover under any float32 evaluation: centre p + 0.5 inside
    the snapped extent -> (first, last), clamped to the frame; first > last: none."""
    return max(0, math.ceil(lo - slack - 0.5 - SNAP)), min(size - 1, math.floor(hi + slack - 0.5 + SNAP))


def check_boxes(fp, boxes, b64, who='', not_drawn=None):
    """Stored boxes (M, 4) against box_bounds64's record -> list of violations, each naming the meshlet, the promise and both values.
    not_drawn: meshlets of shared links of a candidate that is not its layer's representative — bounds_kernel stores them empty."""
    W, H = fp[0], fp[1]
    px = constants()['COMPACT_PX']
    bad = []
    for m, cls in enumerate(b64['cls'].tolist()):
        x0, x1, y0, y1, compact, near = unpack(boxes[m])
        empty = x0 > x1
        say = lambda what, got, want: bad.append(f"{who}meshlet {m} ({cls}): {what}: stored {got}, float64 asks {want}")
        if cls in ('unrendered', 'none in front') or (not_drawn is not None and not_drawn[m]):
            if tuple(int(v) for v in boxes[m]) != EMPTY_BOX:
                say('not drawn, box must be empty', tuple(boxes[m]), EMPTY_BOX)
            continue
        if cls in ('behind', 'near'):
            n13 = int(b64['near'][m])                   # 1: a corner surely inside the near margin, 0: all surely outside, -1: unsure
            if (x0, x1, y0, y1) != (0, W - 1, 0, H - 1) or compact or (n13 >= 0 and near != bool(n13)):
                say('whole frame, not compact, bit 13', (x0, x1, y0, y1, compact, near), (0, W - 1, 0, H - 1, False, n13))
            continue
        if not np.isfinite(b64['lo_x'][m]):
            continue                                    # unsure, and not one corner surely in front: nothing to hold it to
        s = float(b64['slack'][m])
        cols, rows = sample_range(b64['lo_x'][m], b64['hi_x'][m], s, W), sample_range(b64['lo_y'][m], b64['hi_y'][m], s, H)
        if empty:
            if tuple(int(v) for v in boxes[m]) != EMPTY_BOX:
                say('an empty box is stored as', tuple(boxes[m]), EMPTY_BOX)
            if cols[0] <= cols[1] and rows[0] <= rows[1]:
                say('conservative: empty box, but samples', 'none', (cols, rows))
            continue
        if cols[0] <= cols[1] and (x0 > cols[0] or x1 < cols[1]):
            say('conservative in x', (x0, x1), cols)
        if rows[0] <= rows[1] and (y0 > rows[0] or y1 < rows[1]):
            say('conservative in y', (y0, y1), rows)
        if cls != 'plain':
            continue
        if near:
            say('bit 13', near, False)
        if True:
            # no more than one pixel outside floor(lo - 1.5) / ceil(hi + 0.5); the pixel is what a slack of at most 1 can cost
            want = (max(0, math.floor(b64['lo_x'][m] - 1.5) - 1), min(W - 1, math.ceil(b64['hi_x'][m] + 0.5) + 1),
                    max(0, math.floor(b64['lo_y'][m] - 1.5) - 1), min(H - 1, math.ceil(b64['hi_y'][m] + 0.5) + 1))
            if not s <= 1.0 or x0 < want[0] or x1 > want[1] or y0 < want[2] or y1 > want[3]:
                say(f'tight (slack {s:.3g})', (x0, x1, y0, y1), want)
        ext = max(b64['hi_x'][m] - b64['lo_x'][m], b64['hi_y'][m] - b64['lo_y'][m])       # each end is off by at most the slack
        if compact and ext > px + 2 * s:
            say('bit 14 on a meshlet larger than COMPACT_PX', ext, px)
        if not compact and ext <= px - 2 * s:
            say('bit 14 missing', ext, px)
    return bad


def check_masks(fp, boxes, header, n_shared, mask_lo, mask_hi, who=''):
    """Every tile a stored box reaches has its bit in the mask of the box's link group, and no other bit is set -> violations."""
    k = constants()
    W, H, tiles_x, tiles_y = fp
    want = np.zeros((2, mask_words_of(fp)), np.uint32)
    for m in range(len(boxes)):
        x0, x1, y0, y1, _, _ = unpack(boxes[m])
        if x0 > x1:
            continue
        g = 0 if int(header[m][7]) < n_shared else 1
        for ty in range((H - 1 - y1) // k['TILE_H'], (H - 1 - y0) // k['TILE_H'] + 1):
            for tx in range(x0 // k['TILE_W'], x1 // k['TILE_W'] + 1):
                t = ty * tiles_x + tx
                want[g, t >> 5] |= np.uint32(1 << (t & 31))
    bad = []
    for g, got in enumerate((mask_lo, mask_hi)):
        for w in np.flatnonzero(np.asarray(got) != want[g]).tolist():
            bad.append(f"{who}mask_{'lo' if g == 0 else 'hi'} word {w}: stored {int(got[w]):#010x}, the boxes ask {int(want[g, w]):#010x}")
    return bad


def check_vertices(fp, boxes, header, verts, mvp6, n_render, n_shared, mask_lo, mask_hi, who=''):
    """The real robot: every vertex of every rendered meshlet, projected in float64 under the float32 link matrices.  A vertex with
    z + w < 0 forces bit 13 and the whole frame (unless no corner of the meshlet is in front: empty box); every other lies inside its
    meshlet's box by the conservative inequality and, on screen, its tile has the bit of its link group.  -> (violations, counts)."""
    k = constants()
    W, H, tiles_x, tiles_y = fp
    bad, seen = [], dict(vertices=0, near=0, inside=0, on_screen=0)
    header = np.asarray(header, np.uint32).reshape(-1, 8)
    mvp6 = np.asarray(mvp6, F32).reshape(-1, 16)
    for m in range(len(header)):
        l = int(header[m, 7])
        if l >= n_render:
            continue
        v0, nv = int(header[m, 4]), int(header[m, 6] & 0xFFFF)
        sx, sy, cz, cw, slx, sly, Ez, Ew = project64(fp, mvp6[l][None, :], verts[v0:v0 + nv].astype(np.float64))
        x0, x1, y0, y1, compact, near = unpack(boxes[m])
        seen['vertices'] += nv
        behind_near = (cz + cw) < 0.0
        if behind_near.any():
            seen['near'] += 1
            # |z32 + w32 - (z + w)| <= Ez + Ew + u |z + w| is some 1e-6 here, the margin 1e-3: a corner of the box (z + w is affine, the
            # box holds the vertex) is below the threshold in float32 whenever a vertex is below 0 in float64
            assert float((Ez + Ew).max()) < 1.0e-4
            if tuple(int(v) for v in boxes[m]) != EMPTY_BOX and ((x0, x1, y0, y1) != (0, W - 1, 0, H - 1) or not near or compact):
                bad.append(f"{who}meshlet {m} link {l}: vertex {int(np.argmax(behind_near))} has z + w = {float((cz + cw)[behind_near][0]):.6g} < 0, "
                           f"box {(x0, x1, y0, y1)} compact {compact} near {near}")
        for i in np.flatnonzero(~behind_near & (cw > EYE)).tolist():
            # a point covers a sample centre only by chance: the two inequalities are held one by one (first may exceed last by 1)
            cols, rows = sample_range(sx[i], sx[i], float(slx[i]), W), sample_range(sy[i], sy[i], float(sly[i]), H)
            if cols[0] > W - 1 or cols[1] < 0 or rows[0] > H - 1 or rows[1] < 0:
                continue                                # off the frame
            seen['inside'] += 1
            if x0 > x1 or x0 > cols[0] or x1 < cols[1] or y0 > rows[0] or y1 < rows[1]:
                bad.append(f"{who}meshlet {m} link {l} vertex {i} at ({sx[i]:.4f}, {sy[i]:.4f}): samples {cols} x {rows} outside box {(x0, x1, y0, y1)}")
                continue
            px, py = math.floor(sx[i]), math.floor(sy[i])
            if 0 <= px < W and 0 <= py < H:
                seen['on_screen'] += 1
                t = ((H - 1 - py) // k['TILE_H']) * tiles_x + px // k['TILE_W']
                mask = mask_lo if l < n_shared else mask_hi
                if not (int(mask[t >> 5]) >> (t & 31)) & 1:
                    bad.append(f"{who}meshlet {m} link {l} vertex {i} at pixel ({px}, {py}): tile {t} missing in mask_{'lo' if l < n_shared else 'hi'} "
                               f"word {t >> 5} = {int(mask[t >> 5]):#010x}")
    return bad, seen


def robot_tables(rb):
    """The real robot's meshlet tables as rope_set_robot hands them to the kernels: header, vertices and the link-frame boxes
    (centre and half extent rounded outwards, by rope_set_robot's formula)."""
    ml = rb.meshlets
    aabb = np.zeros((len(ml.header), 8), F32)
    for m, h in enumerate(ml.header):
        v = ml.verts[int(h[4]):int(h[4]) + int(h[6] & 0xFFFF)].astype(np.float64)
        lo, hi = v.min(0), v.max(0)
        ctr = (0.5 * (lo + hi)).astype(F32)
        aabb[m, 0:3] = ctr
        aabb[m, 4:7] = (np.maximum(hi - ctr.astype(np.float64), ctr.astype(np.float64) - lo) * (1.0 + 1e-6) + 1e-7).astype(F32)
    return np.ascontiguousarray(ml.header, np.uint32), aabb, np.ascontiguousarray(ml.verts, F32)


# ------------------------------------------------------------------------------------------------ synthetic meshlet tables
# Link-frame boxes under matrices the builder chooses.  'flat' matrices: cw = 1, cz = 0 (far from both planes), cx = x - 1 + shift,
# cy = y - 1, so that a link-frame unit is half a frame and a coordinate X / hw that is a dyadic number lands on pixel X exactly:
# sx = fma(X / hw - 1, hw, hw) = X.  'deep' matrices: cw = z, cz = z - 0.02 (near plane at 1 cm: z + w = 2 z - 0.02), cx = x - z,
# cy = y - z, so that sx = (x / z) hw.  Links 0-2 are flat, link 3 is flat and shifted by 3 px, link 4 is deep, link 5 is 'eye':
# as deep but with cz = 5, which never comes near the near plane, for boxes that straddle the eye plane alone.
def link_matrices(fp, cand):
    """(6, 16) float32 of candidate `cand`: every candidate is shifted by 7 px in x against the one before."""
    W = fp[0]
    mm = np.zeros((6, 16), F32)
    for l in range(6):
        shift = (7.0 * cand + (3.0 if l == 3 else 0.0)) / (0.5 * W)
        if l < 4:
            mm[l] = [1, 0, 0, -1 + shift, 0, 1, 0, -1, 0, 0, 0, 0, 0, 0, 0, 1]
        else:
            mm[l] = [1, 0, -1 + shift, 0, 0, 1, -1, 0, 0, 0, (1 if l == 4 else 0), (-0.02 if l == 4 else 5), 0, 0, 1, 0]
    return mm


def pix_box(fp, X0, X1, Y0, Y1, z=0.0, ez=0.0):
    """aabb row of the link-frame box that a flat link puts on [X0, X1] x [Y0, Y1] px (a deep one at z = 1)."""
    hw, hh = 0.5 * fp[0], 0.5 * fp[1]
    return np.array([(X0 + X1) / (2 * hw), (Y0 + Y1) / (2 * hh), z, 0, (X1 - X0) / (2 * hw), (Y1 - Y0) / (2 * hh), ez, 0], F32)


def _search_f32(lo, hi, pred):
    """Smallest float32 in (lo, hi] for which the monotone pred holds (pred(lo) false, pred(hi) true), by bisecting the bit patterns."""
    a, b = int(F32(lo).view(np.uint32)), int(F32(hi).view(np.uint32))
    assert 0 < a < b < 0x7F800000 and not pred(np.uint32(a).view(F32)) and pred(np.uint32(b).view(F32))
    while b - a > 1:
        mid = (a + b) // 2
        if pred(np.uint32(mid).view(F32)):
            b = mid
        else:
            a = mid
    return np.uint32(b).view(F32)


def _one(fp, row, link):
    """box_exact's record of a single meshlet of `link` under candidate 0."""
    hdr = np.array([[0, 0, 0, 0, 0, 0, 1 << 16, link]], np.uint32)
    return box_exact(fp, hdr, row[None], link_matrices(fp, 0), 6, 0)


@functools.lru_cache(maxsize=None)
def compact_rows(W, H):
    """Boxes whose extent is the largest the frame's float32 coordinates reach that is not above COMPACT_PX ('at': COMPACT_PX itself
    when the half size is a power of two) and the smallest extent above it that the frame's float32 coordinates reach
    ('over'), in x only, in y only and in both — from the frame's corner, where screen coordinates are finest: with a half size that is
    a power of two 'over' is the very next float32 after COMPACT_PX, otherwise the steps of q = x - 1 near -1 (2^-24, doubled by the
    box's 2 a) times the half size are wider than that: 'over' lies within half * 2^-22 of COMPACT_PX.  -> [(name, aabb row, (0 at / 1 over / None in x, the same in y))]"""
    fp, px = frame(W, H), float(constants()['COMPACT_PX'])
    half = {}
    for axis, size in ((0, W), (1, H)):
        def row_of(a, axis=axis):
            r = np.zeros(8, F32)
            r[axis] = r[4 + axis] = a                   # from 0 to 2 a
            r[1 - axis] = r[5 - axis] = F32(10.0 / (0.5 * (H if axis == 0 else W)))  # 20 px the other way
            return r
        extent = lambda a, axis=axis: float((_one(fp, row_of(a), 0)['sxhi' if axis == 0 else 'syhi'] - _one(fp, row_of(a), 0)['sxlo' if axis == 0 else 'sylo'])[0])
        first_over = _search_f32(0.25 * px / (0.5 * size), 2.0 * px / (0.5 * size), lambda a: extent(a) > px)
        last_at = np.nextafter(first_over, F32(0.0))
        half[axis] = (last_at, first_over)
    rows = []
    for name, ix, iy in (('x at', 0, None), ('x over', 1, None), ('y at', None, 0), ('y over', None, 1), ('both at', 0, 0), ('x over y at', 1, 0),
                         ('x at y over', 0, 1)):
        r = np.zeros(8, F32)
        r[0] = r[4] = half[0][ix] if ix is not None else F32(10.0 / (0.5 * W))
        r[1] = r[5] = half[1][iy] if iy is not None else F32(10.0 / (0.5 * H))
        rows.append(('compact ' + name, r, (ix, iy)))
    return rows


@functools.lru_cache(maxsize=None)
def near_rows(W, H):
    """Flat-in-z boxes of the deep link 4 whose depth is the last float32 inside the near margin and the first outside it."""
    fp = frame(W, H)
    row_of = lambda z: np.array([0.01, 0.01, z, 0, 0.002, 0.002, 0, 0], F32)
    outside = _search_f32(0.0102, 0.011, lambda z: not _one(fp, row_of(z), 4)['near'][0])
    return [('near: last inside the margin', row_of(np.nextafter(outside, F32(0.0)))), ('near: first outside the margin', row_of(outside))]


def edge_rows(W, H):
    """[(name, link, aabb row)]: every edge of the list in the module's test, for this frame."""
    k = constants()
    fp = frame(W, H)
    TW, TH, tiles_x, tiles_y = k['TILE_W'], k['TILE_H'], fp[2], fp[3]
    out = []
    add = lambda name, link, row: out.append((name, link, np.asarray(row, F32)))
    midx, midy = min(W, TW) / 2, H - min(H, TH) / 2                              # inside tile (0, 0): the TOP rows of the window
    add('plain', 0, pix_box(fp, midx - 8, midx + 8, midy - 6, midy + 6))
    # columns: x1 = ceil(sxhi + 0.5), x0 = floor(sxlo - 1.5); rows: the tile rows count from the top, window y from the bottom
    x_seams = sorted({TW * t for t in (1, 2, 3, 4, tiles_x - 1) if 0 < t < tiles_x})
    y_seams = sorted({H - TH * t for t in (1, 3, 4, 6, 7, tiles_y - 1) if 0 < t < tiles_y})    # window row y = seam is the lowest row of the tile above
    for sx_ in x_seams:
        for ys in ([midy] + [s + TH / 2 for s in y_seams if s + TH / 2 < H][:6]):
            add(f'x1 on the last column before seam {sx_}', 1, pix_box(fp, sx_ - 20, sx_ - 1.75, ys - 4, ys + 4))
            add(f'x1 one past seam {sx_}', 1, pix_box(fp, sx_ - 20, sx_ - 0.75, ys - 4, ys + 4))
            add(f'x0 on seam {sx_}', 3, pix_box(fp, sx_ + 1.75 - 3, sx_ + 20, ys - 4, ys + 4))       # link 3 is shifted by 3 px
            add(f'x0 one before seam {sx_}', 3, pix_box(fp, sx_ + 0.75 - 3, sx_ + 20, ys - 4, ys + 4))
    for sy_ in y_seams:
        add(f'y0 on the lowest row above seam {sy_}', 2, pix_box(fp, midx - 5, midx + 5, sy_ + 1.75, sy_ + 12))
        add(f'y0 one below seam {sy_}', 2, pix_box(fp, midx - 5, midx + 5, sy_ + 0.75, sy_ + 12))
        add(f'y1 on the highest row below seam {sy_}', 0, pix_box(fp, midx - 5, midx + 5, sy_ - 12, sy_ - 1.75))
        add(f'y1 one above seam {sy_}', 0, pix_box(fp, midx - 5, midx + 5, sy_ - 12, sy_ - 0.75))
    add('clamped at column 0', 0, pix_box(fp, -10, 6, midy - 3, midy + 3))
    add('clamped at column W - 1', 1, pix_box(fp, W - 6, W + 10, midy - 3, midy + 3))
    add('clamped at row 0', 2, pix_box(fp, midx - 3, midx + 3, -10, 6))
    add('clamped at row H - 1', 0, pix_box(fp, midx - 3, midx + 3, H - 6, H + 10))
    add('off the left', 0, pix_box(fp, -30, -3, midy - 3, midy + 3))
    add('off the right', 1, pix_box(fp, W + 3, W + 30, midy - 3, midy + 3))
    add('off the bottom', 2, pix_box(fp, midx - 3, midx + 3, -30, -3))
    add('off the top', 0, pix_box(fp, midx - 3, midx + 3, H + 3, H + 30))
    add('off the left by the margin alone: x1 = -1', 0, pix_box(fp, -30, -1.75, midy - 3, midy + 3))
    add('on column 0 by the margin alone: x1 = 0', 0, pix_box(fp, -30, -0.75, midy - 3, midy + 3))
    add('off the right by the margin alone: x0 = W', 1, pix_box(fp, W + 1.75, W + 30, midy - 3, midy + 3))
    add('on column W - 1 by the margin alone', 1, pix_box(fp, W + 0.25, W + 30, midy - 3, midy + 3))
    add('the whole frame and more', 2, pix_box(fp, -50, W + 50, -50, H + 50))
    px = k['COMPACT_PX']
    dyadic = lambda v, half: (lambda d: d & (d - 1) == 0)(Fraction(int(v), int(half)).denominator)
    if W >= 4 * px and H >= 4 * px and W % 2 == 0 and H % 2 == 0 and all(dyadic(v, W // 2) for v in (170, 170 + px, 175 + px, 190)) \
            and all(dyadic(v, H // 2) for v in (165, 165 + 15, 165 + px)):               # on exact pixels: extents of exactly COMPACT_PX
        add('extent exactly COMPACT_PX in x, inside', 0, pix_box(fp, 170, 170 + px, 165, 165 + 15))
        add('extent exactly COMPACT_PX in y, inside', 1, pix_box(fp, 170, 170 + 20, 165, 165 + px))
        add('extent exactly COMPACT_PX both ways, inside', 2, pix_box(fp, 170, 170 + px, 165, 165 + px))
        add('extent COMPACT_PX + 5 in x, inside', 0, pix_box(fp, 170, 175 + px, 165, 165 + 15))
    for name, row, _ in compact_rows(W, H):
        add(name, 0, row)
    for name, row in near_rows(W, H):
        add(name, 4, row)
    add('deep, clear of both planes', 4, np.array([0.5, 0.5, 1.0, 0, 0.05, 0.05, 0.25, 0], F32))
    add('deep, well inside the near margin', 4, np.array([0.004, 0.004, 0.0101, 0, 0.001, 0.001, 0.00005, 0], F32))
    add('straddles the eye plane and the near plane', 4, np.array([0.1, 0.1, 0.0, 0, 0.05, 0.05, 0.5, 0], F32))
    add('straddles the eye plane alone', 5, np.array([0.1, 0.1, 0.0, 0, 0.05, 0.05, 0.5, 0], F32))
    add('every corner behind the eye', 5, np.array([0.1, 0.1, -1.0, 0, 0.05, 0.05, 0.5, 0], F32))
    add('every corner at w = 1e-4f exactly', 5, np.array([0.0, 0.0, F32(1e-4), 0, 0.00001, 0.00001, 0, 0], F32))
    add('every corner at the float above w = 1e-4f', 5, np.array([0.00005, 0.00005, np.nextafter(F32(1e-4), F32(1)), 0, 0.00001, 0.00001, 0, 0], F32))
    add('clear of the eye plane, no near plane', 5, np.array([0.5, 0.5, 1.0, 0, 0.05, 0.05, 0.25, 0], F32))
    return out


@functools.lru_cache(maxsize=None)
def meshlet_table(W, H, M, seed=0):
    """-> (names, header (M, 8) uint32, aabb (M, 8) float32): the frame's edge rows first (as many as fit), then boxes of 4 to 90 px
    anywhere in and a little around the frame, on every link, flat and deep; triangle counts 1 .. 128, vertex counts in the low half-word."""
    fp = frame(W, H)
    rng = np.random.default_rng(1000 * W + M + seed)
    edges = edge_rows(W, H)
    names, links, rows = [], [], []
    for name, link, row in edges[:M]:
        names.append(name); links.append(link); rows.append(row)
    while len(rows) < M:
        link = int(rng.integers(0, 6))
        w, h = rng.uniform(4, 90, 2)
        X, Y = rng.uniform(-40, W + 40 - w), rng.uniform(-40, H + 40 - h)
        if link < 4:
            row = pix_box(fp, X, X + w, Y, Y + h)
        else:
            z = rng.uniform(0.2, 2.0)
            row = pix_box(fp, X * z, (X + w) * z, Y * z, (Y + h) * z, z, rng.uniform(0, 0.1) * z)
        names.append('filler'); links.append(link); rows.append(row)
    header = np.zeros((M, 8), np.uint32)
    header[:, 0:4] = 0xA5A5A5A5                                                  # centre and radius: no kernel of this group reads them
    header[:, 6] = (rng.integers(1, 129, M).astype(np.uint32) << 16) | rng.integers(1, 65, M).astype(np.uint32)
    header[:, 7] = links
    return names, header, np.ascontiguousarray(np.stack(rows), F32)


# (W, H, meshlets, candidates, n_render, n_shared, lo_first, layers): every frame, count and argument of the list, crossed sparingly
GEOMETRY_CASES = [
    (128, 96, 1, 1, 6, 0, 0, False),
    (128, 96, 255, 1, 6, 3, 0, False),
    (128, 96, 256, 3, 4, 3, 2, True),
    (160, 120, 256, 3, 6, 3, 2, True),
    (160, 120, 257, 1, 6, 6, 0, False),
    (160, 120, 255, 3, 4, 0, 0, False),
    (640, 480, 257, 3, 6, 3, 0, True),
    (640, 480, 1025, 1, 4, 6, 2, False),
    (1280, 720, 1025, 3, 6, 3, 2, True),
    (1280, 720, 257, 1, 6, 0, 0, False),
]
LAYER_OF, LAYER_REP = (0, 0, 1), (0, 2)                  # three candidates: 0 represents layer 0, 1 shares it, 2 represents layer 1


@functools.lru_cache(maxsize=None)
def geometry_case(W, H, M, C, n_render, n_shared, lo_first, layers):
    """-> dict: fp, names, header, aabb, mvp (C, 6, 16), and per candidate box_exact's record (`want`) and box_bounds64's (`b64`)."""
    fp = frame(W, H)
    names, header, aabb = meshlet_table(W, H, M)
    mvp = np.stack([link_matrices(fp, c) for c in range(C)])
    want, b64 = [], []
    for c in range(C):
        skip = layers and n_shared > 0 and LAYER_REP[LAYER_OF[c]] != c
        want.append(box_exact(fp, header, aabb, mvp[c], n_render, n_shared, lo_first, skip))
        b64.append(box_bounds64(fp, header, aabb, mvp[c], n_render))
    return dict(fp=fp, names=names, header=header, aabb=aabb, mvp=mvp, want=want, b64=b64, C=C, n_render=n_render, n_shared=n_shared,
                lo_first=lo_first, layers=layers)


# ------------------------------------------------------------------------------------------------ finalize
def argmin(vals):
    """First index of the smallest; a NaN never beats a number; all NaN: index 0."""
    best, bi = None, 0
    for i, v in enumerate(np.asarray(vals, np.float64).tolist()):
        if v != v:
            continue
        if best is None or v < best:
            best, bi = v, i
    return bi


def argmin_last(vals):
    """The deliberate mistake: the LAST index of the smallest."""
    best, bi = None, 0
    for i, v in enumerate(np.asarray(vals, np.float64).tolist()):
        if v == v and (best is None or v <= best):
            best, bi = v, i
    return bi


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def finalize_ref(sums, total_empty, loss, n_render, n_pix, flags, wrong=()):
    """finalize_one on rows of sums (C, SUM_WORDS) uint64.  total_empty (SUM_WORDS,) or one row per row of sums; flags (8,) or one
    row per row of sums.  -> (errors (C,) float64, the words written back (C, SUM_WORDS) uint64)."""
    k = constants()
    n_words, FULL, LOOKUP, TSWEEP = k['SUM_WORDS'], k['LOSS_FULL'], k['LOSS_LOOKUP'], k['LOSS_TSWEEP']
    sums = np.asarray(sums, np.uint64).reshape(-1, n_words)
    C = len(sums)
    total = np.broadcast_to(np.asarray(total_empty, np.uint64).reshape(-1, n_words), (C, n_words))
    flags = np.broadcast_to(np.asarray(flags, np.uint8).reshape(-1, 8), (C, 8))
    live = [w < SUM_LINK0 or (loss == FULL and w < SUM_LINK0 + 3 * n_render) or 'unrendered words kept' in wrong for w in range(n_words)]
    rows = [[(int(sums[c, w]) + int(total[c, w])) & M64 if live[w] else 0 for w in range(n_words)] for c in range(C)]
    words = np.array(rows, np.uint64).reshape(C, n_words)
    # uint64 -> double is one correctly rounded conversion on both sides (Python's int -> float rounds to nearest even)
    f64 = lambda w: np.array([float(r[w]) for r in rows], np.float64)
    N = np.float64(n_pix)
    with np.errstate(all='ignore'):
        m1 = (f64(SUM_S1) * 2.0 ** -32) / N
        S2 = (f64(SUM_AA) * 2.0 ** 40 + f64(SUM_AB) * 2.0 ** 21) + f64(SUM_BB)
        m2 = (S2 * 2.0 ** -64) / N
        var = m2 - m1 * m1
        var = np.where(var < 0.0, 0.0, var)
        sd = np.sqrt(var)
        if loss == LOOKUP:
            return m1 * sd, words
        if loss == TSWEEP:
            return m1 * -sd, words
        e = np.zeros(C, np.float64)
        if loss == FULL:
            for l in range(1, n_render):
                on = (flags[:, l] & 1) != 0
                e = np.where(on, e + (f64(SUM_LINK0 + 3 * l) / N) * 5.0, e)
                depth = on & (((flags[:, l] & 2) != 0) | ('flag bit 2 ignored' in wrong)) & (words[:, SUM_LINK0 + 3 * l + 1] > 0)
                e = np.where(depth, e + ((f64(SUM_LINK0 + 3 * l + 2) * 2.0 ** -32) / f64(SUM_LINK0 + 3 * l + 1)) * 10.0, e)
        meanD = (f64(SUM_S1) * 2.0 ** -32) / f64(SUM_CNT)
        return e + meanD * sd, words


WRONG_FINALIZE = ('unrendered words kept', 'flag bit 2 ignored')


def finalize_sizes():
    """Either side of every row count at which launch_finalize changes its launch (rope_kernels.hip: 64 / 256 / 1024 threads at
    C <= 64 / <= 256 / more; C > 2048: finalize_only_kernel in front and the argmin block only reduces), read out of its source —
    and 1, 255, 256, 257, 1025 in any case."""
    with open(os.path.join(ROOT, 'rope_s3d_amd', 'csrc', 'rope_kernels.hip')) as f:
        text = f.read()
    body = text[text.index('hipError_t launch_finalize('):text.index('hipError_t launch_finalize_frames(')]
    seams = sorted({int(v) for v in re.findall(r'C\s*(?:<=|>)\s*(\d+)', body)})
    assert seams, body
    return sorted({1, 255, 256, 257, 1025} | {s for v in seams for s in (v, v + 1)}), seams


@functools.lru_cache(maxsize=None)
def negative_variance_row(n_pix):
    """(n, dq): n samples that all have the Q32 value dq give m2 == m1^2 in exact arithmetic; these are the first of a fixed sequence
    for which float64 rounds m2 - m1 * m1 below zero (the var < 0 clamp)."""
    rng = np.random.default_rng(5)
    N = np.float64(n_pix)
    for _ in range(10000):
        n, dq = n_pix, int(rng.integers(1 << 28, 1 << 36))            # every sample of the frame drawn, all at the same value
        a, b = dq >> 20, dq & 0xFFFFF
        m1 = (np.float64(float(n * dq)) * np.float64(2.0 ** -32)) / N
        S2 = (np.float64(float(n * a * a)) * np.float64(2.0 ** 40) + np.float64(float(n * a * b)) * np.float64(2.0 ** 21)) + np.float64(float(n * b * b))
        if (S2 * np.float64(2.0 ** -64)) / N - m1 * m1 < 0.0:
            return n, dq
    raise AssertionError("no row with a negative rounded variance")


def _final_rows(C, n_pix, rng):
    """Plausible FINAL sums (after total_empty): C x SUM_WORDS Python-int rows with a positive variance."""
    n_words, n_links = constants()['SUM_WORDS'], constants()['MAX_LINKS']
    rows = []
    for _ in range(C):
        n = int(rng.integers(1, n_pix + 1))
        r = [0] * n_words
        r[SUM_CNT] = n
        dqs = [int(v) for v in rng.integers(1 << 20, 1 << 34, 3)]
        parts = [n // 3, n // 3, n - 2 * (n // 3)]
        for cnt, dq in zip(parts, dqs):
            a, b = dq >> 20, dq & 0xFFFFF
            r[SUM_S1] += cnt * dq; r[SUM_AA] += cnt * a * a; r[SUM_AB] += cnt * a * b; r[SUM_BB] += cnt * b * b
        for l in range(n_links):
            r[SUM_LINK0 + 3 * l] = int(rng.integers(0, n_pix))
            r[SUM_LINK0 + 3 * l + 1] = int(rng.integers(1, n_pix))
            r[SUM_LINK0 + 3 * l + 2] = int(rng.integers(0, 1 << 50))
        rows.append(r)
    return rows


PLACEMENTS = ('as drawn', 'tie first and last', 'minimum last', 'tie across the first wave seam', 'tie inside one thread', 'nan first', 'nan last',
              'nan at the wave seam', 'all nan', 'count 0 with s1 > 0', 'link count 0 with flag 3', 'negative variance', 'all rows wrap')
FLAG_SETS = {'none': (0, 0, 0, 0, 0, 0, 0, 0), 'mask': (1, 1, 1, 1, 1, 1, 0, 0), 'mask and depth': (3, 3, 3, 3, 3, 3, 0, 0),
             'mixed': (3, 0, 1, 3, 1, 3, 0, 0)}


@functools.lru_cache(maxsize=None)
def finalize_case(C, loss, n_render, flag_set, placement, n_pix=307200):
    """-> dict: sums (C, SUM_WORDS) uint64 as the raster kernels would leave them (before total_empty), total, flags, and the
    reference's err, words, best.  Every row's final sums are chosen first and total_empty subtracted modulo 2^64, so rows whose
    final word is smaller than the total's wrap (`wraps`: how many words do).  `placement` puts chosen rows at chosen indices."""
    k = constants()
    n_words = k['SUM_WORDS']
    rng = np.random.default_rng(C * 131 + loss * 17 + n_render + len(flag_set) + len(placement) * 7)
    flags = np.array(FLAG_SETS[flag_set], np.uint8)
    rows = _final_rows(C, n_pix, rng)
    total = [int(v) for v in rng.integers(1, 1 << 40, n_words)]
    if placement == 'all rows wrap':
        total = [max(total[w], max(r[w] for r in rows) + 1 + w) for w in range(n_words)]             # every final word below the total's
    nan_row = [0] * n_words                                                     # 0 / 0 in meanD (losses with a count)
    err0, _ = finalize_ref(np.array(rows, np.uint64), np.zeros(n_words, np.uint64), loss, n_render, n_pix, flags)
    b = argmin(err0)
    spot = {}

    def put(indices):
        row = rows[b]
        rows[b] = list(rows[(b + 1) % C]) if C > 1 else row
        for i in indices:
            rows[i] = list(row)
        spot['want_best'], spot['at'] = min(indices), sorted(set(indices))

    wave = 64
    if placement == 'tie first and last':
        put([0, C - 1])
    elif placement == 'minimum last':
        put([C - 1])
    elif placement == 'tie across the first wave seam':
        put([min(wave - 1, C - 1), min(wave, C - 1)])
    elif placement == 'tie inside one thread':                                   # i and i + the workgroup's size: the same thread's loop
        group = 64 if C <= 64 else 256 if C <= 256 else 1024
        put([min(C - 1, 5), min(C - 1, 5 + group)] if C > group else [min(C - 1, 5), C - 1])
    elif placement == 'nan first':
        rows[0] = list(nan_row)
    elif placement == 'nan last':
        rows[C - 1] = list(nan_row)
    elif placement == 'nan at the wave seam':
        rows[min(wave - 1, C - 1)] = list(nan_row); rows[min(wave, C - 1)] = list(nan_row)
    elif placement == 'all nan':
        rows = [list(nan_row) for _ in range(C)]
    elif placement == 'count 0 with s1 > 0':
        rows[C // 2][SUM_CNT] = 0
    elif placement == 'link count 0 with flag 3':
        for l in range(k['MAX_LINKS']):
            rows[C // 2][SUM_LINK0 + 3 * l + 1] = 0
        rows[0][SUM_LINK0 + 3 * 3 + 1] = 0
    elif placement == 'negative variance':
        n, dq = negative_variance_row(n_pix)
        a, b2 = dq >> 20, dq & 0xFFFFF
        for i in {0, C // 2, C - 1}:
            rows[i][SUM_CNT:SUM_LINK0] = [n, n * dq, n * a * a, n * a * b2, n * b2 * b2]
    sums = np.array([[(v - t) & M64 for v, t in zip(r, total)] for r in rows], np.uint64)
    wraps = sum(v < t for r in rows for v, t in zip(r, total))
    total = np.array(total, np.uint64)
    err, words = finalize_ref(sums, total, loss, n_render, n_pix, flags)
    return dict(C=C, loss=loss, n_render=n_render, n_pix=float(n_pix), flags=flags, sums=sums, total=total, err=err, words=words,
                best=argmin(err), wraps=wraps, final=rows, placed=spot.get('want_best'), placed_at=spot.get('at'), name=(C, loss, n_render, flag_set, placement))


def finalize_cases():
    """The list of finalize_case arguments the GPU test runs: every size x every loss, flags and n_render crossed over the sizes, and
    every placement at every size for the loss it bears on."""
    k = constants()
    D, F, L, T = k['LOSS_DEPTH'], k['LOSS_FULL'], k['LOSS_LOOKUP'], k['LOSS_TSWEEP']
    sizes, _ = finalize_sizes()
    out = []
    flag_names = list(FLAG_SETS)
    for i, C in enumerate(sizes):
        for j, placement in enumerate(PLACEMENTS):
            loss = (D, F, L, T)[(i + j) % 4]
            if placement in ('nan first', 'nan last', 'nan at the wave seam', 'all nan', 'count 0 with s1 > 0'):
                loss = (D, F)[(i + j) % 2]                                       # only the losses that divide by the count
            if placement == 'link count 0 with flag 3':
                out.append((C, F, 6, 'mask and depth', placement))
                out.append((C, F, 4, 'mixed', placement))
                continue
            n_render = (6, 4)[(i + j) % 2] if loss == F else 6
            out.append((C, loss, n_render, flag_names[(i + j) % 4] if loss == F else 'none', placement))
        out.append((C, F, 6, flag_names[i % 4], 'as drawn'))
        for loss in (D, F, L, T):                                               # every loss at every size, whatever the rotation above gave
            out.append((C, loss, 4 if (loss == F and i % 2) else 6, 'mixed' if loss == F else 'none', 'as drawn'))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c); uniq.append(c)
    return uniq


FRAME_SIZES = (1, 255, 256, 257, 1025)


@functools.lru_cache(maxsize=None)
def finalize_frames_case(C, loss, n_render, n_pix=76800):
    """Three frames with totals and flags of their own, frame_of interleaved (0, 1, 2, 0, ...) with a run of one frame in the
    middle; rows of each frame wrap against its totals."""
    k = constants()
    n_words = k['SUM_WORDS']
    rng = np.random.default_rng(C * 7 + loss + n_render)
    frame_of = (np.arange(C) % 3).astype(np.int32)
    frame_of[C // 3:C // 3 + 5] = 2
    flags = np.array([FLAG_SETS['mixed'], FLAG_SETS['mask and depth'], FLAG_SETS['mask']], np.uint8)
    totals = [[int(v) for v in rng.integers(1, 1 << (20 + 10 * f), n_words)] for f in range(3)]
    rows = _final_rows(C, n_pix, rng)
    sums = np.array([[(v - t) & M64 for v, t in zip(r, totals[int(f)])] for r, f in zip(rows, frame_of)], np.uint64)
    totals = np.array(totals, np.uint64)
    err, words = finalize_ref(sums, totals[frame_of], loss, n_render, n_pix, flags[frame_of])
    return dict(C=C, loss=loss, n_render=n_render, n_pix=float(n_pix), flags=flags, totals=totals, frame_of=frame_of, sums=sums, err=err,
                words=words, final=rows)


# ------------------------------------------------------------------------------------------------ the raster queue's builder
# score_queue_kernel in its three forms (what raster_queue_kernel, bounds_kernel and rope_abi.hip rely on):
#   plain       neither map: a row's pairs are the tiles in hi | lo of the row itself, weighed at the row
#   layers      layer_of set: the pairs are the tiles in hi; lo is that of the row's layer's representative, and every tile in lo & ~hi
#               adds the layer's stored sums of that tile into the row's sums (modulo 2^64)
#   for_layers  cand_of_row set: the pairs are the tiles in lo of rep = cand_of_row[row], weighed at rep; the item names the row
# A pair of weight t goes to class clamp(QUEUE_TOP_LOG2 - floor(log2(t | 1)), 0, QUEUE_CLASSES - 1), t an unsigned 32-bit number;
# without weights every pair goes to the last class.  An item is row | tile << 16.
QUEUE_FORMS = ('plain', 'layers', 'for_layers', 'unweighted plain', 'unweighted layers')
WRONG_QUEUE = ('class one up', 'class one down', 'weights at the row for rep', 'weights at rep for the row', 'lo of the row itself',
               'layer_sums by candidate', 'store for add', 'hi | lo queued with layers')


def queue_class(tris, shift=0):
    k = constants()
    assert 0 <= tris < 1 << 32
    return min(max(k['QUEUE_TOP_LOG2'] - ((tris | 1).bit_length() - 1) + shift, 0), k['QUEUE_CLASSES'] - 1)


def queue_weight_table():
    """0, 1, every power of two from 2^(TOP - CLASSES) to 2^(TOP + 1) with its two neighbours, 2^31 and 2^32 - 1: each side of every
    class border, both clamps, a weight __clz sees as a negative int."""
    k = constants()
    top, n = k['QUEUE_TOP_LOG2'], k['QUEUE_CLASSES']
    assert top - n >= 1 and top + 1 < 31
    t = [0, 1, 1 << 31, 0xFFFFFFFF]
    for e in range(top - n, top + 2):
        t += [(1 << e) - 1, 1 << e, (1 << e) + 1]
    return sorted(set(t))


def _rows_of(a):
    return None if a is None else np.asarray(a).tolist()


def queue_ref(form, mask_lo, mask_hi, n_tiles, weights, layer_of, layer_rep, layer_sums, cand_of_row, sums, wrong=()):
    """mask_lo, mask_hi (candidates, mask_words) uint32; weights (candidates, n_tiles) uint32 or None; layer_of (rows,), layer_rep
    (layers,), layer_sums (layers, n_tiles, SUM_WORDS) uint64 with form 'layers'; cand_of_row (rows,) with 'for_layers'; sums (at least
    rows, SUM_WORDS) uint64.  -> dict: items (per class, the sorted packed pairs), counts, sums (as given but for the rows' additions).
    wrong: names of deliberate mistakes (WRONG_QUEUE), for tests/test_geometry_refs.py only."""
    k = constants()
    n_cls, n_words = k['QUEUE_CLASSES'], k['SUM_WORDS']
    assert form in ('plain', 'layers', 'for_layers') and (layer_of is not None) == (form == 'layers') and (cand_of_row is not None) == (form == 'for_layers')
    lo_rows, hi_rows, w_rows = _rows_of(mask_lo), _rows_of(mask_hi), _rows_of(weights)
    layer_of, layer_rep, cand_of_row, lsums = _rows_of(layer_of), _rows_of(layer_rep), _rows_of(cand_of_row), _rows_of(layer_sums)
    out = _rows_of(sums)
    rows = len(cand_of_row) if form == 'for_layers' else len(hi_rows)
    words = len(lo_rows[0])
    assert 32 * (words - 1) < n_tiles <= 32 * words and rows <= 1 << 16 and n_tiles <= 1 << 16
    past = [t for t in range(n_tiles, 32 * words)]
    bit = lambda row, t: (row[t >> 5] >> (t & 31)) & 1
    shift = 1 if 'class one up' in wrong else -1 if 'class one down' in wrong else 0
    items = [[] for _ in range(n_cls)]
    for row in range(rows):
        layer = None
        if form == 'for_layers':
            rep = cand_of_row[row]
            lo, hi, weigh_at = lo_rows[rep], None, (row if 'weights at the row for rep' in wrong else rep)
        elif form == 'layers':
            layer = layer_of[row]
            lo = lo_rows[row if 'lo of the row itself' in wrong else layer_rep[layer]]
            hi, weigh_at = hi_rows[row], (layer_rep[layer] if 'weights at rep for the row' in wrong else row)
        else:
            lo, hi, weigh_at = lo_rows[row], hi_rows[row], row
        assert not any(bit(lo, t) or (hi is not None and bit(hi, t)) for t in past), "mask bits at or past n_tiles: bounds_kernel sets none"
        acc = [0] * n_words
        for t in range(n_tiles):
            l, h = bit(lo, t), (bit(hi, t) if hi is not None else 0)
            if form == 'for_layers':
                work = l
            elif form == 'layers':
                work = (h | l) if 'hi | lo queued with layers' in wrong else h
            else:
                work = h | l
            if work:
                cls = n_cls - 1 if w_rows is None else queue_class(w_rows[weigh_at][t], shift)
                items[cls].append(row | (t << 16))
            if form == 'layers' and l and not h:
                src = lsums[row % len(lsums) if 'layer_sums by candidate' in wrong else layer][t]
                for w in range(n_words):
                    acc[w] += src[w]
        for w in range(n_words):
            if acc[w] & M64:
                out[row][w] = acc[w] & M64 if 'store for add' in wrong else (out[row][w] + acc[w]) & M64
    return dict(items=[sorted(v) for v in items], counts=[len(v) for v in items], sums=np.array(out, np.uint64).reshape(np.asarray(sums).shape))


def same_queue(a, b):
    return a['items'] == b['items'] and a['counts'] == b['counts'] and np.array_equal(a['sums'], b['sums'])


QUEUE_ROWS, QUEUE_TILES = (1, 7, 8, 9, 257), (1, 4, 32, 33, 80, 256)       # either side of the eight rows a workgroup; 1, 2, 3 and 8 mask words
QUEUE_SIZES = [(r, t) for r in QUEUE_ROWS for t in QUEUE_TILES] + [(65535, 4)]  # and the last row the 16 bits of an item can name
QUEUE_SPARE_ROWS = 2                                     # rows of sums past the last: nothing writes them


def _pack_bits(bits, words):
    n = len(bits)
    full = np.zeros((n, words * 32), np.uint64)
    full[:, :bits.shape[1]] = bits
    return (full.reshape(n, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def queue_case(form, rows, n_tiles, seed=0):
    """Deterministic inputs of one launch_score_queue, inside the contract bounds_kernel and rope_abi.hip give the kernel: no mask bit
    at or past n_tiles, no mask_lo bit on a candidate that is not its layer's representative, segment = rows x mask_words x 32 (0 and
    one class without weights).  The i-th queued pair has the i-th weight of queue_weight_table() (from a drawn start, cyclically).
    With layers, where the sizes allow: `span` is a candidate whose layer-only tiles lie in mask words 0 and 1, `wrapped` one whose
    sums word SUM_S1 takes a layer word of 2^64 - 1 on top of a nonzero start, `zero_layer` a layer whose stored sums are all zero
    (its representative has a layer-only tile), `covered` a candidate whose hi holds all of its layer's lo.
    -> dict of the arguments (args: queue_ref's, in order), the reference's answer (want) and those names."""
    k = constants()
    n_words, n_cls = k['SUM_WORDS'], k['QUEUE_CLASSES']
    base, weighted = form.replace('unweighted ', ''), not form.startswith('unweighted')
    assert form in QUEUE_FORMS and base in ('plain', 'layers', 'for_layers')
    words = (n_tiles + 31) // 32
    rng = np.random.default_rng(QUEUE_FORMS.index(form) * 1000003 + rows * 1009 + n_tiles * 7 + seed)
    n_cands = rows + 3 if base == 'for_layers' else rows
    lo, hi = rng.random((n_cands, n_tiles)) < 0.5, rng.random((n_cands, n_tiles)) < 0.4
    layer_of = layer_rep = layer_sums = cand_of_row = None
    named = dict(span=None, wrapped=None, zero_layer=None, covered=None)
    sums = rng.integers(0, 1 << 64, (rows + QUEUE_SPARE_ROWS, n_words), dtype=np.uint64) | np.uint64(1)
    hi[rows - 1, n_tiles - 1] = True                     # the last row is queued, whatever was drawn
    if base == 'for_layers':
        perm = rng.permutation(n_cands)
        if perm[0] == 0:
            perm[[0, rows]] = perm[[rows, 0]]            # row 0 is not its own representative
        cand_of_row = perm[:rows].astype(np.int32)
        lo[cand_of_row[rows - 1], n_tiles - 1] = True
        weigh_at, work = cand_of_row, lo[cand_of_row]
    elif base == 'layers':
        n_layers = max(1, min(rows // 2, 37))
        perm = rng.permutation(rows)
        layer_rep = perm[:n_layers].astype(np.int32)
        layer_of = rng.integers(0, n_layers, rows).astype(np.int32)
        layer_of[layer_rep] = np.arange(n_layers)
        others = perm[n_layers:].tolist()
        lo[others] = False                               # bounds_kernel skips the shared links of these
        layer_sums = rng.integers(0, 1 << 64, (n_layers, n_tiles, n_words), dtype=np.uint64)
        rep_of = lambda c: int(layer_rep[layer_of[c]])
        if words >= 2 and len(others) >= 2:
            c = named['span'] = others[1]
            lo[rep_of(c), [0, 32]] = True
            hi[c, [0, 32]] = False
        c = named['wrapped'] = named['span'] if named['span'] is not None else (others[-1] if others else 0)
        lo[rep_of(c), 0] = True
        hi[c, 0] = False
        layer_sums[layer_of[c], 0, SUM_S1] = M64
        if n_layers >= 2:
            z = named['zero_layer'] = (int(layer_of[c]) + 1) % n_layers
            layer_sums[z] = 0
            lo[layer_rep[z], n_tiles - 1] = True
            hi[layer_rep[z], n_tiles - 1] = False
        if others and named['wrapped'] != others[0]:
            c = named['covered'] = others[0]
            lo[rep_of(c), 0] = True
            hi[c] |= lo[rep_of(c)]
        weigh_at, work = np.arange(rows), hi
    else:
        weigh_at, work = np.arange(rows), hi | lo
    weights = None
    if weighted:
        table = np.array(queue_weight_table(), np.uint32)
        weights = table[rng.integers(0, len(table), (n_cands, n_tiles))]
        at = np.argwhere(work)
        weights[np.asarray(weigh_at)[at[:, 0]], at[:, 1]] = table[(np.arange(len(at)) + int(rng.integers(0, len(table)))) % len(table)]
    mask_lo, mask_hi = _pack_bits(lo, words), _pack_bits(hi, words)
    args = (base, mask_lo, mask_hi, n_tiles, weights, layer_of, layer_rep, layer_sums, cand_of_row, sums)
    segment = rows * words * 32
    return dict(form=form, base=base, rows=rows, n_tiles=n_tiles, words=words, n_cands=n_cands, args=args, mask_lo=mask_lo, mask_hi=mask_hi,
                weights=weights, layer_of=layer_of, layer_rep=layer_rep, layer_sums=layer_sums, cand_of_row=cand_of_row, sums=sums,
                segment=segment if weighted else 0, n_items=n_cls * segment if weighted else segment, want=queue_ref(*args), **named)


# ------------------------------------------------------------------------------------------------ a kept grid's clearing
CLEAR_SIZES = (0, 1, 11, 12, 256, 257)                   # rows x SUM_WORDS on either side of the 2 x QUEUE_COUNTERS counters (0 rows
#                                                          alone lie below them) and of the 256 threads of one workgroup
WRONG_CLEAR = ('one word short', 'one row more', 'one counter short', "one queue's counters only", 'counters although null')


def clear_pass_ref(sums, C, counters, wrong=()):
    """clear_pass_kernel: the first C x SUM_WORDS words of sums are zero, and the 2 x QUEUE_COUNTERS first ints of counters when there
    are any -> (sums, counters or None), copies."""
    k = constants()
    sums = np.array(sums, np.uint64).reshape(-1)
    n = C * k['SUM_WORDS'] + (-1 if 'one word short' in wrong and C else k['SUM_WORDS'] if 'one row more' in wrong else 0)
    assert n <= len(sums)
    sums[:n] = 0
    if counters is None:
        return sums, (np.zeros(2 * k['QUEUE_COUNTERS'], np.int32) if 'counters although null' in wrong else None)
    counters = np.array(counters, np.int32).reshape(-1)
    n = k['QUEUE_COUNTERS'] if "one queue's counters only" in wrong else 2 * k['QUEUE_COUNTERS'] - ('one counter short' in wrong)
    counters[:n] = 0
    return sums, counters
