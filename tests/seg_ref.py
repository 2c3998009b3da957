"""References and input builders for the inference box kernels (rope_seg.hip: nms_mask_kernel + nms_scan_kernel, roi_align_kernel,
bias_act_kernel) and the annotator's label_mask_kernel (rope_masks.hip), shared by tests/test_seg_refs.py (CPU: the references
against each other and against the product's tensor formulation, every builder against the edge it is named for) and
tests/test_gpu_seg_kernels.py / tests/test_gpu_label_masks.py (the kernels against the references on those inputs).

NMS, bias/act and RoIAlign form (a) are restated operation by operation in numpy float32 (IEEE; the kernels are built with
-ffp-contract=off) with bfloat16 roundings on uint32 views, so they are compared bit for bit.

The RoIAlign bound against float64 (form (b))
---------------------------------------------
One output element is   out = bf(bf(bf(bf(g00 oy) + bf(g10 wy)) ox) + bf(bf(bf(g01 oy) + bf(g11 wy)) wx))   with bf = round to
bfloat16 (nearest even; 8 significant bits, so the unit roundoff is u = 2^-8, not 2^-9: 1 + 2^-8 is a tie), g the four taps (bfloat16 values, exact in float64) and the weights
wy = bf(fy), oy = bf(1 - wy), wx = bf(fx), ox = bf(1 - wx); fy = ys - floor(ys) is exact in float32.  The multiplication by the
inside flag (1 or 0) and the final conversion round nothing.

  * Operations.  Every tap passes through four roundings to bfloat16 (mul, add, mul, add); the float32 products of two bfloat16
    values are exact, the two float32 sums round once more each (2^-24).  With W_i the product of the two ROUNDED weights
        |out - sum g_i W_i| <= c sum |g_i| W_i,        c = (1 + u)^4 (1 + 2^-24)^2 - 1   (4.02 u).
  * Weights.  wy = fy (1 + d), |d| <= u: an error of at most u fy, relative.  oy = fl32(1 - wy)(1 + d'): its error is at most
    u fy + (u + 2^-23)(1 - wy) <= 1.01 u — ABSOLUTE, not relative to 1 - fy (fy = 0.999 gives oy = 0 or 2^-8 for an exact 0.001), which
    is why the bound is not simply 6 u sum |w_i| |g_i|.  With e_y, e_x the errors of a tap's two weights and a_y, a_x their exact values
        |W_i - w_i| <= e_y a_x + e_x a_y + e_y e_x =: d_i        and        W_i <= w_i + d_i.
  * Coordinates.  ys = fl(fl(y1 + fl(t fl(y2 - y1))) hm): four float32 roundings, |ys - ys64| <= 2.01 * 2^-24 * hm (|t (y2 - y1)| +
    |y1 + t (y2 - y1)|) =: dy, likewise dx.  The bilinear surface is continuous and piecewise linear, so moving the sample by (dy, dx)
    changes it by at most dy Ly + dx Lx, with Ly (Lx) the largest difference of vertically (horizontally) adjacent pixels of that
    level, frame and channel.

      |out - ref64| <= c sum |g_i| (w_i + d_i) + sum |g_i| d_i + dy Ly + dx Lx

float64's own error in ref64 is 2^-44 of the first term.  bfloat16 shares float32's exponent range and nothing here flushes, so there
is no underflow term at the magnitudes of the tests.  A sample whose float64 coordinate lies within EDGE_EPS of 0 or of hm / wm
without being exactly on it may see `inside` flip between the two precisions: it is skipped, and the builders keep such samples
below 1 % (dy, dx < EDGE_EPS is asserted)."""
import numpy as np
import torch

U16 = 2.0 ** -8
EDGE_EPS = 1e-4
ROI_SIZE = 512                                      # 224 / 512 = 0.4375: a box of side 0.4375 * 2^k sits on level 4 + k exactly
F32 = np.float32


# ------------------------------------------------------------------------------------------------ bfloat16 on uint32 views
def bf16_bits(x):
    """float32 array -> uint16 bfloat16 bits, round to nearest even (NaN -> 0x7FC0), as rope_seg.hip's f2bf."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC0, r).astype(np.uint16)


def bf16_value(bits):
    """uint16 bfloat16 bits -> float32."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def _bmul(a, b):
    return bf16_round(np.multiply(a, b, dtype=np.float32))


def _badd(a, b):
    return bf16_round(np.add(a, b, dtype=np.float32))


def torch_bf16(bits):
    """uint16 bits -> torch.bfloat16 tensor of the same shape."""
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ NMS
def iou_over_ref(a, b, thr):
    """rope_seg.hip's iou_over for boxes a (m, 4) against one box b (4,), one numpy float32 operation per step."""
    a, b, thr = np.asarray(a, F32).reshape(-1, 4), np.asarray(b, F32), F32(thr)
    zero = F32(0)
    with np.errstate(all='ignore'):
        ih = np.maximum(np.minimum(a[:, 2], b[2]) - np.maximum(a[:, 0], b[0]), zero)
        iw = np.maximum(np.minimum(a[:, 3], b[3]) - np.maximum(a[:, 1], b[1]), zero)
        inter = ih * iw
        area_a = np.maximum(a[:, 2] - a[:, 0], zero) * np.maximum(a[:, 3] - a[:, 1], zero)
        area_b = np.maximum(b[2] - b[0], zero) * np.maximum(b[3] - b[1], zero)
        iou = inter / np.maximum((area_a + area_b) - inter, F32(1e-12))
    assert iou.dtype == np.float32
    return iou > thr, iou


def nms_ref(boxes, groups, valid, limit, thr):
    """Sequential greedy NMS of ONE set of boxes (n, 4) already sorted best first: a candidate is kept unless a box kept before it,
    of the same group, overlaps it by more than thr; invalid boxes are neither kept nor suppress; at most `limit`.  -> keep (n,) uint8."""
    boxes = np.asarray(boxes, F32)
    n = len(boxes)
    keep = np.zeros(n, np.uint8)
    kept = []
    for i in range(n):
        if len(kept) >= limit:
            break
        if valid is not None and not valid[i]:
            continue
        if kept:
            rivals = np.array(kept) if groups is None else np.array([j for j in kept if groups[j] == groups[i]], np.int64)
            if len(rivals) and iou_over_ref(boxes[rivals], boxes[i], thr)[0].any():
                continue
        kept.append(i)
        keep[i] = 1
    return keep


def nms_ref_sets(case):
    g, v = case['groups'], case['valid']
    return np.stack([nms_ref(case['boxes'][s], None if g is None else g[s], None if v is None else v[s], case['limit'], case['thr'])
                     for s in range(len(case['boxes']))])


NMS_SIZES = (1, 63, 64, 65, 127, 128, 129, 1025, 4161)


def _stairs(n, step, x0=0.0):
    """Unit boxes [x0, step i, x0 + 1, step i + 1]: every coordinate a small multiple of 1/8, every float32 step exact."""
    i = np.arange(n, dtype=np.float64)
    return np.stack([np.full(n, x0), step * i, np.full(n, x0 + 1), step * i + 1], 1).astype(F32)


def _case(boxes, limit, thr=0.5, groups=None, valid=None, **meta):
    boxes = np.ascontiguousarray(boxes, F32)
    assert boxes.ndim == 3 and boxes.shape[2] == 4
    d = dict(boxes=boxes, limit=int(limit), thr=float(F32(thr)), meta=meta,
             groups=None if groups is None else np.ascontiguousarray(groups, np.int32),
             valid=None if valid is None else np.ascontiguousarray(valid, np.uint8))
    return d


def nms_staircase(n, limit=None):
    """Three sets: step 0.25 (neighbours overlap by 0.6, next but one by 1/3: exactly the even boxes stay, each kept by the REMOVAL
    of its predecessor — a chain through every block seam), step 0.5 (1/3: all stay), step 0.125 (0.78, 0.6, 0.45: every third)."""
    return _case(np.stack([_stairs(n, 0.25), _stairs(n, 0.5, 3.0), _stairs(n, 0.125, -2.0)]), n if limit is None else limit,
                 expect=[(n + 1) // 2, n, (n + 2) // 3])


def nms_identical(n):
    """Every box of a set the same; set 1's last box stands apart."""
    b = np.stack([np.tile(F32([0, 0, 1, 1]), (n, 1)), np.tile(F32([.5, .25, 2, 3]), (n, 1)), np.tile(F32([-1, -1, 0, 0.5]), (n, 1))])
    if n > 1:
        b[1, -1] = [10, 10, 11, 11]
    return _case(b, n, expect=[1, min(n, 2), 1])


def nms_disjoint(n, limit):
    return _case(np.stack([_stairs(n, 2.0), _stairs(n, 1.0, 5.0), _stairs(n, 3.0, -4.0)]), limit, expect=[min(n, limit)] * 3)


def nms_seven_groups(n):
    """Identical boxes, seven groups dealt three different ways."""
    i = np.arange(n)
    return _case(np.tile(F32([0, 0, 1, 1]), (3, n, 1)), n, groups=np.stack([i % 7, (i * 3 + 2) % 7, (i // 3) % 7]) + 5,
                 expect=[min(n, 7), min(n, 7), len(set(((i // 3) % 7).tolist()))])


def nms_one_set_invalid(n, seed=0):
    """Random clusters with random validity; set 1 has no valid box at all."""
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(0, 4, (3, n, 2)).astype(F32)
    s = rng.uniform(0.5, 1.5, (3, n, 2)).astype(F32)
    valid = rng.random((3, n)) < 0.7
    valid[1] = False
    return _case(np.concatenate([c, c + s], 2), n, 0.3, valid=valid, groups=rng.integers(0, 3, (3, n)))


def nms_invalid_suppressor(n):
    """The step-0.25 staircase with its even boxes invalid: the odd ones, which the even ones would have struck, all stay."""
    i = np.arange(n)
    valid = np.stack([i % 2 == 1, i % 2 == 0, i % 3 != 0])
    return _case(np.stack([_stairs(n, 0.25)] * 3), n, valid=valid, expect=[n // 2, (n + 1) // 2, None])


def nms_far_victim(n=4161):
    """66 words: box 0 of block 0 strikes nothing but the single box of the last block (word 65, the second trip of the row loop's
    lane 0); everything between is disjoint.  Set 1 strikes from block 1, set 2 not at all."""
    b = np.stack([_stairs(n, 2.0), _stairs(n, 2.0, 3.0), _stairs(n, 2.0, -3.0)])
    b[0, -1] = b[0, 0]
    b[1, -1] = b[1, 64]
    return _case(b, n, expect=[n - 1, n - 1, n])


def nms_exact_threshold(below: bool):
    """[0,0,1,1] against [0,0,1,2]: IoU exactly 0.5.  Kept at thr = 0.5 (the comparison is strict), struck just below it."""
    thr = np.nextafter(F32(0.5), F32(0)) if below else F32(0.5)
    b = np.stack([F32([[0, 0, 1, 1], [0, 0, 1, 2]]), F32([[0, 0, 2, 1], [0, 0, 1, 1]]), F32([[3, 3, 4, 4], [3, 3, 4, 5]])])
    return _case(b, 2, thr, expect=[1 if below else 2] * 3)


def nms_degenerate():
    """Zero-area and inverted boxes (IoU 0 against anything, themselves included: all stay), and two tiny identical boxes whose union
    (1e-14) is below the 1e-12 floor: IoU 0.01, both stay."""
    b = np.stack([F32([[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [2, 2, 2, 2]]),
                  F32([[1, 0, 0, 1], [0, 0, 1, 1], [0, 1, 1, 0], [0, 0, 1, 1], [.5, .5, .5, .5], [0, 0, 1, 0], [0, 0, 1, 1]]),
                  F32([[0, 0, 1e-7, 1e-7], [0, 0, 1e-7, 1e-7], [5, 5, 6, 6], [5, 5, 6, 6], [0, 0, 1e-7, 1e-7], [7, 7, 7, 8], [7, 7, 7, 8]])])
    return _case(b, 7, expect=[6, 5, 6])


# ------------------------------------------------------------------------------------------------ RoIAlign
ROI_PYRAMIDS = {
    'tall': ((40, 24), (19, 13), (9, 7), (5, 3)),          # not square, no 2:1 step between levels
    'wide': ((24, 40), (13, 19), (7, 9), (3, 5)),
    'thin': ((40, 24), (1, 12), (10, 1), (5, 3)),          # a level of height 1 and one of width 1
    'small': ((6, 10), (5, 3), (1, 4), (3, 1)),
}
ROI_FRAMES = 3
# (pyramid, channels, pool): every channel count and every pool; pools above 256 / (channels / 8) samples per round are 33 at 64
# channels (32), 7 .. 33 at 512 (4) and everything above 1 at 2048 (1)
ROI_CASES = ([('tall', 8, p) for p in (1, 2, 7, 14, 33)] + [('wide', 16, p) for p in (1, 2, 7, 14, 33)] +
             [('thin', 64, p) for p in (1, 2, 7, 14, 33)] + [('wide', 512, 7), ('tall', 512, 33), ('thin', 512, 2)] +
             [('small', 2048, p) for p in (1, 2, 7, 14)])


def roi_sample_t(pool):
    """The sample positions the product hands the kernel (maskrcnn._roi_align): torch.linspace(0, 1, pool), float32."""
    return torch.linspace(0, 1, pool).numpy().copy()


def roi_features(pyramid, channels, seed=0):
    """Four levels (ROI_FRAMES, C, H, W) of bfloat16 bits (uint16), standard normal, different in every frame -> (levels, rows):
    rows is the packed table the kernel reads, (sum of B H W, C) bits, as maskrcnn._pack_levels lays it out."""
    rng = np.random.default_rng(1000 + seed)
    levels = [bf16_bits(rng.standard_normal((ROI_FRAMES, channels, h, w)).astype(F32)) for h, w in ROI_PYRAMIDS[pyramid]]
    rows = np.concatenate([lv.transpose(0, 2, 3, 1).reshape(-1, channels) for lv in levels])
    return levels, rows


def roi_levels_abi(pyramid):
    hw = np.array(ROI_PYRAMIDS[pyramid], np.int32)
    sizes = [ROI_FRAMES * h * w for h, w in ROI_PYRAMIDS[pyramid]]
    return hw, np.array([sum(sizes[:k]) for k in range(4)], np.int64)


def roi_boxes(n=48, seed=0):
    """Boxes (n, 4) float32 on the 1/1024 grid and their frames.  The first 12 are the named ones: the whole map ([0,0,1,1]: the last
    sample lands exactly on hm and wm), one box per level inside the map, boxes on the edge, across it and wholly beyond it, an
    empty box, a line.  The rest: side 0.4375 * 2^(k + j), k = -2..1 (levels 2..5), |j| <= 0.3, anywhere from -0.3 to 1.3."""
    s = 0.4375
    named = [[0, 0, 1, 1], [.25, .5, .25 + s / 4, .5 + s / 4], [.125, .25, .125 + s / 2, .25 + s / 2], [.5, .125, .5 + s, .125 + s],
             [.0625, .03125, .0625 + 2 * s, .03125 + 2 * s], [0, .5, s, 1], [.75, 0, 1, .5], [-.25, .75, .25, 1.25],
             [1.125, 1.25, 1.5, 1.75], [-2, -2, -1.5, -1.5], [.3125, .3125, .3125, .3125], [.25, .125, .25, .875]]
    rng = np.random.default_rng(77 + seed)
    rest = []
    while len(named) + len(rest) < n:
        k = len(rest) % 4 - 2
        h, w = s * 2.0 ** (k + rng.uniform(-.3, .3)), s * 2.0 ** (k + rng.uniform(-.3, .3))
        y, x = rng.uniform(-.3, 1.3 - h), rng.uniform(-.3, 1.3 - w)
        rest.append([y, x, y + h, x + w])
    b = (np.round(np.array(named + rest)[:n] * 1024) / 1024).astype(F32)
    return b, (np.arange(n) % ROI_FRAMES).astype(np.int32)


def roi_box_count(channels, pool):
    """Fewer boxes where one box is many values: keeps a case's reference within a second or two."""
    return int(min(48, max(12, (1 << 21) // (pool * pool * channels))))


def roi_level_arg64(boxes):
    """The level argument 4 + log2(sqrt(h w) / (224 / size)) in float64, before rounding and clamping."""
    b = np.asarray(boxes, F32).astype(np.float64)
    return 4 + np.log2(np.sqrt(np.maximum((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), 1e-12)) * (ROI_SIZE / 224.0))


def roi_inv_unit():
    return F32(1.0) / F32(224.0 / ROI_SIZE)


def _roi_geometry(pyramid, boxes, frame, t, dtype):
    """Level, sample coordinates and taps of every box, in `dtype` arithmetic in the kernel's order."""
    b = np.asarray(boxes, F32)
    hw, off = roi_levels_abi(pyramid)
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    with np.errstate(all='ignore'):
        lf = np.clip(np.rint(F32(4) + np.log2(np.sqrt(np.maximum(h * w, F32(1e-12))) * roi_inv_unit())), 2, 5)
    li = lf.astype(np.int64) - 2
    Hf, Wf = hw[li, 0].astype(np.int64), hw[li, 1].astype(np.int64)
    base = off[li] + np.asarray(frame, np.int64) * (Hf * Wf)
    b, t = b.astype(dtype), np.asarray(t, F32).astype(dtype)
    hm, wm = (Hf - 1).astype(dtype)[:, None], (Wf - 1).astype(dtype)[:, None]
    ys = (b[:, 0:1] + t[None, :] * (b[:, 2:3] - b[:, 0:1])) * hm                  # (K, P)
    xs = (b[:, 1:2] + t[None, :] * (b[:, 3:4] - b[:, 1:2])) * wm
    assert ys.dtype == dtype and xs.dtype == dtype
    return dict(li=li, Hf=Hf, Wf=Wf, base=base, ys=ys, xs=xs, hm=hm, wm=wm, b=b, t=t)


def _taps(g):
    y0, x0 = np.floor(g['ys']), np.floor(g['xs'])
    Hm, Wm = (g['Hf'] - 1)[:, None], (g['Wf'] - 1)[:, None]
    y0i, x0i = y0.astype(np.int64), x0.astype(np.int64)
    y0c, y1c = np.clip(y0i, 0, Hm), np.clip(y0i + 1, 0, Hm)
    x0c, x1c = np.clip(x0i, 0, Wm), np.clip(x0i + 1, 0, Wm)
    in_y, in_x = (g['ys'] >= 0) & (g['ys'] <= g['hm']), (g['xs'] >= 0) & (g['xs'] <= g['wm'])
    inside = in_y[:, :, None] & in_x[:, None, :]
    Wk, base = g['Wf'][:, None, None], g['base'][:, None, None]

    def row(yi, xi):
        return base + yi[:, :, None] * Wk + xi[:, None, :]
    return y0, x0, inside, (row(y0c, x0c), row(y1c, x0c), row(y0c, x1c), row(y1c, x1c))


def roi_align_ref_bits(pyramid, rows, boxes, frame, pool, t):
    """Form (a): roi_align_kernel step for step in numpy float32 with bfloat16 roundings.  rows (R, C) uint16 -> (K, pool, pool, C) uint16."""
    assert len(t) == pool
    g = _roi_geometry(pyramid, boxes, frame, t, np.float32)
    y0, x0, inside, idx = _taps(g)
    one = F32(1)
    wy, wx = bf16_round(g['ys'] - y0), bf16_round(g['xs'] - x0)
    omwy, omwx = bf16_round(one - wy), bf16_round(one - wx)
    wy, omwy = wy[:, :, None, None], omwy[:, :, None, None]
    wx, omwx = wx[:, None, :, None], omwx[:, None, :, None]
    v00, v10, v01, v11 = [bf16_value(rows[i]) for i in idx]
    left = _bmul(_badd(_bmul(v00, omwy), _bmul(v10, wy)), omwx)
    right = _bmul(_badd(_bmul(v01, omwy), _bmul(v11, wy)), wx)
    val = _bmul(_badd(left, right), inside[..., None].astype(F32))
    return bf16_bits(val)


def roi_align_ref64(pyramid, levels, rows, boxes, frame, pool, t):
    """Form (b): a float64 crop_and_resize of the same features at the same sample positions t, and per element the bound of the
    module docstring.  -> dict: ref, bound (K, pool, pool, C) float64, skip (K, pool, pool) bool (samples a hair off a map edge),
    inside (K, pool, pool) bool, dmax (the largest coordinate error in pixels)."""
    g = _roi_geometry(pyramid, boxes, frame, t, np.float64)
    y0, x0, inside, idx = _taps(g)
    fy, fx = (g['ys'] - y0)[:, :, None, None], (g['xs'] - x0)[:, None, :, None]
    v = [bf16_value(rows[i]).astype(np.float64) for i in idx]                   # g00, g10, g01, g11
    ins = inside[..., None]
    ref = np.where(ins, (v[0] * (1 - fy) + v[1] * fy) * (1 - fx) + (v[2] * (1 - fy) + v[3] * fy) * fx, 0.0)
    u = U16
    ey = (1.01 * u * np.ones_like(fy), u * fy)                                   # errors of oy, wy
    ex = (1.01 * u * np.ones_like(fx), u * fx)
    ay, ax = (1 - fy, fy), (1 - fx, fx)
    ops = (1 + u) ** 4 * (1 + 2.0 ** -24) ** 2 - 1
    bound = np.zeros_like(ref)
    for i, (jy, jx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        d = ey[jy] * ax[jx] + ex[jx] * ay[jy] + ey[jy] * ex[jx]
        bound += np.abs(v[i]) * (ops * (ay[jy] * ax[jx] + d) + d)
    bound = np.where(ins, bound, 0.0)                                            # outside the map both sides give 0
    # coordinates: four float32 roundings, times the steepest neighbour difference of the level, frame and channel
    b, t64 = g['b'], g['t']
    ty, tx = t64[None, :] * (b[:, 2:3] - b[:, 0:1]), t64[None, :] * (b[:, 3:4] - b[:, 1:2])
    dy = 2.01 * 2.0 ** -24 * g['hm'] * (np.abs(ty) + np.abs(b[:, 0:1] + ty))
    dx = 2.01 * 2.0 ** -24 * g['wm'] * (np.abs(tx) + np.abs(b[:, 1:2] + tx))
    C = rows.shape[1]
    Ly, Lx = np.zeros((4, ROI_FRAMES, C)), np.zeros((4, ROI_FRAMES, C))
    for l, lv in enumerate(levels):
        f = bf16_value(lv).astype(np.float64)
        if f.shape[2] > 1:
            Ly[l] = np.abs(np.diff(f, axis=2)).max(axis=(2, 3))
        if f.shape[3] > 1:
            Lx[l] = np.abs(np.diff(f, axis=3)).max(axis=(2, 3))
    fr = np.asarray(frame, np.int64)
    bound += np.where(ins, dy[:, :, None, None] * Ly[g['li'], fr][:, None, None, :] + dx[:, None, :, None] * Lx[g['li'], fr][:, None, None, :], 0.0)

    def near(c, m):
        return ((np.abs(c) < EDGE_EPS) & (c != 0)) | ((np.abs(c - m) < EDGE_EPS) & (c != m))
    skip = near(g['ys'], g['hm'])[:, :, None] | near(g['xs'], g['wm'])[:, None, :]
    return dict(ref=ref, bound=bound, skip=skip, inside=inside, dmax=float(max(dy.max(), dx.max())), level=g['li'] + 2,
                ys=g['ys'], xs=g['xs'], hm=g['hm'], wm=g['wm'])


def check_roi_bound(got_bits, r):
    """got (K, P, P, C) bits against form (b): every element of every sample that is not skipped within its bound.
    -> (worst err / bound, fraction of samples skipped)."""
    got = bf16_value(got_bits).astype(np.float64)
    err = np.abs(got - r['ref'])
    live = ~r['skip'][..., None]
    zero = live & (r['bound'] == 0)
    assert not np.any(err[np.broadcast_to(zero, err.shape)]), "an element with bound 0 (outside the map, or all taps 0) is not 0"
    ratio = np.where(live & (r['bound'] > 0), err / np.where(r['bound'] > 0, r['bound'], 1), 0.0)
    return float(ratio.max()), float(r['skip'].mean())


# ------------------------------------------------------------------------------------------------ bias / residual / ReLU
# (layout, batch, channels, H*W): NCHW with H*W in {8, 24, 960} and C in {1, 3, 64}; channels-last with C in {8, 24, 128}.
# n / 8 is a multiple of 256 only for ('nchw', 2, 64, 960) (15360 = 60 * 256); n = 8 is ('nhwc', 1, 8, 1).
BIAS_SHAPES = ([('nchw', 2, c, hw) for hw in (8, 24, 960) for c in (1, 3, 64)] +
               [('nhwc', 1, 8, 1), ('nhwc', 2, 8, 37), ('nhwc', 1, 24, 37), ('nhwc', 2, 24, 35), ('nhwc', 2, 128, 35), ('nhwc', 2, 128, 128)])
BF_MAX, BF_NEG_ZERO = 0x7F7F, 0x8000


def bias_act_inputs(layout, batch, channels, hw, seed=0):
    """y, residual (n,) and bias (C,) as bfloat16 bits, flat in memory order.  Ordinary values with, sprinkled in: -0.0 and +0.0,
    subnormals of both signs, and +-max in y against +-max in the bias (the sum overflows to an infinity; the residual is always
    finite, so no inf - inf)."""
    n = batch * channels * hw
    rng = np.random.default_rng(seed + n + channels)
    y = bf16_bits(rng.standard_normal(n).astype(F32))
    res = bf16_bits(rng.standard_normal(n).astype(F32))
    bias = bf16_bits(rng.standard_normal(channels).astype(F32))
    special = np.array([BF_NEG_ZERO, 0x0000, 0x0001, 0x007F, 0x8001, 0x807F, 0x0040, BF_MAX, BF_MAX | 0x8000, 0x0080], np.uint16)
    k = rng.integers(0, 3, n)
    y = np.where(k == 0, special[rng.integers(0, len(special), n)], y).astype(np.uint16)
    res = np.where(rng.integers(0, 4, n) == 0, special[rng.integers(0, 7, n)], res).astype(np.uint16)
    bias = np.where(rng.integers(0, 3, channels) == 0, special[rng.integers(0, len(special), channels)], bias).astype(np.uint16)
    m = min(n, len(special))
    y[:m] = special[:m]                                                          # every special value, whatever the draw
    if channels >= 3:
        bias[0], bias[1], bias[2] = BF_MAX, BF_NEG_ZERO, 0x0001
    elif hw == 24:
        bias[0] = BF_MAX
    at = np.nonzero(bias_channel_index(layout, batch, channels, hw) == 0)[0]
    if bias[0] == BF_MAX and n >= 64:                                            # max + max -> +inf, -max + max -> 0
        y[at[-1]], y[at[-2]] = BF_MAX, BF_MAX | 0x8000
    return y, bias, res


def bias_channel_index(layout, batch, channels, hw):
    i = np.arange(batch * channels * hw)
    return (i // hw) % channels if layout == 'nchw' else i % channels


def bias_act_ref(y, bias, res, chan, relu):
    """The separate bfloat16 tensor operations: bf(y + bias[channel]), then bf(. + residual), then max(., 0).  Bits in, bits out."""
    with np.errstate(all='ignore'):
        f = _badd(bf16_value(y), bf16_value(bias)[chan])
        if res is not None:
            f = _badd(f, bf16_value(res))
        if relu:
            f = np.maximum(f, F32(0))
    return bf16_bits(f)


def bias_act_equal(got, want):
    """Bit for bit, except that where the reference gives a zero the kernel may give a zero of either sign (max(-0, 0))."""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    return bool(np.all((got == want) | (((want & 0x7FFF) == 0) & ((got & 0x7FFF) == 0))))


# ------------------------------------------------------------------------------------------------ label masks
MASK_WIDTHS = (1, 2, 3, 5, 127, 129, 131, 257)
MASK_HEIGHTS = (1, 15, 17, 33)
MASK_PADS = (1, 2, 8, 9, 33, 63, 64)
MASK_LABELS = np.arange(8)
BACKGROUND = 255
HI_X, LO_X = 100, 20          # a pixel at column 100 dilates to columns 69..132 at most: within tile 0 only its upper half; 20 -> 0..52


def mask_lut(labels=MASK_LABELS):
    """The table Annotator._mask_color amounts to (tests/test_gpu_annotation.py::host_masks): id k -> bit labels[k], the rest 0."""
    lut = np.zeros(256, np.uint8)
    lut[:len(labels)] = 1 << np.asarray(labels, np.uint8)
    return lut


def _plane_sparse(H, W):
    """Single pixels: id 0 in the four corners, id 1 at columns 127 / 128 on rows 15 / 16 (the tile seams), id 2 only at column
    HI_X, id 3 only at column LO_X, ids 4 and 5 side by side in the middle."""
    p = np.full((H, W), BACKGROUND, np.uint8)
    for y in {15, 16} & set(range(H)):
        for x in {127, 128} & set(range(W)):
            p[y, x] = 1
    if W > HI_X:
        p[H // 2, HI_X] = 2
    if W > LO_X:
        p[H // 3, LO_X] = 3
    if W > 70:
        p[H // 2, 66:68] = (4, 5)
    p[0, 0] = p[0, W - 1] = p[H - 1, 0] = p[H - 1, W - 1] = 0
    return p


def _plane_eight(H, W):
    """All eight ids next to one another around the tile corner (128, 16) where the plane reaches it, else from (0, 0)."""
    p = np.full((H, W), BACKGROUND, np.uint8)
    y0, x0 = (15 if H > 16 else 0), (126 if W > 129 else 0)
    for k in range(8):
        y, x = y0 + k // 4, x0 + k % 4
        if y < H and x < W:
            p[y, x] = k
    return p


def mask_planes(H, W, seed=0):
    """Three id planes with different contents; their order depends on H, so that every kind is plane 0, 1 and 2 somewhere."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    dense = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, BACKGROUND, BACKGROUND], np.uint8), (H, W))
    empty = np.full((H, W), BACKGROUND, np.uint8)
    kinds = {1: (_plane_sparse(H, W), empty, dense), 15: (_plane_eight(H, W), dense, _plane_sparse(H, W)),
             17: (dense, _plane_sparse(H, W), empty), 33: (empty, _plane_eight(H, W), _plane_sparse(H, W))}
    planes = kinds.get(H, (_plane_sparse(H, W), empty, dense))
    names = {1: 'sparse empty dense', 15: 'eight dense sparse', 17: 'dense sparse empty', 33: 'empty eight sparse'}.get(H, 'sparse empty dense')
    return np.stack(planes), names.split()
