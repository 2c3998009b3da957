"""References and input builders for the training kernels (rope_train.hip), shared by tests/test_train_refs.py (CPU: the
references against autograd and by hand, every builder against the edge it is named for) and tests/test_gpu_train_kernels.py
(the kernels against the references on those inputs).

The RoIAlign backward bound
---------------------------
`roi_align_backward_ref` restates maskrcnn._roi_align's float32 steps (level, ys / xs, floor, wy, wx, 1 - wy, 1 - wx, the inside
flag, the four clamped tap rows): those float32 weights are the numbers roi_align_f32_bwd_kernel multiplies by, so they carry
no error of their own.  It then scatters in float64.  Write u = 2^-24 (float32 unit roundoff) and, for one element of the
gradient table, c_i = g_i * wa_i * wb_i for the exact contributions of the m taps that land on it.

  * The kernel forms fl(fl(g * wx) * wy): two roundings, c_i (1 + d1)(1 + d2) with |d| <= u.
  * The m atomic adds happen in some order.  The first add to the zeroed cell is exact; every later one rounds once, so a term
    passes through at most m - 1 more factors (1 + e), |e| <= u, whatever the order.
  * Hence got = sum c_i prod(1 + d), at most m + 1 factors each, and
        |got - sum c_i| <= ((1 + u)^(m + 1) - 1) * sum |c_i| <= (m + 2) u S        while (m + 1)^2 u <= 2, i.e. m < 5000.
  * A sample that lies inside the map touches a row through more than one tap only where a tap index was clamped (ys on the
    last row, xs on the last column); the clamped tap's weight is then exactly 0, adding 0.0 rounds nothing, and so m may be
    taken as n, the number of inside SAMPLES that touch the row.
  * Each add whose result is denormal may be flushed by the memory-side adder: at most 2^-126 lost per add.

      |got - ref| <= (n + 2) * 2^-24 * S + n * 2^-126                  (BWD_N_MAX = 5000 bounds n in the tests)

float64's own error in ref (n * 2^-53 * S) is nine orders below the first term.  Rows no sample touches have S = 0 and n = 0:
the bound is 0 and the kernel must leave its memset zero in place, bit for bit (+0.0)."""
import numpy as np
import torch

U32 = 2.0 ** -24
FLUSH = 2.0 ** -126
BWD_N_MAX = 5000


# ------------------------------------------------------------------------------------------------ RoIAlign backward
def roi_align_taps(feat_shapes, boxes, frame, pool, size):
    """maskrcnn._roi_align's float32 steps on the CPU, in its order, for boxes (K, 4), frame (K,), levels feat_shapes[:4] =
    (B, C, H, W) each.  -> dict: level (K,), rows r00 r10 r01 r11 (K, P, P) int64 into the packed table, weights omwy wy
    (K, P, 1) and omwx wx (K, 1, P) float32, inside (K, P, P) bool, first (three (K, P, P) bools: tap 10 / 01 / 11 lands on a
    row that an earlier tap of the same sample did not)."""
    lv = [tuple(s) for s in feat_shapes[:4]]
    b = torch.as_tensor(np.asarray(boxes, dtype=np.float32))
    frame = torch.as_tensor(np.asarray(frame)).long()
    Hs, Ws = torch.tensor([s[2] for s in lv]), torch.tensor([s[3] for s in lv])
    sizes = [s[0] * s[2] * s[3] for s in lv]
    offs = torch.tensor([sum(sizes[:k]) for k in range(4)])
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    li = (4 + torch.log2((h * w).clamp(min=1e-12).sqrt() / (224.0 / size)).round()).clamp(2, 5).long() - 2
    Hf, Wf = Hs[li], Ws[li]
    base = (offs[li] + frame * (Hf * Wf))[:, None, None]
    t = torch.linspace(0, 1, pool)
    ys = (b[:, 0:1] + t[None, :] * (b[:, 2:3] - b[:, 0:1])) * (Hf - 1)[:, None]
    xs = (b[:, 1:2] + t[None, :] * (b[:, 3:4] - b[:, 1:2])) * (Wf - 1)[:, None]
    assert ys.dtype == torch.float32 and xs.dtype == torch.float32
    y0, x0 = ys.floor(), xs.floor()
    wy, wx = ys - y0, xs - x0
    hm, wm = (Hf - 1)[:, None], (Wf - 1)[:, None]
    inside = ((ys >= 0) & (ys <= hm))[:, :, None] & ((xs >= 0) & (xs <= wm))[:, None, :]
    y0c, y1c = y0.long().clamp(min=0).minimum(hm), (y0.long() + 1).clamp(min=0).minimum(hm)
    x0c, x1c = x0.long().clamp(min=0).minimum(wm), (x0.long() + 1).clamp(min=0).minimum(wm)
    Wk = Wf[:, None, None]

    def row(yi, xi):
        return base + yi[:, :, None] * Wk + xi[:, None, :]
    dy, dx = (y1c != y0c)[:, :, None], (x1c != x0c)[:, None, :]
    ones = torch.ones_like(inside)
    return {'level': li + 2, 'r00': row(y0c, x0c), 'r10': row(y1c, x0c), 'r01': row(y0c, x1c), 'r11': row(y1c, x1c),
            'omwy': (1 - wy)[:, :, None], 'wy': wy[:, :, None], 'omwx': (1 - wx)[:, None, :], 'wx': wx[:, None, :],
            'inside': inside, 'first': (dy & ones, dx & ones, dy & dx), 'n_rows': sum(sizes)}


def roi_align_backward_ref(feat_shapes, boxes, frame, pool, size, grad_out):
    """The transpose of maskrcnn._roi_align for grad_out (K, C, pool, pool) float32, scattered in float64 (module docstring).
    -> ref, S (n_rows, C) float64 and n (n_rows,) int64, n_rows the rows of maskrcnn._pack_levels' table: the gradient, the sum
    of the absolute contributions, and the number of inside samples that touch each row."""
    tp = roi_align_taps(feat_shapes, boxes, frame, pool, size)
    g = torch.as_tensor(np.asarray(grad_out, dtype=np.float32)).permute(0, 2, 3, 1).double()         # (K, P, P, C)
    C = g.shape[3]
    ins = tp['inside'].reshape(-1)
    g = g.reshape(-1, C)[ins]
    ref = torch.zeros((tp['n_rows'], C), dtype=torch.float64)
    S = torch.zeros_like(ref)
    n = torch.zeros(tp['n_rows'], dtype=torch.int64)
    one = torch.ones_like(tp['inside'])
    taps = (('r00', 'omwy', 'omwx', one), ('r10', 'wy', 'omwx', tp['first'][0]), ('r01', 'omwy', 'wx', tp['first'][1]),
            ('r11', 'wy', 'wx', tp['first'][2]))
    for r, a, b, first in taps:
        idx = tp[r].reshape(-1)[ins]
        wgt = (tp[a].double() * tp[b].double()).expand_as(tp['inside']).reshape(-1)[ins]             # exact: 24 + 24 bits
        c = g * wgt[:, None]
        ref.index_add_(0, idx, c)
        S.index_add_(0, idx, c.abs())
        n.index_add_(0, idx, first.reshape(-1)[ins].long())
    return ref, S, n


def backward_bound(S, n):
    """(n + 2) 2^-24 S + n 2^-126 per element (module docstring); S (rows, C), n (rows,)."""
    nn_ = n.double()[:, None]
    return (nn_ + 2) * U32 * S + nn_ * FLUSH


def split_levels(table, feat_shapes):
    """A packed (rows, C) table back into the four (B, C, H, W) level tensors (the inverse of maskrcnn._pack_levels)."""
    out, o = [], 0
    for B, _, H, W in [tuple(s) for s in feat_shapes[:4]]:
        k = B * H * W
        out.append(table[o:o + k].view(B, H, W, -1).permute(0, 3, 1, 2))
        o += k
    return out


def check_backward(grads, feat_shapes, ref, S, n):
    """grads: the four levels' float32 gradients (CPU tensors, None for a level nothing reached); ref, S, n from
    roi_align_backward_ref.  Asserts every element within the bound and S == 0 => exactly +0.0.
    -> (worst err / bound over the elements with S > 0, n.max())."""
    assert int(n.max()) < BWD_N_MAX
    bound = backward_bound(S, n)
    worst = 0.0
    for l, (got, r, s, bd) in enumerate(zip(grads, split_levels(ref, feat_shapes), split_levels(S, feat_shapes),
                                            split_levels(bound, feat_shapes))):
        if got is None:
            got = torch.zeros(r.shape, dtype=torch.float32)
        assert got.dtype == torch.float32 and got.shape == r.shape, (l, got.dtype, got.shape)
        err = (got.double() - r).abs()
        bad = err > bd
        if bool(bad.any()):
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"level {l + 2} element {i}: got {float(got[i])!r} ref {float(r[i])!r} err {float(err[i]):.3e} "
                                 f"bound {float(bd[i]):.3e} ({int(bad.sum())} elements outside)")
        untouched = s == 0
        assert not bool(got[untouched].any()), f"level {l + 2}: an element no sample touches is not 0"
        assert not bool(torch.signbit(got[untouched]).any()), f"level {l + 2}: -0.0 in an untouched element"
        if bool((~untouched).any()):
            worst = max(worst, float((err[~untouched] / bd[~untouched]).max()))
    return worst, int(n.max())


# ------------------------------------------------------------------------------------------------ RoIAlign inputs
ROI_SIZE = 512                                        # the moulded image side the level rule refers to (224 / size)
ROI_CHANNELS = (1, 3, 64, 100, 256)
ROI_LEVELS = {'tall': ((40, 24), (20, 12), (10, 6), (5, 3), (3, 2)), 'wide': ((24, 40), (12, 20), (6, 10), (3, 5), (2, 3))}
ROI_FRAMES = 2


def roi_feat_shapes(orient, channels, frames=ROI_FRAMES):
    return [(frames, channels, h, w) for h, w in ROI_LEVELS[orient]]


def boxes_all_levels(K, seed=0):
    """tests/test_gpu_train.py::_boxes_all_levels on the host: sides for levels 2..5, centres in [-0.1, 1.1]."""
    rng = np.random.default_rng(seed)
    sides = np.array([0.08, 0.22, 0.44, 0.9])[rng.integers(0, 4, K)]
    c = rng.uniform(-0.1, 1.1, (K, 2))
    return np.concatenate([c - sides[:, None] / 2, c + sides[:, None] / 2], 1).astype(np.float32)


def roi_boxes(name):
    """-> boxes (K, 4) float32, frame (K,) int64.
    'full': 300 boxes — 195 of the all-levels mix, 100 identical ones (heavy contention on the same cells), [0, 0, 1, 1], two
            empty boxes (y2 = y1; x2 = x1), a zero-area point, and a box wholly off the map;
    'one':  K = 1; 'offmap': three boxes wholly off the map (every sample outside: no gradient at all)."""
    if name == 'full':
        b = np.concatenate([boxes_all_levels(195, seed=3),
                            np.tile(np.array([[0.31, 0.22, 0.46, 0.37]], np.float32), (100, 1)),
                            np.array([[0, 0, 1, 1], [0.4, 0.2, 0.4, 0.7], [0.2, 0.6, 0.9, 0.6], [0.5, 0.5, 0.5, 0.5],
                                      [1.2, 1.3, 1.6, 1.9]], np.float32)])
        frame = np.arange(len(b)) % ROI_FRAMES
        frame[195:295] = 1                                       # the identical boxes all in one frame
    elif name == 'one':
        b, frame = np.array([[0.13, 0.3, 0.58, 0.71]], np.float32), np.array([1])
    elif name == 'offmap':
        b = np.array([[1.2, 1.3, 1.6, 1.9], [-0.9, 0.1, -0.1, 0.5], [0.2, -2.0, 0.8, -1.5]], np.float32)
        frame = np.array([0, 1, 0])
    else:
        raise KeyError(name)
    return b, frame.astype(np.int64)


# ------------------------------------------------------------------------------------------------ RPN target inputs
GT_STRIDE = 100                                       # MAX_GT_INSTANCES: the kernels' GT_MAX
DECOY = (0.0, 0.0, 512.0, 512.0)                      # fills the GT rows past gt_count: a kernel that reads them changes its labels


def rpn_labels(anchors, gt):
    """Matterport's three-step rule before any subsampling, written apart from training.rpn_targets_host (one (A, G) matrix,
    broadcasting): -> match (A,) int32 in {1, 0, -1}."""
    A = len(anchors)
    if not len(gt):
        return np.full(A, -1, np.int32)
    a, g = anchors[:, None, :], np.asarray(gt, np.float64)[None, :, :]
    ih = np.maximum(np.minimum(a[..., 2], g[..., 2]) - np.maximum(a[..., 0], g[..., 0]), 0)
    iw = np.maximum(np.minimum(a[..., 3], g[..., 3]) - np.maximum(a[..., 1], g[..., 1]), 0)
    inter = iw * ih
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_g = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    iou = inter / (area_g + area_a - inter)
    best = iou.max(1)
    match = np.where(best < 0.3, -1, 0).astype(np.int32)
    match[(iou == iou.max(0)[None, :]).any(1)] = 1
    match[best >= 0.7] = 1
    return match


def hundred_boxes(seed=11, size=512):
    """100 GT boxes with sides of 16..300 px inside the image, integer pixel coordinates (extract_bboxes' kind)."""
    rng = np.random.default_rng(seed)
    hw = rng.integers(16, 301, (100, 2))
    y1 = (rng.uniform(0, 1, 100) * (size - hw[:, 0])).astype(np.int64)
    x1 = (rng.uniform(0, 1, 100) * (size - hw[:, 1])).astype(np.int64)
    return np.stack([y1, x1, y1 + hw[:, 0], x1 + hw[:, 1]], 1).astype(np.float64)


def _pad_gt(gts):
    gt = np.tile(np.array(DECOY, np.float64), (len(gts), GT_STRIDE, 1))
    for f, g in enumerate(gts):
        gt[f, :len(g)] = g
    return gt, np.array([len(g) for g in gts], np.int32)


RPN_BIG_FRAMES = ('hundred', 'hundred_equal_keys', 'hundred_keys_012', 'no_overlap', 'no_gt', 'six')


def rpn_big_batch(anchors):
    """One launch on the full anchor set, gt_stride 100, frames of different kinds side by side (RPN_BIG_FRAMES):
    100 boxes with random keys, the same with all keys equal and with keys from {0, 1, 2}, one box no anchor overlaps (far
    outside the image: every anchor ties at its maximum 0 and is a positive), no GT at all, six boxes (few positives).
    -> gt (B, 100, 4) float64 with decoys past gt_count, gt_count (B,) int32, keys (B, A) uint32."""
    A = len(anchors)
    rng = np.random.default_rng(5)
    hb = hundred_boxes()
    gts = [hb, hb, hb, np.array([[2000.0, 2100.0, 2100.0, 2300.0]]), np.zeros((0, 4)), hundred_boxes(seed=12)[:6]]
    keys = rng.integers(0, 2 ** 32, (len(gts), A), dtype=np.uint32)
    keys[1] = 0x9E3779B9
    keys[2] = rng.integers(0, 3, A, dtype=np.uint32)
    gt, cnt = _pad_gt(gts)
    return gt, cnt, keys


RPN_SMALL_SIZES = (1, 63, 300, 1024, 1025)
RPN_SMALL_GT = np.array([[200.0, 210.0, 264.0, 290.0]])


def rpn_small_set(anchors, A):
    """The A anchors of the real list whose centres lie nearest RPN_SMALL_GT's centre (list order kept), and a batch of three
    frames on them: that GT with random keys, the same with equal keys, and no GT.
    -> anchors (A, 4), gt (3, 100, 4), gt_count (3,), keys (3, A) uint32."""
    g = RPN_SMALL_GT[0]
    cy, cx = (anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2
    d = np.hypot(cy - (g[0] + g[2]) / 2, cx - (g[1] + g[3]) / 2)
    sub = np.ascontiguousarray(anchors[np.sort(np.argsort(d, kind='stable')[:A])])
    rng = np.random.default_rng(100 + A)
    keys = rng.integers(0, 2 ** 32, (3, A), dtype=np.uint32)
    keys[1] = 7
    gt, cnt = _pad_gt([RPN_SMALL_GT, RPN_SMALL_GT, np.zeros((0, 4))])
    return sub, gt, cnt, keys


# ------------------------------------------------------------------------------------------------ detection target inputs
ROI_STRIDE = 2048                                     # the kernels' ROI_MAX (the product uses 2000)
ROI_MASKS = ((96, 160), (160, 96))                    # mask_h, mask_w of the two batches: never square
ROI_FRAME_KINDS = ('hundred_gt', 'forty_equal_keys', 'no_proposals', 'no_gt', 'unit_square')


def _norm(boxes_px, shape):
    h, w = shape
    return ((boxes_px.astype(np.float64) - np.array([0, 0, 1, 1.0])) / np.array([h - 1, w - 1, h - 1, w - 1.0])).astype(np.float32)


def _gt_instances(n, shape, rng):
    """n GT instances on an (H, W) mask: pixel boxes with sides from 6 px to half the side, an ellipse filling each box (so that
    extract_bboxes of the mask is the box), classes 1..6.  -> boxes (n, 4) float32 normalised, classes, masks (n, H, W) uint8."""
    H, W = shape
    hh, ww = rng.integers(6, H // 2, n), rng.integers(6, W // 2, n)
    y1, x1 = (rng.uniform(0, 1, n) * (H - hh)).astype(np.int64), (rng.uniform(0, 1, n) * (W - ww)).astype(np.int64)
    px = np.stack([y1, x1, y1 + hh, x1 + ww], 1)
    masks = np.zeros((n, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, (a, b, c, d) in enumerate(px):
        cy, cx, ry, rx = (a + c - 1) / 2, (b + d - 1) / 2, (c - a) / 2, (d - b) / 2
        masks[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)
    return _norm(px, shape), rng.integers(1, 7, n).astype(np.int32), masks


def _random_props(n, rng):
    c = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    s = rng.uniform(0.02, 0.4, (n, 2)).astype(np.float32)
    return np.concatenate([c - s / 2, c + s / 2], 1).clip(0, 1).astype(np.float32)


def _jittered(gt, n, rng, sigma=0.01):
    return (gt[rng.integers(0, len(gt), n)] + rng.normal(0, sigma, (n, 4)).astype(np.float32)).clip(0, 1).astype(np.float32)


def roi_batch(which):
    """Batch `which` (0: 96 x 160 masks, 1: 160 x 96) of the detection-target cases, one frame per kind in ROI_FRAME_KINDS:
      hundred_gt        100 GT, 2048 proposals of which the first 600 are jittered around GT boxes;
      forty_equal_keys  6 GT, 40 proposals of which 30 are jittered around GT, all keys equal;
      no_proposals      6 GT, prop_count 0;
      no_gt             gt_count 0, 500 proposals;
      unit_square       two GT clipped to the unit square (one touching 0.0 and 1.0 in y, one in x), 40 exact copies as proposals
                        plus 20 random ones.
    Proposal rows past prop_count and GT rows past gt_count hold decoys (a full-frame box, class 9, an all-ones mask).
    -> dict of arrays for training.roi_targets_device: proposals (B, 2048, 4) f32, prop_count, gt (B, 100, 4) f32, gt_class,
    gt_count, gt_masks (B, 100, H, W) u8, keys (B, 2048) u32."""
    shape = ROI_MASKS[which]
    rng = np.random.default_rng(40 + which)
    B = len(ROI_FRAME_KINDS)
    props = np.tile(np.array([0, 0, 1, 1], np.float32), (B, ROI_STRIDE, 1))
    gt = np.tile(np.array([0, 0, 1, 1], np.float32), (B, GT_STRIDE, 1))
    cls = np.full((B, GT_STRIDE), 9, np.int32)
    masks = np.ones((B, GT_STRIDE) + shape, np.uint8)
    keys = rng.integers(0, 2 ** 32, (B, ROI_STRIDE), dtype=np.uint32)
    count, cnt = np.zeros(B, np.int32), np.zeros(B, np.int32)

    def put_gt(f, g, c, m):
        cnt[f] = len(g)
        gt[f, :len(g)], cls[f, :len(g)], masks[f, :len(g)] = g, c, m

    def put_props(f, p):
        count[f] = len(p)
        props[f, :len(p)] = p
    # hundred_gt
    g, c, m = _gt_instances(100, shape, rng)
    put_gt(0, g, c, m)
    p = _random_props(ROI_STRIDE, rng)
    p[:600] = _jittered(g, 600, rng)
    put_props(0, p)
    # forty_equal_keys
    g, c, m = _gt_instances(6, shape, rng)
    put_gt(1, g, c, m)
    p = _random_props(40, rng)
    p[:30] = _jittered(g, 30, rng)
    put_props(1, p[rng.permutation(40)])
    keys[1] = 123456789
    # no_proposals
    put_gt(2, *_gt_instances(6, shape, rng))
    # no_gt
    put_props(3, _random_props(500, rng))
    # unit_square
    H, W = shape
    px = np.array([[0, W // 4, H, W // 4 + W // 3], [H // 3, 0, H // 3 + H // 2, W]])
    g = _norm(px, shape).clip(0, 1)
    m = np.zeros((2,) + shape, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, (a, b, c_, d) in enumerate(px):
        m[i, a:c_, b:d] = ((yy + 2 * xx) % 5 != 0)[a:c_, b:d]                   # a pattern, so the last row and column matter
    put_gt(4, g, np.array([3, 5], np.int32), m)
    put_props(4, np.concatenate([np.repeat(g, 20, 0), _random_props(20, rng)])[rng.permutation(60)])
    return {'proposals': props, 'prop_count': count, 'gt': gt, 'gt_class': cls, 'gt_count': cnt, 'gt_masks': masks, 'keys': keys}


def roi_selection(proposals, gt):
    """The detection targets' counts for one frame, written apart from training.roi_targets_host: float32 IoU, positives
    >= 0.5.  -> (positives available, negatives available)."""
    p, g = proposals.astype(np.float32), gt.astype(np.float32)
    if not len(g):
        return 0, len(p)
    ih = np.maximum(np.minimum(p[:, None, 2], g[None, :, 2]) - np.maximum(p[:, None, 0], g[None, :, 0]), np.float32(0))
    iw = np.maximum(np.minimum(p[:, None, 3], g[None, :, 3]) - np.maximum(p[:, None, 1], g[None, :, 1]), np.float32(0))
    inter = iw * ih
    a1 = ((p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]))[:, None]
    a2 = ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[None, :]
    with np.errstate(invalid='ignore'):
        iou = inter / ((a1 + a2) - inter)
    best = np.where(np.isnan(iou), -np.inf, iou).max(1)
    return int((best >= 0.5).sum()), int((best < 0.5).sum())


def crop_rows_reached(box, shape, size=28):
    """The float32 sample rows / columns of the mask crop for one box: -> (in_y (size,), in_x (size,)) as crop_and_resize_mask
    and roi_targets_kernel compute them."""
    f = np.float32
    H, W = shape
    hm1, wm1, den = f(H - 1), f(W - 1), f(size - 1)
    y1, x1, y2, x2 = [f(v) for v in box]
    hs, ws = f(f(y2 - y1) * hm1) / den, f(f(x2 - x1) * wm1) / den
    k = np.arange(size, dtype=np.float32)
    return (y1 * hm1 + k * hs).astype(np.float32), (x1 * wm1 + k * ws).astype(np.float32)
