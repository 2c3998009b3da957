"""The references and input builders of tests/train_ref.py, held to account without a GPU: the RoIAlign backward reference and
its bound against float32 autograd and a case worked by hand, and every builder run through the host restatements to assert
that it reaches the edge it is named for (tests/test_gpu_train_kernels.py runs the kernels on the same inputs)."""
import numpy as np
import pytest
import torch

import train_ref as R
from rope_s3d_amd import maskrcnn as mr
from rope_s3d_amd import training as tr


# ------------------------------------------------------------------------------------------------ RoIAlign backward
@pytest.mark.parametrize('orient', ['tall', 'wide'])
@pytest.mark.parametrize('pool', [7, 14])
def test_backward_ref_against_autograd(orient, pool):
    """Float32 autograd through mr._roi_align on non-square levels, 96 channels, 300 boxes of which 100 are identical: every
    element within the bound, untouched elements exactly 0, nothing for P6, all four levels chosen, n > 500 on some row."""
    shapes = R.roi_feat_shapes(orient, 96)
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]
    boxes, frame = R.roi_boxes('full')
    assert len(boxes) == 300
    out = mr._roi_align(feats, torch.from_numpy(boxes), pool, R.ROI_SIZE, torch.from_numpy(frame))
    w = torch.randn(out.shape, generator=g)
    (out * w).sum().backward()
    tp = R.roi_align_taps(shapes, boxes, frame, pool, R.ROI_SIZE)
    assert set(tp['level'].tolist()) == {2, 3, 4, 5}
    ref, S, n = R.roi_align_backward_ref(shapes, boxes, frame, pool, R.ROI_SIZE, w)
    worst, n_max = R.check_backward([f.grad for f in feats[:4]], shapes, ref, S, n)
    print(f"autograd {orient} pool {pool}: worst err/bound {worst:.3f}, n max {n_max}")
    assert n_max > 500
    assert feats[4].grad is None
    # the reference is the gradient itself: float64 autograd through the same graph forms 1 - wy and 1 - wx in float64 where the
    # reference (as the kernel) rounds them to float32, one rounding per factor, and agrees in everything else
    f64 = [f.detach().double().requires_grad_(True) for f in feats]
    (mr._roi_align(f64, torch.from_numpy(boxes), pool, R.ROI_SIZE, torch.from_numpy(frame)) * w.double()).sum().backward()
    for a, b, s in zip(f64[:4], R.split_levels(ref, shapes), R.split_levels(S, shapes)):
        assert bool(((a.grad - b).abs() <= 2.5 * R.U32 * s + 1e-13).all())


def test_backward_ref_offmap_and_single():
    shapes = R.roi_feat_shapes('tall', 3)
    boxes, frame = R.roi_boxes('offmap')
    ref, S, n = R.roi_align_backward_ref(shapes, boxes, frame, 7, R.ROI_SIZE, np.ones((len(boxes), 3, 7, 7), np.float32))
    assert not ref.any() and not S.any() and not n.any()
    boxes, frame = R.roi_boxes('one')
    ref, S, n = R.roi_align_backward_ref(shapes, boxes, frame, 7, R.ROI_SIZE, np.ones((1, 3, 7, 7), np.float32))
    assert abs(float(ref.sum()) - 3 * 49) < 1e-4 and int(n.max()) >= 1          # the four weights of an inside sample sum to 1


def test_backward_ref_by_hand():
    """One box, pool 2, a 3 x 2 map (H = 3, W = 2), one channel, one frame.  The box (0.25, 0.125, 0.5, 0.375) has
    sqrt(h w) = 0.25 and size = 224 makes the level unit 1, so its level is round(4 + log2(0.25)) = 2: the 3 x 2 map
    (levels 3..5 are 1 x 1 and unused).
      ys = (0.25, 0.5) * (H - 1) = (0.5, 1.0)       y0 = (0, 1)   wy = (0.5, 0.0)
      xs = (0.125, 0.375) * (W - 1) = (0.125, 0.375) x0 = (0, 0)   wx = (0.125, 0.375)
    Rows of the packed table: level 2 is rows y * 2 + x, 0..5; levels 3, 4, 5 are rows 6, 7, 8."""
    shapes = [(1, 1, 3, 2), (1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1)]
    box = np.array([[0.25, 0.125, 0.5, 0.375]], np.float32)
    g = np.array([[[[1.0, -2.0], [4.0, 8.0]]]], np.float32)                     # g[py][px]
    ref, S, n = R.roi_align_backward_ref(shapes, box, np.array([0]), 2, 224, g)
    want = np.zeros(9)
    absw = np.zeros(9)
    cnt = np.zeros(9, np.int64)
    # sample (py, px): gradient, then (row, wy-factor, wx-factor) of its taps 00, 10, 01, 11
    hand = [
        (1.0, [(0, 0.5, 0.875), (2, 0.5, 0.875), (1, 0.5, 0.125), (3, 0.5, 0.125)]),        # ys 0.5, xs 0.125
        (-2.0, [(0, 0.5, 0.625), (2, 0.5, 0.625), (1, 0.5, 0.375), (3, 0.5, 0.375)]),       # ys 0.5, xs 0.375
        (4.0, [(2, 1.0, 0.875), (4, 0.0, 0.875), (3, 1.0, 0.125), (5, 0.0, 0.125)]),        # ys 1.0, xs 0.125
        (8.0, [(2, 1.0, 0.625), (4, 0.0, 0.625), (3, 1.0, 0.375), (5, 0.0, 0.375)]),        # ys 1.0, xs 0.375
    ]
    for grad, taps in hand:
        for row, a, b in taps:
            want[row] += grad * a * b
            absw[row] += abs(grad * a * b)
            cnt[row] += 1
    assert np.array_equal(ref[:, 0].numpy(), want)                              # dyadic weights: exact in float64
    assert np.array_equal(S[:, 0].numpy(), absw)
    assert np.array_equal(n.numpy(), cnt)
    assert want[0] == 0.5 * 0.875 - 2.0 * 0.5 * 0.625 and want[4] == 0.0 and cnt[4] == 2 and not want[6:].any()
    # and the same numbers from autograd
    feats = [torch.zeros(s, requires_grad=True) for s in shapes] + [torch.zeros((1, 1, 1, 1))]
    out = mr._roi_align(feats, torch.from_numpy(box), 2, 224, torch.zeros(1, dtype=torch.long))
    (out * torch.from_numpy(g)).sum().backward()
    assert np.array_equal(feats[0].grad.reshape(-1).double().numpy(), want[:6])


def test_backward_ref_clamped_tap_counts_once():
    """A sample on the last row (ys == H - 1) reaches that row through taps 00 and 10 (clamped); n counts the sample once and
    the clamped tap's weight is exactly 0."""
    shapes = [(1, 1, 3, 2), (1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1)]
    box = np.array([[0.75, 0.0, 1.0, 0.25]], np.float32)                        # ys = (1.5, 2.0), xs = (0, 0.25)
    tp = R.roi_align_taps(shapes, box, np.array([0]), 2, 224)
    assert tp['level'].tolist() == [2] and bool(tp['inside'].all())
    assert tp['r00'][0, 1].tolist() == [4, 4] and tp['r10'][0, 1].tolist() == [4, 4] and float(tp['wy'][0, 1, 0]) == 0.0
    _, _, n = R.roi_align_backward_ref(shapes, box, np.array([0]), 2, 224, np.ones((1, 1, 2, 2), np.float32))
    assert n.tolist()[:6] == [0, 0, 2, 2, 4, 4]                                 # rows 4, 5: two samples from each sample row


# ------------------------------------------------------------------------------------------------ RPN builders reach their edges
@pytest.fixture(scope='module')
def anchors():
    a = tr.anchors_px(512)
    assert a.shape == (65472, 4)
    return a


def test_rpn_labels_agree_with_host(anchors):
    """The second statement of the three-step rule (train_ref.rpn_labels) and training.rpn_targets_host label alike wherever the
    subsample cannot interfere (six boxes: fewer than 128 positives; the negatives kept are a subset)."""
    gt = R.hundred_boxes(seed=12)[:6]
    keys = np.random.default_rng(0).integers(0, 2 ** 32, len(anchors), dtype=np.uint32)
    lab = R.rpn_labels(anchors, gt)
    m, _, _ = tr.rpn_targets_host(anchors, gt, keys)
    assert 0 < (lab == 1).sum() <= 128 and np.array_equal(m == 1, lab == 1)
    assert (m == -1).sum() == 256 - (lab == 1).sum() and np.all(lab[m == -1] == -1)


def test_rpn_big_batch_reaches_its_edges(anchors):
    gt, cnt, keys = R.rpn_big_batch(anchors)
    names = R.RPN_BIG_FRAMES
    assert gt.shape == (len(names), R.GT_STRIDE, 4) and R.GT_STRIDE == tr.MAX_GT_INSTANCES
    assert cnt.tolist() == [100, 100, 100, 1, 0, 6]                             # mixed gt_count in one launch
    side = np.concatenate([gt[0, :, 2] - gt[0, :, 0], gt[0, :, 3] - gt[0, :, 1]])
    assert side.min() >= 16 and side.max() <= 300 and gt[0].min() >= 0 and gt[0].max() <= 512
    res = {}
    for f, name in enumerate(names):
        lab = R.rpn_labels(anchors, gt[f, :cnt[f]])
        m, bbox, arg = tr.rpn_targets_host(anchors, gt[f, :cnt[f]], keys[f])
        res[name] = (lab, m, bbox)
        print(f"rpn {name}: {int((lab == 1).sum())} positives and {int((lab == -1).sum())} negatives before the cap")
        assert np.all(lab[m == 1] == 1) and np.all(lab[m == -1] == -1)
    for name in names[:3]:                                                      # the positive cap: the bisection runs for label 1
        lab, m, bbox = res[name]
        assert (lab == 1).sum() > 128
        assert (m == 1).sum() == 128 and (m == -1).sum() == 128
        assert bbox[:128].any(1).all()                                          # a full 128 rows of packed deltas
    lab, m, _ = res['hundred_equal_keys']
    assert len(np.unique(keys[1])) == 1
    assert np.array_equal(np.where(m == 1)[0], np.where(lab == 1)[0][:128])     # ties: the lowest indices
    assert np.array_equal(np.where(m == -1)[0], np.where(lab == -1)[0][:128])
    lab, m, _ = res['hundred_keys_012']
    assert set(np.unique(keys[2]).tolist()) == {0, 1, 2}
    pos = np.where(lab == 1)[0]
    k0 = pos[keys[2][pos] == 0]
    assert len(k0) > 128 and np.array_equal(np.where(m == 1)[0], k0[:128])      # within key 0 the index decides
    lab, m, bbox = res['no_overlap']
    assert (lab == 1).sum() == 65472                                            # Matterport's rule: every anchor ties at IoU 0
    assert (m == 1).sum() == 128 and (m == -1).sum() == 0 and bbox[:128].any(1).all()
    lab, m, bbox = res['no_gt']
    assert (lab == -1).all() and (m == -1).sum() == 256 and (m == 1).sum() == 0 and not bbox.any()
    lab, m, _ = res['six']
    assert 0 < (lab == 1).sum() < 128 and (m == -1).sum() == 256 - (lab == 1).sum()


def test_rpn_small_sets_reach_their_edges(anchors):
    assert R.RPN_SMALL_SIZES == (1, 63, 300, 1024, 1025)
    for A in R.RPN_SMALL_SIZES:
        sub, gt, cnt, keys = R.rpn_small_set(anchors, A)
        assert sub.shape == (A, 4) and cnt.tolist() == [1, 1, 0] and keys.shape == (3, A)
        assert len(np.unique(keys[1])) == 1
        lab = R.rpn_labels(sub, gt[0, :1])
        m, bbox, _ = tr.rpn_targets_host(sub, gt[0, :1], keys[0])
        n_pos, n_neg = int((lab == 1).sum()), int((lab == -1).sum())
        print(f"rpn small A={A}: {n_pos} positives, {n_neg} negatives before the cap")
        assert 1 <= n_pos <= 128 and (m == 1).sum() == n_pos
        if A <= 300:
            assert n_neg < 256 - n_pos                                          # keep_smallest returns early: total <= keep
            assert (m == -1).sum() == n_neg
        else:
            assert n_neg > 256 - n_pos and (m == -1).sum() == 256 - n_pos       # the bisection on fewer than / just over 1024
        m0, _, _ = tr.rpn_targets_host(sub, gt[2, :0], keys[2])                 # no GT: min(A, 256) negatives
        assert (m0 == -1).sum() == min(A, 256)


# ------------------------------------------------------------------------------------------------ detection-target builders
@pytest.mark.parametrize('which', [0, 1])
def test_roi_batch_reaches_its_edges(which):
    d = R.roi_batch(which)
    H, W = R.ROI_MASKS[which]
    assert H != W and d['gt_masks'].shape == (5, 100, H, W) and d['proposals'].shape == (5, 2048, 4)
    assert R.ROI_STRIDE == 2048 and d['keys'].shape == (5, 2048) and len(R.ROI_FRAME_KINDS) <= 8
    out = {}
    for f, kind in enumerate(R.ROI_FRAME_KINDS):
        R_, G = d['prop_count'][f], d['gt_count'][f]
        avail = R.roi_selection(d['proposals'][f, :R_], d['gt'][f, :G])
        rois, cls, deltas, masks = tr.roi_targets_host(d['proposals'][f, :R_], d['gt'][f, :G], d['gt_class'][f, :G], d['gt_masks'][f, :G],
                                                       d['keys'][f])
        P = int((cls > 0).sum())
        N = int(rois[P:].any(1).sum())
        out[kind] = (R_, G, avail, P, N, rois, cls, masks)
        print(f"roi batch {which} {kind}: R {R_} G {G} available {avail} P {P} N {N}")
        assert np.all(cls[:P] > 0) and not cls[P:].any() and not masks[P:].any() and not rois[P + N:].any()
    R_, G, avail, P, N, *_ = out['hundred_gt']
    assert (R_, G) == (2048, 100) and avail[0] > 66 and (P, N) == (66, 134) and tr.negative_count(66) == 134
    R_, G, avail, P, N, rois, *_ = out['forty_equal_keys']
    assert R_ == 40 and len(np.unique(d['keys'][1])) == 1
    assert 0 < P == avail[0] and avail[1] < tr.negative_count(P) and N == avail[1] and P + N == 40      # too few negatives
    assert rois[:40].any(1).all() and not rois[40:].any()                       # the zero rows begin at row 40
    R_, G, avail, P, N, rois, cls, masks = out['no_proposals']
    assert R_ == 0 and G == 6 and P == 0 and N == 0 and not rois.any()
    R_, G, avail, P, N, rois, cls, masks = out['no_gt']
    assert R_ == 500 and G == 0 and P == 0 and N == 0 and not rois.any()       # negative_count(0) = 0: nothing kept
    R_, G, avail, P, N, rois, cls, masks = out['unit_square']
    g = d['gt'][4, :2]
    assert g[0, 0] == 0.0 and g[0, 2] == 1.0 and g[1, 1] == 0.0 and g[1, 3] == 1.0
    assert P >= 40 and {tuple(r) for r in rois[:P].tolist()} >= {tuple(r) for r in g.tolist()}
    in_y, _ = R.crop_rows_reached(g[0], (H, W))
    _, in_x = R.crop_rows_reached(g[1], (H, W))
    assert in_y[0] == 0.0 and in_y[-1] == np.float32(H - 1)                     # the last row itself is sampled: floor == ceil
    assert in_x[0] == 0.0 and in_x[-1] == np.float32(W - 1)
    assert masks[:P, -1].any() and masks[:P, :, -1].any()
