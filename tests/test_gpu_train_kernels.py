"""The six training kernels of rope_train.hip at the edges tests/test_gpu_train.py's single configuration does not reach: the
positive cap and tied keys of the RPN subsample, anchor sets below one selection chunk, full GT / proposal strides and empty
frames, non-square masks and feature levels, channel counts off the wave width, and the atomic RoIAlign backward under a
per-element bound (tests/train_ref.py, where the inputs are built; tests/test_train_refs.py asserts on the CPU that every input
reaches the edge it is named for, and the asserts on the host results below say so again)."""
import ctypes

import numpy as np
import pytest
import torch

import train_ref as R

pytestmark = pytest.mark.gpu

ROPE_E_ARG = -1


@pytest.fixture(scope='module')
def mods():
    torch.cuda.init()                                   # torch's context before the engine's
    from rope_s3d_amd import maskrcnn as mr
    from rope_s3d_amd import training as tr
    mr._seg_lib()
    return mr, tr


def _ulp_close(a, b, ulps=1):
    ia, ib = np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)
    return bool(np.all(np.abs(ia - ib) <= ulps))


def _cuda(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


# ------------------------------------------------------------------------------------------------ RPN targets
def _rpn_device(tr, anchors, gt, cnt, keys):
    out = tr.rpn_targets_device(_cuda(anchors), _cuda(gt), _cuda(cnt), _cuda(keys))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _rpn_compare(tr, anchors, gt, cnt, keys, got, tag):
    """Frame by frame against the host restatement; -> the host results."""
    match, bbox, arg = got
    host = []
    for f in range(len(cnt)):
        m, b, a = tr.rpn_targets_host(anchors, gt[f, :cnt[f]], keys[f])
        host.append((m, b, a))
        diff = np.where(match[f] != m)[0]
        assert not len(diff), f"{tag} frame {f}: match differs at {len(diff)} anchors, first {diff[0]}: {match[f][diff[0]]} != {m[diff[0]]}"
        rows = np.where((bbox[f, :, :2].view(np.int64) != b[:, :2].view(np.int64)).any(1))[0]
        assert not len(rows), f"{tag} frame {f}: delta rows differ, first {rows[0]}: {bbox[f, rows[0]]} != {b[rows[0]]}"
        assert _ulp_close(bbox[f, :, 2:], b[:, 2:]), f"{tag} frame {f}: log columns more than 1 ulp apart"
        pos = m == 1
        assert np.array_equal(arg[f][pos], a[pos]), f"{tag} frame {f}: anchor_arg differs at a positive"
    return host


def test_rpn_targets_cap_ties_and_mixed_frames(mods):
    _, tr = mods
    anchors = tr.anchors_px(512)
    gt, cnt, keys = R.rpn_big_batch(anchors)
    assert gt.shape[1] == 100 and len(set(cnt.tolist())) > 3
    got = _rpn_device(tr, anchors, gt, cnt, keys)
    host = dict(zip(R.RPN_BIG_FRAMES, _rpn_compare(tr, anchors, gt, cnt, keys, got, 'big')))
    match, bbox, _ = got
    for f, name in enumerate(R.RPN_BIG_FRAMES[:3]):
        lab = R.rpn_labels(anchors, gt[f, :cnt[f]])
        assert (lab == 1).sum() > 128                                           # the cap's bisection ran for the positives
        assert (match[f] == 1).sum() == 128 and (match[f] == -1).sum() == 128
        assert bbox[f, :128].any(1).all()
        if name == 'hundred_equal_keys':
            assert np.array_equal(np.where(match[f] == 1)[0], np.where(lab == 1)[0][:128])
            assert np.array_equal(np.where(match[f] == -1)[0], np.where(lab == -1)[0][:128])
        if name == 'hundred_keys_012':
            pos = np.where(lab == 1)[0]
            assert np.array_equal(np.where(match[f] == 1)[0], pos[keys[f][pos] == 0][:128])
    f = R.RPN_BIG_FRAMES.index('no_overlap')
    assert (R.rpn_labels(anchors, gt[f, :1]) == 1).sum() == 65472
    assert (match[f] == 1).sum() == 128 and (match[f] == -1).sum() == 0 and bbox[f, :128].any(1).all()
    f = R.RPN_BIG_FRAMES.index('no_gt')
    assert cnt[f] == 0 and (match[f] == -1).sum() == 256 and (match[f] == 1).sum() == 0 and not bbox[f].any()
    assert (host['six'][0] == 1).sum() < 128
    # determinism: the atomic max is order-free, the selection has no race
    again = _rpn_device(tr, anchors, gt, cnt, keys)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('A', R.RPN_SMALL_SIZES)
def test_rpn_targets_small_anchor_sets(mods, A):
    _, tr = mods
    sub, gt, cnt, keys = R.rpn_small_set(tr.anchors_px(512), A)
    assert len(sub) == A and gt.shape[1] == 100
    got = _rpn_device(tr, sub, gt, cnt, keys)
    host = _rpn_compare(tr, sub, gt, cnt, keys, got, f'A={A}')
    lab = R.rpn_labels(sub, gt[0, :1])
    n_pos, n_neg = int((lab == 1).sum()), int((lab == -1).sum())
    assert (got[0][0] == 1).sum() == n_pos >= 1
    if A <= 300:
        assert n_neg < 256 - n_pos and (got[0][0] == -1).sum() == n_neg         # too few negatives: the early return
    else:
        assert n_neg > 256 - n_pos and (got[0][0] == -1).sum() == 256 - n_pos
    assert (got[0][2] == -1).sum() == min(A, 256) and (host[2][0] == -1).sum() == min(A, 256)
    again = _rpn_device(tr, sub, gt, cnt, keys)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ detection targets
@pytest.mark.parametrize('which', [0, 1])
def test_roi_targets_edges_on_nonsquare_masks(mods, which):
    _, tr = mods
    d = R.roi_batch(which)
    H, W = R.ROI_MASKS[which]
    assert H != W and d['gt_masks'].shape[2:] == (H, W) and len(d['prop_count']) <= 8
    names = ('proposals', 'prop_count', 'gt', 'gt_class', 'gt_count', 'gt_masks', 'keys')
    out = tr.roi_targets_device(*[_cuda(d[k]) for k in names])
    torch.cuda.synchronize()
    rois, tcls, deltas, masks = [t.cpu().numpy() for t in out]
    seen = {}
    for f, kind in enumerate(R.ROI_FRAME_KINDS):
        R_, G = d['prop_count'][f], d['gt_count'][f]
        want = tr.roi_targets_host(d['proposals'][f, :R_], d['gt'][f, :G], d['gt_class'][f, :G], d['gt_masks'][f, :G], d['keys'][f])
        for name, a, b in zip(('rois', 'class_ids', 'deltas', 'masks'), (rois[f], tcls[f], deltas[f], masks[f]), want):
            bad = np.where((a.view(np.int32) != b.view(np.int32)).reshape(200, -1).any(1))[0]
            assert not len(bad), f"batch {which} {kind}: {name} differs in {len(bad)} rows, first {bad[0]}: {a[bad[0]]} != {b[bad[0]]}"
        P = int((want[1] > 0).sum())
        N = int(want[0][P:].any(1).sum())
        seen[kind] = (P, N)
        assert np.all(tcls[f, :P] > 0) and not tcls[f, P:].any() and not masks[f, P:].any()
    assert seen['hundred_gt'] == (66, 134)
    P, N = seen['forty_equal_keys']
    avail = R.roi_selection(d['proposals'][1, :40], d['gt'][1, :d['gt_count'][1]])
    assert P == avail[0] > 0 and N == avail[1] < tr.negative_count(P) and P + N == 40
    assert rois[1, :40].any(1).all() and not rois[1, 40:].any()
    assert seen['no_proposals'] == (0, 0) and not rois[2].any() and not deltas[2].any()
    assert seen['no_gt'] == (0, 0) and not rois[3].any()
    P, _ = seen['unit_square']
    g = d['gt'][4]
    in_y, _ = R.crop_rows_reached(g[0], (H, W))
    _, in_x = R.crop_rows_reached(g[1], (H, W))
    assert in_y[-1] == np.float32(H - 1) and in_x[-1] == np.float32(W - 1)
    assert P >= 40 and masks[4, :P, -1].any() and masks[4, :P, :, -1].any()


# ------------------------------------------------------------------------------------------------ RoIAlign float32
def _roi_case(mr, tr, orient, channels, pool, name, seed):
    """Forward bit-equal to the tensor formulation; two backward passes, each inside the bound.  -> worst err/bound, n max."""
    shapes = R.roi_feat_shapes(orient, channels)
    boxes_h, frame_h = R.roi_boxes(name)
    g = torch.Generator(device='cuda').manual_seed(seed)
    feats = [torch.randn(s, device='cuda', generator=g) for s in shapes]
    boxes, frame = torch.from_numpy(boxes_h).cuda(), torch.from_numpy(frame_h).cuda()
    with torch.no_grad():
        ref = mr._roi_align(feats, boxes, pool, R.ROI_SIZE, frame)
    assert ref.dtype == torch.float32
    w = torch.randn(ref.shape, device='cuda', generator=g)
    w_h = w.cpu()
    ref_sn = R.roi_align_backward_ref(shapes, boxes_h, frame_h, pool, R.ROI_SIZE, w_h)
    worst, n_max = 0.0, 0
    for run in range(2):                                # the second pass through a fresh forward: the atomics' order may differ
        f2 = [f.clone().requires_grad_(True) for f in feats]
        got = tr.roi_align_train(f2, boxes, pool, R.ROI_SIZE, frame)
        assert torch.equal(got, ref), (orient, channels, pool, name, run)
        (got * w).sum().backward()
        torch.cuda.synchronize()
        assert f2[4].grad is None or not bool(f2[4].grad.any())
        grads = [f.grad.cpu() for f in f2[:4]]
        wr, n_max = R.check_backward(grads, shapes, *ref_sn)
        worst = max(worst, wr)
        if name == 'offmap':
            assert not any(bool(gr.any()) for gr in grads) and not bool(got.any())
    return worst, n_max


@pytest.mark.parametrize('orient', ['tall', 'wide'])
@pytest.mark.parametrize('pool', [7, 14])
def test_roi_align_f32_channels_levels_and_bound(mods, orient, pool):
    mr, tr = mods
    boxes, frame = R.roi_boxes('full')
    assert len(boxes) == 300
    assert set(R.roi_align_taps(R.roi_feat_shapes(orient, 1), boxes, frame, pool, R.ROI_SIZE)['level'].tolist()) == {2, 3, 4, 5}
    assert R.ROI_CHANNELS == (1, 3, 64, 100, 256)
    n_full = 0
    for channels in R.ROI_CHANNELS:
        for name in ('full', 'one', 'offmap'):
            worst, n_max = _roi_case(mr, tr, orient, channels, pool, name, seed=channels + pool)
            print(f"roi_align bwd {orient} pool {pool} C {channels} {name}: worst err/bound {worst:.3f}, n max {n_max}")
            assert worst <= 1.0
            if name == 'full':
                n_full = max(n_full, n_max)
    assert n_full > 500                                                         # heavy contention: hundreds of adds into one cell


# ------------------------------------------------------------------------------------------------ ABI refusals (no launch)
def test_abi_refuses_out_of_range_arguments(mods):
    mr, _ = mods
    lib = mr._seg_lib()
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    p = buf.data_ptr()
    hw = np.array([[4, 4], [2, 2], [1, 1], [1, 1]], np.int32)
    off = np.array([0, 16, 20, 21], np.int64)
    bad_off = np.array([0, 16, -20, 21], np.int64)

    def rpn(n_anchors=8, gt_stride=4):
        return lib.rope_seg_rpn_targets(p, n_anchors, p, p, gt_stride, 1, p, p, p, p, p, p, None)

    def roi(prop_stride=8, gt_stride=4, mask_h=4, mask_w=4):
        return lib.rope_seg_roi_targets(p, p, prop_stride, p, p, p, gt_stride, p, mask_h, mask_w, 1, p, ctypes.c_float(3.0), p, p, p, p, None)

    def align(fn, channels=4, pool=2, level_off=off):
        return fn(p, p, p, hw.ctypes.data, level_off.ctypes.data, 1, channels, pool, ctypes.c_float(1.0), p, p, None)
    assert rpn(n_anchors=1 << 17) == ROPE_E_ARG
    assert rpn(gt_stride=101) == ROPE_E_ARG
    assert roi(prop_stride=2049) == ROPE_E_ARG
    assert roi(gt_stride=101) == ROPE_E_ARG
    assert roi(mask_h=1) == ROPE_E_ARG
    for fn in (lib.rope_seg_roi_align_float, lib.rope_seg_roi_align_backward):
        assert align(fn, channels=0) == ROPE_E_ARG
        assert align(fn, pool=0) == ROPE_E_ARG
        assert align(fn, level_off=bad_off) == ROPE_E_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())                                                  # nothing was launched on it
