"""GPU: the overlap counts of the segmentation evaluation (rope_seg_mask_overlaps, csrc/rope_eval.hip; evaluation.mask_overlaps)
against numpy, exactly, at the sizes where the kernel's cut of a plane into head, 16-byte body and tail can go wrong; then the
evaluator end to end on a stub segmenter whose detections are built from the ground truth itself, against eval_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng
from rope_s3d_amd import evaluation as ev

import eval_ref

pytestmark = pytest.mark.gpu

E_ARG = -1
GARBAGE = 0x5A5A5A5A
VALUES = np.array([0, 1, 2, 255], np.uint8)


def _numpy_counts(pred, first, gt):
    """(pred != 0) & ((gt >> b) & 1), summed."""
    F = len(gt)
    frame_of = np.repeat(np.arange(F), np.diff(first))
    labels = ((gt[:, None] >> np.arange(8, dtype=np.uint8)[None, :, None, None]) & 1).astype(bool)          # (F, 8, H, W)
    on = pred != 0
    inter = np.array([[(on[k] & labels[frame_of[k], b]).sum() for b in range(8)] for k in range(len(pred))], np.int64).reshape(-1, 8)
    return inter, on.sum(axis=(1, 2)).astype(np.int64), labels.sum(axis=(2, 3)).astype(np.int64)


def _device_bytes(a, offset):
    """The array's bytes on the GPU, starting `offset` bytes into an allocation: the base address is then not 16-byte aligned."""
    flat = torch.empty(a.size + offset + 16, dtype=torch.uint8, device='cuda')
    view = flat[offset:offset + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return view.reshape(a.shape)


def _call(pred, first, gt, offsets=(0, 0)):
    """The C entry point on outputs filled with garbage -> (rc, inter, area_pred, area_gt) as uint32 arrays, garbage included."""
    F, H, W = gt.shape
    K = int(first[-1])
    d_pred, d_gt = _device_bytes(pred, offsets[0]), _device_bytes(gt, offsets[1])
    out = [torch.full(s, GARBAGE, dtype=torch.int32, device='cuda') for s in ((K, 8), (K,), (F, 8))]
    first = np.ascontiguousarray(first, np.int32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None                                            # noqa: E731
    rc = eng.load_library().rope_seg_mask_overlaps(p(d_pred), first.ctypes.data_as(C.c_void_p), F, p(d_gt), H, W, *[p(t) for t in out],
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy().view(np.uint32) for t in out)


def _planes(rng, counts, H, W):
    """Seeded planes with bytes from {0, 1, 2, 255}, one of them all ones; label planes using all eight bits (they overlap), one
    of them all zero when there are several frames."""
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pred = rng.choice(VALUES, (int(first[-1]), H, W), p=[0.55, 0.15, 0.15, 0.15])
    if len(pred):
        pred[len(pred) // 2] = 255
    gt = rng.integers(0, 256, (len(counts), H, W), dtype=np.uint8)
    gt[..., -1, -1] |= 0x80                                                                                  # bit 7 at the last pixel
    if len(counts) > 1:
        gt[int(np.argmax(counts))] = 0
    return pred, first, gt


def _check(pred, first, gt, offsets=(0, 0)):
    rc, inter, area_pred, area_gt = _call(pred, first, gt, offsets)
    want = _numpy_counts(pred, first, gt)
    assert rc == 0
    for name, got, w in zip(('inter', 'area_pred', 'area_gt'), (inter, area_pred, area_gt), want):
        assert got.shape == w.shape and np.array_equal(got.astype(np.int64), w), (name, gt.shape, list(first), offsets)


SIZES = [(1, 1), (3, 5), (7, 9), (16, 16), (33, 31), (120, 160)]
LAYOUTS = [[3], [0, 1, 5], [1, 0, 5], [1, 5, 0]]


@pytest.mark.parametrize('H,W', SIZES)
def test_counts_equal_numpy(H, W):
    """Every layout at every size; at 3 x 5 no plane holds a whole vector, at 33 x 31 (1 023 bytes) every plane after the first
    starts at another offset from a 16-byte boundary."""
    rng = np.random.default_rng(1000 * H + W)
    for counts in LAYOUTS:
        _check(*_planes(rng, counts, H, W))


@pytest.mark.parametrize('H,W', [(7, 9), (33, 31), (16, 16)])
def test_counts_with_misaligned_base_addresses(H, W):
    """The stack of planes and the label planes themselves start off a 16-byte boundary, each by another amount."""
    rng = np.random.default_rng(77 + H)
    for offsets in ((3, 0), (0, 5), (13, 6), (1, 1)):
        _check(*_planes(rng, [2, 0, 4], H, W), offsets=offsets)


def test_hundred_instances_in_one_frame():
    _check(*_planes(np.random.default_rng(100), [100], 33, 31))


def test_full_size_planes_are_split_over_workgroups():
    """480 x 640 with three planes: a plane is cut over many workgroups, whose sums meet in the atomics."""
    pred, first, gt = _planes(np.random.default_rng(480), [3], 480, 640)
    _check(pred, first, gt)
    _check(pred[:, :, :639].copy(), first, gt[:, :, :639].copy())                                            # 480 x 639: misaligned planes, split


def test_all_ones_planes_and_empty_labels():
    H, W = 33, 31
    pred = np.full((2, H, W), 1, np.uint8)
    gt = np.zeros((2, H, W), np.uint8)
    gt[1] = 0xFF
    rc, inter, area_pred, area_gt = _call(pred, [0, 1, 2], gt)
    assert rc == 0 and area_pred.tolist() == [H * W] * 2
    assert inter.tolist() == [[0] * 8, [H * W] * 8] and area_gt.tolist() == [[0] * 8, [H * W] * 8]


def test_same_input_twice_gives_identical_bytes():
    pred, first, gt = _planes(np.random.default_rng(9), [4, 3], 120, 160)
    a, b = _call(pred, first, gt), _call(pred, first, gt)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def test_no_instance_still_fills_area_gt():
    _, first, gt = _planes(np.random.default_rng(4), [0, 0], 33, 31)
    rc, inter, area_pred, area_gt = _call(np.zeros((0, 33, 31), np.uint8), first, gt)
    assert rc == 0 and inter.shape == (0, 8) and np.array_equal(area_gt.astype(np.int64), _numpy_counts(np.zeros((0, 33, 31), np.uint8), first, gt)[2])
    i, a, g = ev.mask_overlaps(None, [0, 0, 0], torch.from_numpy(gt).cuda())
    assert i.shape == (0, 8) and a.shape == (0,) and np.array_equal(g, area_gt.astype(np.int64))


def test_decreasing_inst_first_is_refused_on_the_host():
    """ROPE_E_ARG before anything is enqueued: the outputs keep the garbage they were filled with."""
    pred, _, gt = _planes(np.random.default_rng(5), [2, 1], 16, 16)
    rc, inter, area_pred, area_gt = _call(pred, np.array([0, 3, 2], np.int32), gt)
    assert rc == E_ARG
    assert (inter == GARBAGE).all() and (area_pred == GARBAGE).all() and (area_gt == GARBAGE).all()
    with pytest.raises(ValueError):
        ev.mask_overlaps(torch.from_numpy(pred[:2]).cuda(), [0, 3, 2], torch.from_numpy(gt).cuda())


def test_mask_overlaps_takes_views_and_refuses_other_dtypes():
    rng = np.random.default_rng(6)
    pred, first, gt = _planes(rng, [2, 3], 33, 31)
    want = _numpy_counts(pred, first, gt)
    d_gt = torch.from_numpy(gt).cuda()
    wide = torch.zeros((5, 33, 62), dtype=torch.uint8, device='cuda')
    wide[:, :, ::2] = torch.from_numpy(pred).cuda()
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    for masks in (view, torch.from_numpy(pred).cuda(), torch.from_numpy(pred != 0).cuda()):
        got = ev.mask_overlaps(masks, first, d_gt)
        assert all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want))
    tall = torch.from_numpy(np.ascontiguousarray(gt.transpose(0, 2, 1))).cuda().transpose(1, 2)            # label planes as a view, too
    assert not tall.is_contiguous() and all(np.array_equal(g, w) for g, w in zip(ev.mask_overlaps(view, first, tall), want))
    for bad in (torch.from_numpy(pred).cuda().float(), torch.from_numpy(pred).cuda().to(torch.int32)):
        with pytest.raises(ValueError):
            ev.mask_overlaps(bad, first, d_gt)
    with pytest.raises(ValueError):
        ev.mask_overlaps(torch.from_numpy(pred).cuda()[:, :32], first, d_gt)                                # another plane size
    with pytest.raises(ValueError):
        ev.mask_overlaps(torch.from_numpy(pred).cuda()[:4], first, d_gt)                                    # fewer planes than inst_first names
    with pytest.raises(ValueError):
        ev.mask_overlaps(torch.from_numpy(pred).cuda(), first, d_gt.to(torch.int32))


# ---------------------------------------------------------------------------------------------- the evaluator, end to end
N_CLASSES = 6
CLASS_NAMES = [f'link{b}' for b in range(N_CLASSES)]
SHIFT = 3


@pytest.fixture(scope='module')
def scene():
    """Label planes of five poses at 160 x 120 (Renderer.render_masks_batch) and a sixth frame with no label."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.simulation.render import Renderer
    r = Renderer('seg', DEFAULT_CAMERA_POSE, '640_480_color', intrinsic_ds_factor=4)
    lim = r.robot.joint_limits
    q = np.zeros((5, 6))
    q[:, :3] = np.random.default_rng(11).uniform(lim[:3, 0], lim[:3, 1], (5, 3))
    masks, _ = r.render_masks_batch(q, pad=3)
    r.engine.close()
    assert masks.shape == (5, 120, 160) and max(bin(int(np.bitwise_or.reduce(m, axis=None))).count('1') for m in masks) >= 2
    gt = np.concatenate([masks, np.zeros((1, 120, 160), np.uint8)])
    gt.setflags(write=False)
    return gt


def _exact(gt):
    """Per frame the planes of its labels as detections: (masks (K, H, W) bool, class ids, scores)."""
    frames = []
    for plane in gt:
        labels = [b for b in range(N_CLASSES) if ((plane >> b) & 1).any()]
        masks = np.stack([((plane >> b) & 1).astype(bool) for b in labels]) if labels else np.zeros((0,) + plane.shape, bool)
        frames.append((masks, np.array([b + 1 for b in labels], np.int32), np.array([0.95 - 0.01 * b for b in labels], np.float32)))
    return frames


class StubSegmenter:
    """batches_device of MaskRCNNSegmenter, with the detections given: frames are handed out in order, whatever the colours."""
    device = 'cuda:0'

    def __init__(self, frames, stacked):
        self.frames, self.stacked = frames, stacked

    def batches_device(self, groups):
        at = 0
        for g in groups:
            mine = self.frames[at:at + len(g)]
            at += len(g)
            dev = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m, _, _ in mine]
            stack, first = (torch.cat(dev), np.concatenate([[0], np.cumsum([len(m) for m in dev])])) if self.stacked else (None, None)
            yield [{'class_ids': c, 'scores': s, 'masks_device': stack[first[j]:first[j + 1]] if self.stacked else dev[j],
                    'masks_stacked': (stack, int(first[j])) if self.stacked else None} for j, (_, c, s) in enumerate(mine)]


def _run(frames, gt, stacked, batch=4):
    colors = np.zeros((len(gt), 120, 160, 3), np.uint8)
    return ev.SegmentationEvaluator(StubSegmenter(frames, stacked), CLASS_NAMES, batch).run(colors, gt)


def _same_as_ref(got, frames, gt):
    want = eval_ref.evaluate(frames, gt, N_CLASSES)
    assert got['frames'] == len(gt) and got['frames_skipped'] == want['frames_skipped']
    for key in ('AP', 'AP50', 'AP75'):
        assert abs(got[key] - want[key]) <= 1e-12, key
    assert np.allclose(got['AP50_per_frame'], want['AP50_per_frame'], rtol=0, atol=1e-12, equal_nan=True)
    for b, name in enumerate(CLASS_NAMES):
        c = got['classes'][name]
        assert c['frames'] == want['frames_present'][b]
        assert abs(c['detection_rate'] - want['detection_rate'][b]) <= 1e-12 and abs(c['mean_iou'] - want['mean_iou'][b]) <= 1e-12
    return want


@pytest.mark.parametrize('stacked', [True, False])
def test_evaluator_on_detections_built_from_the_ground_truth(scene, stacked):
    gt = scene
    # (a) exact copies, (d) the empty frame is skipped
    got = _run(_exact(gt), gt, stacked)
    assert got['frames_skipped'] == 1 and np.isnan(got['AP50_per_frame'][5]) and (got['AP50_per_frame'][:5] == 1.0).all()
    assert got['AP'] == got['AP50'] == got['AP75'] == 1.0
    assert all(c['mean_iou'] == 1.0 and c['detection_rate'] == 1.0 for c in got['classes'].values() if c['frames'])
    assert sum(c['frames'] for c in got['classes'].values()) == sum(len(m) for m, _, _ in _exact(gt))
    _same_as_ref(got, _exact(gt), gt)

    # (b) the largest label of the first frame, shifted by SHIFT columns
    frames = _exact(gt)
    assert len(frames[0][0])
    masks, cls, sc = frames[0]
    k = int(np.argmax(masks.reshape(len(masks), -1).sum(axis=1)))
    b = int(cls[k]) - 1
    moved = np.zeros_like(masks[k])
    moved[:, SHIFT:] = masks[k][:, :-SHIFT]
    label = ((gt[0] >> b) & 1).astype(bool)
    iou = (moved & label).sum() / (moved | label).sum()
    assert 0.0 < iou < 1.0
    masks = masks.copy()
    masks[k] = moved
    frames[0] = (masks, cls, sc)
    got = _run(frames, gt, stacked)
    name = CLASS_NAMES[b]
    n = got['classes'][name]['frames']
    assert abs(got['classes'][name]['mean_iou'] - ((n - 1) + (iou if iou >= 0.5 else 0.0)) / n) <= 1e-12
    assert (got['AP50'] == 1.0) == (iou >= 0.5) and (got['AP75'] == 1.0) == (iou >= 0.75) and got['AP'] < 1.0
    assert (got['classes'][name]['detection_rate'] == 1.0) == (iou >= 0.5)
    _same_as_ref(got, frames, gt)

    # (c) one label dropped, one duplicated with a lower score
    frames = _exact(gt)
    f = int(np.argmax([len(m) for m, _, _ in frames]))                                                       # the frame with the most labels
    masks, cls, sc = frames[f]
    assert len(masks) >= 2
    frames[f] = (np.concatenate([masks[1:], masks[1:2]]), np.concatenate([cls[1:], cls[1:2]]), np.concatenate([sc[1:], [0.5]]).astype(np.float32))
    got = _run(frames, gt, stacked)
    want = _same_as_ref(got, frames, gt)
    dropped = CLASS_NAMES[int(cls[0]) - 1]
    assert got['classes'][dropped]['detection_rate'] == (got['classes'][dropped]['frames'] - 1) / got['classes'][dropped]['frames']
    assert got['AP50'] < 1.0 and want['AP50'] < 1.0

    # (e) the size of the groups changes nothing
    one, four = _run(frames, gt, stacked, batch=1), _run(frames, gt, stacked, batch=4)
    assert one['AP50_per_frame'].tobytes() == four['AP50_per_frame'].tobytes()
    assert {k: v for k, v in one.items() if k != 'AP50_per_frame'} == {k: v for k, v in four.items() if k != 'AP50_per_frame'}
