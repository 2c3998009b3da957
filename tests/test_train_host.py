"""Host side of Mask R-CNN training: labelme reading, the target restatements, losses, weight files and one CPU step."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from rope_s3d_amd import maskrcnn as mr
from rope_s3d_amd import training as tr
from rope_s3d_amd.data.annotation import encode_png
from rope_s3d_amd.data.labelme import decode_png, fill_polygon, read_annotation


# ------------------------------------------------------------------------------------------------ labelme
def test_fill_square_triangle_concave():
    sq = fill_polygon([(1, 1), (4, 1), (4, 4), (1, 4)], (6, 6))
    want = np.zeros((6, 6), bool)
    want[1:5, 1:5] = True                                   # closed rule: centres on all four edges and the corners are in
    assert np.array_equal(sq, want)
    tri = fill_polygon([(0.5, 0.5), (6.5, 0.5), (0.5, 6.5)], (8, 8))
    R, Cc = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
    assert np.array_equal(tri, (R >= 1) & (Cc >= 1) & (R + Cc <= 7))      # the centres on the hypotenuse x + y = 7 are in
    L = fill_polygon([(0.5, 0.5), (3.5, 0.5), (3.5, 2.5), (1.5, 2.5), (1.5, 4.5), (0.5, 4.5)], (6, 6))
    want = np.zeros((6, 6), bool)
    want[1:3, 1:4] = True
    want[3:5, 1] = True
    assert np.array_equal(L, want)
    # a concave L with integer vertices: the reflex corner (2, 2) and the inner edges are in, nothing outside the L is
    L2 = fill_polygon([(0, 0), (4, 0), (4, 2), (2, 2), (2, 4), (0, 4)], (6, 6))
    want = np.zeros((6, 6), bool)
    want[0:3, 0:5] = True
    want[0:5, 0:3] = True
    assert np.array_equal(L2, want)


def test_fill_vertices_on_centres():
    # a diamond with its vertices on pixel centres: every vertex and every centre on an edge is in (|r - 2| + |c - 2| <= 2)
    d = fill_polygon([(0, 2), (2, 0), (4, 2), (2, 4)], (5, 5))
    R, Cc = np.meshgrid(np.arange(5), np.arange(5), indexing='ij')
    assert np.array_equal(d, np.abs(R - 2) + np.abs(Cc - 2) <= 2) and d.sum() == 13
    # a centre just off an edge stays out; one on a vertex far from the others is in
    thin = fill_polygon([(0, 0), (6, 0), (6, 0.5)], (3, 8))
    assert thin[0].tolist() == [True] * 7 + [False] and not thin[1:].any()


def test_fill_round_trip_of_traced_plane():
    """A hole-free label plane traced by rope_trace_contours and written as a labelme shape fills back to the plane exactly: the
    contour runs through the centres of the border pixels, which the closed rule keeps.  Under a half-open rule (pnpoly's) the
    right and lower border pixels would be the ones to differ; they are counted here and all present."""
    from rope_s3d_amd.data.annotation import label_shapes
    Y, X = np.mgrid[0:40, 0:50]
    plane = (((Y - 18) ** 2 + (X - 22) ** 2 < 150) | ((Y > 20) & (Y < 34) & (X > 25) & (X < 44)))   # hole-free
    shapes = label_shapes(plane.astype(np.uint8), ['a'])
    assert len(shapes) == 1
    filled = fill_polygon(shapes[0]['points'], plane.shape)
    # border pixels whose right or lower neighbour is outside the region: what the edge rule decides
    pad = np.pad(plane, 1)
    decided = plane & (~pad[1:-1, 2:] | ~pad[2:, 1:-1])
    assert decided.sum() > 20
    assert int((filled != plane).sum()) == 0
    assert filled[decided].all()


def _png(rows_filters, img):
    h, w, c = img.shape
    bpp, stride = c, w * c
    raw, prev = b'', np.zeros(stride, np.int32)
    for y in range(h):
        line = img[y].reshape(-1).astype(np.int32)
        ft = rows_filters[y % len(rows_filters)]
        left = np.concatenate([np.zeros(bpp, np.int32), line[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        if ft == 0:
            enc = line
        elif ft == 1:
            enc = line - left
        elif ft == 2:
            enc = line - prev
        elif ft == 3:
            enc = line - ((left + prev) >> 1)
        else:
            p = left + prev - upleft
            pa, pb, pc = abs(p - left), abs(p - prev), abs(p - upleft)
            enc = line - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        raw += bytes([ft]) + (enc & 0xFF).astype(np.uint8).tobytes()
        prev = line

    def chunk(k, d):
        return struct.pack('>I', len(d)) + k + d + struct.pack('>I', zlib.crc32(k + d) & 0xFFFFFFFF)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw))
            + chunk(b'IEND', b''))


def test_png_decoder():
    rng = np.random.default_rng(1)
    bgr = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    assert np.array_equal(decode_png(encode_png(bgr)), bgr[..., ::-1])
    img = rng.integers(0, 256, (10, 9, 3), dtype=np.uint8)
    assert np.array_equal(decode_png(_png([0, 1, 2, 3, 4], img)), img)


def test_read_annotation(tmp_path):
    from rope_s3d_amd.data.annotation import write_annotation
    img = np.zeros((20, 30, 3), np.uint8)
    img[..., 1] = 7
    shapes = [{'label': 'b', 'points': [[2, 2], [10, 2], [10, 8], [2, 8]], 'group_id': None, 'shape_type': 'polygon', 'flags': {}},
              {'label': 'zz', 'points': [[0, 0], [3, 0], [3, 3]], 'group_id': None, 'shape_type': 'polygon', 'flags': {}}]
    write_annotation(img, shapes, str(tmp_path / '00000'))
    rgb, masks, ids = read_annotation(str(tmp_path / '00000.json'), ['a', 'b'])
    assert np.array_equal(rgb, img[..., ::-1]) and masks.shape == (1, 20, 30) and ids.tolist() == [2]
    assert masks[0].sum() == 9 * 7                          # columns 2..10, rows 2..8: the edges are in


# ------------------------------------------------------------------------------------------------ targets
def test_negative_count_float32():
    assert tr.negative_count(66) == 134
    assert tr.negative_count(0) == 0
    assert tr.ROI_POS_MAX == 66


def test_rpn_targets_low_iou_gt_gets_argmax_ties():
    an = np.array([[0, 0, 10, 10], [0, 10, 10, 20], [50, 50, 60, 60], [100, 100, 110, 110]], np.float64)
    gt = np.array([[0, 5, 4, 15]], np.float64)               # IoU 20/120 with anchors 0 and 1 alike, < 0.3
    match, bbox, arg = tr.rpn_targets_host(an, gt, np.arange(4, dtype=np.uint32))
    assert match.tolist() == [1, 1, -1, -1]
    assert np.all(bbox[2:] == 0) and np.all(bbox[:2, 2] == np.log(4 / 10) / 0.2)
    assert bbox[0, 1] == ((10.0 - 5.0) / 10) / 0.1 and bbox[1, 1] == ((10.0 - 15.0) / 10) / 0.1


def test_rpn_targets_cap_and_fill():
    an = np.stack([np.array([0, i * 0.005, 10, 10 + i * 0.005]) for i in range(200)] + [np.array([500, 500, 510, 510])] * 300)
    gt = np.array([[0, 0, 10, 10]], np.float64)
    keys = np.random.default_rng(3).integers(0, 2 ** 32, len(an), dtype=np.uint32)
    match, bbox, _ = tr.rpn_targets_host(an, gt, keys)
    assert (match == 1).sum() == 128 and (match == -1).sum() == 128
    kept = np.where(match[:200] == 1)[0]
    assert set(kept) == set(np.argsort(keys[:200], kind='stable')[:128])
    assert np.all(bbox[128:] == 0) and np.all(np.abs(bbox[:128]).sum(1) >= 0)


def test_rpn_targets_no_gt():
    an = tr.anchors_px(64)
    match, bbox, _ = tr.rpn_targets_host(an, np.zeros((0, 4)), np.arange(len(an), dtype=np.uint32)[::-1].copy())
    assert (match == -1).sum() == 256 and (match == 1).sum() == 0 and not bbox.any()
    assert np.all(match[-256:] == -1)                          # the smallest keys: the last anchors


def test_roi_targets_counts_padding_and_masks():
    rng = np.random.default_rng(0)
    gt = np.array([[0.1, 0.1, 0.5, 0.5]], np.float32)
    pos = gt + rng.uniform(-0.01, 0.01, (100, 4)).astype(np.float32)
    neg = np.array([[0.7, 0.7, 0.9, 0.9]], np.float32) + rng.uniform(-0.05, 0.05, (300, 4)).astype(np.float32)
    props = np.concatenate([pos, neg])
    m = np.zeros((1, 64, 64), np.uint8)
    m[0, 10:30, 10:40] = 1
    keys = rng.integers(0, 2 ** 32, len(props), dtype=np.uint32)
    rois, cls, deltas, masks = tr.roi_targets_host(props, gt, np.array([3], np.int32), m, keys)
    assert (cls == 3).sum() == 66 and np.all(cls[66:] == 0)
    assert np.all(rois[66:200].any(1)) and not deltas[66:].any() and not masks[66:].any()
    want = np.argsort(keys[:100], kind='stable')[:66]
    assert np.array_equal(rois[:66], props[want])
    # fewer proposals: 5 positives, int(float32(1/0.33) * 5) - 5 = 10 negatives, then zero rows
    rois, cls, _, _ = tr.roi_targets_host(props[95:110], gt, np.array([3], np.int32), m, keys[95:110])
    assert (cls == 3).sum() == 5 and rois[5:15].any(1).all() and not rois[15:].any()
    # no GT: every row padding
    rois, cls, deltas, masks = tr.roi_targets_host(props, np.zeros((0, 4), np.float32), np.zeros(0, np.int32), m[:0], keys)
    assert not rois.any() and not cls.any()


def test_roi_targets_zero_area_gt_is_no_overlap():
    # a zero-area GT box (a one-pixel-thin mask, normalised) against a zero-area proposal that misses it: IoU 0/0 counts as no
    # overlap, so the proposal is a negative (numpy's max / argmax alone would carry the NaN and drop it from both sets)
    gt = np.array([[0.2, 0.2, 0.2, 0.6]], np.float32)
    props = np.array([[0.9, 0.1, 0.9, 0.3]] * 5, np.float32)
    m = np.zeros((1, 16, 16), np.uint8)
    rois, cls, _, _ = tr.roi_targets_host(props, gt, np.array([2], np.int32), m, np.arange(5, dtype=np.uint32))
    assert not cls.any() and not rois.any()               # no positive: negative_count(0) = 0 rows of negatives
    gt2 = np.concatenate([gt, [[0.5, 0.5, 0.7, 0.7]]]).astype(np.float32)
    props2 = np.concatenate([props, [[0.5, 0.5, 0.7, 0.7]]]).astype(np.float32)
    rois, cls, _, _ = tr.roi_targets_host(props2, gt2, np.array([2, 4], np.int32), np.zeros((2, 16, 16), np.uint8),
                                          np.arange(6, dtype=np.uint32))
    assert cls.tolist()[:1] == [4] and np.array_equal(rois[1:3], props[:2])   # 1 positive, then int(3.03) - 1 = 2 negatives


def test_augment_acts_on_the_moulded_frame():
    x = torch.arange(3 * 8 * 8, dtype=torch.float32).view(3, 8, 8)
    m = np.zeros((1, 8, 8), np.uint8)
    m[0, :, :2] = 1

    class Draws:                                          # Sometimes fires, Fliplr fires, sigma 0 (no blur)
        def __init__(self):
            self.v = [0.1, 0.1]

        def random(self):
            return self.v.pop(0)

        def uniform(self, a, b):
            return 0.0
    y, mm = tr.augment(x, m, Draws())
    assert torch.equal(y, x.flip(-1)) and mm[0, :, 6:].all() and not mm[0, :, :6].any()
    b = tr.gaussian_blur(torch.ones(3, 16, 16), 2.0)
    assert torch.allclose(b, torch.ones(3, 16, 16), atol=1e-6)


def test_mask_target_by_hand():
    m = np.zeros((29, 29), np.uint8)
    m[0:15, :] = 1                                           # top half (rows 0..14)
    t = tr.crop_and_resize_mask(m, np.array([0, 0, 1, 1], np.float32))
    assert t.shape == (28, 28)
    # sample y of the full box sits at y * 28 / 27 pixels: rows <= 14 -> y <= 13.5
    assert np.all(t[:14] == 1) and np.all(t[14:] == 0)


# ------------------------------------------------------------------------------------------------ losses
def test_losses_by_hand():
    d = torch.tensor([0.5, 1.0, 2.0])
    assert tr.smooth_l1(d).tolist() == [0.125, 0.5, 1.5]
    match = torch.tensor([[1, 0, -1]])
    logits = torch.tensor([[[0.0, 0.0], [5.0, 1.0], [1.0, 0.0]]])
    want = (np.log(2) + np.log(1 + np.exp(-1))) / 2
    assert abs(float(tr.rpn_class_loss(match, logits)) - want) < 1e-6
    y = torch.tensor([[[0.0, 2.0], [-1.0, 0.0]]])
    t = torch.tensor([[[0.0, 1.0], [1.0, 0.0]]])
    got = tr.mrcnn_mask_loss(t, torch.tensor([1]), torch.stack([torch.zeros(2, 2), y[0]])[None])
    p = 1 / (1 + np.exp(-np.array([0.0, 2.0, -1.0, 0.0])))
    want = -np.mean([np.log(1 - p[0]), np.log(p[1]), np.log(p[2]), np.log(1 - p[3])])
    assert abs(float(got) - want) < 1e-6
    empty = tr.mrcnn_bbox_loss(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 7, 4))
    assert float(empty) == 0.0 and not torch.isnan(empty)
    assert float(tr.rpn_bbox_loss(torch.tensor([[0, -1]]), torch.zeros(1, 256, 4), torch.zeros(1, 2, 4))) == 0.0
    assert float(tr.mrcnn_mask_loss(torch.zeros(2, 28, 28), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 7, 28, 28))) == 0.0


def test_weight_decay_formula():
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.Linear(4, 5))
    want = sum(1e-4 * float((p.double() ** 2).sum()) / p.numel() for p in (net[0].weight, net[0].bias, net[2].weight, net[2].bias))
    assert abs(float(tr.weight_decay_term(net)) - want) < 1e-9


# ------------------------------------------------------------------------------------------------ weights and models
def test_save_load_matterport_round_trip(tmp_path, monkeypatch):
    from rope_s3d_amd.data import hdf5
    if not hdf5.available():
        pytest.skip("libhdf5 not found")
    torch.manual_seed(5)
    sd = mr.MaskRCNN(7).state_dict()
    path = mr.save_matterport_weights(sd, str(tmp_path / 'w.h5'))
    back = mr.load_matterport_weights(path, 7)
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    f = hdf5.H5File(path)
    attrs = f.attrs() if callable(getattr(f, 'attrs', None)) else f.attrs
    names = [n.decode() if isinstance(n, bytes) else n for n in np.asarray(attrs['layer_names']).tolist()]
    assert names[0] == 'conv1' and 'rpn_model' in names and 'mrcnn_mask' in names
    assert 'rpn_model/rpn_conv_shared/kernel:0' in set(f.walk())
    # Keras' loader takes a file without keras_version for a Keras 1 file and converts its deconvolution kernels
    txt = lambda v: v.decode() if isinstance(v, bytes) else str(np.asarray(v).item() if np.ndim(v) == 0 else v)
    assert txt(attrs['keras_version']) == '2.4.0' and txt(attrs['backend']) == 'tensorflow'
    f.close()
    ex = mr.load_matterport_weights(path, 7, exclude=('mrcnn_mask',))
    assert not torch.equal(ex['mask.14.weight'], sd['mask.14.weight']) and torch.equal(ex['mask.0.weight'], sd['mask.0.weight'])


def test_allocate_new_then_dynamic_load(tmp_path, monkeypatch):
    from rope_s3d_amd.data import hdf5
    from rope_s3d_amd.models import ModelManager, ModelData
    from rope_s3d_amd.config import Paths
    from rope_s3d_amd.data.dataset import SyntheticDataset
    monkeypatch.setenv('ROPE_OUTPUT', str(tmp_path / 'output'))
    anno = SyntheticDataset.link_anno_path_of('synthetic:4')
    assert anno == os.path.join(Paths().OUTPUT, 'synthetic_4_7919_640_480_color', 'link_annotations')
    for sub, n in (('train', 3), ('test', 1)):                 # the split annotate.py would leave: JSON + PNG per frame
        os.makedirs(os.path.join(anno, sub))
        for i in range(n):
            for ext in ('.json', '.png'):
                open(os.path.join(anno, sub, f'{i:05d}{ext}'), 'w').close()
    mm = ModelManager(str(tmp_path / 'models'))
    folder = mm.allocateNew('synthetic:4', ['a', 'b'])
    md = ModelData(folder)
    assert md.dataset == 'synthetic:4' and md.dataset_size == 4 and md.classes == ['a', 'b'] and len(md.id) == 4
    assert md.train_size == 3 and md.valid_size == 1
    ck = os.path.join(folder, 'mask_rcnn_model.003-1.250000.h5')
    if hdf5.available():
        mr.save_matterport_weights(mr.MaskRCNN(7).state_dict(), ck)
    else:
        open(ck, 'wb').close()
    assert ModelManager(str(tmp_path / 'models')).dynamicLoad(dataset='synthetic:4') == ck
    assert ModelManager(str(tmp_path / 'models')).info[md.id].epochs_trained == 3


# ------------------------------------------------------------------------------------------------ one CPU step
def _toy_samples(n, size=96, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        img = rng.integers(0, 60, (size, size, 3), dtype=np.uint8)
        masks = np.zeros((2, size, size), bool)
        y, x = rng.integers(5, 40, 2)
        masks[0, y:y + 30, x:x + 25] = True
        masks[1, 60:85, 10:50] = True
        img[masks[0]] = (200, 30, 30)
        img[masks[1]] = (30, 200, 30)
        out.append((img, masks, np.array([1, 2], np.int32)))
    return out


def test_cpu_step_heads_only_changes_heads():
    torch.manual_seed(0)
    net = mr.MaskRCNN(7, image_size=128)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    trainer = tr.MaskRCNNTrainer(net, layers='heads', seed=0, augmentation=False)
    out = trainer.step(_toy_samples(2))
    assert all(np.isfinite(out[k]) for k in tr.LOSS_NAMES)
    after = net.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed and all(k.startswith(tr.HEADS_PREFIXES) for k in changed)
    assert not any(k.endswith(('running_mean', 'running_var')) for k in changed)
    assert any(k.startswith('fpn.') for k in changed) and any(k.startswith('mask.') for k in changed)
