"""Mask R-CNN training on PyTorch-ROCm: the link between annotated renders and the segmentation stage (reference: train.py,
which runs PixelLib 0.5.6 instance_custom_training, i.e. Matterport's training graph, mrcnn/model.py).

`MaskRCNNTrainer` trains `maskrcnn.MaskRCNN`'s own modules in float32; the inference path (detect*, _fold_batchnorm, the
bfloat16 kernels) is not touched.  The steps of a training step that are not library convolutions run as HIP kernels on the GPU
(rope_train.hip): the RPN targets, the detection targets and the float32 pyramid RoIAlign with its backward pass.  The host
restatements below (`rpn_targets_host`, `roi_targets_host`) are what those kernels are tested against, and what a CPU run uses.

Matterport's settings (mrcnn/config.py, model.py), as PixelLib's modelConfig leaves them:
  RPN_TRAIN_ANCHORS_PER_IMAGE 256 (at most half positive), RPN IoU < 0.3 negative / >= 0.7 positive, POST_NMS_ROIS_TRAINING 2000,
  TRAIN_ROIS_PER_IMAGE 200, ROI_POSITIVE_RATIO 0.33, MAX_GT_INSTANCES 100, MASK_SHAPE 28, TRAIN_BN False,
  LEARNING_RATE 0.001, LEARNING_MOMENTUM 0.9, WEIGHT_DECAY 0.0001, GRADIENT_CLIP_NORM 5.0, every loss weight 1.
Deviations: per-element keys from one seeded generator stand in for np.random.choice / tf.random_shuffle; GT masks
are kept at the moulded image's resolution (no 56 x 56 mini mask); the gradient clip is per tensor (tf.keras' clipnorm, which
PixelLib's TF 2 stack uses); the augmentation rule is restated from memory and could not be checked; an IoU of 0/0 in the
detection targets counts as no overlap.
"""
import logging
import math
import os
from typing import List

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import maskrcnn as mr

RPN_ANCHORS_PER_IMAGE, RPN_POS_MAX = 256, 128
RPN_NEG_IOU, RPN_POS_IOU = 0.3, 0.7
POST_NMS_ROIS_TRAINING = 2000
TRAIN_ROIS_PER_IMAGE, ROI_POSITIVE_RATIO = 200, 0.33
ROI_POS_MAX = int(TRAIN_ROIS_PER_IMAGE * ROI_POSITIVE_RATIO)            # 66
INV_POSITIVE_RATIO = np.float32(1.0 / ROI_POSITIVE_RATIO)              # r = 1.0 / ROI_POSITIVE_RATIO, a float32 tensor in the graph
MAX_GT_INSTANCES = 100
LEARNING_RATE, LEARNING_MOMENTUM, WEIGHT_DECAY, GRADIENT_CLIP_NORM = 0.001, 0.9, 0.0001, 5.0
HEADS_PREFIXES = ('fpn.', 'rpn.', 'head.', 'cls.', 'box.', 'mask.')    # layers='heads': r"(mrcnn\_.*)|(rpn\_.*)|(fpn\_.*)"
LOSS_NAMES = ('rpn_class_loss', 'rpn_bbox_loss', 'mrcnn_class_loss', 'mrcnn_bbox_loss', 'mrcnn_mask_loss')


def negative_count(positives: int) -> int:
    """tf.cast(r * tf.cast(positive_count, tf.float32), tf.int32) - positive_count, in float32 (134 for 66 positives)."""
    return int(np.float32(INV_POSITIVE_RATIO * np.float32(positives))) - positives


# ------------------------------------------------------------------------------------------------ anchors and GT
def anchors_px(size: int) -> np.ndarray:
    """utils.generate_pyramid_anchors (anchor stride 1) in float64 pixel coordinates, the order of the RPN heads' outputs."""
    out = []
    for scale, stride in zip(mr.RPN_ANCHOR_SCALES, mr.BACKBONE_STRIDES):
        n = int(math.ceil(size / stride))
        scales, ratios = np.meshgrid(np.array([scale], np.float64), np.array(mr.RPN_ANCHOR_RATIOS, np.float64))
        scales, ratios = scales.flatten(), ratios.flatten()
        heights, widths = scales / np.sqrt(ratios), scales * np.sqrt(ratios)
        shifts = np.arange(0, n) * stride
        sx, sy = np.meshgrid(shifts, shifts)
        bw, bcx = np.meshgrid(widths, sx)
        bh, bcy = np.meshgrid(heights, sy)
        centers = np.stack([bcy, bcx], axis=2).reshape([-1, 2])
        sizes = np.stack([bh, bw], axis=2).reshape([-1, 2])
        out.append(np.concatenate([centers - 0.5 * sizes, centers + 0.5 * sizes], axis=1))
    return np.ascontiguousarray(np.concatenate(out, axis=0))


def extract_bboxes(masks: np.ndarray) -> np.ndarray:
    """utils.extract_bboxes of (G, H, W) masks -> (G, 4) int32 (y1, x1, y2, x2), y2 and x2 one past the last pixel."""
    out = np.zeros((len(masks), 4), np.int32)
    for i, m in enumerate(masks):
        ys, xs = np.where(m.any(axis=1))[0], np.where(m.any(axis=0))[0]
        if len(ys):
            out[i] = (ys[0], xs[0], ys[-1] + 1, xs[-1] + 1)
    return out


def norm_boxes(boxes: np.ndarray, shape) -> np.ndarray:
    """utils.norm_boxes: (boxes - (0, 0, 1, 1)) / (h - 1, w - 1, h - 1, w - 1) in float64, then float32."""
    h, w = shape
    scale = np.array([h - 1, w - 1, h - 1, w - 1], np.float64)
    shift = np.array([0, 0, 1, 1], np.float64)
    return np.divide(boxes.astype(np.float64) - shift, scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ host restatements
def rpn_targets_host(anchors: np.ndarray, gt: np.ndarray, keys: np.ndarray):
    """build_rpn_targets of one frame (float64, pixel coordinates) with keys for np.random.choice: the kept positives (at
    most 128) and negatives (256 - positives) are those with the smallest (key, index).
    -> match (A,) int32 (1 / -1 / 0), bbox (256, 4) float64, anchor_arg (A,) int32.  No GT: every anchor is a negative."""
    A = len(anchors)
    match = np.zeros(A, np.int32)
    if len(gt):
        gt = gt.astype(np.float64)
        gt_area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
        a_area = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
        ov = np.zeros((A, len(gt)))
        for i in range(len(gt)):                          # utils.compute_overlaps -> compute_iou(gt_i, anchors, ...)
            y1, y2 = np.maximum(gt[i, 0], anchors[:, 0]), np.minimum(gt[i, 2], anchors[:, 2])
            x1, x2 = np.maximum(gt[i, 1], anchors[:, 1]), np.minimum(gt[i, 3], anchors[:, 3])
            inter = np.maximum(x2 - x1, 0) * np.maximum(y2 - y1, 0)
            ov[:, i] = inter / (gt_area[i] + a_area[:] - inter[:])
        arg = np.argmax(ov, axis=1).astype(np.int32)
        amax = ov[np.arange(A), arg]
        match[amax < RPN_NEG_IOU] = -1
        match[np.argwhere(ov == np.max(ov, axis=0))[:, 0]] = 1
        match[amax >= RPN_POS_IOU] = 1
    else:
        arg = np.zeros(A, np.int32)
        match[:] = -1
    comp = (keys.astype(np.uint64) << np.uint64(17)) | np.arange(A, dtype=np.uint64)

    def keep_smallest(lab, keep):
        ids = np.where(match == lab)[0]
        if len(ids) > keep:
            drop = ids[np.argsort(comp[ids], kind='stable')[keep:]]
            match[drop] = 0
    keep_smallest(1, RPN_POS_MAX)
    keep_smallest(-1, RPN_ANCHORS_PER_IMAGE - int(np.sum(match == 1)))
    bbox = np.zeros((RPN_ANCHORS_PER_IMAGE, 4))
    std = np.array(mr.RPN_BBOX_STD_DEV)
    for ix, i in enumerate(np.where(match == 1)[0]):
        a, g = anchors[i], gt[arg[i]]
        gh, gw = g[2] - g[0], g[3] - g[1]
        gcy, gcx = g[0] + 0.5 * gh, g[1] + 0.5 * gw
        ah, aw = a[2] - a[0], a[3] - a[1]
        acy, acx = a[0] + 0.5 * ah, a[1] + 0.5 * aw
        bbox[ix] = [(gcy - acy) / ah, (gcx - acx) / aw, np.log(gh / ah), np.log(gw / aw)]
        bbox[ix] /= std
    return match, bbox, arg


def crop_and_resize_mask(mask: np.ndarray, box: np.ndarray, size: int = mr.MASK_SHAPE) -> np.ndarray:
    """tf.image.crop_and_resize (bilinear, extrapolation 0) of one (H, W) 0/1 mask over a normalised box, float32 steps."""
    H, W = mask.shape
    f = np.float32
    hm1, wm1, den = f(H - 1), f(W - 1), f(size - 1)
    y1, x1, y2, x2 = [f(v) for v in box]
    hs, ws = f(f(y2 - y1) * hm1) / den, f(f(x2 - x1) * wm1) / den
    out = np.zeros((size, size), np.float32)
    for y in range(size):
        in_y = f(f(y1 * hm1) + f(f(y) * hs))
        if in_y < 0 or in_y > hm1:
            continue
        t, b = int(np.floor(in_y)), int(np.ceil(in_y))
        yl = f(in_y - f(t))
        for x in range(size):
            in_x = f(f(x1 * wm1) + f(f(x) * ws))
            if in_x < 0 or in_x > wm1:
                continue
            l, r = int(np.floor(in_x)), int(np.ceil(in_x))
            xl = f(in_x - f(l))
            tl, tr, bl, br = f(mask[t, l]), f(mask[t, r]), f(mask[b, l]), f(mask[b, r])
            top = f(tl + f(f(tr - tl) * xl))
            bot = f(bl + f(f(br - bl) * xl))
            out[y, x] = f(top + f(f(bot - top) * yl))
    return np.rint(out)                                    # tf.round: half to even


def roi_targets_host(proposals: np.ndarray, gt: np.ndarray, gt_class: np.ndarray, gt_masks: np.ndarray, keys: np.ndarray):
    """DetectionTargetLayer of one frame (float32, normalised boxes) with keys for tf.random_shuffle: positives (IoU >= 0.5, at
    most 66) and negatives (< 0.5, negative_count(positives) at most) in ascending (key, index) order.
    -> rois (200, 4), class_ids (200,) int32, deltas (200, 4), masks (200, 28, 28), all float32 but the ids; zero rows last."""
    R, G = len(proposals), len(gt)
    p, g = proposals.astype(np.float32), gt.astype(np.float32)
    if G:
        y1 = np.maximum(p[:, None, 0], g[None, :, 0]); x1 = np.maximum(p[:, None, 1], g[None, :, 1])
        y2 = np.minimum(p[:, None, 2], g[None, :, 2]); x2 = np.minimum(p[:, None, 3], g[None, :, 3])
        inter = np.maximum(x2 - x1, np.float32(0)) * np.maximum(y2 - y1, np.float32(0))
        a1 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
        a2 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
        ov = inter / ((a1[:, None] + a2[None, :]) - inter)
        # an IoU of 0/0 (a zero-area GT, from a one-pixel-thin mask, against a proposal that misses it) counts as no overlap
        # (-inf): the kernel's first-maximum scan skips NaN the same way, where numpy's max / argmax would return the NaN
        ov = np.where(np.isnan(ov), np.float32(-np.inf), ov)
        best, arg = ov.max(axis=1), ov.argmax(axis=1)
    else:
        best, arg = np.full(R, -np.inf, np.float32), np.zeros(R, np.int64)
    comp = (keys[:R].astype(np.uint64) << np.uint64(11)) | np.arange(R, dtype=np.uint64)
    pos, neg = np.where(best >= 0.5)[0], np.where(best < 0.5)[0]
    pos = pos[np.argsort(comp[pos], kind='stable')][:ROI_POS_MAX]
    neg = neg[np.argsort(comp[neg], kind='stable')][:negative_count(len(pos))]
    rois = np.zeros((TRAIN_ROIS_PER_IMAGE, 4), np.float32)
    cls = np.zeros(TRAIN_ROIS_PER_IMAGE, np.int32)
    deltas = np.zeros((TRAIN_ROIS_PER_IMAGE, 4), np.float32)
    masks = np.zeros((TRAIN_ROIS_PER_IMAGE, mr.MASK_SHAPE, mr.MASK_SHAPE), np.float32)
    P = len(pos)
    rois[:P], rois[P:P + len(neg)] = p[pos], p[neg]
    if P:
        b, t = p[pos], g[arg[pos]]
        h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        cy, cx = b[:, 0] + np.float32(0.5) * h, b[:, 1] + np.float32(0.5) * w
        gh, gw = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
        gcy, gcx = t[:, 0] + np.float32(0.5) * gh, t[:, 1] + np.float32(0.5) * gw
        log = lambda r: np.log(r.astype(np.float64)).astype(np.float32)     # float64 log rounded: the kernel's bits
        d = np.stack([(gcy - cy) / h, (gcx - cx) / w, log(gh / h), log(gw / w)], axis=1)
        deltas[:P] = d / np.array(mr.BBOX_STD_DEV, np.float32)
        cls[:P] = gt_class[arg[pos]]
        for r in range(P):
            masks[r] = crop_and_resize_mask(gt_masks[arg[pos[r]]], b[r])
    return rois, cls, deltas, masks


# ------------------------------------------------------------------------------------------------ device targets
def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def rpn_targets_device(anchors: torch.Tensor, gt: torch.Tensor, gt_count: torch.Tensor, keys: torch.Tensor):
    """rope_seg_rpn_targets: anchors (A, 4) float64, gt (B, G, 4) float64, gt_count (B,) int32, keys (B, A) int32 (the uint32
    bits) -> match (B, A) int32, bbox (B, 256, 4) float64, anchor_arg (B, A) int32 (all on the device)."""
    B, A = keys.shape
    G = max(gt.shape[1], 1)
    dev = anchors.device
    if gt.shape[1] == 0:
        gt = torch.zeros((B, 1, 4), dtype=torch.float64, device=dev)
    amax = torch.empty((B, A), dtype=torch.float64, device=dev)
    arg = torch.empty((B, A), dtype=torch.int32, device=dev)
    gmax = torch.empty((B, G), dtype=torch.int64, device=dev)
    match = torch.empty((B, A), dtype=torch.int32, device=dev)
    bbox = torch.empty((B, RPN_ANCHORS_PER_IMAGE, 4), dtype=torch.float64, device=dev)
    gt, gt_count, keys = gt.contiguous(), gt_count.contiguous(), keys.contiguous()
    rc = mr._seg_lib().rope_seg_rpn_targets(anchors.data_ptr(), A, gt.data_ptr(), gt_count.data_ptr(), G, B, keys.data_ptr(),
                                            amax.data_ptr(), arg.data_ptr(), gmax.data_ptr(), match.data_ptr(), bbox.data_ptr(), _stream(anchors))
    if rc != 0:
        raise RuntimeError(f"rope_seg_rpn_targets failed ({rc})")
    return match, bbox, arg


def roi_targets_device(proposals, prop_count, gt, gt_class, gt_count, gt_masks, keys):
    """rope_seg_roi_targets: proposals (B, R, 4) float32, prop_count (B,) int32, gt (B, G, 4) float32, gt_class / gt_count int32,
    gt_masks (B, G, H, W) uint8, keys (B, R) int32 -> rois (B, 200, 4), class_ids (B, 200) int32, deltas (B, 200, 4),
    masks (B, 200, 28, 28)."""
    B, R = keys.shape
    dev = proposals.device
    if gt.shape[1] == 0:
        gt = torch.zeros((B, 1, 4), dtype=torch.float32, device=dev)
        gt_class = torch.zeros((B, 1), dtype=torch.int32, device=dev)
        gt_masks = torch.zeros((B, 1) + tuple(gt_masks.shape[2:]), dtype=torch.uint8, device=dev)
    G, H, W = gt.shape[1], gt_masks.shape[2], gt_masks.shape[3]
    rois = torch.empty((B, TRAIN_ROIS_PER_IMAGE, 4), dtype=torch.float32, device=dev)
    cls = torch.empty((B, TRAIN_ROIS_PER_IMAGE), dtype=torch.int32, device=dev)
    deltas = torch.empty((B, TRAIN_ROIS_PER_IMAGE, 4), dtype=torch.float32, device=dev)
    masks = torch.empty((B, TRAIN_ROIS_PER_IMAGE, mr.MASK_SHAPE, mr.MASK_SHAPE), dtype=torch.float32, device=dev)
    args = [t.contiguous() for t in (proposals, prop_count, gt, gt_class, gt_count, gt_masks, keys)]
    rc = mr._seg_lib().rope_seg_roi_targets(args[0].data_ptr(), args[1].data_ptr(), R, args[2].data_ptr(), args[3].data_ptr(),
                                            args[4].data_ptr(), G, args[5].data_ptr(), H, W, B, args[6].data_ptr(), float(INV_POSITIVE_RATIO),
                                            rois.data_ptr(), cls.data_ptr(), deltas.data_ptr(), masks.data_ptr(), _stream(proposals))
    if rc != 0:
        raise RuntimeError(f"rope_seg_roi_targets failed ({rc})")
    return rois, cls, deltas, masks


def _levels(feats):
    lv = feats[:4]
    sizes = [f.shape[0] * f.shape[2] * f.shape[3] for f in lv]
    return (np.array([[f.shape[2], f.shape[3]] for f in lv], np.int32), np.array([sum(sizes[:k]) for k in range(4)], np.int64))


class RoIAlignF32(torch.autograd.Function):
    """rope_seg_roi_align_float and its transpose rope_seg_roi_align_backward: the float32 pyramid RoIAlign of maskrcnn._roi_align
    with a gradient for the feature rows (none for the boxes: PyramidROIAlign stops it, as Matterport does)."""

    @staticmethod
    def forward(ctx, rows, boxes, frame, level_hw, level_off, pool, inv_unit):
        K, C = len(boxes), rows.shape[1]
        t = torch.linspace(0, 1, pool, device=rows.device)
        out = torch.empty((K, pool, pool, C), dtype=torch.float32, device=rows.device)
        rows_c, b, f32 = rows.contiguous(), boxes.float().contiguous(), frame.to(torch.int32).contiguous()
        rc = mr._seg_lib().rope_seg_roi_align_float(rows_c.data_ptr(), b.data_ptr(), f32.data_ptr(), level_hw.ctypes.data, level_off.ctypes.data,
                                                  K, C, pool, float(inv_unit), t.data_ptr(), out.data_ptr(), _stream(rows))
        if rc != 0:
            raise RuntimeError(f"rope_seg_roi_align_float failed ({rc})")
        ctx.save_for_backward(b, f32, t)
        ctx.meta = (level_hw, level_off, pool, inv_unit, rows.shape)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad):
        b, f32, t = ctx.saved_tensors
        level_hw, level_off, pool, inv_unit, shape = ctx.meta
        g = grad.permute(0, 2, 3, 1).contiguous().float()
        grad_rows = torch.zeros(shape, dtype=torch.float32, device=g.device)
        rc = mr._seg_lib().rope_seg_roi_align_backward(g.data_ptr(), b.data_ptr(), f32.data_ptr(), level_hw.ctypes.data, level_off.ctypes.data,
                                                       len(b), shape[1], pool, float(inv_unit), t.data_ptr(), grad_rows.data_ptr(), _stream(g))
        if rc != 0:
            raise RuntimeError(f"rope_seg_roi_align_backward failed ({rc})")
        return grad_rows, None, None, None, None, None, None


def roi_align_train(feats, boxes, pool, size, frame):
    """Pyramid RoIAlign for training (float32, differentiable in the features): the HIP pair on the GPU, the tensor formulation of
    maskrcnn._roi_align on the CPU."""
    packed = mr._pack_levels(feats)
    if boxes.is_cuda:
        level_hw, level_off = _levels(feats)
        inv_unit = np.float32(1.0) / np.float32(224.0 / size)
        return RoIAlignF32.apply(packed[0], boxes, frame, level_hw, level_off, pool, inv_unit)
    return mr._roi_align(feats, boxes, pool, size, frame, packed)


# ------------------------------------------------------------------------------------------------ losses
def smooth_l1(diff: torch.Tensor) -> torch.Tensor:
    """Matterport smooth_l1_loss (sigma 1): 0.5 d^2 where |d| < 1, |d| - 0.5 elsewhere."""
    d = diff.abs()
    less = (d < 1.0).to(d.dtype)
    return less * 0.5 * d ** 2 + (1 - less) * (d - 0.5)


def _mean_or_zero(x: torch.Tensor) -> torch.Tensor:
    return x.mean() if x.numel() else x.new_zeros(())            # K.switch(tf.size(loss) > 0, K.mean(loss), 0)


def rpn_class_loss(match: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """Cross-entropy of the non-neutral anchors (target: positive), mean."""
    sel = match != 0
    return _mean_or_zero(F.cross_entropy(logits[sel], (match[sel] == 1).long(), reduction='none'))


def rpn_bbox_loss(match: torch.Tensor, target_bbox: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    """Smooth L1 of the positive anchors' deltas against the packed targets (first n rows of every frame), mean of all elements."""
    pos = match == 1
    counts = pos.sum(1)
    rows = torch.arange(target_bbox.shape[1], device=match.device)[None, :] < counts[:, None]
    return _mean_or_zero(smooth_l1(target_bbox[rows].float() - pred[pos]))


def mrcnn_class_loss(target_ids: torch.Tensor, logits: torch.Tensor, active: torch.Tensor = None) -> torch.Tensor:
    """Cross-entropy over every row, weighted by the predicted class being active in the dataset: sum / sum(active)."""
    ce = F.cross_entropy(logits, target_ids.long(), reduction='none')
    w = torch.ones_like(ce) if active is None else active[logits.argmax(1)].to(ce.dtype)
    return (ce * w).sum() / w.sum().clamp(min=1.0) if ce.numel() else ce.new_zeros(())


def mrcnn_bbox_loss(target_deltas, target_ids, pred):
    """Smooth L1 of the true class's deltas over the positive rows, mean of all elements."""
    pos = (target_ids > 0).nonzero().squeeze(1)
    return _mean_or_zero(smooth_l1(target_deltas[pos] - pred[pos, target_ids[pos].long()]))


def mrcnn_mask_loss(target_masks, target_ids, pred_logits):
    """Binary cross-entropy of the true class's 28 x 28 mask over the positive rows, mean (computed from the logits)."""
    pos = (target_ids > 0).nonzero().squeeze(1)
    y = pred_logits[pos, target_ids[pos].long()]
    return _mean_or_zero(F.binary_cross_entropy_with_logits(y, target_masks[pos], reduction='none'))


def _bn_param_ids(net: nn.Module) -> set:
    return {id(p) for m in net.modules() if isinstance(m, nn.BatchNorm2d) for p in (m.weight, m.bias)}


def weight_decay_term(net: nn.Module, decay: float = WEIGHT_DECAY) -> torch.Tensor:
    """sum over trainable weights but BN gamma / beta of l2(decay)(w) / size(w) = decay * sum(w^2) / size(w)."""
    bn = _bn_param_ids(net)
    terms = [decay * (p ** 2).sum() / p.numel() for p in net.parameters() if p.requires_grad and id(p) not in bn]
    return torch.stack(terms).sum() if terms else torch.zeros(())


# ------------------------------------------------------------------------------------------------ data
def mould_sample(image: np.ndarray, masks: np.ndarray, size: int):
    """resize_image(mode='square') geometry of maskrcnn.MaskRCNN._mould for the masks: nearest sample at the pixel centre,
    then the same padding.  -> masks (G, size, size) uint8 (instances that vanish are dropped by the caller)."""
    H, W = image.shape[:2]
    scale = size / max(H, W)
    nh, nw = round(H * scale), round(W * scale)
    top, left = (size - nh) // 2, (size - nw) // 2
    ys = np.minimum(((np.arange(nh) + 0.5) * H / nh).astype(np.int64), H - 1)
    xs = np.minimum(((np.arange(nw) + 0.5) * W / nw).astype(np.int64), W - 1)
    out = np.zeros((len(masks), size, size), np.uint8)
    out[:, top:top + nh, left:left + nw] = masks[:, ys][:, :, xs]
    return out


def gaussian_blur(x: torch.Tensor, sigma: float) -> torch.Tensor:
    """Separable Gaussian blur of a (C, H, W) float image, radius round(4 sigma), edges reflected (stand-in for imgaug's
    GaussianBlur)."""
    if sigma < 0.01:
        return x
    C, H, W = x.shape
    r = min(max(1, int(4 * sigma + 0.5)), H - 1, W - 1)
    k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=x.dtype, device=x.device) / sigma) ** 2)
    k = k / k.sum()
    y = F.conv2d(F.pad(x[None], (r, r, 0, 0), mode='reflect'), k.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)
    y = F.conv2d(F.pad(y, (0, 0, r, r), mode='reflect'), k.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return y[0]


def augment(x: torch.Tensor, masks: np.ndarray, rng: np.random.Generator):
    """Sometimes(0.5, [Fliplr(0.5), GaussianBlur(sigma=(0, 5))]) on the MOULDED frame, as load_image_gt applies it after
    resize_image and its padding: with probability 1/2 the frame (x: (3, size, size), masks: (G, size, size)) is flipped
    left-right with probability 1/2, then blurred with sigma uniform in [0, 5].  The blur acts on the mean-subtracted image
    (where MaskRCNN._mould's padding is 0) and is not rounded to uint8 as imgaug's is."""
    if rng.random() < 0.5:
        if rng.random() < 0.5:
            x, masks = x.flip(-1), np.ascontiguousarray(masks[:, :, ::-1])
        x = gaussian_blur(x, float(rng.uniform(0.0, 5.0)))
    return x, masks


# ------------------------------------------------------------------------------------------------ trainer
class MaskRCNNTrainer:
    """Trains `net` (a float32 MaskRCNN) on (RGB image, masks (G, H, W), class ids) samples.

    layers: 'all' or 'heads' (RPN, FPN and the mrcnn_* heads).  Batch norms run in inference mode with frozen statistics
    (TRAIN_BN False) while gamma and beta train with their layer.  All random choices (batch order, augmentation, the keys of the
    target kernels) come from one np.random.Generator(seed)."""

    def __init__(self, net: mr.MaskRCNN, layers: str = 'all', seed: int = 0, augmentation: bool = True,
                 lr: float = LEARNING_RATE, momentum: float = LEARNING_MOMENTUM, clip_norm: float = GRADIENT_CLIP_NORM):
        if layers not in ('all', 'heads'):
            raise ValueError(f"layers must be 'all' or 'heads', not {layers!r}")
        self.net, self.layers, self.augmentation, self.clip_norm = net.float().eval(), layers, augmentation, clip_norm
        self.rng = np.random.default_rng(seed)
        self.device = next(net.parameters()).device
        for name, p in net.named_parameters():
            p.requires_grad_(layers == 'all' or name.startswith(HEADS_PREFIXES))
        self.params = [p for p in net.parameters() if p.requires_grad]
        self.opt = torch.optim.SGD(self.params, lr=lr, momentum=momentum)
        self.size = net.size
        self._anchors = torch.from_numpy(anchors_px(self.size)).to(self.device)
        self.active = torch.ones(net.num_classes, device=self.device)

    # ---- one batch
    def _prepare(self, samples, augment_: bool):
        xs, gts, ids, gms = [], [], [], []
        for image, masks, class_ids in samples:
            x, _ = self.net._mould([torch.from_numpy(np.ascontiguousarray(image)).to(self.device)])
            x = x[0].float()
            m = mould_sample(image, masks.astype(np.uint8), self.size)
            if augment_:
                x, m = augment(x, m, self.rng)
            keep = m.reshape(len(m), -1).any(1) if len(m) else np.zeros(0, bool)
            m, c = m[keep][:MAX_GT_INSTANCES], np.asarray(class_ids, np.int32)[keep][:MAX_GT_INSTANCES]
            xs.append(x)
            gts.append(extract_bboxes(m))
            ids.append(c)
            gms.append(m)
        B, G = len(samples), max([len(g) for g in gts] + [0])
        gt = np.zeros((B, G, 4), np.int32)
        cls = np.zeros((B, G), np.int32)
        gm = np.zeros((B, G, self.size, self.size), np.uint8)
        for f in range(B):
            n = len(gts[f])
            gt[f, :n], cls[f, :n], gm[f, :n] = gts[f], ids[f], gms[f]
        cnt = np.array([len(g) for g in gts], np.int32)
        return torch.stack(xs), gt, cls, gm, cnt

    def _rpn_targets(self, gt, cnt):
        B, A = len(gt), len(self._anchors)
        keys = self.rng.integers(0, 2 ** 32, size=(B, A), dtype=np.uint32)
        if self.device.type == 'cuda':
            match, bbox, _ = rpn_targets_device(self._anchors, torch.from_numpy(gt.astype(np.float64)).to(self.device),
                                                torch.from_numpy(cnt).to(self.device), torch.from_numpy(keys.view(np.int32)).to(self.device))
            return match, bbox
        an = self._anchors.numpy()
        out = [rpn_targets_host(an, gt[f, :cnt[f]].astype(np.float64), keys[f]) for f in range(B)]
        return torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.stack([o[1] for o in out]))

    def _proposals(self, logits, deltas):
        """ProposalLayer with POST_NMS_ROIS_TRAINING, no gradient: (B, 2000, 4) zero-padded and the count per frame."""
        with torch.no_grad():
            probs = logits.softmax(-1)[..., 1]
            B, dev = probs.shape[0], probs.device
            anchors = mr._pyramid_anchors(self.size, dev)
            k = min(mr.PRE_NMS_LIMIT, probs.shape[1])
            top_p, top_idx = probs.topk(k, dim=1)
            d = deltas.gather(1, top_idx[..., None].expand(-1, -1, 4)) * mr._const(mr.RPN_BBOX_STD_DEV, dev)
            boxes = mr._apply_deltas(anchors[top_idx].reshape(-1, 4), d.reshape(-1, 4)).clamp(0, 1).view(B, k, 4)
            keep = mr._nms_batched(boxes, top_p, mr.RPN_NMS_THRESHOLD, POST_NMS_ROIS_TRAINING)
            out = torch.zeros((B, POST_NMS_ROIS_TRAINING, 4), device=dev)
            count = keep.sum(1)
            rank = keep.cumsum(1) - 1                                            # kept boxes by anchor rank (score order)
            f, i = keep.nonzero(as_tuple=True)
            out[f, rank[f, i]] = boxes[f, i]
            return out, count.to(torch.int32)

    def _roi_targets(self, props, count, gt, cls, gm, cnt):
        B = len(gt)
        gtn = np.stack([norm_boxes(gt[f], (self.size, self.size)) for f in range(B)]) if gt.shape[1] else np.zeros((B, 0, 4), np.float32)
        keys = self.rng.integers(0, 2 ** 32, size=(B, POST_NMS_ROIS_TRAINING), dtype=np.uint32)
        if self.device.type == 'cuda':
            d = self.device
            return roi_targets_device(props, count, torch.from_numpy(gtn).to(d), torch.from_numpy(cls).to(d), torch.from_numpy(cnt).to(d),
                                      torch.from_numpy(gm).to(d), torch.from_numpy(keys.view(np.int32)).to(d))
        pr, pc = props.numpy(), count.numpy()
        out = [roi_targets_host(pr[f, :pc[f]], gtn[f, :cnt[f]], cls[f, :cnt[f]], gm[f, :cnt[f]], keys[f]) for f in range(B)]
        return tuple(torch.from_numpy(np.stack([o[j] for o in out])) for j in range(4))

    def losses(self, samples, augment_: bool = False) -> dict:
        """The five losses of one batch (and 'weight_decay'), with the graph for a backward pass."""
        x, gt, cls, gm, cnt = self._prepare(samples, augment_)
        net, B = self.net, len(samples)
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.layers == 'all'):
            c = net.backbone(x)
        feats = net.fpn(c)
        logits, deltas = [], []
        for p in feats:
            h = F.relu(net.rpn.shared(p))
            logits.append(net.rpn.cls(h).permute(0, 2, 3, 1).reshape(B, -1, 2))
            deltas.append(net.rpn.box(h).permute(0, 2, 3, 1).reshape(B, -1, 4))
        logits, deltas = torch.cat(logits, 1), torch.cat(deltas, 1)
        match, rpn_bbox = self._rpn_targets(gt, cnt)
        props, count = self._proposals(logits.detach(), deltas.detach())
        rois, t_cls, t_deltas, t_masks = self._roi_targets(props, count, gt, cls, gm, cnt)
        boxes = rois.reshape(-1, 4)
        frame = torch.arange(B, device=x.device).repeat_interleave(TRAIN_ROIS_PER_IMAGE)
        h = net.head(roi_align_train(feats, boxes, mr.POOL_SIZE, self.size, frame)).flatten(1)
        cls_logits, box = net.cls(h), net.box(h).view(-1, net.num_classes, 4)
        mask_logits = net.mask(roi_align_train(feats, boxes, mr.MASK_POOL_SIZE, self.size, frame))
        t_cls, t_deltas, t_masks = t_cls.reshape(-1), t_deltas.reshape(-1, 4), t_masks.reshape(-1, mr.MASK_SHAPE, mr.MASK_SHAPE)
        out = {'rpn_class_loss': rpn_class_loss(match, logits), 'rpn_bbox_loss': rpn_bbox_loss(match, rpn_bbox, deltas),
               'mrcnn_class_loss': mrcnn_class_loss(t_cls, cls_logits, self.active),
               'mrcnn_bbox_loss': mrcnn_bbox_loss(t_deltas, t_cls, box), 'mrcnn_mask_loss': mrcnn_mask_loss(t_masks, t_cls, mask_logits)}
        out['weight_decay'] = weight_decay_term(net).to(x.device)
        return out

    def step(self, samples) -> dict:
        """One SGD step on a batch -> the losses as floats ('loss' = their sum with the weight decay)."""
        ls = self.losses(samples, self.augmentation)
        total = sum(ls.values())
        self.opt.zero_grad(set_to_none=True)
        total.backward()
        with torch.no_grad():
            for p in self.params:                                 # tf.keras clipnorm: every gradient clipped to norm 5 on its own
                if p.grad is not None:
                    p.grad.mul_(self.clip_norm / p.grad.norm().clamp(min=self.clip_norm))
        self.opt.step()
        out = {k: float(v.detach()) for k, v in ls.items()}
        out['loss'] = float(total.detach())
        return out

    @torch.no_grad()
    def validation_loss(self, samples, batch: int) -> float:
        tot, n = 0.0, 0
        for i in range(0, len(samples), batch):
            ls = self.losses(samples[i:i + batch], False)
            tot += float(sum(ls.values()))
            n += 1
        return tot / max(n, 1)

    def train(self, train_samples, val_samples, epochs: int, batch: int, dest: str = None, log=print) -> List[dict]:
        """epochs x ceil(len(train) / batch) steps; after every epoch the validation loss, and a checkpoint
        mask_rcnn_model.<epoch:03d>-<val_loss:f>.h5 in `dest` when it improved (ModelCheckpoint save_best_only)."""
        from .maskrcnn import save_matterport_weights
        best, history = math.inf, []
        for epoch in range(1, epochs + 1):
            order = self.rng.permutation(len(train_samples))
            losses = [self.step([train_samples[j] for j in order[i:i + batch]]) for i in range(0, len(order), batch)]
            val = self.validation_loss(val_samples, batch)
            rec = {'epoch': epoch, 'loss': float(np.mean([l['loss'] for l in losses])), 'val_loss': val}
            history.append(rec)
            log(f"epoch {epoch}: loss {rec['loss']:.4f} val_loss {val:.4f}")
            if dest is not None and val < best:
                best = val
                path = os.path.join(dest, f"mask_rcnn_model.{epoch:03d}-{val:f}.h5")
                save_matterport_weights(self.net.state_dict(), path)
                logging.info(f"checkpoint {path}")
        return history
