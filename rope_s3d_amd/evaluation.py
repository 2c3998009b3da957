"""How good is a trained segmentation model: mask IoU and average precision of its detections against ground-truth labels.

The chain annotate.py -> train.py -> Predictor(model_ds=...) reports a validation loss and nothing else; this module measures a
checkpoint the way Matterport's Mask R-CNN does (mrcnn/utils.py: compute_matches, compute_ap), on masks.

The heavy part is pairwise mask overlap: up to 100 instance planes per frame at full frame size against every label of the frame.
The planes are on the GPU already (MaskRCNNSegmenter.batches_device), so they are counted there (rope_seg_mask_overlaps,
csrc/rope_eval.hip): exact integer counts come back, a few hundred numbers per frame, and everything after them — IoU, matching,
AP — is host arithmetic in float64.

Ground truth is one (H, W) uint8 plane per frame, bit b set where the pixel belongs to label b (class id b + 1; class 0 is the
background): the form rope_render_masks writes.  At most 8 labels, one instance per label, which is what this project's scenes
have; labels may overlap (dilated ones do)."""
import ctypes as C
import glob
import os
from datetime import datetime

import numpy as np

N_LABELS = 8
AP_THRESHOLDS = tuple(0.5 + 0.05 * i for i in range(10))            # COCO's 0.50:0.05:0.95


def mask_overlaps(masks, inst_first, gt_bits):
    """rope_seg_mask_overlaps on the tensors' device and the current torch stream.
      masks       (K, H, W) torch.bool or torch.uint8 on the GPU, non-zero = inside the instance; None for K == 0
      inst_first  F + 1 offsets: frame i owns planes inst_first[i] .. inst_first[i + 1] - 1
      gt_bits     (F, H, W) torch.uint8 on the same device
    -> (inter (K, 8), area_pred (K,), area_gt (F, 8)) int64 numpy arrays.  Tensors that are not contiguous are made so; wrong
    dtypes or shapes are a ValueError, and so is an inst_first the library refuses."""
    import torch
    from .engine import load_library
    if not isinstance(gt_bits, torch.Tensor) or gt_bits.dtype != torch.uint8 or gt_bits.dim() != 3:
        raise ValueError("gt_bits: a (F, H, W) torch.uint8 tensor")
    if not gt_bits.is_cuda:
        raise ValueError("gt_bits: not on a GPU (the counts are a kernel; there is no host path)")
    F, H, W = gt_bits.shape
    if H < 1 or W < 1:
        raise ValueError(f"gt_bits: empty planes {H} x {W}")
    first = np.ascontiguousarray(np.asarray(inst_first).reshape(-1), np.int32)
    if len(first) != F + 1:
        raise ValueError(f"inst_first: {len(first)} offsets for {F} frames")
    K = int(first[-1])
    if masks is None:
        if K != 0:
            raise ValueError(f"inst_first names {K} planes, masks is None")
    else:
        if not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.bool, torch.uint8):
            raise ValueError("masks: a torch.bool or torch.uint8 tensor")
        if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W):
            raise ValueError(f"masks: shape {tuple(masks.shape)}, expected (K, {H}, {W})")
        if masks.shape[0] != K:
            raise ValueError(f"inst_first names {K} planes, masks has {masks.shape[0]}")
        if masks.device != gt_bits.device:
            raise ValueError(f"masks on {masks.device}, gt_bits on {gt_bits.device}")
        masks = masks.contiguous()
    gt_bits = gt_bits.contiguous()
    dev = gt_bits.device
    with torch.cuda.device(dev):
        inter = torch.empty((K, N_LABELS), dtype=torch.int32, device=dev)
        area_pred = torch.empty((K,), dtype=torch.int32, device=dev)
        area_gt = torch.empty((F, N_LABELS), dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None      # noqa: E731
        rc = load_library().rope_seg_mask_overlaps(p(masks), first.ctypes.data_as(C.c_void_p), F, p(gt_bits), H, W, p(inter), p(area_pred),
                                                   p(area_gt), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc == -1:
            raise ValueError("rope_seg_mask_overlaps refused its arguments (inst_first starts at 0 and never decreases)")
        if rc != 0:
            raise RuntimeError(f"rope_seg_mask_overlaps failed ({rc})")
        u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)                      # noqa: E731
        return u32(inter), u32(area_pred), u32(area_gt)


def ious(inter, area_pred, area_gt, inst_first) -> list:
    """Per frame the (K_i, 8) float64 IoU of its planes with its labels: inter / (area_pred + area_gt - inter), 0 where the union
    is empty.  An absent label (area 0) gives a column of zeros."""
    inter, area_pred, area_gt = np.asarray(inter, np.int64), np.asarray(area_pred, np.int64), np.asarray(area_gt, np.int64)
    out = []
    for i in range(len(area_gt)):
        a, b = int(inst_first[i]), int(inst_first[i + 1])
        union = area_pred[a:b, None] + area_gt[i][None, :] - inter[a:b]
        iou = np.zeros(union.shape, np.float64)
        np.divide(inter[a:b], union, out=iou, where=union > 0)
        iou[:, area_gt[i] == 0] = 0.0
        out.append(iou)
    return out


def score_order(scores) -> np.ndarray:
    """Predictions in descending score, equal scores in their given order."""
    return np.argsort(-np.asarray(scores, np.float64), kind='stable')


def match_detections(iou, class_ids, scores, gt_present, thr: float):
    """Matterport's compute_matches on one frame's IoU table.  Predictions are taken in descending score (stable); each looks at
    the present labels in descending IoU (equal IoUs: the lower label first), stops at the first IoU below `thr`, skips labels
    that are matched already, and takes the first one left whose class it has (label bit b is class b + 1).
    -> (gt_match (8,), pred_match (K,)): gt_match[b] is the RANK of the prediction matched to label b (its place in score_order),
    pred_match[r] the label of the prediction of rank r; -1 = none.  Both as compute_matches returns them: in score order."""
    iou = np.asarray(iou, np.float64).reshape(-1, N_LABELS)
    class_ids, present = np.asarray(class_ids).reshape(-1), np.asarray(gt_present, bool).reshape(N_LABELS)
    order = score_order(scores)
    gt_match, pred_match = np.full(N_LABELS, -1, np.int64), np.full(len(order), -1, np.int64)
    for rank, k in enumerate(order):
        for b in np.argsort(-iou[k], kind='stable'):
            if iou[k, b] < thr:
                break
            if not present[b] or gt_match[b] > -1:
                continue
            if class_ids[k] == b + 1:
                gt_match[b], pred_match[rank] = rank, b
                break
    return gt_match, pred_match


def average_precision(pred_match, n_gt: int) -> float:
    """Matterport's compute_ap from the matches in score order: cumulative precision and recall, padded with (0, 0) and (1, 0),
    precision made monotone from the right, summed over the steps of recall.  0 when there is nothing to find."""
    if n_gt < 1:
        return 0.0
    hit = np.asarray(pred_match).reshape(-1) > -1
    tp = np.cumsum(hit)
    precisions = np.concatenate([[0.0], tp / (np.arange(len(hit)) + 1.0), [0.0]])
    recalls = np.concatenate([[0.0], tp / float(n_gt), [1.0]])
    for i in range(len(precisions) - 2, -1, -1):
        precisions[i] = max(precisions[i], precisions[i + 1])
    at = np.where(recalls[:-1] != recalls[1:])[0] + 1
    return float(np.sum((recalls[at] - recalls[at - 1]) * precisions[at]))


class SegmentationEvaluator:
    """Runs a segmenter over frames and scores what it finds against label bit planes.
      segmenter    has batches_device(groups) like MaskRCNNSegmenter: per frame {'class_ids', 'scores', 'masks_device',
                   'masks_stacked'}, the masks on the GPU
      class_names  label b is class_names[b], class id b + 1 (at most 8)
      batch        frames per pass of the segmenter and per rope_seg_mask_overlaps call"""

    def __init__(self, segmenter, class_names, batch: int = 8):
        if not 1 <= len(class_names) <= N_LABELS:
            raise ValueError(f"1 to {N_LABELS} classes, got {len(class_names)}")
        if batch < 1:
            raise ValueError("batch must be at least 1")
        self.seg, self.class_names, self.batch = segmenter, list(class_names), int(batch)

    @staticmethod
    def _planes(results):
        """(the frames' planes as one (sum K_i, H, W) tensor or None, inst_first): the segmenter's own stack when the frames'
        planes lie in it back to back ('masks_stacked'), the concatenated 'masks_device' otherwise."""
        import torch
        counts = [int(r['masks_device'].shape[0]) for r in results]
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        if first[-1] == 0:
            return None, first
        where = [r.get('masks_stacked') for r in results]
        if all(w is not None and w[0] is where[0][0] for w in where) and \
                all(w[1] == where[0][1] + int(a) for w, a in zip(where, first[:-1])):
            return where[0][0][where[0][1]:where[0][1] + int(first[-1])], first
        return torch.cat([r['masks_device'] for r, n in zip(results, counts) if n]), first

    def run(self, colors, gt_bits) -> dict:
        """colors: N frames (H, W, 3) uint8 BGR; gt_bits: (N, H, W) uint8 label planes.  -> {'frames', 'frames_skipped' (no label:
        they count for nothing), 'AP50', 'AP75', 'AP' (mean over IoU 0.50:0.05:0.95) — each the mean of the per-frame AP over the
        frames that have a label —, 'AP50_per_frame' (NaN for a skipped frame), 'classes': {name: {'frames' the label is present
        in, 'mean_iou' of the detection matched to it at IoU 0.5 (0 when it was missed), 'detection_rate' at IoU 0.5}}}."""
        import torch
        gt_bits = np.ascontiguousarray(gt_bits, np.uint8)
        n = len(gt_bits)
        if len(colors) != n:
            raise ValueError(f"{len(colors)} frames, {n} label planes")
        device = torch.device(getattr(self.seg, 'device', 'cuda:0'))
        n_cls = len(self.class_names)
        ap = np.full((n, len(AP_THRESHOLDS)), np.nan)
        present_n, hit_n, iou_sum = np.zeros(N_LABELS, np.int64), np.zeros(N_LABELS, np.int64), np.zeros(N_LABELS)
        starts = list(range(0, n, self.batch))
        groups = ([colors[j] for j in range(a, min(n, a + self.batch))] for a in starts)
        for a, results in zip(starts, self.seg.batches_device(groups)):
            gt_dev = torch.from_numpy(np.array(gt_bits[a:a + len(results)])).to(device)       # one upload per group
            planes, first = self._planes(results)
            inter, area_pred, area_gt = mask_overlaps(planes, first, gt_dev)
            for j, (r, iou) in enumerate(zip(results, ious(inter, area_pred, area_gt, first))):
                present = area_gt[j] > 0
                present[n_cls:] = False
                n_gt = int(present.sum())
                if n_gt == 0:
                    continue
                for t, thr in enumerate(AP_THRESHOLDS):
                    gt_match, pred_match = match_detections(iou, r['class_ids'], r['scores'], present, thr)
                    ap[a + j, t] = average_precision(pred_match, n_gt)
                    if t == 0:
                        order = score_order(r['scores'])
                        present_n += present
                        for b in np.nonzero(gt_match > -1)[0]:
                            hit_n[b] += 1
                            iou_sum[b] += iou[order[gt_match[b]], b]
        counted = ~np.isnan(ap[:, 0])
        mean = lambda v: float(np.mean(v)) if len(v) else 0.0                                 # noqa: E731
        return {'frames': int(n), 'frames_skipped': int(n - counted.sum()),
                'AP50': mean(ap[counted, 0]), 'AP75': mean(ap[counted, 5]), 'AP': mean(ap[counted].mean(axis=1) if counted.any() else []),
                'AP50_per_frame': ap[:, 0].copy(),
                'classes': {name: {'frames': int(present_n[b]), 'mean_iou': float(iou_sum[b] / present_n[b]) if present_n[b] else 0.0,
                                   'detection_rate': float(hit_n[b] / present_n[b]) if present_n[b] else 0.0}
                            for b, name in enumerate(self.class_names)}}


def gt_from_annotations(folder: str, class_names, return_images: bool = False):
    """Label planes of the labelme files of one split folder (annotate.py's train/ or test/), in file-name order: what the model
    was trained against.  Every polygon of a label goes into that label's bit.  -> (N, H, W) uint8; with return_images also the
    frames the files hold, as (N, H, W, 3) uint8 BGR, and the files' base names."""
    from .data.labelme import read_annotation
    class_names = list(class_names)
    if len(class_names) > N_LABELS:
        raise ValueError(f"at most {N_LABELS} labels, got {len(class_names)}")
    files = sorted(glob.glob(os.path.join(folder, '*.json')))
    if not files:
        raise FileNotFoundError(f"no labelme files in {folder}")
    planes, images = [], []
    for f in files:
        img, masks, ids = read_annotation(f, class_names)
        bits = np.zeros(img.shape[:2], np.uint8)
        for m, c in zip(masks, ids):
            bits |= m.astype(np.uint8) << np.uint8(c - 1)
        planes.append(bits)
        images.append(img[..., ::-1])
    if any(p.shape != planes[0].shape for p in planes):
        raise ValueError(f"the frames of {folder} differ in size")
    gt = np.stack(planes)
    if return_images:
        return gt, np.ascontiguousarray(np.stack(images)), [os.path.splitext(os.path.basename(f))[0] for f in files]
    return gt


def gt_from_renders(dataset, idx, pad: int = 3, chunk: int = 64) -> np.ndarray:
    """Label planes of the frames `idx` of a dataset from renders at their recorded joint angles and camera poses
    (DatasetRenderer.render_masks_batch, the planes annotate.py traces): no annotation needed.  `dataset`: a name, an opened
    dataset, or a DatasetRenderer (left in mode 'seg').  -> (N, H, W) uint8."""
    from .simulation.render import DatasetRenderer
    rend = dataset if isinstance(dataset, DatasetRenderer) else DatasetRenderer(dataset, 'seg')
    rend.setMode('seg')
    idx = np.asarray(idx, np.int64).reshape(-1)
    H, W = rend.resolution
    out = np.empty((len(idx), H, W), np.uint8)
    for a in range(0, len(idx), chunk):
        sel = idx[a:a + chunk]
        out[a:a + chunk] = rend.render_masks_batch(rend._ds_angles[sel], rend._ds_poses[sel], pad)[0]
    return out


def benchmark_record(result: dict, dataset: str, split: str, gt_source: str) -> dict:
    """What ModelManager.add_benchmark stores of a SegmentationEvaluator.run result."""
    return {'dataset': dataset, 'split': split, 'gt': gt_source, 'frames': result['frames'], 'frames_skipped': result['frames_skipped'],
            'AP': result['AP'], 'AP50': result['AP50'], 'AP75': result['AP75'], 'classes': result['classes'], 'date': str(datetime.now())}


def print_table(result: dict):
    """The result as a table, in the style of prediction/analysis.py's error tables."""
    w = max([5] + [len(c) for c in result['classes']])
    print(f"\nSegmentation ({result['frames'] - result['frames_skipped']} frames, {result['frames_skipped']} without a label skipped):")
    print(f"\t{' ' * w}   Frames  MeanIoU  Det@.5")
    for name, c in result['classes'].items():
        print(f"\t{name:>{w}}: {c['frames']:7d} {c['mean_iou']:8.3f} {c['detection_rate']:7.3f}")
    print(f"\tAP {result['AP']:.3f} | AP50 {result['AP50']:.3f} | AP75 {result['AP75']:.3f}")
