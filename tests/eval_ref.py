"""A deliberately plain restatement of the segmentation evaluation (rope_s3d_amd/evaluation.py), written on its own: loops over
predictions and labels, Python numbers, nothing vectorised.  Counts, IoU, Matterport's compute_matches and compute_ap
(mrcnn/utils.py as published), and the evaluator's summary."""
import numpy as np


def counts(pred, inst_first, gt):
    """pred (K, H, W) any integer/bool, gt (F, H, W) uint8 -> (inter (K, 8), area_pred (K,), area_gt (F, 8)) int64: the numpy
    expression of the kernel's contract, plane by plane."""
    pred, gt = np.asarray(pred), np.asarray(gt, np.uint8)
    F = len(gt)
    K = int(inst_first[F])
    inter, area_pred, area_gt = np.zeros((K, 8), np.int64), np.zeros(K, np.int64), np.zeros((F, 8), np.int64)
    for i in range(F):
        for b in range(8):
            label = ((gt[i] >> b) & 1).astype(bool)
            area_gt[i, b] = label.sum()
            for k in range(int(inst_first[i]), int(inst_first[i + 1])):
                inter[k, b] = ((pred[k] != 0) & label).sum()
        for k in range(int(inst_first[i]), int(inst_first[i + 1])):
            area_pred[k] = (pred[k] != 0).sum()
    return inter, area_pred, area_gt


def ious(inter, area_pred, area_gt, inst_first):
    out = []
    for i in range(len(area_gt)):
        rows = []
        for k in range(int(inst_first[i]), int(inst_first[i + 1])):
            row = []
            for b in range(8):
                union = int(area_pred[k]) + int(area_gt[i][b]) - int(inter[k][b])
                row.append(0.0 if union == 0 or int(area_gt[i][b]) == 0 else int(inter[k][b]) / union)
            rows.append(row)
        out.append(np.array(rows, np.float64).reshape(-1, 8))
    return out


def ranking(scores):
    """Indices by descending score; equal scores keep their order."""
    left, out = list(range(len(scores))), []
    while left:
        best = left[0]
        for k in left[1:]:
            if scores[k] > scores[best]:
                best = k
        out.append(best)
        left.remove(best)
    return out


def match(iou, class_ids, scores, gt_present, thr):
    """-> (gt_match [8], pred_match [K]) in score order, -1 = none."""
    order = ranking(scores)
    gt_match, pred_match = [-1] * 8, [-1] * len(order)
    for rank, k in enumerate(order):
        labels = [b for b in range(8) if gt_present[b]]
        # descending IoU, the lower label first among equals (insertion sort: nothing clever)
        for a in range(1, len(labels)):
            j = a
            while j > 0 and iou[k][labels[j]] > iou[k][labels[j - 1]]:
                labels[j], labels[j - 1] = labels[j - 1], labels[j]
                j -= 1
        for b in labels:
            if iou[k][b] < thr:
                break
            if gt_match[b] > -1:
                continue
            if int(class_ids[k]) == b + 1:
                gt_match[b], pred_match[rank] = rank, b
                break
    return gt_match, pred_match


def ap(pred_match, n_gt):
    if n_gt < 1:
        return 0.0
    precisions, recalls, tp = [0.0], [0.0], 0
    for r, m in enumerate(pred_match):
        tp += 1 if m > -1 else 0
        precisions.append(tp / (r + 1))
        recalls.append(tp / n_gt)
    precisions.append(0.0)
    recalls.append(1.0)
    for i in range(len(precisions) - 2, -1, -1):
        precisions[i] = max(precisions[i], precisions[i + 1])
    total = 0.0
    for i in range(1, len(recalls)):
        if recalls[i] != recalls[i - 1]:
            total += (recalls[i] - recalls[i - 1]) * precisions[i]
    return total


THRESHOLDS = [0.5 + 0.05 * i for i in range(10)]


def evaluate(frames, gt, n_classes):
    """frames: per frame (masks (K, H, W), class_ids, scores); gt (N, H, W) uint8 -> the evaluator's figures."""
    ap_rows, skipped = [], 0
    present_n, hit_n, iou_sum = [0] * n_classes, [0] * n_classes, [0.0] * n_classes
    ap50 = []
    for i, (masks, cls, sc) in enumerate(frames):
        inter, area_pred, area_gt = counts(masks, [0, len(masks)], gt[i:i + 1])
        iou = ious(inter, area_pred, area_gt, [0, len(masks)])[0]
        present = [b < n_classes and area_gt[0][b] > 0 for b in range(8)]
        n_gt = sum(present)
        if n_gt == 0:
            skipped += 1
            ap50.append(float('nan'))
            continue
        row = []
        for thr in THRESHOLDS:
            gm, pm = match(iou, cls, sc, present, thr)
            row.append(ap(pm, n_gt))
            if thr == THRESHOLDS[0]:
                order = ranking(sc)
                for b in range(n_classes):
                    if present[b]:
                        present_n[b] += 1
                        if gm[b] > -1:
                            hit_n[b] += 1
                            iou_sum[b] += iou[order[gm[b]]][b]
        ap_rows.append(row)
        ap50.append(row[0])
    n = len(ap_rows)
    return {'frames_skipped': skipped, 'AP50': sum(r[0] for r in ap_rows) / n if n else 0.0, 'AP75': sum(r[5] for r in ap_rows) / n if n else 0.0,
            'AP': sum(sum(r) / len(r) for r in ap_rows) / n if n else 0.0, 'AP50_per_frame': ap50,
            'frames_present': present_n, 'detection_rate': [h / p if p else 0.0 for h, p in zip(hit_n, present_n)],
            'mean_iou': [s / p if p else 0.0 for s, p in zip(iou_sum, present_n)]}
