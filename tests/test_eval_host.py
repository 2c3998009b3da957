"""CPU: the host side of the segmentation evaluation (rope_s3d_amd/evaluation.py) against the plain restatement in eval_ref.py and
against hand cases with known answers; the ground truth read back from labelme files; ModelManager.add_benchmark."""
import json
import os
import re

import numpy as np
import pytest

from rope_s3d_amd import evaluation as ev

import eval_ref

SCORES = np.array([0.99, 0.9, 0.9, 0.8, 0.75, 0.75, 0.75, 0.7])


def _random_frame(rng):
    """Integer counts of one frame as the kernel would give them, built to hit the corners: equal scores, equal IoUs (duplicated
    planes), absent labels, no prediction, no label, predictions of the wrong class sitting exactly on a label."""
    K = int(rng.choice([0, 1, 2, 3, 5, 9]))
    area_gt = rng.integers(1, 400, 8)
    area_gt[rng.random(8) < rng.choice([0.0, 0.3, 1.0], p=[0.5, 0.4, 0.1])] = 0
    area_pred, inter, cls = np.zeros(K, np.int64), np.zeros((K, 8), np.int64), np.zeros(K, np.int64)
    for k in range(K):
        if k and rng.random() < 0.25:                                    # the same plane again: every IoU ties
            area_pred[k], inter[k] = area_pred[k - 1], inter[k - 1]
        else:
            b = int(rng.integers(0, 8))
            how = rng.random()
            if how < 0.3 and area_gt[b]:                                 # exactly the label
                area_pred[k] = area_gt[b]
                inter[k, b] = area_gt[b]
            else:
                area_pred[k] = rng.integers(0, 400)
                inter[k] = rng.integers(0, 1 + np.minimum(area_pred[k], area_gt))
            if rng.random() < 0.4:                                       # half the label, half outside: IoU 1/2 or 1/3 exactly
                inter[k, b] = area_gt[b] // 2
                area_pred[k] = max(area_pred[k], inter[k].max())
        best = int(np.argmax(inter[k]))
        cls[k] = best + 1 if rng.random() < 0.6 else rng.integers(0, 8)   # often right, else anything (0 = background)
    if rng.random() < 0.3:                                               # two labels with the same pixels: their IoUs tie in every row
        b1, b2 = rng.choice(8, 2, replace=False)
        area_gt[b2], inter[:, b2] = area_gt[b1], inter[:, b1]
    scores = rng.choice(SCORES, K) if rng.random() < 0.7 else rng.random(K)
    return inter, area_pred, area_gt[None].astype(np.int64), cls, scores


def test_ious_matches_and_ap_equal_the_plain_restatement():
    rng = np.random.default_rng(20240607)
    seen = {'tie_score': 0, 'tie_iou': 0, 'absent': 0, 'no_pred': 0, 'no_gt': 0, 'wrong_class_high_iou': 0, 'matched': 0}
    for _ in range(400):
        inter, area_pred, area_gt, cls, scores = _random_frame(rng)
        first = [0, len(cls)]
        iou = ev.ious(inter, area_pred, area_gt, first)[0]
        want = eval_ref.ious(inter, area_pred, area_gt, first)[0]
        assert iou.shape == want.shape == (len(cls), 8) and np.array_equal(iou, want)
        present = area_gt[0] > 0
        seen['tie_score'] += len(set(scores.tolist())) < len(scores)
        seen['tie_iou'] += any(len(set(r[r > 0].tolist())) < int((r > 0).sum()) for r in iou)
        seen['absent'] += 0 < present.sum() < 8
        seen['no_pred'] += len(cls) == 0
        seen['no_gt'] += present.sum() == 0
        seen['wrong_class_high_iou'] += any(iou[k, b] >= 0.9 and cls[k] != b + 1 for k in range(len(cls)) for b in range(8))
        for thr in (0.5, 0.75, 0.95, 1.0 / 3.0):
            gm, pm = ev.match_detections(iou, cls, scores, present, thr)
            gm_ref, pm_ref = eval_ref.match(iou, cls, scores, present, thr)
            assert gm.tolist() == gm_ref and pm.tolist() == pm_ref, (iou, cls, scores, thr)
            seen['matched'] += any(m > -1 for m in pm_ref)
            n_gt = int(present.sum())
            assert abs(ev.average_precision(pm, n_gt) - eval_ref.ap(pm_ref, n_gt)) <= 1e-12
    assert all(v >= 10 for v in seen.values()), {k: int(v) for k, v in seen.items()}


def test_absent_label_is_a_column_of_zeros_and_empty_union_is_zero():
    inter = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0]])
    iou = ev.ious(inter, [0, 6], [[6, 0, 0, 0, 0, 0, 0, 9]], [0, 2])[0]
    assert iou[0].tolist() == [0.0] * 8                                  # an empty plane: union 6 with label 0, 0 with label 1
    assert iou[1].tolist() == [3 / 9, 0, 0, 0, 0, 0, 0, 0]
    two = ev.ious(np.zeros((1, 8)), [5], [[0] * 8, [5] + [0] * 7], [0, 0, 1])
    assert two[0].shape == (0, 8) and two[1].tolist() == [[0.0] * 8]


def _ap(iou_rows, cls, scores, present, thr=0.5):
    gm, pm = ev.match_detections(np.array(iou_rows, float), cls, scores, present, thr)
    return ev.average_precision(pm, int(np.sum(present))), gm.tolist(), pm.tolist()


def test_hand_cases():
    row = lambda b, v=0.9: [v if j == b else 0.0 for j in range(8)]      # noqa: E731
    two = [True, True] + [False] * 6
    one = [True] + [False] * 7
    # perfect detections
    assert _ap([row(0), row(1)], [1, 2], [0.9, 0.8], two) == (1.0, [0, 1] + [-1] * 6, [0, 1])
    # one of two labels missed
    assert _ap([row(0)], [1], [0.9], two)[0] == 0.5
    # a false positive ranked first, then a hit on the only label
    assert _ap([row(3, 0.0), row(0)], [4, 1], [0.9, 0.8], one) == (0.5, [1] + [-1] * 7, [-1, 0])
    # a false positive ranked last
    assert _ap([row(0), row(3, 0.0)], [1, 4], [0.9, 0.8], one)[0] == 1.0
    # IoU exactly at the threshold matches; just below does not
    assert _ap([row(0, 0.5)], [1], [0.9], one, 0.5)[0] == 1.0
    assert _ap([row(0, 0.75)], [1], [0.9], one, 0.75)[0] == 1.0
    assert _ap([row(0, np.nextafter(0.75, 0))], [1], [0.9], one, 0.75)[0] == 0.0
    # a wrong-class prediction on top of a label takes nothing, and the right one behind it still matches
    assert _ap([row(0, 1.0), row(0, 0.6)], [2, 1], [0.9, 0.8], one) == (0.5, [1] + [-1] * 7, [-1, 0])
    # a duplicate of a matched label is a false positive; equal scores keep their order
    assert _ap([row(0), row(0)], [1, 1], [0.8, 0.8], one) == (1.0, [0] + [-1] * 7, [0, -1])
    # nothing predicted, nothing to find
    assert _ap(np.zeros((0, 8)), [], [], two)[0] == 0.0
    assert ev.average_precision([], 0) == 0.0


def test_gt_from_annotations_round_trip(tmp_path):
    from rope_s3d_amd.data.annotation import write_annotation
    names = ['base_link', 'link_s', 'link_l']
    H, W = 12, 17
    rng = np.random.default_rng(5)
    boxes = [{'base_link': [(1, 1, 6, 5)], 'link_l': [(4, 3, 15, 10)], 'other': [(0, 0, 16, 11)]},
             {'link_s': [(2, 2, 5, 9), (9, 0, 12, 4)]}]                  # two polygons of one label; a label the model does not know
    want, images = np.zeros((2, H, W), np.uint8), rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    for i, frame in enumerate(boxes):
        shapes = []
        for label, rects in frame.items():
            for x0, y0, x1, y1 in rects:
                shapes.append({'label': label, 'points': [[x0, y0], [x1, y0], [x1, y1], [x0, y1]], 'group_id': None, 'shape_type': 'polygon',
                               'flags': {}})
                if label in names:
                    want[i, y0:y1 + 1, x0:x1 + 1] |= 1 << names.index(label)       # closed rule: the border pixels belong
        write_annotation(images[i], shapes, str(tmp_path / f'{i:05d}'))
    got = ev.gt_from_annotations(str(tmp_path), names)
    assert got.dtype == np.uint8 and got.shape == (2, H, W) and np.array_equal(got, want)
    assert int(np.bitwise_or.reduce(got, axis=None)) == 0b111
    got2, imgs, files = ev.gt_from_annotations(str(tmp_path), names, return_images=True)
    assert np.array_equal(got2, want) and np.array_equal(imgs, images) and files == ['00000', '00001']
    with pytest.raises(FileNotFoundError):
        ev.gt_from_annotations(str(tmp_path / 'nothing'), names)
    with pytest.raises(ValueError):
        ev.gt_from_annotations(str(tmp_path), [f'c{i}' for i in range(9)])


def test_add_benchmark_appends_and_rewrites(tmp_path):
    from rope_s3d_amd.models import MODELDATA_FILE_NAME, ModelManager
    folder = tmp_path / 'ABCD'
    folder.mkdir()
    md = {'id': 'ABCD', 'dataset': 'set10', 'dataset_size': 10, 'train_size': 4, 'valid_size': 1, 'classes': ['a', 'b'],
          'epochs_trained': 0, 'date_trained': '2024-01-01 00:00:00.000000', 'benchmarks': []}
    (folder / MODELDATA_FILE_NAME).write_text(json.dumps(md, indent=4))
    mm = ModelManager(str(tmp_path))
    result = {'frames': 5, 'frames_skipped': 1, 'AP': 0.5, 'AP50': 0.75, 'AP75': 0.25, 'AP50_per_frame': np.zeros(5),
              'classes': {'a': {'frames': 4, 'mean_iou': 0.8, 'detection_rate': 1.0}}}
    rec = ev.benchmark_record(result, 'set10', 'test', 'annotations')
    path = mm.add_benchmark('ABCD', rec)
    mm.add_benchmark('ABCD', dict(rec, split='train'))
    with open(path) as f:
        back = json.load(f)
    assert {k: back[k] for k in md if k != 'benchmarks'} == {k: md[k] for k in md if k != 'benchmarks'}
    assert [b['split'] for b in back['benchmarks']] == ['test', 'train']
    first = back['benchmarks'][0]
    assert (first['dataset'], first['gt'], first['frames'], first['AP50'], first['classes']) == ('set10', 'annotations', 5, 0.75, result['classes'])
    assert re.match(r'\d{4}-\d\d-\d\d ', first['date'])
    assert [b['split'] for b in ModelManager(str(tmp_path)).info['ABCD'].benchmarks] == ['test', 'train']
    with pytest.raises(AssertionError):
        mm.add_benchmark('NOPE', rec)


def test_entry_point_is_declared_bound_and_refuses_on_the_host():
    """The ABI: declared in the header, bound with ten arguments, part of the library's sources; the refusals that need no device."""
    from rope_s3d_amd import build, engine as eng
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)
    hdr = open(os.path.join(root, 'include', 'rope_s3d.h')).read()
    assert re.search(r'int rope_seg_mask_overlaps\(([^;]*)\);', hdr).group(1).count(',') == 9
    assert 'rope_eval.hip' in build._SOURCES and 'rope_eval.hip' in build._DEPS
    lib = eng.load_library()
    assert 'rope_seg_mask_overlaps' in eng.ABI_SYMBOLS and len(lib.rope_seg_mask_overlaps.argtypes) == 10
    one = 1                                                              # a non-null "pointer": refused calls never read it

    def call(first, n, H=4, W=4, ptr=one):
        arr = None if first is None else np.asarray(first, np.int32)     # alive across the call
        return lib.rope_seg_mask_overlaps(ptr, None if arr is None else arr.ctypes.data, n, ptr, H, W, ptr, ptr, ptr, None)
    assert call([0, 2, 1], 2) == -1                                      # decreases
    assert call([1, 2], 1) == -1                                         # does not start at 0
    assert call([0, 1], -1) == -1 and call([0, 1], 1, H=0) == -1 and call([0, 1], 1, W=0) == -1
    assert call(None, 1) == -1 and call([0, 1], 1, ptr=None) == -1       # null pointers where planes exist
    assert call([0], 0, ptr=None) == 0                                   # no frame: nothing to do, nothing touched
