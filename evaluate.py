#!/usr/bin/env python3
"""Evaluate a trained segmentation model on a dataset: mask IoU per class and average precision (AP50, AP75, AP 0.50:0.95)
against ground truth from the dataset's annotations (what train.py trained on) or from renders at the recorded poses.  The model
is the one Predictor(model_ds=dataset) would load, or -model ID.  The result is printed and appended to the model's
ModelData.json (`benchmarks`).  `dataset` may be a 'synthetic:<frames>[:<seed>[:<intrinsics preset>]]' or 'photo:...' name."""
import argparse
import logging
import os


def evaluate(dataset, model=None, split='test', gt='annotations', batch=8, min_confidence=0.7, device='cuda:0', record=True):
    """-> (the SegmentationEvaluator.run result, the model's id)."""
    import numpy as np
    from rope_s3d_amd.maskrcnn import MaskRCNNSegmenter, load_matterport_weights
    from rope_s3d_amd.models import ModelManager
    from rope_s3d_amd.robot import RobotModel

    class_names = list(RobotModel.from_urdf().link_names[:6])      # train.py's classes
    mm = ModelManager()
    path = mm.loadByID(model) if model is not None else mm.dynamicLoad(dataset=dataset)
    if path is None:
        raise SystemExit(f"no trained segmentation model under {mm.dir}: run train.py on the dataset first")
    model_id = next(i for i, d in mm.info.items() if os.path.dirname(os.path.abspath(path)) == os.path.abspath(d.folder))
    # the segmenter BEFORE any Engine: torch's HIP runtime has to take the GPU first (MaskRCNNSegmenter's docstring)
    seg = MaskRCNNSegmenter(len(class_names) + 1, device=device, state_dict=load_matterport_weights(path, len(class_names) + 1),
                            min_confidence=min_confidence)

    from rope_s3d_amd import evaluation as ev
    from rope_s3d_amd.data.dataset import open_dataset
    ds = open_dataset(dataset)
    if gt == 'annotations':
        folders = ['train', 'test'] if split == 'all' else [split]
        parts = [ev.gt_from_annotations(os.path.join(ds.link_anno_path, f), class_names, return_images=True) for f in folders]
        gt_bits, colors = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    else:
        if split == 'all':
            idx = np.arange(ds.length)
        else:                                                      # the frames of the split, by the annotation files' names
            from rope_s3d_amd.data.labelme import split_files
            files = split_files(ds.link_anno_path)[0 if split == 'train' else 1]
            idx = np.array([int(os.path.splitext(os.path.basename(f))[0]) for f in files])
        gt_bits = ev.gt_from_renders(ds, idx)
        colors = [np.asarray(ds.og_img[int(i)]) for i in idx]
    result = ev.SegmentationEvaluator(seg, class_names, batch).run(colors, gt_bits)
    ev.print_table(result)
    if record:
        where = mm.add_benchmark(model_id, ev.benchmark_record(result, str(dataset), split, gt))
        print(f"recorded in {where}")
    return result, model_id


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset', type=str, help="The dataset to evaluate on. Can be a partial name.")
    parser.add_argument('-model', type=str, default=None, help="Model id; default: the newest model trained on the dataset.")
    parser.add_argument('-split', type=str, choices=['test', 'train', 'all'], default='test', help="Which frames.")
    parser.add_argument('-gt', type=str, choices=['annotations', 'renders'], default='annotations', help="Where the ground truth comes from.")
    parser.add_argument('-batch', type=int, default=8, help="Frames per pass of the network.")
    parser.add_argument('-min_confidence', type=float, default=0.7, help="Detections below this score are dropped by the network.")
    args = parser.parse_args()
    evaluate(args.dataset, args.model, args.split, args.gt, args.batch, args.min_confidence)
