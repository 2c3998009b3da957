#!/usr/bin/env python3
"""Train the segmentation network on a dataset's annotated renders (same command line as the reference's train.py, plus
-epochs and -base).  The annotations and their train / test split come from annotate.py.  `dataset` may be a
'synthetic:<frames>[:<seed>[:<intrinsics preset>]]' or 'photo:...' name.  Checkpoints go to a new model folder (ModelManager.allocateNew),
where Predictor(model_ds=dataset) finds them."""
import argparse
import logging
import os


def train(dataset, batch=2, cont=False, cont_from=None, epochs=300, base=None, image_size=512, device='cuda:0', seed=0, log=print):
    """-> the model folder the checkpoints were written to."""
    import numpy as np
    import torch
    if torch.device(device).type == 'cuda':
        torch.cuda.init()                          # torch's HIP context before the engine's (MaskRCNNSegmenter's docstring)
    from rope_s3d_amd.data.dataset import open_dataset
    from rope_s3d_amd.data.labelme import read_annotation, split_files
    from rope_s3d_amd.maskrcnn import MaskRCNN, load_matterport_weights
    from rope_s3d_amd.models import ModelManager
    from rope_s3d_amd.robot import RobotModel
    from rope_s3d_amd.training import MaskRCNNTrainer

    ds = open_dataset(dataset)
    train_files, test_files = split_files(ds.link_anno_path)       # fails with a message naming annotate.py
    class_names = list(RobotModel.from_urdf().link_names[:6])      # DatasetRenderer(dataset, 'seg').color_dict's names
    mm = ModelManager()
    base_path = None
    if cont or cont_from is not None:
        base_path = mm.dynamicLoad(dataset=(cont_from if cont_from is not None else dataset))
    if base_path is None:
        base_path = base
    torch.manual_seed(seed)
    net = MaskRCNN(len(class_names) + 1, image_size)
    if base_path is None:
        log("no base model (COCO weights are not available offline): training from random weights")
    else:
        # PixelLib's load_pretrained_model: the class-specific heads are left out when the base has another class count
        try:
            sd = load_matterport_weights(base_path, len(class_names) + 1)
        except ValueError:
            sd = load_matterport_weights(base_path, len(class_names) + 1,
                                         exclude=('mrcnn_class_logits', 'mrcnn_bbox_fc', 'mrcnn_mask'))
        net.load_state_dict(sd)
        log(f"starting from {base_path}")
    dest = mm.allocateNew(dataset, class_names)
    net = net.to(device)
    load = lambda files: [read_annotation(f, class_names) for f in files]
    trainer = MaskRCNNTrainer(net, layers='all', seed=seed, augmentation=True)
    trainer.train(load(train_files), load(test_files), epochs, batch, dest=os.path.abspath(dest), log=log)
    mm.update()
    return dest


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset', type=str, help="The dataset to train on. Can be a partial name.")
    parser.add_argument('-batch_size', type=int, choices=[1, 2, 4, 8, 12, 16], default=2, help="Batch size for training")
    parser.add_argument('-cont', action='store_true', help="Continue latest trained model.")
    parser.add_argument('-cont_from', type=str, default=None, help="Last model to build from.")
    parser.add_argument('-epochs', type=int, default=300, help="Epochs to train (the reference's fixed 300).")
    parser.add_argument('-base', type=str, default=None, help="Weight file to start from when no model is continued.")
    args = parser.parse_args()
    train(args.dataset, args.batch_size, args.cont, args.cont_from, args.epochs, args.base)
