#!/usr/bin/env python3
"""Images/s of a full Mask R-CNN training step (layers='all', 512 x 512, float32) at batch 2 and 8, on seeded synthetic frames.
For the split between the trunk's library kernels and this library's training kernels, run it once under
`rocprofv3 --kernel-trace --stats -- python tools/bench_train.py --batches 2` and read the kernel_stats file (the rope_train.hip
kernels are rpn_*_kernel, roi_targets_kernel and roi_align_f32*_kernel)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def samples(n, size=640, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        img = rng.integers(0, 80, (size * 3 // 4, size, 3), dtype=np.uint8)
        k = int(rng.integers(2, 7))
        masks = np.zeros((k,) + img.shape[:2], bool)
        for i in range(k):
            y, x = rng.integers(0, img.shape[0] - 120), rng.integers(0, size - 120)
            masks[i, y:y + int(rng.integers(30, 120)), x:x + int(rng.integers(30, 120))] = True
            img[masks[i]] = rng.integers(100, 255, 3)
        out.append((img, masks, np.arange(1, k + 1, dtype=np.int32) % 6 + 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[2, 8])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from rope_s3d_amd import maskrcnn as mr
    from rope_s3d_amd import training as tr
    res = {}
    for b in a.batches:
        torch.manual_seed(0)
        trainer = tr.MaskRCNNTrainer(mr.MaskRCNN(7).cuda(), layers='all', seed=0, augmentation=False)
        data = samples(b)
        for _ in range(a.warmup):
            trainer.step(data)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            trainer.step(data)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        res[f'batch_{b}'] = {'step_ms': dt * 1e3, 'images_per_s': b / dt}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
