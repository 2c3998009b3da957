#!/usr/bin/env python3
"""BASELINE configs[2] shape: synthetic RGB-D set -> Mask R-CNN stage (PyTorch-ROCm) -> HIP engine -> stage machine.

    python tools/bench_pipeline.py [n_frames]
    python tools/bench_pipeline.py [n_frames] --device-targets [--intrin 640_480_color --ds-factor 1] [--segmenters color,maskrcnn] [--repeats 3]

Random network weights (none exist offline): detections and therefore predictions are meaningless, the frame rate
of the whole pipeline is what this measures.  min_confidence 0 keeps all 100 detections per frame (worst case).

--device-targets: per segmenter, predict_dataset.py without and with -device_targets in turn, `--repeats` times each after one
warm-up of both, on the same set in the same process; every run and the medians are printed.  A segmenter that does not leave its
masks on the GPU (color) runs the same path either way: its pair of figures shows the spread of the measurement."""
import argparse, os, statistics, sys, tempfile, time
os.environ['ROPE_TIMING'] = '1'      # predict_dataset prints set-up and frame time apart
import numpy as np
import torch
torch.cuda.init()        # torch's bundled HIP runtime has to come up before librope_hip.so brings in the system one
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
import predict_dataset as pd
from rope_s3d_amd.data.dataset import make_synthetic_dataset

ap = argparse.ArgumentParser()
ap.add_argument('n_frames', type=int, nargs='?', default=40)
ap.add_argument('--device-targets', action='store_true', help="compare Predictor(device_targets=False / True), alternating")
ap.add_argument('--intrin', default='1280_720_color')
ap.add_argument('--ds-factor', type=int, default=8)
ap.add_argument('--segmenters', default='color,maskrcnn')
ap.add_argument('--repeats', type=int, default=3)
opt = ap.parse_args()
n = opt.n_frames


def timed(args):
    t0 = time.perf_counter()
    out = pd.run(argparse.Namespace(**vars(args)))
    return time.perf_counter() - t0, out


with tempfile.TemporaryDirectory() as tmp:
    d = make_synthetic_dataset(os.path.join(tmp, 'pipe'), n, base_intrin=opt.intrin, seed=7919)
    os.chdir(tmp)
    base = dict(dataset=d, angs='SLU', ds_factor=opt.ds_factor, weights=None, lookup_divisions=None, predictors=int(os.environ.get('ROPE_PREDICTORS', '1')), batch=None)
    if not opt.device_targets:
        for seg in (None, 'color', 'maskrcnn'):
            args = argparse.Namespace(segmenter=seg, **base)
            pd.run(argparse.Namespace(**{**vars(args)}))                 # warm-up incl. construction
            dt, out = timed(args)
            print(f"segmenter={seg}: {n} frames in {dt:.2f} s = {n / dt:.1f} frames/s (includes Predictor construction and lookup-table build)")
    else:
        print(f"{n} frames of {opt.intrin} / {opt.ds_factor}, device_targets off and on in turn, {opt.repeats} runs each (construction and lookup-table build included)")
        for seg in opt.segmenters.split(','):
            variants = {flag: argparse.Namespace(segmenter=seg, device_targets=flag, **base) for flag in (False, True)}
            angles = {flag: timed(a)[1] for flag, a in variants.items()}             # warm-up of both
            print(f"segmenter={seg}: angles equal with and without the flag: {bool(np.array_equal(angles[False], angles[True]))}")
            rates = {False: [], True: []}
            for r in range(opt.repeats):
                for flag, a in variants.items():
                    dt, _ = timed(a)
                    rates[flag].append(n / dt)
                    print(f"segmenter={seg} device_targets={'on' if flag else 'off'} run {r + 1}: {n} frames in {dt:.2f} s = {n / dt:.1f} frames/s")
            off, on = statistics.median(rates[False]), statistics.median(rates[True])
            print(f"segmenter={seg}: median {off:.1f} frames/s off, {on:.1f} frames/s on ({on / off:.3f} x)")
