#!/usr/bin/env python3
"""Times the depth conditioning (prediction/conditioning.py, csrc/rope_feed.hip) on raw 1280x720 z16 frames with the reference's
LiveCamera settings: the whole chain (decimate by 2 -> spatial, 2 iterations -> temporal -> align to a 1280x720 colour sensor)
for ONE frame, which is the live case, and for 64 frames in one process_many, with the split over the four entry points; beside
them Predictor.run's time per frame from the same session and the 33.3 ms frame period of a 30 fps camera.  Times are device
events around `reps` calls on one stream (a chain = 1 memset + 8 kernels), frames resident on the device: the upload of a raw
frame and the download of the aligned plane are not in them (not measured here).  For every figure the bytes of the planes the
calls touch are given, and whether they fit the 256 MiB Infinity Cache: if they do, repeated calls can have been served from it
and the figure is no HBM rate.  Before anything is timed the chain is compared with tests/feed_ref.py on a small crop.
Usage: python tools/bench_feed.py [--reps 200] [--out profiles/feed_condition.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

INFINITY_CACHE = 256 * 2 ** 20
H, W, SCALE = 720, 1280, 0.001
SENSOR = {'width': W, 'height': H, 'fx': 640.0, 'fy': 640.0, 'cx': 639.5, 'cy': 359.5}
EXTRIN = {'rotation': [1, 0, 0, 0, 1, 0, 0, 0, 1], 'translation': [0.015, 0.0, 0.0]}


def timed(fn, reps, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps                              # ms per call


def frames(n, h=H, w=W, seed=0):
    """A slanted surface 0.8 .. 2.3 m away with a step edge, +-6 units of noise from frame to frame, 12 % holes: (n, h, w) uint16."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 800 + xx + (yy // 2) + 500 * (xx > w // 2)
    z = base[None] + rng.integers(-6, 7, (n, h, w))
    z[rng.random((n, h, w)) < 0.12] = 0
    return z.astype(np.uint16)


def check_crop():
    import feed_ref
    from rope_s3d_amd.prediction.conditioning import DepthConditioner
    h, w = 48, 96
    raw = frames(3, h, w, seed=3)
    sensor = dict(SENSOR, width=w, height=h, cx=47.5, cy=23.5, fx=50.0, fy=50.0)
    terms = [sensor[k] for k in ('fx', 'fy', 'cx', 'cy')]
    ref = feed_ref.Chain(terms, terms, EXTRIN['rotation'] + EXTRIN['translation'], SCALE, (h, w))
    got = DepthConditioner(sensor, sensor, EXTRIN, SCALE).process_many(raw)
    assert np.array_equal(got, ref.process_many(raw)), "the chain differs from tests/feed_ref.py"


def main():
    import torch
    from rope_s3d_amd import engine as eng
    from rope_s3d_amd.prediction.conditioning import DepthConditioner
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--no-predictor', action='store_true')
    args = ap.parse_args()
    lib = eng.load_library()
    check_crop()
    lines = [f"depth conditioning, {torch.cuda.get_device_name(0)}, build {lib.rope_build_id().decode()}: raw {W}x{H} z16 -> decimate 2 -> "
             f"spatial (2, 0.5, 20) -> temporal (0.5, 20, 3) -> align to {W}x{H}; device events around repeated calls on one stream, frames "
             "resident on the device (upload and download not measured); equal to tests/feed_ref.py on a 96x48 crop of 3 frames",
             f"{'frames per call':<17}{'step':<11}{'ms per call':>12}{'ms per frame':>14}{'MB touched':>12}{'fits L3':>9}"]
    p = lambda t: C.c_void_p(t.data_ptr())                        # noqa: E731
    chain_ms = {}
    for N, reps in ((1, args.reps), (64, max(10, args.reps // 10))):
        raw = torch.from_numpy(frames(N, seed=N).view(np.int16)).cuda()
        c = DepthConditioner(SENSOR, SENSOR, EXTRIN, SCALE)
        h, w = c.conditioned_shape(H, W)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        planes = torch.empty((N, h, w), dtype=torch.int16, device='cuda')
        last, hist = torch.zeros((h, w), dtype=torch.int16, device='cuda'), torch.zeros((h, w), dtype=torch.uint8, device='cuda')
        scratch, out = torch.empty((N, H, W), dtype=torch.int32, device='cuda'), torch.empty((N, H, W), dtype=torch.int16, device='cuda')
        d, k, e = (C.c_double * 4)(*c.align_terms), (C.c_double * 4)(*c.color_terms), (C.c_double * 12)(*c.extrin)

        def ok(rc):
            assert rc == 0, rc
        steps = [('decimate', lambda: ok(lib.rope_depth_decimate(p(raw), N, H, W, 2, p(planes), st)), 2 * N * (H * W + h * w)),
                 ('spatial', lambda: ok(lib.rope_depth_spatial(p(planes), N, h, w, 0.5, 20, 2, st)), 2 * N * h * w * 2),
                 ('temporal', lambda: ok(lib.rope_depth_temporal(p(planes), N, h, w, 0.5, 20, 3, p(last), p(hist), st)), 2 * N * h * w * 2 + 6 * h * w),
                 ('align', lambda: ok(lib.rope_depth_align(p(planes), N, h, w, d, k, e, SCALE, H, W, p(scratch), p(out), st)),
                  N * (2 * h * w + 6 * H * W))]
        whole = 2 * N * H * W + 2 * N * h * w + 6 * N * H * W + 3 * h * w             # raw, planes, scratch + out, state: each counted once
        t = timed(lambda: c.process_many_device(raw), reps)
        chain_ms[N] = t / N
        lines.append(f"{N:<17}{'chain':<11}{t:>12.4f}{t / N:>14.4f}{whole / 1e6:>12.1f}{'yes' if whole <= INFINITY_CACHE else 'no':>9}")
        for name, fn, nbytes in steps:                            # in the chain's order, so that every step sees what it would see
            t = timed(fn, reps)
            lines.append(f"{N:<17}{name:<11}{t:>12.4f}{t / N:>14.4f}{nbytes / 1e6:>12.1f}{'yes' if nbytes <= INFINITY_CACHE else 'no':>9}")
        del raw, planes, scratch, out, c
    lines.append("the spatial step is 2 x (1 row kernel + 1 column kernel), the align step 1 memset + 2 kernels; a step's bytes are its planes "
                 "read or written once (the spatial sweeps pass over theirs 4 times per iteration)")
    if not args.no_predictor:
        from rope_s3d_amd import SyntheticPredictor
        from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
        sp = SyntheticPredictor(DEFAULT_CAMERA_POSE, '1280_720_color', 8, 'SLU', noise=False, seed=5)
        lim = sp.urdf_reader.joint_limits
        sp.renderer.setJointAngles(np.random.default_rng(9).uniform(lim[:, 0] * .4, lim[:, 1] * .4) * np.array([1, 1, 1, 0, 0, 0]))
        color, depth = sp.renderer.render()
        for _ in range(3):
            sp.predictor.run(color, depth)
        t0 = time.perf_counter()
        n = 20
        for _ in range(n):
            sp.predictor.run(color, depth)
        run_ms = (time.perf_counter() - t0) * 1e3 / n
        lines.append(f"Predictor.run, 1280x720 frame at ds_factor 8, SLU, host clock over {n} runs (each ends with its result on the host): "
                     f"{run_ms:.3f} ms per frame")
    else:
        lines.append("Predictor.run: not measured (--no-predictor)")
    lines.append(f"frame period of a 30 fps camera: 33.333 ms; the chain for one frame is {chain_ms[1]:.4f} ms of it, "
                 f"{chain_ms[64]:.4f} ms per frame in a batch of 64")
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
