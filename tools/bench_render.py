#!/usr/bin/env python3
"""Bulk rendering: poses/s of the Renderer.render() loop against Renderer.render_batch (rope_render_batch), with the
renderer's camera and with a camera per pose, and the frames/s of a SyntheticDataset slice read (og_img[a:b] then
depthmaps[a:b]) frame by frame, as it was read before SyntheticDataset.frames, and through it.  Every batch is checked
against the loop before its rate is printed.

    python tools/bench_render.py [--poses 1024] [--slice 256] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE  # noqa: E402
from rope_s3d_amd.data.dataset import SyntheticDataset  # noqa: E402
from rope_s3d_amd.simulation.render import Renderer  # noqa: E402

SIZES = [('1280_720_color', 8), ('640_480_color', 1), ('1280_720_color', 1)]


def timed(fn, reps=1):
    fn()                                                    # warm: buffers sized, kernels loaded
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=1024)
    ap.add_argument('--slice', type=int, default=256)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    results = []
    for preset, ds in SIZES:
        r = Renderer('seg', DEFAULT_CAMERA_POSE, preset, intrinsic_ds_factor=ds if ds > 1 else None)
        lim = r.robot.joint_limits
        rng = np.random.default_rng(2024)
        q = np.zeros((args.poses, 6))
        q[:, :3] = rng.uniform(lim[:3, 0], lim[:3, 1], (args.poses, 3))
        cams = np.array(DEFAULT_CAMERA_POSE, float) + rng.uniform(-0.1, 0.1, (args.poses, 6)) * [1, 1, 1, 0.2, 0.2, 0.2]
        H, W = r.resolution

        def loop():
            c = np.empty((args.poses, H, W, 3), np.uint8)
            d = np.empty((args.poses, H, W), np.float32)
            for k in range(args.poses):
                r.setJointAngles(q[k])
                c[k], d[k] = r.render()
            return c, d
        t_loop, (c_loop, d_loop) = timed(loop)
        t_batch, (c_b, d_b) = timed(lambda: r.render_batch(q))
        assert np.array_equal(c_b, c_loop) and d_b.tobytes() == d_loop.tobytes(), "render_batch differs from the render() loop"
        del c_b, d_b, c_loop, d_loop
        t_cams, (c_v, d_v) = timed(lambda: r.render_batch(q, cams))
        for k in np.linspace(0, args.poses - 1, 16).astype(int):   # per-pose cameras against setCameraPose + render
            r.setCameraPose(cams[k])
            r.setJointAngles(q[k])
            c1, d1 = r.render()
            assert np.array_equal(c_v[k], c1) and d_v[k].tobytes() == d1.tobytes(), f"per-pose camera {k} differs"
        r.setCameraPose(DEFAULT_CAMERA_POSE)
        del c_v, d_v

        # SyntheticDataset slice reads: frame by frame (each plane's slice renders every frame: twice per frame), and batched
        sd = SyntheticDataset(args.slice, preset if ds == 1 else f'{preset}_{ds}', seed=5)
        n = args.slice

        def per_frame():
            og = np.stack([sd.frame(i)[0] for i in range(n)])
            dm = np.stack([sd.frame(i)[1].astype(np.float64) for i in range(n)])
            return og, dm

        def batched():
            sd._block = (None, None)
            return sd.og_img[0:n], sd.depthmaps[0:n]
        t_old, (og0, dm0) = timed(per_frame)
        t_new, (og1, dm1) = timed(batched)
        assert np.array_equal(og0, og1) and dm0.tobytes() == dm1.tobytes(), "slice read differs from per-frame reads"
        del og0, dm0, og1, dm1
        row = {'size': f'{W}x{H}', 'poses': args.poses, 'loop_poses_per_s': args.poses / t_loop,
               'batch_poses_per_s': args.poses / t_batch, 'batch_cameras_poses_per_s': args.poses / t_cams,
               'slice_frames': n, 'slice_read_before_frames_per_s': n / t_old, 'slice_read_after_frames_per_s': n / t_new}
        results.append(row)
        print(f"{row['size']:>9}: render() loop {row['loop_poses_per_s']:8.0f} poses/s | render_batch {row['batch_poses_per_s']:8.0f} | "
              f"per-pose cameras {row['batch_cameras_poses_per_s']:8.0f} | slice read {row['slice_read_before_frames_per_s']:7.0f} -> "
              f"{row['slice_read_after_frames_per_s']:7.0f} frames/s", flush=True)
        r.engine.close()
        sd._r.engine.close()
    print(json.dumps(results))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
