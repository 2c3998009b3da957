#!/usr/bin/env python3
"""Times the photographs of synthetic frames (csrc/rope_shade.hip) on the GPU: rope_shade_frames alone on rendered planes (with
noise and drawn backgrounds, and as default_params' scene without either), Renderer.render_photo_batch_device (render + shade),
and beside them the existing way to a lit picture, Renderer.render_batch in mode 'real' (planes copied down, shade_depth's numpy
loop per frame) on the same poses — for a batch of 64 poses at 1280x720 and at 640x480.  Kernel figures are device events around
`reps` calls on one stream; the others a host clock around calls that end in a synchronise.  Bytes per pixel are what the
algorithm must move (depth 4 + ids 1 in, picture 3 + depth 4 out, + 3 of background picture where a frame has one), computed from
the shapes; the rate is those bytes over the kernel's time.  The working set is compared with the 256 MiB Infinity Cache: where it
fits, repeated calls re-read it on-die and the figure is no HBM rate.
Usage: python tools/bench_shade.py [--reps 50] [--host-frames 8] [--out profiles/shade_frames.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

INFINITY_CACHE = 256 * 2 ** 20


def timed_events(fn, reps, warmup=5):
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


def timed_host(fn, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    import torch
    from rope_s3d_amd import engine as eng
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.simulation.render import Renderer
    from rope_s3d_amd.simulation.shading import default_params, draw_params, make_backgrounds
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--host-frames', type=int, default=8)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    N, n_bg = 64, 8
    lines = [f"rope_shade_frames, {torch.cuda.get_device_name(0)}, build {eng.load_library().rope_build_id().decode()}, batch of {N} poses, "
             f"{args.reps} calls per kernel figure (device events), render + shade by a host clock over {max(3, args.reps // 10)} calls, "
             f"mode 'real' (host loop) over {args.host_frames} of the same poses, once",
             "command: python tools/bench_shade.py" + ''.join(f' {a}' for a in sys.argv[1:]),
             f"{'shape':<14}{'scene':<22}{'B/pixel':>8}{'MB moved':>10}{'fits L3':>9}{'kernel ms':>11}{'ms/frame':>10}{'GB/s':>8}"]
    tail = []
    for preset in ('1280_720_color', '640_480_color'):
        r = Renderer('seg', DEFAULT_CAMERA_POSE, preset)
        H, W = r.resolution
        lim = r.robot.joint_limits
        angles = np.stack([np.random.default_rng(7919 + f).uniform(lim[:, 0], lim[:, 1]) * [1, 1, 1, 0, 0, 0] for f in range(N)])
        depth, ids = r.render_ids_batch_device(angles)
        backs = torch.from_numpy(make_backgrounds(1, n_bg, H, W)).cuda()
        intr = (r.intrinsics.fx, r.intrinsics.fy, r.intrinsics.cx, r.intrinsics.cy)
        out, dout = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda'), torch.empty_like(depth)
        robot = float((ids < 6).float().mean())
        for scene, params, bg in (('drawn: noise, pictures', draw_params(1, np.arange(N), 6, n_bg), backs), ('default: neither', default_params(N), None)):
            fn = lambda: r.engine.shade_frames(depth, ids, params, intr, 6, bg, 0, 1, depth_out=dout, out=out)        # noqa: E731
            ms = timed_events(fn, args.reps)
            per_px = 4 + 1 + 3 + 4 + (3.0 * float(np.mean(params['bg_index'] >= 0)) if bg is not None else 0.0)
            nbytes = per_px * N * H * W
            lines.append(f"{f'{W}x{H}':<14}{scene:<22}{per_px:>8.1f}{nbytes / 1e6:>10.1f}{'yes' if nbytes <= INFINITY_CACHE else 'no':>9}{ms:>11.4f}"
                         f"{ms / N:>10.5f}{nbytes / ms / 1e6:>8.0f}")
        params = draw_params(1, np.arange(N), 6, n_bg)
        ms_photo = timed_host(lambda: r.render_photo_batch_device(angles, None, params, backs, 0, 1), max(3, args.reps // 10))
        ms_ids = timed_host(lambda: r.render_ids_batch_device(angles), max(3, args.reps // 10))
        real = Renderer('real', DEFAULT_CAMERA_POSE, preset)
        k = args.host_frames
        t = time.perf_counter()
        real.render_batch(angles[:k])
        ms_real = (time.perf_counter() - t) * 1e3 / k
        tail.append(f"{W}x{H}: robot pixels {100 * robot:.1f} %; render_ids_batch_device {ms_ids / N:.4f} ms/frame; render_photo_batch_device "
                    f"{ms_photo / N:.4f} ms/frame (host clock, {N} poses a call); render_batch mode 'real' {ms_real:.1f} ms/frame "
                    f"({k} poses, planes copied down + shade_depth per frame): {ms_real / (ms_photo / N):.0f} x")
        del depth, ids, backs, out, dout
    lines += tail
    lines.append("fits L3: whether the bytes of one call fit the 256 MiB Infinity Cache; 'no' means the repeated calls stream through HBM.")
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
