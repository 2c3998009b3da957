#!/usr/bin/env python3
"""What the outline term's second direction costs and what it buys (csrc/rope_silhouette_reverse.hip, prediction/refinement.py:
BundleRefiner(silhouette=, both_ways=True)) -> profiles/silhouette_two_way.txt.

    python tools/bench_silhouette_two_way.py kernels     # rope_render_nearest and the reverse equations beside their forward siblings
    python tools/bench_silhouette_two_way.py recovery    # tools/bench_silhouette.py's ten frames, one way and both ways, with depth and without
    python tools/bench_silhouette_two_way.py gap         # the same frames with U started so far off that the forearm's outline leaves the mask's reach
    python tools/bench_silhouette_two_way.py wall N 0|1  # one fresh process: seconds a round of BundleRefiner.refine on N frames, both_ways off / on;
                                                         # `wall N 0` also runs from a copy of this file in a checkout of the parent commit
    python tools/bench_silhouette_two_way.py trace DIR   # the per-kernel rows of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- ... kernels` run

`kernels`: tools/bench_silhouette.py's planes (renders of random poses at 160x90 and 640x480, 512 frames, masks of renders 0.02 rad
away); the four calls are made in turn, 20 times each per shape, through the C entry points on buffers made beforehand.  It prints
stream-event times, which include the launches' host side; the kernels' own times come from a kernel trace of the same run, read by
`trace`."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

SHAPES = [('1280_720_color', 8, 512), ('640_480_color', 1, 512)]
CALLS = 20
RADIUS = 8
SLU = np.array([1, 1, 1, 0, 0, 0])


def kernels():
    import torch
    from rope_s3d_amd import engine as eng
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import PoseRefiner, camera_twists
    from rope_s3d_amd.projection import Intrinsics
    from rope_s3d_amd.simulation.render import Renderer
    lib = eng.load_library()
    vp = C.c_void_p
    print(f"radius {RADIUS}, 6 joints + 6 twists; stream events around one call, {CALLS} calls each a shape, taken in turn; median (min .. max), microseconds")
    for preset, ds, n in SHAPES:
        intr = Intrinsics(preset)
        intr.downscale(ds)
        rend = Renderer('seg', DEFAULT_CAMERA_POSE, intr)
        ref = PoseRefiner(rend, DEFAULT_CAMERA_POSE, intr)
        rng = np.random.default_rng(5)
        truth = rng.uniform(ref.limits[:, 0], ref.limits[:, 1], (n, 6)) * SLU
        q = truth + rng.uniform(-.02, .02, (n, 6)) * SLU
        _, ti = rend.render_ids_batch_device(truth)
        rd, ri = rend.render_ids_batch_device(q)
        mask = (ti < ref.n_links).to(torch.uint8).contiguous()
        cover = (ri < ref.n_links).to(torch.uint8).contiguous()
        joints = torch.from_numpy(ref.joint_axes(q)).cuda()
        twists = torch.from_numpy(np.tile(camera_twists(DEFAULT_CAMERA_POSE)[None], (n, 1, 1))).cuda()
        H, W = intr.height, intr.width
        sd2 = torch.empty((n, H, W), dtype=torch.int32, device='cuda')
        sd2c = torch.empty((n, H, W), dtype=torch.int32, device='cuda')
        near = torch.empty((n, H, W), dtype=torch.int16, device='cuda')
        out = torch.empty((n, 96), dtype=torch.float64, device='cuda')
        work = torch.empty(lib.rope_silhouette_normal_workspace(n, H, W) // 8, dtype=torch.float64, device='cuda')
        st = vp(torch.cuda.current_stream().cuda_stream)
        f4 = [float(v) for v in (intr.fx, intr.fy, intr.cx, intr.cy)]
        cols = (vp(joints.data_ptr()), 6, vp(twists.data_ptr()), 6, RADIUS, vp(out.data_ptr()), vp(work.data_ptr()), st)
        calls = {
            'distance(mask)': lambda: lib.rope_mask_distance(vp(mask.data_ptr()), n, H, W, RADIUS, vp(sd2.data_ptr()), st),
            'distance(coverage)': lambda: lib.rope_mask_distance(vp(cover.data_ptr()), n, H, W, RADIUS, vp(sd2c.data_ptr()), st),
            'nearest(ids)': lambda: lib.rope_render_nearest(vp(ri.data_ptr()), n, H, W, ref.n_links, RADIUS, vp(near.data_ptr()), st),
            'forward': lambda: lib.rope_silhouette_normal_equations(vp(rd.data_ptr()), vp(ri.data_ptr()), vp(sd2.data_ptr()), n, H, W, ref.n_links, *f4, *cols),
            'reverse': lambda: lib.rope_silhouette_normal_equations_reverse(vp(mask.data_ptr()), vp(near.data_ptr()), vp(rd.data_ptr()), vp(ri.data_ptr()), n, H,
                                                                            W, ref.n_links, *f4, *cols)}
        times, words = {k: [] for k in calls}, {}
        for rep in range(CALLS + 3):                    # in turn: what drifts over the session drifts for all; three rounds to warm up
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = call()
                b.record()
                b.synchronize()
                assert rc == 0, (k, rc)
                if rep >= 3:
                    times[k].append(a.elapsed_time(b) * 1e3)
                if rep == 0 and k in ('forward', 'reverse'):
                    words[k] = out.cpu().numpy().copy()
        print(f"  {W}x{H} x {n} frames: forward {words['forward'][:, 0].mean():.0f} contour pixels and {words['forward'][:, 2].mean():.0f} inliers a frame, "
              f"reverse {words['reverse'][:, 0].mean():.0f} and {words['reverse'][:, 2].mean():.0f}")
        for k, t in times.items():
            t = np.array(t)
            print(f"  {W}x{H} x {n} frames {k:19}: {np.median(t):10.2f} ({t.min():.2f} .. {t.max():.2f})  = {np.median(t) / n:8.3f} us a frame", flush=True)
        rend.engine.close()


def _ten_frames():
    """tools/bench_silhouette.py recovery's scene -> (renderer, true pose, truth, depth T, masks, start pose, start angles)"""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.projection import camera_matrix
    from rope_s3d_amd.simulation.render import Renderer
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])
    rend = Renderer('seg', true_pose, '1280_720_color', intrinsic_ds_factor=8)
    rng = np.random.default_rng(4242)
    lim = rend.robot.joint_limits
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (10, 6)) * SLU
    T, ti = rend.engine.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, rend.intrinsics)[None], (10, 1, 1)))
    near = true_pose + np.array([.001, -.001, .001, .002, -.002, .002])
    start = truth + rng.choice([-.0075, .0075], (10, 6)) * SLU
    return rend, true_pose, truth, T, ti < 6, near, start


def _rows(rend, true_pose, truth, T, mask, near, start, cases, rounds):
    from rope_s3d_amd.prediction.refinement import BundleRefiner
    fmt = lambda v: ' '.join(f"{x:.2e}" for x in v)
    ang = lambda q: np.abs(q - truth)[:, :3].mean()
    print(f"  start:                                      pose {fmt(np.abs(near - true_pose))}  angles {ang(start):.3e}  (S {np.abs(start - truth)[:, 0].mean():.3e} "
          f"L {np.abs(start - truth)[:, 1].mean():.3e} U {np.abs(start - truth)[:, 2].mean():.3e})")
    for name, kw, depth in cases:
        for iterations in rounds:
            b = BundleRefiner(rend, rend.intrinsics, joints='frame', iterations=iterations, **kw).refine(near, start, T if depth else None, mask)
            d = np.abs(b.angles - truth)
            print(f"  {name}, {iterations} rounds: pose {fmt(np.abs(b.pose - true_pose))}  angles {ang(b.angles):.3e} (S {d[:, 0].mean():.3e} L {d[:, 1].mean():.3e} "
                  f"U {d[:, 2].mean():.3e})  ({b.steps_taken} steps, depth cost {b.cost_before:.3e} -> {b.cost_after:.3e} m^2, outline cost "
                  f"{b.cost_silhouette_before:.3e} -> {b.cost_silhouette_after:.3e} px^2, outline inliers {b.inliers_silhouette:.0f} + "
                  f"{b.inliers_silhouette_reverse:.0f})", flush=True)


CASES = (("depth + outline one way  (silhouette=1)      ", dict(silhouette=1.0), True),
         ("depth + outline both ways (.., both_ways=True)", dict(silhouette=1.0, both_ways=True), True),
         ("outline alone one way   (depth=None)         ", dict(silhouette=1.0), False),
         ("outline alone both ways (depth=None)         ", dict(silhouette=1.0, both_ways=True), False))


def recovery():
    rend, true_pose, truth, T, mask, near, start = _ten_frames()
    print("10 synthetic frames 1280x720 / 8 (160x90), tools/bench_silhouette.py recovery's: the camera starts one lattice step off (1 mm, 2 mrad), S, L, U of "
          "every frame one Descent step (0.0075 rad) off; 'frame' mode, radius 8; |pose - true| x y z (m) a3 a4 a5 (rad), mean |angle - true| over S, L, U (rad)")
    _rows(rend, true_pose, truth, T, mask, near, start, CASES, (5, 10))
    rend.engine.close()


def gap():
    """U of every frame started 0.35 rad off: the forearm's outline in the render lies beyond the radius of the mask's for most of its
    length, so the render's contour pixels there are FAR and carry nothing one way."""
    rend, true_pose, truth, T, mask, near, start = _ten_frames()
    start = start.copy()
    start[:, 2] = truth[:, 2] + 0.35 * np.where(np.arange(10) % 2, 1.0, -1.0)
    print("the same ten frames with U of every frame started 0.35 rad off (alternating sign), the camera and S, L as above; radius 8")
    _rows(rend, true_pose, truth, T, mask, near, start, CASES[2:] + CASES[:2], (10,))
    rend.engine.close()


def wall(n, both):
    import torch
    from rope_s3d_amd.prediction.refinement import BundleRefiner
    rend, true_pose, truth, T, mask, near, start = _ten_frames()
    reps = -(-n // 10)
    tile = lambda a: (a.repeat(reps, 1, 1) if isinstance(a, torch.Tensor) else np.tile(a, (reps, 1)))[:n]
    T, mask, start = tile(T).contiguous(), tile(mask).contiguous(), tile(start)
    r = BundleRefiner(rend, rend.intrinsics, joints='frame', iterations=5, silhouette=1.0, **(dict(both_ways=True) if both else {}))     # runs on the parent's tree too
    r.refine(near, start, T, mask)                      # warm
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.refine(near, start, T, mask)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 6)       # iterations + 1 rounds
    print(f"  {n} frames at 160x90, both_ways={both}: {np.median(ts) * 1e3:.3f} ms a round (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}; 3 calls of 6 rounds)",
          flush=True)
    rend.engine.close()


def trace(d):
    """Per kernel of the outline files: calls, mean and minimum duration, from the trace's per-dispatch table.  Each shape makes 23
    calls a kernel; the kernels of the two shapes are told apart by their grids."""
    import csv
    import glob
    import re
    rows = [r for f in glob.glob(os.path.join(d, '**', '*_kernel_trace.csv'), recursive=True) for r in csv.DictReader(open(f))]
    groups = {}
    for r in rows:
        name = r['Kernel_Name']
        if not any(k in name for k in ('mask_distance_kernel', 'render_nearest_kernel', 'sneq_', 'rneq_')):
            continue
        key = (re.search(r'\w+_kernel', name).group(0), int(r['Grid_Size_X']) * int(r['Grid_Size_Y']))
        groups.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3)
    for (name, grid), t in sorted(groups.items()):
        t = np.array(t[3:] if len(t) > 3 else t)                        # the warm-up rounds come first
        print(f"  {name:24} grid {grid:10d} threads: {len(t):3d} dispatches, median {np.median(t):9.2f} us (min {t.min():.2f}, max {t.max():.2f})")


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    if mode == 'wall':
        wall(int(sys.argv[2]), bool(int(sys.argv[3])))
    elif mode == 'trace':
        trace(sys.argv[2])
    else:
        {'kernels': kernels, 'recovery': recovery, 'gap': gap}[mode]()
