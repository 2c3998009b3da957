#!/usr/bin/env python3
"""What the silhouette term costs and what it buys (csrc/rope_silhouette.hip, prediction/refinement.py: BundleRefiner(silhouette=))
-> profiles/silhouette.txt.

    python tools/bench_silhouette.py kernels     # rope_mask_distance and rope_silhouette_normal_equations beside rope_bundle_normal_equations
    python tools/bench_silhouette.py recovery    # tools/bench_bundle_refine.py's ten frames in 'frame' mode, with and without the term

`kernels`: renders of random poses at 160x90 and 640x480, 512 frames; the masks are those of renders 0.02 rad away.  The three calls
are made in turn, 20 times each per shape, straight through the C entry points on buffers made beforehand, each between two events of
the stream; median (min .. max) of a call."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

SHAPES = [('1280_720_color', 8, 512), ('640_480_color', 1, 512)]
CALLS = 20
RADIUS = 8


def kernels():
    import torch
    from rope_s3d_amd import engine as eng
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import PoseRefiner, camera_twists
    from rope_s3d_amd.projection import Intrinsics
    from rope_s3d_amd.simulation.render import Renderer
    lib = eng.load_library()
    vp = C.c_void_p
    print(f"rope_mask_distance (radius {RADIUS}) and rope_silhouette_normal_equations beside rope_bundle_normal_equations (6 joints + 6 twists each) on "
          f"the same planes; stream events around one call, {CALLS} calls each a shape, taken in turn; median (min .. max) of a call, microseconds")
    for preset, ds, n in SHAPES:
        intr = Intrinsics(preset)
        intr.downscale(ds)
        rend = Renderer('seg', DEFAULT_CAMERA_POSE, intr)
        ref = PoseRefiner(rend, DEFAULT_CAMERA_POSE, intr)
        lim = ref.limits
        rng = np.random.default_rng(5)
        truth = rng.uniform(lim[:, 0], lim[:, 1], (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
        q = truth + rng.uniform(-.02, .02, (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
        T, ti = rend.render_ids_batch_device(truth)
        rd, ri = rend.render_ids_batch_device(q)
        mask = (ti < ref.n_links).to(torch.uint8).contiguous()
        joints = torch.from_numpy(ref.joint_axes(q)).cuda()
        twists = torch.from_numpy(np.tile(camera_twists(DEFAULT_CAMERA_POSE)[None], (n, 1, 1))).cuda()
        H, W = intr.height, intr.width
        sd2 = torch.empty((n, H, W), dtype=torch.int32, device='cuda')
        out = torch.empty((n, 96), dtype=torch.float64, device='cuda')
        work = torch.empty(max(lib.rope_bundle_normal_workspace(n, H, W), lib.rope_silhouette_normal_workspace(n, H, W)) // 8, dtype=torch.float64,
                           device='cuda')
        st = vp(torch.cuda.current_stream().cuda_stream)
        f4 = [float(v) for v in (intr.fx, intr.fy, intr.cx, intr.cy)]
        calls = {
            'distance': lambda: lib.rope_mask_distance(vp(mask.data_ptr()), n, H, W, RADIUS, vp(sd2.data_ptr()), st),
            'silhouette': lambda: lib.rope_silhouette_normal_equations(vp(rd.data_ptr()), vp(ri.data_ptr()), vp(sd2.data_ptr()), n, H, W, ref.n_links, *f4,
                                                                       vp(joints.data_ptr()), 6, vp(twists.data_ptr()), 6, RADIUS, vp(out.data_ptr()),
                                                                       vp(work.data_ptr()), st),
            'bundle': lambda: lib.rope_bundle_normal_equations(vp(rd.data_ptr()), vp(ri.data_ptr()), vp(T.data_ptr()), n, H, W, ref.n_links, *f4,
                                                               vp(joints.data_ptr()), 6, vp(twists.data_ptr()), 6, ref.clip, vp(out.data_ptr()),
                                                               vp(work.data_ptr()), st)}
        times = {k: [] for k in calls}
        for rep in range(CALLS + 3):                    # in turn: what drifts over the session drifts for all three; three rounds to warm up
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = call()
                b.record()
                b.synchronize()
                assert rc == 0, (k, rc)
                if rep >= 3:
                    times[k].append(a.elapsed_time(b) * 1e3)
            if rep == 0:
                words = out.cpu().numpy().copy()        # the last call was the bundle's
                lib.rope_silhouette_normal_equations(vp(rd.data_ptr()), vp(ri.data_ptr()), vp(sd2.data_ptr()), n, H, W, ref.n_links, *f4, vp(joints.data_ptr()),
                                                     6, vp(twists.data_ptr()), 6, RADIUS, vp(out.data_ptr()), vp(work.data_ptr()), st)
                sil = out.cpu().numpy().copy()
        print(f"  {W}x{H} x {n} frames: a frame has {words[:, 0].mean():.0f} BOTH pixels and {words[:, 2].mean():.0f} depth inliers, "
              f"{sil[:, 0].mean():.0f} contour pixels and {sil[:, 2].mean():.0f} outline inliers on average")
        for k, t in times.items():
            t = np.array(t)
            print(f"  {W}x{H} x {n} frames {k:10}: {np.median(t):10.2f} ({t.min():.2f} .. {t.max():.2f})  = {np.median(t) / n:8.3f} us a frame", flush=True)
        rend.engine.close()


def recovery():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import BundleRefiner
    from rope_s3d_amd.projection import camera_matrix
    from rope_s3d_amd.simulation.render import Renderer
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])
    rend = Renderer('seg', true_pose, '1280_720_color', intrinsic_ds_factor=8)
    intr, e = rend.intrinsics, rend.engine
    rng = np.random.default_rng(4242)
    lim, slu = rend.robot.joint_limits, np.array([1, 1, 1, 0, 0, 0])
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (10, 6)) * slu
    T, ti = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (10, 1, 1)))
    mask = ti < 6
    near = true_pose + np.array([.001, -.001, .001, .002, -.002, .002])
    start = truth + rng.choice([-.0075, .0075], (10, 6)) * slu
    fmt = lambda v: ' '.join(f"{x:.2e}" for x in v)
    ang = lambda q: np.abs(q - truth)[:, :3].mean()
    print("10 synthetic frames 1280x720 / 8 (160x90), tools/bench_bundle_refine.py's: the camera starts one lattice step off (1 mm, 2 mrad), S, L, U of "
          "every frame one Descent step (0.0075 rad) off; 'frame' mode; |pose - true| x y z (m) a3 a4 a5 (rad), mean |angle - true| over S, L, U (rad)")
    print(f"  start:                          pose {fmt(np.abs(near - true_pose))}  angles {ang(start):.3e}")
    for name, kw, depth in (("depth alone (silhouette=0)", {}, T), ("depth + outline (silhouette=1)", dict(silhouette=1.0), T),
                            ("depth + outline (silhouette=4)", dict(silhouette=4.0), T), ("outline alone (silhouette=1)", dict(silhouette=1.0), None)):
        for iterations in (5, 10):
            b = BundleRefiner(rend, intr, joints='frame', iterations=iterations, **kw).refine(near, start, depth, mask)
            print(f"  {name}, {iterations} rounds: pose {fmt(np.abs(b.pose - true_pose))}  angles {ang(b.angles):.3e}  ({b.steps_taken} steps, depth "
                  f"cost {b.cost_before:.3e} -> {b.cost_after:.3e} m^2, outline cost {b.cost_silhouette_before:.3e} -> {b.cost_silhouette_after:.3e} px^2)")
            print(f"    formal sigma of the pose {fmt(b.sigma_pose)}; median formal sigma of S, L, U {fmt(np.median(b.sigma_angles[:, :3], axis=0))}",
                  flush=True)
    e.close()


if __name__ == '__main__':
    {'kernels': kernels, 'recovery': recovery}[sys.argv[1] if len(sys.argv) > 1 else 'kernels']()
