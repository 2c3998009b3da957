#!/usr/bin/env python3
"""What the robust weights of the bundle polish cost and what they buy (csrc/rope_robust.hip, prediction/refinement.py:
BundleRefiner(robust=)) -> profiles/robust.txt.

    python tools/bench_robust.py kernels [--parent LIB]   # the robust equations and the histogram beside rope_bundle_normal_equations
    python tools/bench_robust.py recovery                 # tools/bench_bundle_refine.py's ten frames with an occluder: plain, Huber, Tukey

`kernels`: renders of random poses at 160x90 and 640x480, 512 frames, against the renders 0.02 rad away, as tools/bench_silhouette.py
takes them.  The calls are made in turn, 20 times each per shape after three rounds of warm-up, straight through the C entry points
on buffers made beforehand, each between two events of the stream; median (min .. max) of a call.  --parent LIB: a librope_hip.so
built from the parent commit, loaded beside this build's; its rope_bundle_normal_equations joins the turn on the same buffers, so
the plain path is timed on both builds in one session, alternating.  The same call appears twice in the turn ('bundle' and 'bundle
again'): what the two differ by is the session's own spread.
`recovery`: the ten synthetic 160x90 frames of profiles/bundle_refine.txt, 'frame' mode from the same start, with an occluder
planted in every frame: a disc about the centroid of the drawn pixels, a seventh of them, 2 cm in front of the surface."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

SHAPES = [('1280_720_color', 8, 512), ('640_480_color', 1, 512)]
CALLS = 20
OCCLUDER = 0.02


def kernels(parent=None):
    import torch
    from rope_s3d_amd import engine as eng
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import PoseRefiner, camera_twists
    from rope_s3d_amd.projection import Intrinsics
    from rope_s3d_amd.simulation.render import Renderer
    lib = eng.load_library()
    old = C.CDLL(parent) if parent else None
    vp = C.c_void_p
    if old is not None:
        old.rope_bundle_normal_equations.argtypes = list(lib.rope_bundle_normal_equations.argtypes)
        old.rope_build_id.restype = C.c_char_p
    print(f"rope_bundle_normal_equations_robust (Huber and Tukey at scale clip / 4) and rope_residual_histogram beside "
          f"rope_bundle_normal_equations (6 joints + 6 twists each) on the same planes, {torch.cuda.get_device_name(0)}, build {eng.build_id()}"
          + (f", parent build {old.rope_build_id().decode()}" if old is not None else '')
          + f"; stream events around one call, {CALLS} calls each a shape, taken in turn; median (min .. max) of a call, microseconds")
    for preset, ds, n in SHAPES:
        intr = Intrinsics(preset)
        intr.downscale(ds)
        rend = Renderer('seg', DEFAULT_CAMERA_POSE, intr)
        ref = PoseRefiner(rend, DEFAULT_CAMERA_POSE, intr)
        lim = ref.limits
        rng = np.random.default_rng(5)
        truth = rng.uniform(lim[:, 0], lim[:, 1], (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
        q = truth + rng.uniform(-.02, .02, (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
        T, _ = rend.render_ids_batch_device(truth)
        rd, ri = rend.render_ids_batch_device(q)
        joints = torch.from_numpy(ref.joint_axes(q)).cuda()
        twists = torch.from_numpy(np.tile(camera_twists(DEFAULT_CAMERA_POSE)[None], (n, 1, 1))).cuda()
        H, W = intr.height, intr.width
        out = torch.empty((n, 96), dtype=torch.float64, device='cuda')
        hist = torch.empty((n, 258), dtype=torch.int32, device='cuda')
        work = torch.empty(max(lib.rope_bundle_normal_workspace(n, H, W), lib.rope_bundle_normal_workspace_robust(n, H, W)) // 8, dtype=torch.float64,
                           device='cuda')
        st = vp(torch.cuda.current_stream().cuda_stream)
        f4 = [float(v) for v in (intr.fx, intr.fy, intr.cx, intr.cy)]
        head = (vp(rd.data_ptr()), vp(ri.data_ptr()), vp(T.data_ptr()), n, H, W, ref.n_links, *f4, vp(joints.data_ptr()), 6, vp(twists.data_ptr()), 6,
                ref.clip)
        tail = (vp(out.data_ptr()), vp(work.data_ptr()), st)
        plain = lambda: lib.rope_bundle_normal_equations(*head, *tail)
        calls = {'bundle': plain}
        if old is not None:
            calls['bundle, parent'] = lambda: old.rope_bundle_normal_equations(*head, *tail)
        calls.update({'huber': lambda: lib.rope_bundle_normal_equations_robust(*head, 1, ref.clip / 4, *tail),
                      'tukey': lambda: lib.rope_bundle_normal_equations_robust(*head, 2, ref.clip / 4, *tail),
                      'histogram': lambda: lib.rope_residual_histogram(*head[:7], ref.clip, vp(hist.data_ptr()), st),
                      'bundle again': plain})
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
                elif rep == 0 and k != 'histogram':
                    words[k] = out.cpu().numpy().copy()
        h = hist.cpu().numpy().view(np.uint32)
        assert (h.sum(axis=1) == H * W).all() and np.array_equal(h[:, :257].sum(axis=1), words['bundle'][:, 0])
        if old is not None:
            assert words['bundle, parent'].tobytes() == words['bundle'].tobytes() == words['bundle again'].tobytes()
        print(f"  {W}x{H} x {n} frames: a frame has {words['bundle'][:, 0].mean():.0f} BOTH pixels and {words['bundle'][:, 2].mean():.0f} inliers on "
              f"average ({words['huber'][:, 2].mean():.0f} Huber's, {words['tukey'][:, 2].mean():.0f} Tukey's); {h[:, :256].sum() / n:.0f} residuals "
              f"within clip, {h[:, 256].sum() / n:.0f} beyond"
              + ("; the parent's words are this build's, byte for byte" if old is not None else ''))
        for k, t in times.items():
            t = np.array(t)
            print(f"  {W}x{H} x {n} frames {k:15}: {np.median(t):10.2f} ({t.min():.2f} .. {t.max():.2f})  = {np.median(t) / n:8.3f} us a frame", flush=True)
        rend.engine.close()


def recovery():
    import torch
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
    T_t, ti = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (10, 1, 1)))
    clean, drawn = T_t.cpu().numpy(), ti.cpu().numpy() < 6
    T = clean.copy()
    yy, xx = np.mgrid[0:T.shape[1], 0:T.shape[2]]
    share = []
    for f in range(10):                                 # a disc about the centroid of the drawn pixels that holds a seventh of them
        cy, cx = yy[drawn[f]].mean(), xx[drawn[f]].mean()
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        patch = drawn[f] & (d2 <= np.sort(d2[drawn[f]])[drawn[f].sum() // 7])
        T[f][patch] -= np.float32(OCCLUDER)
        share.append(patch.sum() / drawn[f].sum())
    near = true_pose + np.array([.001, -.001, .001, .002, -.002, .002])
    start = truth + rng.choice([-.0075, .0075], (10, 6)) * slu
    fmt = lambda v: ' '.join(f"{x:.2e}" for x in v)
    ang = lambda q: np.abs(q - truth)[:, :3].mean()
    print(f"10 synthetic frames 1280x720 / 8 (160x90), tools/bench_bundle_refine.py's: the camera starts one lattice step off (1 mm, 2 mrad), S, L, U "
          f"of every frame one Descent step (0.0075 rad) off; 'frame' mode, 5 rounds; an occluder {OCCLUDER * 1e3:.0f} mm in front of the surface on "
          f"{np.mean(share):.3f} of a frame's drawn pixels (clip 31 mm); |pose - true| x y z (m) a3 a4 a5 (rad), mean |angle - true| over S, L, U (rad)")
    print(f"  start:                     pose {fmt(np.abs(near - true_pose))}  angles {ang(start):.3e}")
    for frames, label in ((clean, 'clean frames'), (T, 'with the occluder')):
        for name, kw in (('plain', {}), ('Huber', dict(robust='huber')), ('Tukey', dict(robust='tukey'))):
            b = BundleRefiner(rend, intr, joints='frame', **kw).refine(near, start, torch.from_numpy(frames).cuda())
            print(f"  {label}, {name:5}: pose {fmt(np.abs(b.pose - true_pose))}  angles {ang(b.angles):.3e}  ({b.steps_taken} steps, cost "
                  f"{b.cost_before:.3e} -> {b.cost_after:.3e} m^2, {int(b.inliers)} inliers, scale {b.robust_scale * 1e3:.3f} mm)", flush=True)
    e.close()


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    if mode == 'kernels':
        kernels(sys.argv[sys.argv.index('--parent') + 1] if '--parent' in sys.argv else None)
    else:
        recovery()
