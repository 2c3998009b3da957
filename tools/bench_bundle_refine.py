#!/usr/bin/env python3
"""What one solve for angles and camera costs and what it buys (csrc/rope_bundle.hip, prediction/refinement.py: BundleRefiner)
-> profiles/bundle_refine.txt.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_bundle_refine.py kernels
    python tools/bench_bundle_refine.py trace DIR       # the trace of that run, per shape and kernel (no GPU)
    python tools/bench_bundle_refine.py recovery        # ten synthetic 160x90 frames: 'frame' mode against the two-pass polish, 'offset' mode

`kernels` calls rope_bundle_normal_equations (6 joints, 6 twists), rope_camera_normal_equations and rope_pose_normal_equations in
turn, 20 times each per shape, on the same planes: renders of random poses at 160x90 and 640x480, 512 frames.  A shape is told from
the others by the grid (frames x ceil(H W / 2048) workgroups of 256).
`recovery`: the camera starts one lattice step (1 mm, 2 mrad) off and S, L, U one Descent step (0.0075 rad) off; where 'frame' mode
ends, against PoseRefiner and then CameraPoseRefiner from the same start; and for 'offset' mode a planted offset of a few mrad a
joint and what comes back."""
import csv
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

SHAPES = [('1280_720_color', 8, 512), ('640_480_color', 1, 512)]
CALLS = 20
KINDS = (('bundle', ('bneq_partial_kernel',), 'bneq_gather_kernel'), ('camera', ('neq_partial_kernel<true>', 'neq_partial_kernelILb1E'), 'neq_gather_kernel'),
         ('pose', ('neq_partial_kernel<false>', 'neq_partial_kernelILb0E'), 'neq_gather_kernel'))


def kernels():
    import torch
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import PoseRefiner, camera_twists
    from rope_s3d_amd.projection import Intrinsics
    from rope_s3d_amd.simulation.render import Renderer
    for preset, ds, n in SHAPES:
        intr = Intrinsics(preset)
        intr.downscale(ds)
        rend = Renderer('seg', DEFAULT_CAMERA_POSE, intr)
        ref = PoseRefiner(rend, DEFAULT_CAMERA_POSE, intr)
        lim = ref.limits
        rng = np.random.default_rng(5)
        truth = rng.uniform(lim[:, 0], lim[:, 1], (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
        q = truth + rng.uniform(-.02, .02, (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
        T = rend.render_ids_batch_device(truth)[0]
        rd, ri = rend.render_ids_batch_device(q)
        joints = torch.from_numpy(ref.joint_axes(q)).cuda()
        twists = torch.from_numpy(np.tile(camera_twists(DEFAULT_CAMERA_POSE)[None], (n, 1, 1))).cuda()
        intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
        for _ in range(CALLS):                          # in turn: what drifts over the session drifts for all three
            words = ref.engine.bundle_normal_equations(rd, ri, T, joints, twists, ref.n_links, ref.clip, intr4)
            ref.engine.camera_normal_equations(rd, ri, T, twists, ref.n_links, ref.clip, intr4)
            ref.engine.pose_normal_equations(rd, ri, T, joints, ref.n_links, ref.clip, intr4)
        torch.cuda.synchronize()
        print(f"{intr.width}x{intr.height} x {n}: {CALLS} calls each, grid {n * -(-intr.width * intr.height // 2048)} workgroups; a frame has "
              f"{words[:, 0].mean():.0f} BOTH pixels and {words[:, 2].mean():.0f} inliers on average", flush=True)
        rend.engine.close()


def trace(folder):
    files = sorted(glob.glob(os.path.join(folder, '**', '*_kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(files[-1])), key=lambda r: int(r['Start_Timestamp']))
    from rope_s3d_amd.projection import Intrinsics
    print(f"rope_bundle_normal_equations (6 joints + 6 twists) beside the two 6-column calls on the same planes, kernel time from rocprofv3 "
          f"--kernel-trace ({os.path.basename(files[-1])}), {CALLS} calls each a shape, taken in turn; median (min .. max) of a call, microseconds")
    for preset, ds, n in SHAPES:
        intr = Intrinsics(preset)
        intr.downscale(ds)
        groups = n * -(-intr.width * intr.height // 2048)
        total = {}
        for kind, names, gather in KINDS:
            part, gat = [], []
            for i, r in enumerate(rows):                # a call is a partial launch and the gather launch that follows it
                if any(s in r['Kernel_Name'] for s in names) and int(r['Grid_Size_X']) // int(r['Workgroup_Size_X']) == groups:
                    part.append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                    nxt = next((g for g in rows[i + 1:i + 4] if gather in g['Kernel_Name'] and ('bneq' in g['Kernel_Name']) == (kind == 'bundle')), None)
                    if nxt is not None:
                        gat.append((int(nxt['End_Timestamp']) - int(nxt['Start_Timestamp'])) / 1e3)
            if not part:
                print(f"  {intr.width}x{intr.height} x {n} {kind}: no launch with {groups} workgroups in the trace")
                continue
            p, g = np.array(part[-CALLS:]), np.array(gat[-CALLS:]) if gat else np.zeros(1)
            total[kind] = np.median(p) + np.median(g)
            print(f"  {intr.width}x{intr.height} x {n:3d} frames {kind:6}: partial {np.median(p):9.2f} ({p.min():.2f} .. {p.max():.2f})  gather "
                  f"{np.median(g):6.2f} ({g.min():.2f} .. {g.max():.2f})  = {total[kind] / n:8.3f} us a frame ({len(p)} launches)")
        if len(total) == 3:
            two = total['camera'] + total['pose']
            print(f"  {intr.width}x{intr.height} x {n:3d} frames: bundle {total['bundle'] / n:.3f} us a frame against camera + pose {two / n:.3f} "
                  f"({total['bundle'] / two:.2f} of the two)")


def recovery():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import BundleRefiner, CameraPoseRefiner, PoseRefiner
    from rope_s3d_amd.projection import camera_matrix
    from rope_s3d_amd.simulation.render import Renderer
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])
    rend = Renderer('seg', true_pose, '1280_720_color', intrinsic_ds_factor=8)
    intr, e = rend.intrinsics, rend.engine
    rng = np.random.default_rng(4242)
    lim, slu = rend.robot.joint_limits, np.array([1, 1, 1, 0, 0, 0])
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (10, 6)) * slu
    T = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (10, 1, 1)))[0]
    near = true_pose + np.array([.001, -.001, .001, .002, -.002, .002])
    start = truth + rng.choice([-.0075, .0075], (10, 6)) * slu
    fmt = lambda v: ' '.join(f"{x:.2e}" for x in v)
    ang = lambda q: np.abs(q - truth)[:, :3].mean()
    print("10 synthetic frames 1280x720 / 8 (160x90); the camera starts one lattice step off (1 mm, 2 mrad), S, L, U of every frame one Descent step "
          "(0.0075 rad) off; |pose - true| x y z (m) a3 a4 a5 (rad), mean |angle - true| over S, L, U (rad)")
    print(f"  start:                        pose {fmt(np.abs(near - true_pose))}  angles {ang(start):.3e}")
    b = BundleRefiner(rend, intr, joints='frame').refine(near, start, T)
    print(f"  bundle, 'frame' mode:         pose {fmt(np.abs(b.pose - true_pose))}  angles {ang(b.angles):.3e}  ({b.steps_taken} steps, cost "
          f"{b.cost_before:.3e} -> {b.cost_after:.3e} m^2, {int(b.inliers)} inliers)")
    print(f"    formal sigma of the pose {fmt(b.sigma_pose)}; median formal sigma of S, L, U {fmt(np.median(b.sigma_angles[:, :3], axis=0))}")
    p1 = PoseRefiner(rend, near, intr).refine(start, T)
    c1 = CameraPoseRefiner(rend, intr).refine(near, p1.angles, T)
    print(f"  PoseRefiner, then CameraPoseRefiner: pose {fmt(np.abs(c1.pose - true_pose))}  angles {ang(p1.angles):.3e}  ({int(p1.steps_taken.sum())} + "
          f"{c1.steps_taken} steps, pooled cost {c1.cost_before:.3e} -> {c1.cost_after:.3e} m^2)")
    print(f"    formal sigma of the pose, the angles taken as exact {fmt(c1.sigma)}")
    c2 = CameraPoseRefiner(rend, intr).refine(near, start, T)
    p2 = PoseRefiner(rend, c2.pose, intr).refine(start, T)
    print(f"  CameraPoseRefiner, then PoseRefiner: pose {fmt(np.abs(c2.pose - true_pose))}  angles {ang(p2.angles):.3e}  ({c2.steps_taken} + "
          f"{int(p2.steps_taken.sum())} steps)")
    planted = np.array([.004, -.003, .005, 0, 0, 0])
    o = BundleRefiner(rend, intr, joints='offset').refine(near, truth - planted, T)
    print(f"  'offset' mode, recorded angles = truth - ({fmt(planted[:3])}) rad on S, L, U:")
    print(f"    offsets back {' '.join(f'{x:+.3e}' for x in o.offsets[:3])} (formal sigma {fmt(o.sigma_offsets[:3])}); pose {fmt(np.abs(o.pose - true_pose))} "
          f"(formal sigma {fmt(o.sigma_pose)}); {o.steps_taken} steps, cost {o.cost_before:.3e} -> {o.cost_after:.3e} m^2", flush=True)
    e.close()


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    {'kernels': kernels, 'recovery': recovery}.get(mode, lambda: trace(sys.argv[2]))()
