#!/usr/bin/env python3
"""What the camera-pose polish costs and what it buys (csrc/rope_refine.hip, prediction/refinement.py: CameraPoseRefiner)
-> profiles/camera_refine.txt.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_camera_refine.py kernels
    python tools/bench_camera_refine.py trace DIR       # the trace of that run, per shape and kernel (no GPU)
    python tools/bench_camera_refine.py predictor       # both camera predictors on tools/bench_camera.py's end-to-end scene

`kernels` calls rope_camera_normal_equations and rope_pose_normal_equations in turn, 20 times each per shape, on the same planes:
renders of random poses at 160x90 and 640x480, 10 and 512 frames.  The two partial kernels are the instantiations <true> and
<false> of neq_partial_kernel; a shape is told from the others by the grid (frames x ceil(H W / 2048) workgroups of 256).
`predictor`: 10 synthetic frames of 1280x720 at ds_factor 8, the true pose and the start of bench_camera.py; the pose error per
parameter after the stages and after the polish, the pooled formal sigmas, and the time the polish adds (host clock, the run ends
in a device synchronise: the words are downloaded); then the same frames polished from one lattice step (1 mm, 2 mrad) off the
truth, the regime the polish is for."""
import csv
import glob
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

SHAPES = [('1280_720_color', 8, 10), ('1280_720_color', 8, 512), ('640_480_color', 1, 10), ('640_480_color', 1, 512)]
CALLS = 20
KINDS = (('camera', ('neq_partial_kernel<true>', 'neq_partial_kernelILb1E')), ('pose', ('neq_partial_kernel<false>', 'neq_partial_kernelILb0E')))


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
        for _ in range(CALLS):                          # in turn: what drifts over the session drifts for both
            ref.engine.camera_normal_equations(rd, ri, T, twists, ref.n_links, ref.clip, intr4)
            ref.engine.pose_normal_equations(rd, ri, T, joints, ref.n_links, ref.clip, intr4)
        torch.cuda.synchronize()
        print(f"{intr.width}x{intr.height} x {n}: {CALLS} calls each, grid {n * -(-intr.width * intr.height // 2048)} workgroups", flush=True)
        rend.engine.close()


def trace(folder):
    files = sorted(glob.glob(os.path.join(folder, '**', '*_kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(files[-1])), key=lambda r: int(r['Start_Timestamp']))
    from rope_s3d_amd.projection import Intrinsics
    print(f"rope_camera_normal_equations beside rope_pose_normal_equations, kernel time from rocprofv3 --kernel-trace "
          f"({os.path.basename(files[-1])}), {CALLS} calls each a shape, taken in turn; median (min .. max) of a call, microseconds")
    for preset, ds, n in SHAPES:
        intr = Intrinsics(preset)
        intr.downscale(ds)
        groups = n * -(-intr.width * intr.height // 2048)
        for kind, names in KINDS:
            part, gat = [], []
            for i, r in enumerate(rows):                # a call is a partial launch and the gather launch that follows it
                if any(s in r['Kernel_Name'] for s in names) and int(r['Grid_Size_X']) // int(r['Workgroup_Size_X']) == groups:
                    part.append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                    nxt = next((g for g in rows[i + 1:i + 4] if 'neq_gather_kernel' in g['Kernel_Name']), None)
                    if nxt is not None:
                        gat.append((int(nxt['End_Timestamp']) - int(nxt['Start_Timestamp'])) / 1e3)
            if not part:
                print(f"  {intr.width}x{intr.height} x {n} {kind}: no launch with {groups} workgroups in the trace")
                continue
            p, g = np.array(part[-CALLS:]), np.array(gat[-CALLS:]) if gat else np.zeros(1)
            print(f"  {intr.width}x{intr.height} x {n:3d} frames {kind:6}: partial {np.median(p):9.2f} ({p.min():.2f} .. {p.max():.2f})  gather "
                  f"{np.median(g):6.2f} ({g.min():.2f} .. {g.max():.2f})  = {(np.median(p) + np.median(g)) / n:8.3f} us a frame ({len(p)} launches)")


def predictor():
    from rope_s3d_amd import CameraPredictor, ModellessCameraPredictor, Renderer
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.segmentation import ColorSegmenter
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])        # bench_camera.py's scene
    rb = Renderer('seg', DEFAULT_CAMERA_POSE, '1280_720_color')
    rng = np.random.default_rng(4242)
    lim = rb.robot.joint_limits
    qs = rng.uniform(lim[:, 0], lim[:, 1], (10, 6)) * np.array([1, 1, 1, 0, 0, 0])
    rb.setCameraPose(true_pose)
    cs, ds = [], []
    for q in qs:
        rb.setJointAngles(q)
        d, i = rb.render_ids()
        cs.append(rb._lut[i]); ds.append(d.astype(np.float64))
    cs, ds = np.stack(cs), np.stack(ds)
    start = np.array(DEFAULT_CAMERA_POSE, float)
    names = ['BG'] + rb.robot.link_names[:6]
    print("10 synthetic frames 1280x720 / 8 (160x90), true pose = default + (.06 -.05 .04 .01 -.015 .02), start = default; "
          "|pose - true| per parameter x y z (m) a3 a4 a5 (rad)")
    fmt = lambda v: ' '.join(f"{x:.2e}" for x in v)
    for name, mk in (('modelless', lambda **kw: ModellessCameraPredictor(start, 8, **kw)),
                     ('segmented', lambda **kw: CameraPredictor(start, 8, segmenter=ColorSegmenter(names), **kw))):
        times = {}
        for refine in (False, True):
            p = mk(refine=refine)
            p.run(cs, ds, qs)                           # warm-up (buffers, first launches)
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = p.run(cs, ds, qs)
                runs.append(time.perf_counter() - t0)
            times[refine] = (runs, got, p)
        off, on = times[False], times[True]
        res = on[2].last_refinement
        t0 = time.perf_counter()
        for _ in range(5):
            on[2]._polish(off[1].copy())
        polish = (time.perf_counter() - t0) / 5
        print(f"  {name}: after the stages  {fmt(np.abs(off[1] - true_pose))}")
        print(f"  {name}: after the polish  {fmt(np.abs(on[1] - true_pose))}   ({res.steps_taken} steps accepted, cost {res.cost_before:.3e} -> "
              f"{res.cost_after:.3e} m^2, {int(res.inliers)} inliers)")
        print(f"  {name}: pooled formal sigma {fmt(res.sigma)}")
        print(f"  {name}: frame cost {fmt(res.frame_cost)}")
        print(f"  {name}: run without polish {['%.3f' % x for x in off[0]]} s, with {['%.3f' % x for x in on[0]]} s; the polish alone "
              f"({on[2]._refiner.iterations + 1} renders and kernel calls of 10 frames, host solves) {polish * 1e3:.2f} ms, mean of 5", flush=True)
        # the regime the polish is for: a search that ended one lattice step (1 mm, 2 mrad) from the truth on every parameter
        near = true_pose + np.array([.001, -.001, .001, .002, -.002, .002])
        res = on[2]._refiner.refine(near, qs, np.asarray(on[2]._tgt_depths, np.float32))
        print(f"  {name}: from one lattice step off the truth {fmt(np.abs(near - true_pose))}")
        print(f"  {name}:   after the polish  {fmt(np.abs(res.pose - true_pose))}   ({res.steps_taken} steps accepted, cost {res.cost_before:.3e} -> "
              f"{res.cost_after:.3e} m^2, {int(res.inliers)} inliers)")
        print(f"  {name}:   pooled formal sigma {fmt(res.sigma)}", flush=True)
        for r in (off, on):
            r[2].engine.close()


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    {'kernels': kernels, 'predictor': predictor}.get(mode, lambda: trace(sys.argv[2]))()
