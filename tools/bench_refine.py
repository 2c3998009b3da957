#!/usr/bin/env python3
"""What the pose refinement costs and what it buys (csrc/rope_refine.hip, prediction/refinement.py) -> profiles/refine.txt.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_refine.py kernels
    python tools/bench_refine.py trace DIR          # the trace of that run, per shape (no GPU)
    python tools/bench_refine.py predictor          # run_many with and without refine, host clock, and the refiner's host share
    python tools/bench_refine.py mae                # synth.py -num 512 -batch 512 with and without -refine, without and with -noise

`kernels` calls rope_pose_normal_equations 20 times per shape on renders of random poses: 160x90 and 640x480, 1 and 512 frames.
A shape is told from the others in the trace by the grid of neq_partial_kernel (frames x ceil(H W / 2048) workgroups of 256)."""
import csv
import glob
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

SHAPES = [('1280_720_color', 8, 1), ('1280_720_color', 8, 512), ('640_480_color', 1, 1), ('640_480_color', 1, 512)]
CALLS = 20


def kernels():
    import torch
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import PoseRefiner
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
        for _ in range(CALLS):
            ref.engine.pose_normal_equations(rd, ri, T, joints, ref.n_links, ref.clip, (intr.fx, intr.fy, intr.cx, intr.cy))
        torch.cuda.synchronize()
        print(f"{intr.width}x{intr.height} x {n}: {CALLS} calls, grid {n * -(-intr.width * intr.height // 2048)} workgroups", flush=True)
        rend.engine.close()


def trace(folder):
    files = sorted(glob.glob(os.path.join(folder, '**', '*_kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(files[-1])), key=lambda r: int(r['Start_Timestamp']))
    from rope_s3d_amd.projection import Intrinsics
    print(f"rope_pose_normal_equations, kernel time from rocprofv3 --kernel-trace ({os.path.basename(files[-1])}), {CALLS} calls a shape, "
          "median (min .. max) of a call, microseconds")
    for preset, ds, n in SHAPES:
        intr = Intrinsics(preset)
        intr.downscale(ds)
        groups = n * -(-intr.width * intr.height // 2048)
        part, gat = [], []
        for i, r in enumerate(rows):                # a call is a partial launch and the gather launch that follows it
            if 'neq_partial_kernel' in r['Kernel_Name'] and int(r['Grid_Size_X']) // int(r['Workgroup_Size_X']) == groups:
                part.append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                nxt = next((g for g in rows[i + 1:i + 4] if 'neq_gather_kernel' in g['Kernel_Name']), None)
                if nxt is not None:
                    gat.append((int(nxt['End_Timestamp']) - int(nxt['Start_Timestamp'])) / 1e3)
        if not part:
            print(f"  {intr.width}x{intr.height} x {n}: no launch with {groups} workgroups in the trace")
            continue
        p, g = np.array(part[-CALLS:]), np.array(gat[-CALLS:]) if gat else np.zeros(1)
        print(f"  {intr.width}x{intr.height} x {n:3d} frames: partial {np.median(p):9.2f} ({p.min():.2f} .. {p.max():.2f})  gather {np.median(g):6.2f} "
              f"({g.min():.2f} .. {g.max():.2f})  = {(np.median(p) + np.median(g)) / n:8.3f} us a frame ({len(p)} launches)")


def _frames(n, seed, noise):
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.synthetic import SyntheticPredictor
    return SyntheticPredictor(DEFAULT_CAMERA_POSE, '1280_720_color', 8, 'SLU', noise=noise, seed=seed)


def predictor():
    """run_many on 512 frames of 1280x720 at ds_factor 8 (160x90 working resolution), frames given as host arrays: wall time of
    three runs each with refine off and on; then PoseRefiner.refine alone on the same frames with its host parts timed."""
    from rope_s3d_amd import Predictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    sp = _frames(512, 7, False)
    lim = sp.urdf_reader.joint_limits
    rng = np.random.default_rng(7)
    poses = rng.uniform(lim[:, 0], lim[:, 1], (512, 6)) * np.array([1, 1, 1, 0, 0, 0])
    colors, depths = sp.renderer.render_batch(poses)
    colors, depths = list(colors), list(depths)
    out = {}
    for refine in (False, True):
        p = sp.predictor if not refine else Predictor(DEFAULT_CAMERA_POSE, 8, base_intrin='1280_720_color', color_dict=sp.renderer.color_dict, refine=True)
        p.run_many(colors[:32], depths[:32], batch=32)
        times = []
        for _ in range(3):
            t = time.perf_counter()
            ang = p.run_many(colors, depths, batch=512)
            times.append(time.perf_counter() - t)
        out[refine] = (min(times), ang, p)
        print(f"run_many, 512 frames 1280x720 / 8, batch 512, refine={refine}: {['%.3f' % x for x in times]} s, best {min(times) * 1e3 / 512:.3f} ms a frame", flush=True)
    off, on = out[False][0], out[True][0]
    print(f"refine=True adds {(on - off) * 1e3:.1f} ms to a batch of 512 ({(on - off) / off * 100:.1f} % of the unrefined run, {(on - off) / on * 100:.1f} % of the refined one)")
    p = out[True][2]
    ref, res = p._refiner, p.last_refinement
    import torch
    T = torch.zeros((512, p.intrinsics.height, p.intrinsics.width), dtype=torch.float32, device='cuda')
    parts = {}
    orig_axes, orig_eq = ref.joint_axes, ref.engine.pose_normal_equations
    orig_render = ref._render

    def timed(name, fn):
        def wrapped(*a, **k):
            t = time.perf_counter()
            r = fn(*a, **k)
            parts[name] = parts.get(name, 0.0) + time.perf_counter() - t
            return r
        return wrapped
    ref.joint_axes, ref._render = timed('joint axes (host FK)', orig_axes), timed('render', orig_render)
    ref.engine.pose_normal_equations = timed('kernel call + download', orig_eq)
    t = time.perf_counter()
    ref.refine(out[False][1], T + 1.0)
    total = time.perf_counter() - t
    ref.joint_axes, ref._render, ref.engine.pose_normal_equations = orig_axes, orig_render, orig_eq
    rest = total - sum(parts.values())
    print(f"PoseRefiner.refine alone, 512 frames, {ref.iterations + 1} rounds: {total * 1e3:.1f} ms = " +
          ', '.join(f"{k} {v * 1e3:.1f}" for k, v in parts.items()) + f", per-frame solves and the rest of the host loop {rest * 1e3:.1f}")
    print(f"accepted steps per frame in the run above: mean {res.steps_taken.mean():.2f}")


def mae():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.synthetic import SyntheticPredictor
    print("synth.py -num 512 -batch 512 (1280_720_color, ds_factor 8, SLU; the same 512 poses in every row), |predicted - actual| in rad")
    for noise in (False, True):
        for refine in (False, True):
            sp = SyntheticPredictor(DEFAULT_CAMERA_POSE, '1280_720_color', 8, 'SLU', noise=noise, seed=7, refine=refine)
            sp.run_batch(16, os.path.join(os.environ.get('TMPDIR', '/tmp'), 'bench_refine_warm'), batch=16)
            sp.rng = np.random.default_rng(7)
            t = time.perf_counter()
            res = sp.run_batch(512, os.path.join(os.environ.get('TMPDIR', '/tmp'), 'bench_refine_mae'), batch=512)
            dt = time.perf_counter() - t
            err = np.abs(res[1] - res[0])[:, :3]
            line = (f"  noise {str(noise):5} refine {str(refine):5}: MAE S L U {err.mean(axis=0)[0]:.6f} {err.mean(axis=0)[1]:.6f} {err.mean(axis=0)[2]:.6f}  "
                    f"median {np.median(err, axis=0)[0]:.6f} {np.median(err, axis=0)[1]:.6f} {np.median(err, axis=0)[2]:.6f}  "
                    f"max {err.max(axis=0)[0]:.4f} {err.max(axis=0)[1]:.4f} {err.max(axis=0)[2]:.4f}  {dt:.3f} s")
            if refine:
                r = sp.predictor.last_refinement
                fin = np.isfinite(r.sigma[:, :3])
                line += (f"\n      accepted steps mean {r.steps_taken.mean():.2f}, frames with none {int((r.steps_taken == 0).sum())}; "
                         f"median formal sigma S L U {np.median(r.sigma[:, 0]):.2e} {np.median(r.sigma[:, 1]):.2e} {np.median(r.sigma[:, 2]):.2e}, "
                         f"inf on {int((~fin).sum())} of {fin.size}")
            print(line, flush=True)
            sp.renderer.engine.close()
            sp.predictor.engine.close()


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    {'kernels': kernels, 'predictor': predictor, 'mae': mae}.get(mode, lambda: trace(sys.argv[2]))()
