#!/usr/bin/env python3
"""The native bundle polish beside the host loop (csrc/rope_bundle_polish.hip, prediction/refinement.py) -> profiles/bundle_native.txt.

    python tools/bench_bundle_native.py all                      # alternating fresh processes: host, native, host, native per shape
    python tools/bench_bundle_native.py one frame|offset 10|512 host|native
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_bundle_native.py one frame 512 native
    python tools/bench_bundle_native.py trace DIR                # the kernels of that run (no GPU)

BundleRefiner.refine on N frames at 1280x720 / 8 (160x90), 6 rounds (5 iterations), 'SLU' and all six camera parameters; frames =
renders of random S/L/U poses under a camera 5 mm / 4 mrad from the start, the angles up to 0.0075 rad off ('frame') or all off by
the same offsets ('offset').  One call to warm up, then three timed by the host's clock (the call is complete on return).  Every
`one` is a process of its own, so neither loop inherits the other's allocator, caches or clocks; `all` lists every run.  The host
run also times its own parts: the solves (schur_step / bundle_columns_step, the sigmas) and pool_bundle."""
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

REPEATS, PROCESSES = 3, 2
SHAPES = (('frame', 10), ('frame', 512), ('offset', 10), ('offset', 512))


def one(mode, n, how):
    import torch
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction import refinement as rf
    from rope_s3d_amd.projection import Intrinsics, camera_matrix
    from rope_s3d_amd.simulation.render import Renderer
    intr = Intrinsics('1280_720_color')
    intr.downscale(8)
    rend = Renderer('seg', DEFAULT_CAMERA_POSE, intr)
    ref = rf.BundleRefiner(rend, intr, joints=mode, native=how == 'native')
    lim = ref.limits
    rng = np.random.default_rng(5)
    slu = np.array([1, 1, 1, 0, 0, 0])
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (n, 6)) * slu
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])
    pose = true_pose + rng.uniform(-1, 1, 6) * np.array([.005, .005, .005, .004, .004, .004])
    q = truth + rng.uniform(-.0075, .0075, (n, 6)) * slu if mode == 'frame' else truth - np.array([.004, -.003, .005, 0, 0, 0])
    T = rend.engine.render_batch_device(truth, ref.n_links, np.tile(camera_matrix(true_pose, intr)[None], (n, 1, 1)))[0].clone()
    parts = {}
    if how == 'host':
        def timed(name, fn):
            def wrapped(*a, **k):
                t = time.perf_counter()
                r = fn(*a, **k)
                parts[name] = parts.get(name, 0.0) + time.perf_counter() - t
                return r
            return wrapped
        for name, key in (('schur_step', 'solve'), ('bundle_columns_step', 'solve'), ('schur_sigma', 'sigma'), ('bundle_columns_sigma', 'sigma'),
                          ('pool_bundle', 'pool')):
            setattr(rf, name, timed(key, getattr(rf, name)))
        ref.joint_axes = timed('axes', ref.joint_axes)
    ref.refine(pose, q, T)
    parts.clear()
    times = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = ref.refine(pose, q, T)
        times.append(time.perf_counter() - t)
    print(json.dumps(dict(mode=mode, n=n, how=how, ms=[round(x * 1e3, 3) for x in times], parts_ms={k: round(v * 1e3 / REPEATS, 3) for k, v in parts.items()},
                          steps=int(res.steps_taken), cost=[float(res.cost_before), float(res.cost_after)], pose_sum=float(res.pose.sum()))), flush=True)


def everything():
    """Fresh processes in turn: host, native, host, native per shape; every run listed, medians and spread at the end."""
    runs = {}
    for mode, n in SHAPES:
        for _ in range(PROCESSES):
            for how in ('host', 'native'):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), 'one', mode, str(n), how], capture_output=True, text=True, timeout=600)
                line = next((l for l in r.stdout.splitlines() if l.startswith('{')), None)
                if r.returncode != 0 or line is None:
                    print(f"{mode} {n} {how}: failed ({r.returncode})\n{r.stderr[-2000:]}")
                    return 1
                d = json.loads(line)
                runs.setdefault((mode, n, how), []).append(d)
                print(f"  {mode:6s} {n:4d} {how:6s} process {len(runs[(mode, n, how)])}: {d['ms']} ms  steps {d['steps']}  cost {d['cost']}" +
                      (f"  host parts {d['parts_ms']}" if d.get('parts_ms') else ''), flush=True)
    print()
    for mode, n in SHAPES:
        med = {}
        for how in ('host', 'native'):
            ms = np.array([x for d in runs[(mode, n, how)] for x in d['ms']])
            med[how] = float(np.median(ms))
            print(f"{mode:6s} {n:4d} {how:6s}: median {np.median(ms):8.2f} ms of {len(ms)} calls in {PROCESSES} processes (min {ms.min():.2f}, max {ms.max():.2f})")
        parts = runs[(mode, n, 'host')][-1]['parts_ms']
        print(f"{mode:6s} {n:4d}: host loop {med['host']:.2f} ms, native {med['native']:.2f} ms; the host loop's own solves, sigmas and pools: "
              f"{sum(v for k, v in parts.items() if k != 'axes'):.2f} ms a call, its joint axes {parts.get('axes', 0.0):.2f} ms")
    return 0


def trace(folder):
    files = sorted(glob.glob(os.path.join(folder, '**', '*_kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    rows = list(csv.DictReader(open(files[-1])))
    print(f"kernel time from rocprofv3 --kernel-trace ({os.path.basename(files[-1])}): launches, median (min .. max) microseconds, total ms")
    for name in ('bundle_pool_kernel', 'schur_frame_kernel', 'schur_reduce_kernel', 'schur_back_kernel', 'schur_var_frame_kernel',
                 'schur_var_reduce_kernel', 'schur_var_back_kernel', 'columns_step_kernel', 'columns_variance_kernel', 'bundle_init_kernel',
                 'bundle_verdict_kernel', 'bundle_take_kernel', 'bundle_finish_kernel', 'tile_twists_kernel', 'joint_axes_kernel', 'bneq_', 'raster_'):
        us = np.array([(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if name in r['Kernel_Name']])
        if len(us):
            print(f"  {name:26s} {len(us):5d} launches  {np.median(us):9.2f} ({us.min():.2f} .. {us.max():.2f})  total {us.sum() / 1e3:8.3f} ms")


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'all'
    if mode == 'one':
        one(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    elif mode == 'trace':
        trace(sys.argv[2])
    else:
        sys.exit(everything())
