#!/usr/bin/env python3
"""The native polish beside the host loop (csrc/rope_polish.hip, prediction/refinement.py) -> profiles/polish_native.txt.

    python tools/bench_polish.py all                 # alternating fresh processes, three each: refine alone, then run_many
    python tools/bench_polish.py one refine host|native
    python tools/bench_polish.py one run_many off|host|native
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_polish.py one refine native
    python tools/bench_polish.py trace DIR           # the kernels of that run (no GPU)

`refine`: PoseRefiner.refine alone on 512 frames at 1280x720 / 8 (160x90), 6 rounds (5 iterations), frames = renders of random
S/L/U poses with the start up to 0.02 rad off; one call to warm up, then three timed by the host's clock (the call is complete on
return).  `run_many`: tools/bench_refine.py's predictor mode, 512 frames in one batch, refine=False / True / 'native'.
Every `one` is a process of its own, so neither loop inherits the other's allocator, caches or clocks; `all` lists every run."""
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

N, REPEATS = 512, 3


def refine(mode):
    import torch
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import PoseRefiner
    from rope_s3d_amd.projection import Intrinsics
    from rope_s3d_amd.simulation.render import Renderer
    intr = Intrinsics('1280_720_color')
    intr.downscale(8)
    rend = Renderer('seg', DEFAULT_CAMERA_POSE, intr)
    ref = PoseRefiner(rend, DEFAULT_CAMERA_POSE, intr, native=mode == 'native')
    lim = ref.limits
    rng = np.random.default_rng(5)
    truth = rng.uniform(lim[:, 0], lim[:, 1], (N, 6)) * np.array([1, 1, 1, 0, 0, 0])
    q = truth + rng.uniform(-.02, .02, (N, 6)) * np.array([1, 1, 1, 0, 0, 0])
    rend.setMaxParts(None)
    T = rend.render_ids_batch_device(truth)[0]
    parts = {}
    if mode == 'host':                                      # the host loop's parts, as profiles/refine.txt splits them
        def timed(name, fn):
            def wrapped(*a, **k):
                t = time.perf_counter()
                r = fn(*a, **k)
                parts[name] = parts.get(name, 0.0) + time.perf_counter() - t
                return r
            return wrapped
        ref.joint_axes, ref._render = timed('axes', ref.joint_axes), timed('render', ref._render)
        ref.engine.pose_normal_equations = timed('equations', ref.engine.pose_normal_equations)
    ref.refine(q, T)
    parts.clear()
    times = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = ref.refine(q, T)
        times.append(time.perf_counter() - t)
    print(json.dumps(dict(what='refine', mode=mode, ms=[round(x * 1e3, 3) for x in times], parts_ms={k: round(v * 1e3 / REPEATS, 3) for k, v in parts.items()},
                          steps_mean=float(res.steps_taken.mean()), angles_sum=float(res.angles.sum()))), flush=True)


def run_many(mode):
    from rope_s3d_amd import Predictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.synthetic import SyntheticPredictor
    sp = SyntheticPredictor(DEFAULT_CAMERA_POSE, '1280_720_color', 8, 'SLU', noise=False, seed=7)
    lim = sp.urdf_reader.joint_limits
    poses = np.random.default_rng(7).uniform(lim[:, 0], lim[:, 1], (N, 6)) * np.array([1, 1, 1, 0, 0, 0])
    colors, depths = sp.renderer.render_batch(poses)
    colors, depths = list(colors), list(depths)
    flag = {'off': False, 'host': True, 'native': 'native'}[mode]
    p = sp.predictor if flag is False else Predictor(DEFAULT_CAMERA_POSE, 8, base_intrin='1280_720_color', color_dict=sp.renderer.color_dict, refine=flag)
    p.run_many(colors[:32], depths[:32], batch=32)
    times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        p.run_many(colors, depths, batch=N)
        times.append(time.perf_counter() - t)
    print(json.dumps(dict(what='run_many', mode=mode, ms=[round(x * 1e3, 3) for x in times])), flush=True)


def everything():
    """Fresh processes in turn: host, native, host, native, ...; every run listed, medians and spread at the end."""
    runs = {}
    for what, modes in (('refine', ('host', 'native')), ('run_many', ('off', 'host', 'native'))):
        for _ in range(3):
            for mode in modes:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), 'one', what, mode], capture_output=True, text=True, timeout=600)
                line = next((l for l in r.stdout.splitlines() if l.startswith('{')), None)
                if r.returncode != 0 or line is None:
                    print(f"{what} {mode}: failed ({r.returncode})\n{r.stderr[-2000:]}")
                    return 1
                d = json.loads(line)
                runs.setdefault((what, mode), []).append(d)
                print(f"  {what:8s} {mode:6s} process {len(runs[(what, mode)])}: {d['ms']} ms" + (f"  parts {d['parts_ms']}" if d.get('parts_ms') else '') +
                      (f"  steps mean {d['steps_mean']:.2f}" if 'steps_mean' in d else ''), flush=True)
    print()
    best = {}
    for (what, mode), ds in runs.items():
        ms = np.array([x for d in ds for x in d['ms']])
        best[(what, mode)] = float(np.median(ms))
        print(f"{what:8s} {mode:6s}: median {np.median(ms):8.2f} ms of {len(ms)} calls in {len(ds)} processes (min {ms.min():.2f}, max {ms.max():.2f})")
    print(f"refine alone, {N} frames, 6 rounds: host loop {best[('refine', 'host')]:.1f} ms, native {best[('refine', 'native')]:.1f} ms")
    off = best[('run_many', 'off')]
    print(f"run_many: refine=True adds {best[('run_many', 'host')] - off:.1f} ms to a batch of {N}, refine='native' adds {best[('run_many', 'native')] - off:.1f} ms")
    return 0


def trace(folder):
    files = sorted(glob.glob(os.path.join(folder, '**', '*_kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    rows = list(csv.DictReader(open(files[-1])))
    print(f"kernel time from rocprofv3 --kernel-trace ({os.path.basename(files[-1])}): launches, median (min .. max) microseconds, total ms")
    for name in ('joint_axes_kernel', 'levenberg_step_kernel', 'formal_variance_kernel', 'polish_accept_kernel', 'polish_init_kernel', 'polish_inliers_kernel',
                 'neq_partial_kernel', 'neq_gather_kernel', 'raster_'):
        us = np.array([(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if name in r['Kernel_Name']])
        if len(us):
            print(f"  {name:24s} {len(us):5d} launches  {np.median(us):9.2f} ({us.min():.2f} .. {us.max():.2f})  total {us.sum() / 1e3:8.3f} ms")


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'all'
    if mode == 'one':
        {'refine': refine, 'run_many': run_many}[sys.argv[2]](sys.argv[3])
    elif mode == 'trace':
        trace(sys.argv[2])
    else:
        sys.exit(everything())
