#!/usr/bin/env python3
"""Frames/s of a synthetic run (synth.py's defaults: 1280x720 renders, ds_factor 8, 'SLU'), batched on the GPU against the per-frame
loop, with and without depth holes.

Every figure is a host clock around work that ends in a device synchronise (results on the host).  The batched runs are timed
over --num frames after a warm-up run of one group; the loop, the code path of a run without -batch, over --loop-frames frames
(and --loop-noise-frames with holes, where NoiseMaker.holes takes seconds a frame) and SCALED to --num: the scaled lines say so.
The parts of the batched path are timed in a pass of their own with a synchronise after each part, so their sum is an upper
bound of the run's time per frame, not a breakdown of it.

bench.py's headline does not pass through any of this; that it did not move is shown by running it on a checkout of the parent
commit and on this build in the same session, each into a file, and handing both to --headline, which quotes them at the end:

    python bench.py --gpus 1 --steps 20 --warmup 3 > this.json          (and the same in the parent's checkout > parent.json)
    python tools/bench_synth.py --headline parent=parent.json --headline 'this build=this.json' --out profiles/synth_batch.txt"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def parts(sp, poses, seed, sub):
    """ms per frame of each part of the batched path, each followed by a device synchronise."""
    import torch
    from rope_s3d_amd.constants import LOOKUP_NUM_RENDERED
    p, r = sp.predictor, sp.renderer
    blue_of_id, link_blue = r.blue_of_id, [int(p.color_dict[k][0]) for k in p.link_names]
    p._setStages()
    n = len(poses)
    t = {'render': 0.0, 'holes': 0.0, 'targets': 0.0, 'stages': 0.0}

    def clock(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t[key] += time.perf_counter() - t0
        return out
    for j0 in range(0, n, sub):
        j1 = min(j0 + sub, n)
        depth_t, ids_t = clock('render', lambda: r.render_ids_batch_device(poses[j0:j1]))
        clock('holes', lambda: r.engine.depth_holes(depth_t, seed, frame0=j0))
        clock('targets', lambda: p.engine.stage_targets_synthetic(depth_t, ids_t, int(p.ds_factor), blue_of_id, link_blue, LOOKUP_NUM_RENDERED,
                                                                  n, j0, p._has_tsweep()))
    clock('targets', p.engine.commit_targets)
    clock('stages', lambda: p._run_resident(n))
    return {k: 1e3 * v / n for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--num', type=int, default=2500)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--loop-frames', type=int, default=250)
    ap.add_argument('--loop-noise-frames', type=int, default=2)
    ap.add_argument('--intrinsics', default='1280_720_color')
    ap.add_argument('--ds-factor', type=int, default=8)
    ap.add_argument('--headline', action='append', default=[], metavar='LABEL=FILE',
                    help="quote bench.py's result line kept in FILE (the last line of it that is JSON) under LABEL; may be repeated")
    ap.add_argument('--out', default=None, help="also write the lines to this file")
    a = ap.parse_args()

    from rope_s3d_amd import engine as eng
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.synthetic import SyntheticPredictor
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sp = SyntheticPredictor(DEFAULT_CAMERA_POSE, a.intrinsics, a.ds_factor, 'SLU', noise=False, seed=0)
    if not sp._batched_ok():
        raise SystemExit("the batched path does not take this configuration")
    poses = np.array([sp._generatePose() for _ in range(a.num)])
    say(f"synthetic run, {a.intrinsics} / {a.ds_factor}, 'SLU', {a.num} poses, groups of {a.batch}, library {eng.build_id()}")
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, 'bench_synth')
        rates = {}
        for noise in (False, True):
            sp.do_noise = noise
            sp.run_batch_poses(list(poses[:a.batch]), f, batch=a.batch)                     # warm-up: one group of the timed size
            dt, res = timed(lambda: sp.run_batch_poses(list(poses), f, batch=a.batch))
            rates[noise] = a.num / dt
            err = np.abs(res[1] - res[0])[:, :3]
            say(f"batched{' -noise' if noise else '       '}: {a.num} frames in {dt:8.2f} s = {a.num / dt:9.1f} frames/s"
                f"   (median |error| S L U: {np.median(err, 0).round(5).tolist()} rad)")
        sp.do_noise = False
        sp.run_batch_poses(list(poses[:3]), f)
        k = min(a.loop_frames, a.num)
        dt, _ = timed(lambda: sp.run_batch_poses(list(poses[:k]), f))
        say(f"loop          : {k} frames in {dt:8.2f} s = {k / dt:9.1f} frames/s   SCALED to {a.num}: {dt * a.num / k:.1f} s;  batched is {rates[False] * dt / k:.1f}x")
        sp.do_noise = True
        k = min(a.loop_noise_frames, a.num)
        dt, _ = timed(lambda: sp.run_batch_poses(list(poses[:k]), f))
        say(f"loop -noise   : {k} frames in {dt:8.2f} s = {k / dt:9.3f} frames/s   SCALED to {a.num}: {dt * a.num / k / 60:.1f} min;  batched is {rates[True] * dt / k:.0f}x")
        n = min(a.batch, a.num)
        ms = parts(sp, poses[:n], 12345, sp.SUB_BATCH)
        say(f"parts of the batched -noise path over one group of {n}, a synchronise after each, ms/frame: " +
            ', '.join(f"{key} {v:.3f}" for key, v in ms.items()))
    for item in a.headline:
        label, _, path = item.partition('=')
        with open(path) as fh:
            r = [json.loads(ln) for ln in fh if ln.lstrip().startswith('{')][-1]
        say(f"bench.py headline, {label}: {r['value']:.0f} {r.get('unit', '')} (library {r.get('roofline', {}).get('build_id', '?')})")
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
