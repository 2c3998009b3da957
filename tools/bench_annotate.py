#!/usr/bin/env python3
"""Frames/s of AutomaticAnnotator.run on synthetic sets, and of the host-only path on the same frames.

    python tools/bench_annotate.py [--frames 256 1024] [--sizes 640_480_color 1280_720_color] [--out DIR]

Per (size, frames): the whole run() (device masks, tracing and writing overlapped, then the split), then its parts one at a
time: render + masks (rope_render_masks in the annotator's chunks), tracing (rope_trace_contours on the thread pool), and
PNG + JSON writing (the PNG encoder alone beside it).  The host-only path renders colours (Renderer.render_batch) and runs
Annotator.annotate on the same thread pool.  Both paths' files are compared byte for byte before a rate is printed.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
from rope_s3d_amd.data import annotation as ann
from rope_s3d_amd.simulation.render import DatasetRenderer
from rope_s3d_amd.utils import cpu_budget


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def one(preset: str, n: int, root: str, threads: int) -> dict:
    name = f'synthetic:{n}:7919:{preset}'
    rend = DatasetRenderer(name)
    dest = os.path.join(root, 'device')
    auto = ann.AutomaticAnnotator(name, rend, preview=False, dest_path=dest)
    auto.run()                                                  # warm-up: allocations, first launches, page cache
    t_run, _ = timed(auto.run)
    labels, C, pad = list(auto.anno.color_dict), auto.CHUNK, auto.PAD_SIZE
    angles, poses = rend._ds_angles, rend._ds_poses
    og = np.concatenate([np.asarray(rend.ds.og_img[a:a + C]) for a in range(0, n, C)])
    t_masks, chunks = timed(lambda: [rend.render_masks_batch(angles[a:a + C], poses[a:a + C], pad) for a in range(0, n, C)])
    masks = np.concatenate([m for m, _ in chunks])
    boxes = np.concatenate([b for _, b in chunks])
    scratch = os.path.join(root, 'parts')
    os.makedirs(scratch, exist_ok=True)
    with ThreadPoolExecutor(threads) as pool:
        t_trace, shapes = timed(lambda: list(pool.map(lambda f: ann.label_shapes(masks[f], labels, boxes[f]), range(n))))
        t_png, _ = timed(lambda: list(pool.map(lambda f: ann.encode_png(og[f]), range(n))))
        t_write, _ = timed(lambda: list(pool.map(lambda f: ann.write_annotation(og[f], shapes[f], os.path.join(scratch, f'{f:05d}')),
                                                 range(n))))
        # host-only path: colour renders, then the reference's per-frame annotate, to the same path strings
        host = os.path.join(root, 'host')
        shutil.rmtree(host, ignore_errors=True)
        os.makedirs(host)
        a = ann.Annotator(pad_size=pad, color_dict=auto.anno.color_dict)

        def host_path():
            jobs = []
            for s in range(0, n, C):
                colours, _ = rend.render_batch(angles[s:s + C], poses[s:s + C])
                jobs += [pool.submit(a.annotate, og[f], colours[f - s], os.path.join(dest, f'{f:05d}')) for f in range(s, min(n, s + C))]
            for j in jobs:
                j.result()
        t_host, _ = timed(host_path)
    # compare: the host path wrote dest/xxxxx.{json,png} beside the split folders the device run moved its files into
    where = {f: sub for sub in ('train', 'test', 'ignore') for f in os.listdir(os.path.join(dest, sub))}
    for f in range(n):
        for ext in ('.json', '.png'):
            mine = open(os.path.join(dest, f'{f:05d}{ext}'), 'rb').read()
            if mine != open(os.path.join(dest, where[f'{f:05d}{ext}'], f'{f:05d}{ext}'), 'rb').read():
                raise SystemExit(f"{preset} x {n}: frame {f} {ext} differs between the device and the host path")
    rend.close()
    H, W = masks.shape[1:]
    return {'size': f'{W}x{H}', 'frames': n, 'threads': threads, 'run_fps': n / t_run, 'host_path_fps': n / t_host,
            'parts_s': {'render_masks': t_masks, 'trace': t_trace, 'png_json_write': t_write, 'png_encode_alone': t_png},
            'run_s': t_run, 'host_path_s': t_host, 'shapes_per_frame': sum(len(s) for s in shapes) / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--sizes', nargs='+', default=['640_480_color', '1280_720_color'])
    ap.add_argument('--out', default=None, help="scratch folder (default: a temporary one, removed)")
    args = ap.parse_args()
    threads = max(1, cpu_budget() - 1)
    for preset in args.sizes:
        for n in args.frames:
            root = args.out or tempfile.mkdtemp(prefix='bench_annotate_')
            try:
                r = one(preset, n, os.path.join(root, f'{preset}_{n}'), threads)
            finally:
                if args.out is None:
                    shutil.rmtree(root, ignore_errors=True)
            p = r['parts_s']
            print(f"{r['size']:>9} x {n:5d}: run {r['run_fps']:7.1f} frames/s | host path {r['host_path_fps']:7.1f} frames/s | "
                  f"parts (s): render+masks {p['render_masks']:.3f}, trace {p['trace']:.3f}, png+json {p['png_json_write']:.3f} "
                  f"(png alone {p['png_encode_alone']:.3f}) | {r['shapes_per_frame']:.1f} shapes/frame", flush=True)
            print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
