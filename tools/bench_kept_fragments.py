#!/usr/bin/env python3
"""What keeping a fixed grid's drawn fragments from pass to pass is worth, against the PARENT commit's build, in one session on one box.

    python tools/bench_kept_fragments.py --parent <checkout of the parent commit, its library built> [--runs 3] [--trace]

Writes profiles/kept_fragments.txt:
  * bench.py --steps 20 --warmup 3 (and with --loss full, --workload cfg5), parent and this build alternating, each run a fresh
    process, every run listed; the parent's max - min is the run-to-run spread the medians are held against;
  * this build under ROPE_STRATEGY=128 (NO_KEPT_FRAGMENTS), the same way;
  * profile_eval's intervals on this build: steady passes with the store on and off, and the one pass that builds it;
  * the store's bytes, groups and (row, tile) pairs for cfg1 and cfg5, what the default budget makes of them, and what the first hit
    of a grid over the budget costs;
  * bench.py --dump-outputs of both builds, compared file for file;
  * rope_eval of the same 4096-row grid against changing targets, host clock per call, parent and this build;
  * with --trace: rocprofv3 --kernel-trace --stats (no counters) of the bench command on both builds, the launches per kernel.
Every child process runs under a time limit, and the tool stops at the first that fails.
"""
import argparse
import csv
import filecmp
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
WORKLOADS = (('cfg1 depth', []), ('cfg1 full', ['--loss', 'full']), ('cfg5', ['--workload', 'cfg5']))
TRACE_ARGS = ['--steps', '5', '--warmup', '1', '--no-cpu-baseline', '--no-unshared', '--no-end-to-end']

HOST_LOOP = r'''
import json, sys, time
import numpy as np
sys.path.insert(0, '.')
from bench import slu_grid
from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR
from rope_s3d_amd.projection import Intrinsics, camera_matrix
from rope_s3d_amd.robot import RobotModel
robot = RobotModel.from_urdf()
intr = Intrinsics('640_480_color')
e = eng.Engine(0)
e.set_robot(robot)
e.set_camera(camera_matrix(DEFAULT_CAMERA_POSE, intr, ZNEAR, ZFAR), intr.width, intr.height, ZNEAR, ZFAR)
rng = np.random.default_rng(7919)
targets = []
for _ in range(4):
    q = rng.uniform(robot.joint_limits[:, 0], robot.joint_limits[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
    depth, _ = e.render(q, 6)
    targets.append(eng.pack_target(depth.astype(np.float64), None))
cand = slu_grid(robot.joint_limits, 16)
flags = np.zeros(8, np.uint8)
out = {}
for k in range(5 + int(sys.argv[1])):
    e.set_target(targets[k % 4], None, flags)
    t0 = time.perf_counter()
    e.eval(cand, 6, eng.LOSS_DEPTH)
    out.setdefault('ms', []).append(1e3 * (time.perf_counter() - t0))
out['ms'] = out['ms'][5:]
if hasattr(e, 'geometry_cache_stats'):
    out['hits'], out['misses'] = e.geometry_cache_stats()
if hasattr(e, 'fragment_store_stats'):
    out['builds'], out['served'] = e.fragment_store_stats()[:2]
print('HOSTLOOP ' + json.dumps(out))
'''

INTERVALS = r'''
import json, sys
import numpy as np
sys.path.insert(0, '.')
from bench import slu_grid
from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR
from rope_s3d_amd.projection import Intrinsics, camera_matrix
from rope_s3d_amd.robot import RobotModel
import os
from rope_s3d_amd.urdf import URDFReader
cfg5 = sys.argv[1] == 'cfg5'
if cfg5:
    robot = RobotModel.from_urdf(URDFReader(os.path.join('urdfs', 'motoman_mh50_support', 'urdf', 'mh50.urdf')))
    intr, pose, div = Intrinsics('1280_720_color'), [0, -4.0, 1.5, 0, 0, 0], 32
else:
    robot = RobotModel.from_urdf()
    intr, pose, div = Intrinsics('640_480_color'), DEFAULT_CAMERA_POSE, 16
e = eng.Engine(0)
e.set_robot(robot)
e.set_camera(camera_matrix(pose, intr, ZNEAR, ZFAR), intr.width, intr.height, ZNEAR, ZFAR)
q = np.random.default_rng(7919).uniform(robot.joint_limits[:, 0], robot.joint_limits[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
depth, _ = e.render(q, 6)
e.set_target(eng.pack_target(depth.astype(np.float64), None), None, np.zeros(8, np.uint8))
e.upload_candidates(slu_grid(robot.joint_limits, div))
out = {}
e.set_fragment_budget(1e-3)                         # 1 KiB: the count is taken and the store declined — what a grid over the budget pays once
e.eval_resident(6, eng.LOSS_DEPTH)
e.sync()
out['declined'] = e.profile_eval(6, eng.LOSS_DEPTH, None, reps=1)          # the first hit: draws and counts, keeps nothing, scores as before
assert e.fragment_store_stats() == (0, 0, 0, 0)
e.set_strategy(0)                                   # drops the geometry: the next hit is a first hit again
e.set_fragment_budget(1 << 20)                      # a TiB: whatever the grid comes to is kept, so that it can be measured
e.eval_resident(6, eng.LOSS_DEPTH)
e.sync()
out['building'] = e.profile_eval(6, eng.LOSS_DEPTH, None, reps=1)          # the first hit: builds, then scores from the store
out['store'] = dict(zip(('builds', 'served', 'bytes', 'groups'), e.fragment_store_stats()), pairs=e.fragment_store_pairs())
out['default_budget_bytes'] = int(8192 * 2 ** 20 / 10)
for name, flag in (('kept', 0), ('off_128', 128), ('kept_again', 0), ('off_128_again', 128)):
    e.set_strategy(flag)
    for _ in range(5):
        e.eval_resident(6, eng.LOSS_DEPTH)
    e.sync()
    out[name] = e.profile_eval(6, eng.LOSS_DEPTH, None, reps=40)
print('INTERVALS ' + json.dumps(out))
'''


def run(cmd, cwd, limit, env=None):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=limit, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)} in {cwd} failed ({r.returncode}):\n{(r.stdout + r.stderr)[-3000:]}")
    return r.stdout


def bench_line(tree, extra, env=None):
    out = run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '3'] + extra, tree, 300, env)
    line = [l for l in out.splitlines() if l.startswith('{')][-1]
    return json.loads(line)


def tagged(out, tag):
    return json.loads([l for l in out.splitlines() if l.startswith(tag + ' ')][-1][len(tag) + 1:])


def trace(tree, lines, label):
    if not shutil.which('rocprofv3'):
        lines.append(f"kernel trace ({label}): no rocprofv3 on this box")
        return
    with tempfile.TemporaryDirectory() as tmp:
        run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, 'bench.py'] + TRACE_ARGS, tree, 420)
        files = glob.glob(os.path.join(tmp, '**', '*_kernel_stats.csv'), recursive=True)
        rows = list(csv.DictReader(open(files[0]))) if files else []
    lines.append(f"kernel trace ({label}): bench.py {' '.join(TRACE_ARGS)} — 1 warm-up + 5 timed passes; calls, average us, share")
    for r in rows[:12]:
        lines.append(f"  {int(r['Calls']):5d}  {float(r['AverageNs']) / 1e3:10.1f}  {float(r['Percentage']):6.2f} %  {r['Name'][:110]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kept_fragments.txt'))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    ids = {name: run([sys.executable, '-c', 'from rope_s3d_amd import engine; print(engine.build_id())'], tree, 120).split()[-1]
           for name, tree in (('parent', parent), ('this', ROOT))}
    lines = [f"Drawn fragments kept from pass to pass: parent build {ids['parent']} against this build {ids['this']}, one session, one box.",
             "bench.py --gpus 1 --steps 20 --warmup 3 [workload], fresh process per run, builds alternating; value = poses/s.",
             "The 3 warm-up passes are the miss, the first hit (which builds the store) and one served pass: the 20 timed passes are steady state.",
             "'this, store off' = this build with ROPE_STRATEGY=128 (NO_KEPT_FRAGMENTS): every hit draws the rows' own links, as the parent does.", ""]
    for label, extra in WORKLOADS:
        vals = {'parent': [], 'this': [], 'off': []}
        for _ in range(a.runs):
            for who, tree, env in (('parent', parent, None), ('this', ROOT, None), ('off', ROOT, {'ROPE_STRATEGY': '128'})):
                r = bench_line(tree, extra, env)
                vals[who].append(r['value'])
                print(f"{label} {who} {r['value']:.0f}", flush=True)
        med = {k: statistics.median(v) for k, v in vals.items()}
        spread = max(vals['parent']) - min(vals['parent'])
        lines += [f"{label}:",
                  "  parent          " + '  '.join(f"{v:12.0f}" for v in vals['parent']) + f"   median {med['parent']:.0f}   spread (max - min) {spread:.0f}",
                  "  this            " + '  '.join(f"{v:12.0f}" for v in vals['this']) + f"   median {med['this']:.0f}",
                  "  this, store off " + '  '.join(f"{v:12.0f}" for v in vals['off']) + f"   median {med['off']:.0f}",
                  f"  gain {med['this'] - med['parent']:+.0f} poses/s = {100 * (med['this'] / med['parent'] - 1):+.2f} % = {(med['this'] - med['parent']) / max(spread, 1e-9):.1f} spreads"
                  f" (wanted: at least 3);  store off against parent {med['off'] - med['parent']:+.0f} poses/s = {(med['off'] - med['parent']) / max(spread, 1e-9):+.1f} spreads"
                  " (wanted: no worse than -1)", ""]
    for wl in ('cfg1', 'cfg5'):
        iv = tagged(run([sys.executable, '-c', INTERVALS, wl], ROOT, 600), 'INTERVALS')
        st = iv.pop('store')
        budget = iv.pop('default_budget_bytes')
        lines.append(f"profile_eval intervals on this build, {wl} depth, ms per pass (declined: the first hit under a budget of 1 KiB; building: the one pass that builds the store, build recorded in 'score'; "
                     "the others: 40 steady passes, 'off_128' with ROPE_STRATEGY_NO_KEPT_FRAGMENTS):")
        for name, d in iv.items():
            lines.append(f"  {name:15s} fk {d['fk']:.4f}  layer {d['layer']:.4f}  score {d['score']:.4f}  finalize {d['finalize']:.4f}  total {d['total']:.4f}")
        lines.append(f"  building pass over a plain hit pass: {iv['building']['total'] - iv['off_128']['total']:+.3f} ms (it draws the own links twice, compacts, and waits for the stream)")
        lines.append(f"  first hit of a grid over the budget (draws and counts once, keeps nothing, then scores as before) over a plain hit pass: {iv['declined']['total'] - iv['off_128']['total']:+.3f} ms")
        lines.append(f"  store of {wl}: {st['pairs']} (row, tile) pairs with a group, {st['groups']} groups = {st['bytes']} bytes ({st['bytes'] / 2 ** 20:.1f} MiB; 36 B a group + 8 B a (row, tile) slot); "
                     f"default budget {budget} bytes: " + ("kept by default" if st['bytes'] <= budget else "NOT kept by default — such passes run as without the store"))
        lines.append("")
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for who, tree in (('parent', parent), ('this', ROOT)):
            dirs[who] = os.path.join(tmp, who)
            run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '5', '--warmup', '1', '--dump-outputs', dirs[who]], tree, 300)
        names = sorted(os.listdir(dirs['parent']))
        same = names == sorted(os.listdir(dirs['this'])) and all(filecmp.cmp(os.path.join(dirs['parent'], n), os.path.join(dirs['this'], n), shallow=False) for n in names)
        lines += [f"bench.py --dump-outputs, parent against this build: {len(names)} files ({', '.join(names)}) — " + ("identical, file for file" if same else "DIFFERENT"), ""]
    lines.append(f"rope_eval of the same 4096-row grid against changing targets (set_target not timed), host clock per call, {a.calls} calls after 5:")
    for who, tree in (('parent', parent), ('this', ROOT)):
        h = tagged(run([sys.executable, '-c', HOST_LOOP, str(a.calls)], tree, 300), 'HOSTLOOP')
        m = sorted(h['ms'])
        lines.append(f"  {who:7s} median {m[len(m) // 2]:.3f} ms  min {m[0]:.3f}  max {m[-1]:.3f}" + (f"   (hits {h['hits']}, misses {h['misses']})" if 'hits' in h else '') + (f" (stores built {h['builds']}, passes served {h['served']})" if 'builds' in h else ''))
    lines.append("")
    if a.trace:
        trace(parent, lines, 'parent')
        lines.append("")
        trace(ROOT, lines, 'this build')
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    if not same:
        sys.exit("outputs differ between the builds")


if __name__ == '__main__':
    main()
