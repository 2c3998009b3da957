#!/usr/bin/env python3
"""Condense a tools/rocprof_bench.sh output directory into the files committed under profiles/.

    python tools/summarize_prof.py gpurun_out/prof_<tag> <tag>

Writes profiles/<tag>_kernel_stats.csv (rocprofv3 --kernel-trace --stats, verbatim),
profiles/<tag>_pmc.json (every collected counter for the scoring interval of a pass — with kept fragments the per-pass sums over the
kernels between ev[2] and ev[3] of the timed passes, see below; without, per-launch averages of the raster kernel) and
profiles/traffic.json (HBM bytes per scoring interval: FETCH_SIZE x 2 + WRITE_SIZE, in bytes — the
gfx950 correction of MI355X_MICROARCH.md §HBM: FETCH_SIZE reports half of a coalesced read stream).
"""
import collections
import csv
import glob
import json
import os
import shutil
import sys

src, tag = sys.argv[1], sys.argv[2]
root = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
sys.path.insert(0, root)
from rope_s3d_amd.build import source_hash                  # what the profiled library was built from (run this on the same tree)
BUILD_ID = source_hash()
out = os.path.join(root, 'profiles')
os.makedirs(out, exist_ok=True)

def newest(pattern):
    """gpurun merges every call's files into gpurun_out/: of several runs of the same pass only the last one counts"""
    files = sorted(glob.glob(pattern), key=os.path.getmtime)
    return files[-1:]


stats = newest(os.path.join(src, 'stats', '*', '*_kernel_stats.csv'))
if stats:
    shutil.copy(stats[0], os.path.join(out, f'{tag}_kernel_stats.csv'))
# The "scoring launch" is whatever runs between ev[2] and ev[3] of rope_profile_eval (bench.py's score_launch_ms).  With kept
# fragments that is no single kernel: the timed passes of the profiled command are one pass that builds the store (score_queue_kernel
# + raster_queue_kernel<DEPTH, LAYER> over the rows' own links, twice, fragment_count_kernel / fragment_fill_kernel, then
# fragment_score_kernel<DEPTH>) and STEPS - 1 passes that are fragment_score_kernel<DEPTH> alone.  The counters are those kernels'
# sums over the timed passes, per pass — what bench.py divides by its live per-pass time of the same interval.  The warm-up pass (the
# miss: its shared-layer launch and its one raster_queue_kernel<DEPTH, SCORE>) is left out: every dispatch up to and including that
# SCORE launch.  A build without the store (ROPE_STRATEGY=128, or an older library) has a SCORE launch per pass: then those are taken,
# per launch, as before.
STEPS = 3
INTERVAL = ('score_queue_kernel', 'raster_queue_kernel<0, 3', 'fragment_count_kernel', 'fragment_fill_kernel', 'fragment_score_kernel<0')
SCORE = ('raster_queue_kernel<0, 0', 'raster_score_kernel<0, 0')


def dispatches(path):
    rows = list(csv.DictReader(open(path)))
    if rows and 'Dispatch_Id' in rows[0]:
        rows.sort(key=lambda r: int(r['Dispatch_Id']))
    return rows


def timed_interval(rows, name_col):
    """rows of the scoring interval's kernels in the timed passes; None when every pass has a SCORE launch (no store)"""
    score_at = [i for i, r in enumerate(rows) if any(k in r[name_col] for k in SCORE)]
    if not score_at or not any('fragment_score_kernel<0' in r[name_col] for r in rows):
        return None
    first_id = rows[score_at[0]].get('Dispatch_Id')
    after = [r for i, r in enumerate(rows) if (int(r['Dispatch_Id']) > int(first_id) if first_id is not None else i > score_at[0])]
    return [r for r in after if any(k in r[name_col] for k in INTERVAL + SCORE)]


pmc = collections.defaultdict(list)
by_kernel = collections.defaultdict(lambda: collections.defaultdict(list))
per_pass = False
for d in ('pmc_sq', 'pmc_sq2', 'pmc_lanes', 'pmc_fetch', 'pmc_write'):
    for f in newest(os.path.join(src, d, '*', '*_counter_collection.csv')):
        rows = dispatches(f)
        timed = timed_interval(rows, 'Kernel_Name')
        if timed is None:
            for r in rows:
                if any(k in r['Kernel_Name'] for k in SCORE):       # <LOSS = DEPTH, MODE = SCORE>
                    pmc[r['Counter_Name']].append(float(r['Counter_Value']))
            continue
        per_pass = True
        total = collections.defaultdict(float)
        for r in timed:
            total[r['Counter_Name']] += float(r['Counter_Value'])
            for k in INTERVAL:                               # and every kernel of the interval on its own, per launch
                if k in r['Kernel_Name']:
                    by_kernel[k][r['Counter_Name']].append(float(r['Counter_Value']))
        for k, v in total.items():
            pmc[k].append(v / STEPS)
summary = {k: {'launches': len(v), 'avg_per_launch': sum(v) / len(v)} for k, v in sorted(pmc.items())}
if 'SQ_THREAD_CYCLES_VALU' in summary and 'SQ_ACTIVE_INST_VALU' in pmc:
    # both from the pmc_lanes pass: lanes active per VALU instruction cycle, of 64
    lanes = [t / a for t, a in zip(pmc['SQ_THREAD_CYCLES_VALU'][-len(pmc['SQ_ACTIVE_INST_VALU']):], pmc['SQ_ACTIVE_INST_VALU'][-len(pmc['SQ_THREAD_CYCLES_VALU']):]) if a]
    if lanes:
        summary['active_lanes'] = {'launches': len(lanes), 'avg_per_launch': sum(lanes) / len(lanes)}
# the clock during the profiled scoring interval: GRBM_GUI_ACTIVE is summed over the 8 XCDs (MI355X_MICROARCH.md, "DVFS give-back")
clock_grbm = None
kernel_ns = {}
if stats and 'GRBM_GUI_ACTIVE' in summary:
    traces = newest(os.path.join(src, 'stats', '*', '*_kernel_trace.csv'))
    if per_pass and traces:
        # per pass: the wall span of the interval — first start to last end of its kernels, a pass ending with its fragment_score_kernel
        # — gaps, memsets and the build's waits for the stream included: the chip's average clock over the interval, not a kernel's
        rows = dispatches(traces[0])
        timed = timed_interval(rows, 'Kernel_Name') or []
        span, start = 0.0, None
        for r in timed:
            start = float(r['Start_Timestamp']) if start is None else start
            if 'fragment_score_kernel<0' in r['Kernel_Name']:
                span += float(r['End_Timestamp']) - start
                start = None
        if span:
            clock_grbm = summary['GRBM_GUI_ACTIVE']['avg_per_launch'] / 8.0 / (span / STEPS)
        for k in INTERVAL:                                   # a kernel's own clock: its GRBM_GUI_ACTIVE per launch over its average duration
            d = [float(r['End_Timestamp']) - float(r['Start_Timestamp']) for r in timed if k in r['Kernel_Name']]
            if d:
                kernel_ns[k] = sum(d) / len(d)
    else:
        for r in csv.DictReader(open(stats[0])):
            if 'raster_queue_kernel<0, 0' in r['Name']:
                clock_grbm = summary['GRBM_GUI_ACTIVE']['avg_per_launch'] / 8.0 / float(r['AverageNs'])
what = ('the scoring interval (rope_profile_eval ev[2]..ev[3]) of the timed passes, per pass: one pass that builds the fragment store (score_queue_kernel + '
        'raster_queue_kernel<DEPTH,LAYER> over the own links twice, fragment_count_kernel, fragment_fill_kernel, fragment_score_kernel<DEPTH>) and '
        f'{STEPS - 1} served passes (fragment_score_kernel<DEPTH> alone); "avg_per_launch" is per PASS, "launches" the profiling runs it was seen in'
        if per_pass else 'raster_queue_kernel<DEPTH,SCORE> (the scoring launch of large batches; raster_score_kernel<DEPTH,SCORE> before the queue)')
separate = {}
for k, counters in by_kernel.items():
    rec = {n: {'launches': len(v), 'avg_per_launch': sum(v) / len(v)} for n, v in sorted(counters.items())}
    if k in kernel_ns:
        rec['average_ns'] = kernel_ns[k]
        # (only for kernels of 0.1 ms and more: a counter run lengthens a short kernel, and its cycles over the trace run's duration mean nothing)
        if 'GRBM_GUI_ACTIVE' in rec and kernel_ns[k] >= 1e5:
            rec['clock_ghz_grbm'] = rec['GRBM_GUI_ACTIVE']['avg_per_launch'] / 8.0 / kernel_ns[k]
    separate[k] = rec
json.dump({'build_id': BUILD_ID, 'clock_ghz_grbm': clock_grbm, 'kernel': what, 'by_kernel': separate,
           'command': f'bench.py --steps {STEPS} --warmup 1 --no-cpu-baseline --no-unshared --no-end-to-end',
           'counters': summary}, open(os.path.join(out, f'{tag}_pmc.json'), 'w'), indent=1)
if 'FETCH_SIZE' in summary and 'WRITE_SIZE' in summary:
    fetch_kb, write_kb = summary['FETCH_SIZE']['avg_per_launch'], summary['WRITE_SIZE']['avg_per_launch']
    json.dump({'build_id': BUILD_ID, 'source': f'profiles/{tag}_pmc.json', 'fetch_size_kb_raw': fetch_kb, 'write_size_kb': write_kb,
               'correction': 'FETCH_SIZE x 2 (gfx950, MI355X_MICROARCH.md HBM section); counters are in KB',
               'hbm_bytes_per_launch': (2 * fetch_kb + write_kb) * 1024.0},
              open(os.path.join(out, 'traffic.json'), 'w'), indent=1)
print(json.dumps(summary, indent=1))
