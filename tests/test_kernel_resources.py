"""CPU: scratch and spills of every raster kernel instantiation in the shipped build, from the compiler's own report.

raster_tile<LOSS, MODE, CLIP> becomes some 46 kernels, each register-allocated on its own, and the one unexplained wrong result of
this project (profiles/r03_clip_fault.txt) came from an instantiation that had begun to spill.  No GPU is needed to
see spilling: build.resource_usage() compiles rope_kernels.hip device-only with the product's flags (and ROPE_HIPCC_EXTRA, so a
variant build is judged by the same rule) and the kernel-resource-usage remarks.  Two kinds of assertion:

  * conditions, fixed by DESIGN.md §6a: no CLIP instantiation spills a VGPR or uses scratch; no raster_score_kernel uses
    scratch (which is what makes it the twin every queue kernel is compared with in tests/test_gpu_instantiations.py); the
    instantiations the launch functions can select are exactly those compiled and those in the committed table;
  * a pin: VGPR spills and scratch bytes of every instantiation equal tests/golden/kernel_resources_gfx950.json.  It is meant to
    fail after a compiler update or an edit that moves the register allocation — that is the alarm.
"""
import json
import os
import re
import shutil

import pytest

from rope_s3d_amd import build

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
CSRC = os.path.join(ROOT, 'rope_s3d_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kernel_resources_gfx950.json')


def key(kernel, loss, mode, clip) -> str:
    return f"{kernel}<{loss}, {mode}, {'CLIP' if clip else 'plain'}>"


@pytest.fixture(scope='module')
def table():
    """One device-only compile (a minute or two) -> {key: record} of the raster kernels."""
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip("no hipcc: the resource table needs the compiler")
    recs = [r for r in build.resource_usage() if r['loss'] is not None]
    out = {key(r['kernel'], r['loss'], r['mode'], r['clip']): r for r in recs}
    assert len(out) == len(recs), "an instantiation reported twice"
    return out


def _enum(text, first):
    """names of the `enum { first = 0, ... }` / `ROPE_LOSS_x = n` list that starts with `first`, by value"""
    body = re.search(r'\b' + first + r'\s*=\s*0\b[^}]*', text).group(0)
    pairs = re.findall(r'\b([A-Z][A-Z0-9_]*)\s*=\s*(\d+)', body)
    names = [None] * len(pairs)
    for n, v in pairs:
        names[int(v)] = n
    return names


def selectable():
    """Every (kernel, LOSS, MODE, CLIP) that launch_raster, launch_raster_queue and launch_layer_queue can select, read from their
    source: each launch_one<LOSS, MODE> / launch_queue_one<LOSS, MODE> there picks the CLIP or the plain kernel at run time."""
    with open(os.path.join(CSRC, 'rope_kernels.hip')) as f:
        src = f.read()
    body = src[src.index('hipError_t launch_raster('):src.index('hipError_t launch_score_gtile(')]
    found = set()
    for helper, kernel in (('launch_one', 'raster_score_kernel'), ('launch_queue_one', 'raster_queue_kernel')):
        for loss, mode in re.findall(r'\b' + helper + r'<ROPE_LOSS_(\w+),\s*MODE_(\w+)>', body):
            found |= {key(kernel, loss, mode, True), key(kernel, loss, mode, False)}
    return found


def test_names_of_template_arguments_match_the_headers():
    with open(os.path.join(ROOT, 'include', 'rope_s3d.h')) as f:
        losses = _enum(f.read(), 'ROPE_LOSS_DEPTH')
    with open(os.path.join(CSRC, 'rope_kernels.h')) as f:
        modes = _enum(f.read(), 'MODE_SCORE')
    assert tuple(n[len('ROPE_LOSS_'):] for n in losses) == build.LOSS_NAMES
    assert tuple(n[len('MODE_'):] for n in modes) == build.MODE_NAMES


def test_parser_reads_the_remark_format():
    text = '\n'.join(f"rope_kernels.hip:1358:1: remark: {l} [-Rpass-analysis=kernel-resource-usage]" for l in (
        "Function Name: _ZN4rope19raster_queue_kernelILi4ELi0ELb0EEEvNS_11FrameParamsENS_11RobotParamsENS_10RasterArgsEPKjmPi",
        "    TotalSGPRs: 106", "    VGPRs: 80", "    AGPRs: 0", "    ScratchSize [bytes/lane]: 204", "    Dynamic Stack: False",
        "    Occupancy [waves/SIMD]: 6", "    SGPRs Spill: 94", "    VGPRs Spill: 218", "    LDS Size [bytes/block]: 81480",
        "Function Name: _ZN4rope13fk_mvp_kernelEPKdiiS1_S1_S1_PKiPfPmPjS6_iPiS6_S6_i", "    VGPRs: 166"))
    a, b = build.parse_resource_remarks(text)
    assert (a['kernel'], a['loss'], a['mode'], a['clip']) == ('raster_queue_kernel', 'CAMFULL', 'SCORE', False)
    assert (a['vgprs'], a['vgpr_spills'], a['sgpr_spills'], a['scratch_bytes'], a['occupancy']) == (80, 218, 94, 204, 6)
    assert (b['kernel'], b['loss'], b['vgprs']) == ('fk_mvp_kernel', None, 166)


def test_every_selectable_instantiation_is_compiled_and_in_the_committed_table(table):
    want = selectable()
    assert len(want) >= 46
    assert want == set(table), f"launch functions and compiled kernels differ: {sorted(want ^ set(table))}"
    with open(GOLDEN) as f:
        pinned = set(json.load(f)['kernels'])
    assert want == pinned, (f"instantiations without a row in {os.path.relpath(GOLDEN, ROOT)}, or rows without a kernel: {sorted(want ^ pinned)} "
                            "(python tests/golden/make_kernel_resources.py)")


def test_clip_instantiations_need_no_scratch(table):
    """the kernels that can clip are compiled at ROPE_MIN_WAVES_CLIP waves/SIMD so that nothing of theirs lives in
    scratch — the build in which they spilled gave sums that changed from run to run."""
    bad = {k: (r['vgpr_spills'], r['scratch_bytes']) for k, r in table.items() if r['clip'] and (r['vgpr_spills'] or r['scratch_bytes'])}
    assert not bad, f"CLIP kernels with (VGPR spills, scratch bytes/lane): {bad}"


def test_score_kernels_need_no_scratch(table):
    """raster_score_kernel is the scratch-free twin that set_strategy(NO_QUEUE) selects for every queue kernel."""
    bad = {k: r['scratch_bytes'] for k, r in table.items() if r['kernel'] == 'raster_score_kernel' and r['scratch_bytes']}
    assert not bad, f"raster_score_kernel instantiations with scratch bytes/lane: {bad}"


def test_spills_and_scratch_equal_the_committed_table(table):
    with open(GOLDEN) as f:
        golden = json.load(f)
    diff = []
    for k in sorted(set(table) & set(golden['kernels'])):
        old, r = golden['kernels'][k], table[k]
        new = {'vgpr_spills': r['vgpr_spills'], 'scratch_bytes': r['scratch_bytes']}
        if new != old:
            diff.append(f"  {k}: committed {old['vgpr_spills']} VGPR spills / {old['scratch_bytes']} B scratch, now "
                        f"{new['vgpr_spills']} / {new['scratch_bytes']} ({r['vgprs']} VGPRs, {r['occupancy']} waves/SIMD)")
    assert not diff, ("register allocation of the raster kernels changed (committed with: " + golden.get('compiler', '?') + "):\n" + '\n'.join(diff) +
                      "\nRun tests/test_gpu_instantiations.py on a GPU once — it holds every instantiation to its scratch-free twin and the "
                      "oracle — and only then re-record with python tests/golden/make_kernel_resources.py")
