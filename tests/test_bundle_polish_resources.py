"""CPU: scratch, spills and LDS of the kernels of csrc/rope_bundle_polish.hip in the shipped build, from the compiler's own report,
as tests/test_polish_resources.py does for rope_polish.hip.  The eliminations search their pivot rows at run time; a per-thread
array indexed that way would go to scratch, which is why every system lies in LDS — a workgroup's 64 frames element-major in the
per-frame kernels, one word an element where one thread solves — and that none of the kernels touches scratch is pinned here.
tests/golden/bundle_polish_resources_gfx950.json records what the compiler reported when they were written; occupancy may not
fall below it, and LDS is what the layouts imply."""
import json
import os
import shutil

import pytest

from rope_s3d_amd import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bundle_polish_resources_gfx950.json')
# doubles a kernel holds in LDS (include/rope_s3d.h): a frame a thread and 64 threads for the per-frame kernels (6 x 13: D | B | g;
# 6 x 18: A | B | I), one word an element for the systems one thread solves (6 x 7, 6 x 12 beside 64 int32 counts, 12 x 13 beside the
# six offsets the workgroup shares, 12 x 24), one int32 for the verdict
LDS = {'schur_frame_kernel': 6 * 13 * 64 * 8, 'schur_var_frame_kernel': 6 * 18 * 64 * 8, 'schur_reduce_kernel': 6 * 7 * 8,
       'schur_var_reduce_kernel': 6 * 12 * 8 + 64 * 4, 'columns_step_kernel': (12 * 13 + 6) * 8, 'columns_variance_kernel': 12 * 24 * 8,
       'bundle_verdict_kernel': 4}


@pytest.fixture(scope='module')
def records():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip("no hipcc: the resource table needs the compiler")
    return build.resource_usage(source='rope_bundle_polish.hip')


def test_source_is_part_of_the_library():
    assert 'rope_bundle_polish.hip' in build._SOURCES and 'rope_bundle_polish.hip' in build._DEPS


def test_no_kernel_of_the_file_uses_scratch_or_spills_and_lds_is_the_layouts(records):
    with open(GOLDEN) as f:
        golden = json.load(f)['kernels']
    names = [r['symbol'] for r in records]
    assert len(records) == len(golden) == 14 and all(any(k in n for n in names) for k in golden), names
    for r in records:
        print(r['symbol'], {k: r[k] for k in ('vgprs', 'agprs', 'sgprs', 'lds_bytes', 'occupancy', 'scratch_bytes', 'vgpr_spills', 'sgpr_spills')})
        assert r['scratch_bytes'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, r
        name, want = next((k, v) for k, v in golden.items() if k in r['symbol'])
        assert r['occupancy'] >= want['occupancy'], (r, want)
        assert r['lds_bytes'] == LDS.get(name, 0) == want['lds_bytes'], (r, want)
