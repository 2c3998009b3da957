"""CPU: scratch and spills of the kernels of csrc/rope_polish.hip in the shipped build, from the compiler's own report, as
tests/test_silhouette_resources.py does for rope_silhouette.hip.  The step and variance kernels search their pivot rows at run
time; a per-thread array indexed that way would go to scratch, which is why a workgroup's systems lie in LDS element-major — and
that none of the kernels touches scratch is pinned here.  tests/golden/polish_resources_gfx950.json records what the compiler
reported when they were written; LDS may not grow and occupancy may not fall below it."""
import json
import os
import shutil

import pytest

from rope_s3d_amd import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'polish_resources_gfx950.json')


@pytest.fixture(scope='module')
def records():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip("no hipcc: the resource table needs the compiler")
    return build.resource_usage(source='rope_polish.hip')


def test_no_kernel_of_the_file_uses_scratch_or_spills(records):
    with open(GOLDEN) as f:
        golden = json.load(f)['kernels']
    names = [r['symbol'] for r in records]
    assert len(records) == len(golden) == 6 and all(any(k in n for n in names) for k in golden), names
    for r in records:
        print(r['symbol'], {k: r[k] for k in ('vgprs', 'agprs', 'sgprs', 'lds_bytes', 'occupancy', 'scratch_bytes', 'vgpr_spills', 'sgpr_spills')})
        assert r['scratch_bytes'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, r
        want = next(v for k, v in golden.items() if k in r['symbol'])
        assert r['lds_bytes'] <= want['lds_bytes'] and r['occupancy'] >= want['occupancy'], (r, want)
    # one frame a thread, 64 threads: 6 x 7 doubles a frame for the step, six variances more for the other
    step = next(r for r in records if 'levenberg_step_kernel' in r['symbol'])
    var = next(r for r in records if 'formal_variance_kernel' in r['symbol'])
    assert step['lds_bytes'] == 42 * 64 * 8 and var['lds_bytes'] == 48 * 64 * 8
