"""CPU: scratch and spills of the kernels of csrc/rope_silhouette.hip in the shipped build, from the compiler's own report, as
tests/test_bundle_resources.py does for rope_bundle.hip.  sneq_partial_kernel has bneq_partial_kernel's shape (the inliers packed
into LDS, threads owning words) and mask_distance_kernel is integer work on two 64-word arrays: neither has a reason to touch
scratch, and that is pinned here.  tests/golden/silhouette_resources_gfx950.json records what the compiler reported when they were
written; LDS may not grow and occupancy may not fall below it."""
import json
import os
import shutil

import pytest

from rope_s3d_amd import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'silhouette_resources_gfx950.json')


@pytest.fixture(scope='module')
def records():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip("no hipcc: the resource table needs the compiler")
    return build.resource_usage(source='rope_silhouette.hip')


def test_no_kernel_of_the_file_uses_scratch_or_spills(records):
    with open(GOLDEN) as f:
        golden = json.load(f)['kernels']
    names = [r['symbol'] for r in records]
    assert len(records) == len(golden) == 3 and all(any(k in n for n in names) for k in golden), names
    for r in records:
        print(r['symbol'], {k: r[k] for k in ('vgprs', 'agprs', 'sgprs', 'lds_bytes', 'occupancy', 'scratch_bytes', 'vgpr_spills', 'sgpr_spills')})
        assert r['scratch_bytes'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, r
        want = next(v for k, v in golden.items() if k in r['symbol'])
        assert r['lds_bytes'] <= want['lds_bytes'] and r['occupancy'] >= want['occupancy'], (r, want)
    partial = next(r for r in records if 'sneq_partial_kernel' in r['symbol'])
    assert partial['lds_bytes'] <= 64 * 1024 and partial['occupancy'] >= 2
