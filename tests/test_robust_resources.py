"""CPU: scratch, spills, LDS and occupancy of the kernels of csrc/rope_robust.hip in the shipped build, from the compiler's own
report (build.resource_usage, as tests/test_bundle_resources.py reads it for csrc/rope_bundle.hip).

The robust partial kernels are the plain one's body (rope_neq.h: bneq_pack_and_own_words, 26 KB of packed rows in LDS) behind
another pixel functor, so the conditions are its sibling's: nothing in scratch, at most 64 KB of LDS, two waves a SIMD or more."""
import os
import shutil

import pytest

from rope_s3d_amd import build


@pytest.fixture(scope='module')
def records():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip("no hipcc: the resource table needs the compiler")
    return build.resource_usage(source='rope_robust.hip')


def test_no_kernel_of_the_file_uses_scratch_or_spills(records):
    names = [r['symbol'] for r in records]
    assert len(records) == 4, names                                       # the partial kernel for Huber and for Tukey, the gather, the histogram
    assert sum('robust_partial_kernel' in n for n in names) == 2 and any('robust_gather_kernel' in n for n in names)
    assert any('resid_histogram_kernel' in n for n in names)
    for r in records:
        print(r['symbol'], {k: r[k] for k in ('vgprs', 'agprs', 'sgprs', 'lds_bytes', 'occupancy', 'scratch_bytes', 'vgpr_spills', 'sgpr_spills')})
        assert r['scratch_bytes'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, r


def test_the_partial_kernels_keep_their_siblings_lds_and_occupancy(records):
    partial = [r for r in records if 'robust_partial_kernel' in r['symbol']]
    assert len(partial) == 2
    for r in partial:
        assert r['lds_bytes'] <= 64 * 1024 and r['occupancy'] >= 2, r
    hist = next(r for r in records if 'resid_histogram_kernel' in r['symbol'])
    assert hist['lds_bytes'] == 258 * 4                                  # the workgroup's counts and nothing else
