"""CPU: scratch and spills of the kernels of csrc/rope_bundle.hip in the shipped build, from the compiler's own report.

94 sums a pixel are three times what rope_refine.hip keeps in a thread's registers, so bneq_partial_kernel packs the inliers into
LDS and lets threads own words.  That it keeps everything in registers and LDS is a condition, not a hope:
build.resource_usage(source='rope_bundle.hip') compiles the file device-only with the product's flags and reads the
kernel-resource-usage remarks, as tests/test_kernel_resources.py does for the raster kernels."""
import shutil
import os

import pytest

from rope_s3d_amd import build


@pytest.fixture(scope='module')
def records():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip("no hipcc: the resource table needs the compiler")
    return build.resource_usage(source='rope_bundle.hip')


def test_no_kernel_of_the_file_uses_scratch_or_spills(records):
    names = [r['symbol'] for r in records]
    assert len(records) == 2 and any('bneq_partial_kernel' in n for n in names) and any('bneq_gather_kernel' in n for n in names), names
    for r in records:
        print(r['symbol'], {k: r[k] for k in ('vgprs', 'agprs', 'sgprs', 'lds_bytes', 'occupancy', 'scratch_bytes', 'vgpr_spills', 'sgpr_spills')})
        assert r['scratch_bytes'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, r
    partial = next(r for r in records if 'bneq_partial_kernel' in r['symbol'])
    assert partial['lds_bytes'] <= 64 * 1024 and partial['occupancy'] >= 2


def test_the_source_argument_is_checked_and_the_default_is_unchanged():
    import inspect
    assert inspect.signature(build.resource_usage).parameters['source'].default == 'rope_kernels.hip'
    assert 'rope_bundle.hip' in build._SOURCES and 'rope_bundle.hip' in build._DEPS
    with pytest.raises(ValueError):
        build.resource_usage(source='no_such_file.hip')
