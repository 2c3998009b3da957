"""Host-only checks of the bulk-render feature: the lookup-file writer of RobotLookupCreator (the reference's layout,
lookup.py:88-106) and the rope_render_batch entry point of the library and of its ctypes binding.  No device is opened."""
import os

import numpy as np
import pytest

from rope_s3d_amd import engine as eng


def test_lookup_file_layout(tmp_path):
    from rope_s3d_amd.data import hdf5
    from rope_s3d_amd.simulation.lookup import write_lookup_file
    if not hdf5.available():
        pytest.skip("no libhdf5 on this machine")
    rng = np.random.default_rng(5)
    angles = rng.uniform(-1, 1, (12, 6))
    depth = np.zeros((12, 40, 56))
    depth[:, 10:20, 5:30] = rng.uniform(1.0, 3.0, (12, 10, 25)).astype(np.float32)
    pose = np.array([1.5, -0.2, 0.4, 0.0, 0.1, 3.1])
    changed = np.array([True, True, True, False, False, False])
    divisions = np.array([3, 2, 2, 1, 1, 1])
    path = write_lookup_file(str(tmp_path / 'lookup.h5'), angles, depth, pose, '1280_720_color', 4, changed, divisions, 'mh5l')
    with hdf5.H5File(path) as f:
        a = f.attrs
        assert set(a) == {'pose', 'intrinsics', 'num_links_rendered', 'angles_changed', 'divisions', 'urdf'}
        assert np.array_equal(a['pose'], pose) and a['intrinsics'] == '1280_720_color' and a['num_links_rendered'] == 4
        assert a['angles_changed'].dtype.kind == 'i' and np.array_equal(a['angles_changed'], changed.astype(int))
        assert np.array_equal(a['divisions'], divisions) and a['urdf'] == 'mh5l'
        assert 'angles' in f and 'depth' in f
        assert f['angles'].dtype == np.float64 and f['angles'].shape == (12, 6)
        assert f['depth'].dtype == np.float64 and f['depth'].shape == (12, 40, 56)
        assert np.array_equal(f['angles'][:], angles) and np.array_equal(f['depth'][:], depth)
        assert np.array_equal(f['depth'][3:7], depth[3:7])
    # depth is stored gzip-compressed: a mostly empty table takes a fraction of its raw size
    assert os.path.getsize(path) < depth.nbytes // 4


def test_write_arrays_gzip_per_array(tmp_path):
    from rope_s3d_amd.data import hdf5
    if not hdf5.available():
        pytest.skip("no libhdf5 on this machine")
    z = np.zeros((64, 64, 64))
    big = hdf5.write_arrays(str(tmp_path / 'plain.h5'), {'a': z, 'b': z}, gzip={'a': 1})
    small = hdf5.write_arrays(str(tmp_path / 'both.h5'), {'a': z, 'b': z}, gzip=1)
    assert os.path.getsize(big) > z.nbytes > 20 * os.path.getsize(small)
    with hdf5.H5File(big) as f:
        assert np.array_equal(f['a'][:], z) and np.array_equal(f['b'][:], z)


def test_library_exports_render_batch():
    lib = eng.load_library()
    assert 'rope_render_batch' in eng.ABI_SYMBOLS
    assert hasattr(lib, 'rope_render_batch')
    # ctx, q, PV, N, n_render, crop, depth, ids
    assert lib.rope_render_batch.argtypes == [eng.C.c_void_p, eng.C.c_void_p, eng.C.c_void_p, eng.C.c_int, eng.C.c_int,
                                              eng.C.c_void_p, eng.C.c_void_p, eng.C.c_void_p]
    hdr = open(os.path.join(os.path.dirname(eng.__file__), os.pardir, 'include', 'rope_s3d.h')).read()
    assert 'int rope_render_batch(rope_ctx *ctx, const double *q, const double *PV, int N, int n_render, const int32_t *crop,' in hdr


def test_bulk_renderers_are_exported():
    import robotpose
    from rope_s3d_amd import simulation
    from rope_s3d_amd.simulation.render import Renderer
    assert issubclass(simulation.DatasetRenderer, Renderer) and issubclass(simulation.RobotLookupCreator, Renderer)
    assert robotpose.DatasetRenderer is simulation.DatasetRenderer
    for name in ('render_batch', 'render_ids_batch'):
        assert callable(getattr(Renderer, name))
    for name in ('render_at', 'setPosesFromDS', 'render_range', 'render_indices', 'close'):
        assert callable(getattr(simulation.DatasetRenderer, name))
    for name in ('load_config', '_generate_depth_array', 'run'):
        assert callable(getattr(simulation.RobotLookupCreator, name))
