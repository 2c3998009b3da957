"""The rasteriser on meshes built for its edges (tests/raster_ref.py): on every scene the engine gives the oracle's bits — the
render, and the sums, errors and argmin of the depth and the full loss — through every launch structure that draws triangles.
tests/test_raster_refs.py holds the oracle to the exact rasteriser on the same scenes, on the CPU; scene 'nearplane' (triangles cut
at the near plane, which the exact rasteriser does not do) is held to the oracle only, here, by the instantiations that can cut:
the host chooses them for its camera by itself, and CLIP_KERNELS asks for them again.  The profiling build counts its index
violations on it as well."""
import os

import numpy as np
import pytest

from rope_s3d_amd import engine as eng

import helpers
import raster_ref as rr

pytestmark = pytest.mark.gpu
NAMES = list(rr.SCENES)
_oracle = {}


def oracle_render(name):
    """The oracle, its render of the scene's own row, and the target made of its render of a slightly turned row (one that is not
    among the candidates: a row equal to the target has no error, NaN): worked out once per scene."""
    if name not in _oracle:
        sc = rr.scene(name)
        o = rr.make_oracle(sc)
        d, ids = o.render(sc.rows[0], 6)
        _oracle[name] = (sc, o, d, ids, helpers.synthetic_target(*o.render(rr.TARGET_ROW, 6)))
    return _oracle[name]


@pytest.fixture(scope='module')
def engine():
    e = eng.Engine(0)
    yield e
    e.close()


def load(e, sc):
    e.set_strategy(0)
    e.set_robot(sc.model)
    e.set_camera(sc.PV, sc.W, sc.H, sc.znear, sc.zfar)


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[2] == b[2]


@pytest.mark.parametrize('name', NAMES)
def test_render_gives_the_oracles_bits(engine, name):
    """Engine.render of the scene's own row and of a slightly turned one, with all six links and with four; twice."""
    sc, o, d_ref, id_ref, _ = oracle_render(name)
    e = engine
    load(e, sc)
    for own, q in ((True, sc.rows[0]), (False, rr.many_rows(60)[59])):
        for n in (6, 4):
            want_d, want_id = (d_ref, id_ref) if (n == 6 and own) else o.render(q, n)
            for again in range(2):
                d, ids = e.render(q, n)
                assert np.array_equal(ids, want_id), f"{name}: {(ids != want_id).sum()} ids differ (n_render {n}, pass {again})"
                assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), f"{name}: depth differs (n_render {n}, pass {again})"
    e.set_strategy(e.CLIP_KERNELS)                       # the instantiations that carry the cutting code draw the same
    try:
        d, ids = e.render(sc.rows[0], 6)
    finally:
        e.set_strategy(0)
    assert np.array_equal(ids, id_ref) and np.array_equal(d.view(np.uint32), d_ref.view(np.uint32)), name


@pytest.mark.parametrize('name', NAMES)
def test_eval_gives_the_oracles_bits_through_every_launch_structure(engine, name):
    """Row counts 1 and 2 (the split path, geometry inside the raster's workgroups) and 257 (the queue kernel with shared layers),
    each also under the strategy flags that choose the other launch structures, for the depth and the full loss, with six links and
    with four; a second pass on the same context gives the same bits."""
    sc, o, d_ref, id_ref, (tq, t32, flags, *_) = oracle_render(name)
    e = engine
    load(e, sc)
    e.set_target(tq, t32, flags)
    rows = rr.many_rows(257)
    for n_rows, strategies in ((1, (e.NO_SPLIT, e.SEPARATE_GEOMETRY, e.CLIP_KERNELS)), (2, (e.NO_SPLIT, e.SEPARATE_GEOMETRY, e.CLIP_KERNELS)),
                               (257, (e.NO_QUEUE, e.NO_LAYERS, e.NO_LAYERS | e.NO_QUEUE, e.CLIP_KERNELS))):
        cand = rows[:n_rows]
        for loss, n in ((eng.LOSS_DEPTH, 6), (eng.LOSS_FULL, 6), (eng.LOSS_FULL, 4)):
            err_ref, sums_ref = o.eval(cand, loss, n, tq, t32, None, flags, threads=8, want_sums=True)
            want = (err_ref, sums_ref, int(np.argmin(err_ref)))
            used = 23 if loss == eng.LOSS_FULL else 5
            err, sums, bi, be = e.eval(cand, n, loss, want_sums=True)
            assert np.array_equal(sums[:, :used], sums_ref[:, :used]), f"{name}: sums differ on rows {np.nonzero((sums[:, :used] != sums_ref[:, :used]).any(1))[0][:8]} of {n_rows} (loss {loss}, n_render {n})"
            assert same((err, sums[:, :used], bi), (want[0], want[1][:, :used], want[2])) and be == err_ref[bi] and np.isfinite(err).all(), (name, n_rows, loss, n)
            for flag in strategies + (0,):               # the last: the default again, on buffers the others have used
                e.set_strategy(flag)
                try:
                    err2, sums2, bi2, _ = e.eval(cand, n, loss, want_sums=True)
                finally:
                    e.set_strategy(0)
                assert same((err2, sums2, bi2), (err, sums, bi)), (name, n_rows, loss, n, flag)


def test_profiling_build_finds_no_index_out_of_range_on_the_capacity_scenes():
    """The profiling build checks every index into the raster kernels' shared arrays at run time: the full row-item queue (6144
    items, 96 chunks: the last word of s_qmask) and the full meshlet list (2048 entries) leave the violation count at zero."""
    import subprocess
    import sys
    import textwrap
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
    lib = os.path.join(root, 'rope_s3d_amd', 'csrc', 'librope_hip_profile.so')
    if not os.path.exists(lib):
        pytest.skip("librope_hip_profile.so not built (python tools/build_variants.py profile)")
    code = textwrap.dedent('''
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import helpers, raster_ref as rr
        from rope_s3d_amd import engine as eng
        e = eng.Engine(0)
        for name in ('queue63', 'queue64', 'queue65', 'limits_many', 'limits_full', 'nearplane'):
            sc = rr.scene(name)
            e.set_robot(sc.model)
            e.set_camera(sc.PV, sc.W, sc.H, sc.znear, sc.zfar)
            d, ids = e.render(sc.rows[0], 6)
            assert (ids != 255).any()
            tq, t32, flags, *_ = helpers.synthetic_target(*e.render(rr.TARGET_ROW, 6))
            e.set_target(tq, t32, flags)
            for n_rows in (1, 2, 257):
                for flag in (0, e.NO_SPLIT, e.NO_QUEUE, e.NO_LAYERS, e.CLIP_KERNELS):
                    e.set_strategy(flag)
                    e.eval(rr.many_rows(n_rows), 6, eng.LOSS_FULL)
            e.set_strategy(0)
            assert e.debug_bounds() == 0, (name, e.debug_bounds())
        print('bounds ok')
    ''') % (root, os.path.join(root, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, env=dict(os.environ, ROPE_HIP_LIB=lib))
    assert r.returncode == 0 and 'bounds ok' in r.stdout, r.stdout + r.stderr
