"""GPU: a fixed grid's geometry kept from pass to pass (rope_ctx::geo, csrc/rope_abi.hip) — a pass that runs on what the pass before
it left (no fk_mvp / bounds / MODE_LAYER launch; clear_pass_kernel + layer_sums_kernel instead) gives the bits of a pass that builds
everything, and everything that must drop the kept geometry does.

The smallest shape that takes the cached path: the tests' camera at 160x120 (2 x 2 tiles of 128 x 96, partial on both edges) and a
grid of 8 x 8 x 5 = 320 rows — 64 layers of 5 under 8 parents, so layers are engaged (64 x 4 <= 320) and the batch is a large one
(320 > 256).  All comparisons are exact: the sums are integers and the errors are computed from them.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rope_s3d_amd import build, engine as eng
from rope_s3d_amd.constants import ZFAR, ZNEAR

import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
LOSSES = [eng.LOSS_DEPTH, eng.LOSS_FULL, eng.LOSS_LOOKUP, eng.LOSS_TSWEEP]
NEAR = ([0.3, -0.12, 0.77, 0, 0.2, 0.3], [0, 0, 0, 0, 0, 0])       # test_clipping_kernels_layers_queue_and_every_loss's first camera
Q_A, Q_B = [0.4, 0.3, 0.8, 0, 0, 0], [0.1, 0.5, 0.6, 0.2, -0.3, 0.1]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def grid(q0, spread=.3):
    """8 x 8 x 5 rows about q0: 8 values of S, 8 of L under each, 5 of U under each pair; joint 0 slowest (any order will do)"""
    q0 = np.asarray(q0, float)
    s, l, u = (q0[k] + np.linspace(-spread, spread, n) for k, n in ((0, 8), (1, 8), (2, 5)))
    S, L, U = np.meshgrid(s, l, u, indexing='ij')
    cand = np.tile(q0, (320, 1))
    cand[:, 0], cand[:, 1], cand[:, 2] = S.ravel(), L.ravel(), U.ravel()
    return cand


def target_of(o, q):
    d, ids = o.render(q, 6)
    tq, t32, flags, tgt, _, _ = helpers.synthetic_target(d, ids)
    return dict(tq=tq, t32=t32, flags=flags, full=np.ascontiguousarray(tgt, np.float32))


def give_target(e, t):
    e.set_target(t['tq'], t['t32'], t['flags'])
    e.set_target_tsweep(t['full'])


def new_engine(s, target=None):
    e = eng.Engine(0)
    e.set_robot(s['rb'])
    e.set_camera(s['PV'], s['W'], s['H'], ZNEAR, ZFAR)
    if target is not None:
        give_target(e, target)
    return e


def make_scene(pose, q_a, q_b, ds=4):
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=ds, pose=pose) if pose is not None else helpers.camera('640_480_color', ds=ds)
    o = helpers.make_oracle(rb, intr, PV)
    H, W = intr.height, intr.width
    s = dict(rb=rb, PV=PV, W=W, H=H, o=o, A=target_of(o, q_a), B=target_of(o, q_b), cand=grid(q_a),
             crop=[int(H * .15), int(H * .9), int(W * .1), int(W * .95)])      # rows 18..108, columns 16..152: cuts through all four tiles
    s['e'] = new_engine(s)
    return s


@pytest.fixture(scope='module')
def scene():
    return make_scene(None, Q_A, Q_B)


@pytest.fixture(scope='module')
def fresh_b(scene):
    """Per loss: target B on a context that never saw anything else — computed once, shared, left alone."""
    s = scene
    e = new_engine(s, s['B'])
    e.set_strategy(e.NO_GEOMETRY_CACHE)                   # four losses on one context: DEPTH's geometry would serve FULL
    out = {loss: e.eval(s['cand'], 6, loss, crop=crop_of(s, loss), want_sums=True) for loss in LOSSES}
    assert e.geometry_cache_stats() == (0, 4)
    e.close()
    return out


def crop_of(s, loss):
    return s['crop'] if loss == eng.LOSS_LOOKUP else None


def resident(e, loss, crop):
    e.eval_resident(6, loss, crop)
    return e.download(want_err=True, want_sums=True)


def assert_same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: sums differ"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: errors differ"
    assert got[2] == want[2] and _bits(got[3])[0] == _bits(want[3])[0], f"{what}: argmin differs"


def delta(e, before):
    h, m = e.geometry_cache_stats()
    return h - before[0], m - before[1]


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    build.build()
    csrc = os.path.dirname(build.LIB_PATH)
    out = str(tmp_path_factory.mktemp('geomcache_shim') / 'libgeomcache_shim.so')
    subprocess.check_call([build.shutil.which('hipcc') or '/opt/rocm/bin/hipcc'] + build.HIPCC_FLAGS +
                          [os.path.join(ROOT, 'tests', 'geomcache_shim.hip'), '-L' + csrc, '-lrope_hip', '-Wl,-rpath,' + csrc, '-o', out])
    eng.load_library()                    # the library first: the shim then binds to the copy the engine uses
    lib = C.CDLL(out)
    lib.shim_layer_shape.argtypes = [C.c_void_p, C.c_void_p]
    lib.shim_layer_read.argtypes = [C.c_void_p] * 4
    return lib


def layer_sums(shim, e):
    """-> (sums (layers, tiles, 23), live (layers, tiles) bool: the representative's mask_lo bit)"""
    shape = np.zeros(5, np.int32)
    assert shim.shim_layer_shape(e._ctx, shape.ctypes.data) == 0
    n_layers, n_tiles, words, n_cand, sw = (int(x) for x in shape)
    assert sw == eng.SUM_WORDS
    sums = np.zeros((n_layers, n_tiles, sw), np.uint64)
    rep = np.zeros(n_layers, np.int32)
    mask = np.zeros((n_cand, words), np.uint32)
    assert shim.shim_layer_read(e._ctx, sums.ctypes.data, rep.ctypes.data, mask.ctypes.data) == 0
    tiles = np.arange(n_tiles)
    live = ((mask[rep][:, tiles >> 5] >> (tiles & 31).astype(np.uint32)) & 1).astype(bool)
    return sums, live


# ---------------------------------------------------------------- 1. a hit gives the bits of a miss
@pytest.mark.parametrize('loss', LOSSES)
def test_hit_equals_miss_fresh_context_and_oracle(scene, fresh_b, loss):
    s = scene
    e, o, cand, cr = s['e'], s['o'], s['cand'], crop_of(s, loss)
    e.set_strategy(0)
    give_target(e, s['A'])
    e.upload_candidates(cand)
    before = e.geometry_cache_stats()
    resident(e, loss, cr)                                 # against A: builds
    assert delta(e, before) == (0, 1)
    give_target(e, s['B'])
    hit = resident(e, loss, cr)
    assert delta(e, before) == (1, 1), "the second pass of the same grid did not run on the kept geometry"
    assert_same(hit, fresh_b[loss], "hit against a fresh context")
    again = resident(e, loss, cr)                         # a hit on a hit
    assert delta(e, before) == (2, 1)
    assert_same(again, hit, "second hit")
    # the same context with the cache off, with and without the queues (NO_QUEUE: the second sharing level draws the layers)
    for flags in (e.NO_GEOMETRY_CACHE, e.NO_GEOMETRY_CACHE | e.NO_QUEUE):
        e.set_strategy(flags)
        mark = e.geometry_cache_stats()
        for k in range(2):
            assert_same(resident(e, loss, cr), hit, f"strategy {flags} pass {k}")
        assert delta(e, mark) == (0, 2), "NO_GEOMETRY_CACHE: every pass is a miss"
    e.set_strategy(e.NO_QUEUE)                            # parents + one workgroup per pair, kept
    mark = e.geometry_cache_stats()
    give_target(e, s['A'])
    resident(e, loss, cr)
    give_target(e, s['B'])
    assert_same(resident(e, loss, cr), hit, "hit under NO_QUEUE")
    assert delta(e, mark) == (1, 1)
    e.set_strategy(0)
    rows = np.arange(7, 320, 37)                          # nine rows for the oracle
    t = s['B']
    err_ref, sums_ref = o.eval(cand[rows], loss, 6, t['tq'], t['full'] if loss == eng.LOSS_TSWEEP else t['t32'], cr, t['flags'], threads=8, want_sums=True)
    assert np.array_equal(hit[1][rows], sums_ref) and np.array_equal(_bits(hit[0][rows]), _bits(err_ref))


# ---------------------------------------------------------------- 2. the layer sums themselves
@pytest.mark.parametrize('loss', LOSSES)
def test_layer_sums_of_a_hit_equal_a_miss(scene, shim, loss):
    s = scene
    e, cr = s['e'], crop_of(s, loss)
    e.set_strategy(e.NO_GEOMETRY_CACHE)
    give_target(e, s['B'])
    e.upload_candidates(s['cand'])
    e.eval_resident(6, loss, cr)
    want, live = layer_sums(shim, e)                      # what the MODE_LAYER launch wrote against B
    assert live.any() and want[live].any()
    e.set_strategy(0)
    give_target(e, s['A'])
    before = e.geometry_cache_stats()
    e.eval_resident(6, loss, cr)
    mid, live_a = layer_sums(shim, e)
    give_target(e, s['B'])
    e.eval_resident(6, loss, cr)
    assert delta(e, before) == (1, 1)
    got, live_b = layer_sums(shim, e)
    assert np.array_equal(live_a, live) and np.array_equal(live_b, live)
    assert not np.array_equal(mid[live], want[live]), "targets A and B give the same layer sums: the comparison below shows nothing"
    assert np.array_equal(got[live], want[live])


@pytest.mark.parametrize('W,H', [(158, 118)])
def test_layer_sums_on_a_width_that_is_no_multiple_of_four(scene, shim, W, H):
    """158 columns: score_tile fetches its target words one by one there, and the last group of a row is cut"""
    s = scene
    e = eng.Engine(0)
    e.set_robot(s['rb'])
    e.set_camera(s['PV'], W, H, ZNEAR, ZFAR)
    targets = []
    for q in (Q_A, Q_B):
        d, ids = e.render(np.asarray(q, float), 6)
        tq, t32, flags, tgt, _, _ = helpers.synthetic_target(d, ids)
        targets.append(dict(tq=tq, t32=t32, flags=flags, full=np.ascontiguousarray(tgt, np.float32)))
    for loss in (eng.LOSS_DEPTH, eng.LOSS_TSWEEP):
        e.set_strategy(e.NO_GEOMETRY_CACHE)
        give_target(e, targets[1])
        miss = e.eval(s['cand'], 6, loss, want_sums=True)
        want, live = layer_sums(shim, e)
        e.set_strategy(0)
        give_target(e, targets[0])
        e.eval(s['cand'], 6, loss)
        give_target(e, targets[1])
        before = e.geometry_cache_stats()
        hit = e.eval(s['cand'], 6, loss, want_sums=True)
        assert delta(e, before) == (1, 0)
        got, _ = layer_sums(shim, e)
        assert live.any() and np.array_equal(got[live], want[live])
        assert_same(hit, miss, f"loss {loss} at {W}x{H}")
    e.close()


# ---------------------------------------------------------------- 3. the same through rope_eval
def test_rope_eval_with_equal_rows_hits_and_one_changed_bit_misses(scene, fresh_b):
    s = scene
    e, loss = s['e'], eng.LOSS_DEPTH
    e.set_strategy(0)
    give_target(e, s['A'])
    e.eval(s['cand'], 6, loss)
    give_target(e, s['B'])
    before = e.geometry_cache_stats()
    hit = e.eval(s['cand'].copy(), 6, loss, want_sums=True)          # other memory, equal bytes
    assert delta(e, before) == (1, 0)
    assert_same(hit, fresh_b[loss], "rope_eval on equal rows")
    other = s['cand'].copy()
    other[200, 2] = np.nextafter(other[200, 2], np.inf)              # one angle, its last bit
    got = e.eval(other, 6, loss, want_sums=True)
    assert delta(e, before) == (1, 1), "rows that differ in one bit ran on the kept geometry"
    f = new_engine(s, s['B'])
    assert_same(got, f.eval(other, 6, loss, want_sums=True), "changed rows against a fresh context")
    f.close()


# ---------------------------------------------------------------- 4. everything that must drop the kept geometry
def _drops(s):
    """name -> what to do to the engine between two passes; each leaves target B set and the grid to be uploaded again if need be"""
    e, cand = s['e'], s['cand']
    return {
        'set_camera, same values': lambda: e.set_camera(s['PV'], s['W'], s['H'], ZNEAR, ZFAR),      # values are not compared: any call drops
        'set_robot': lambda: e.set_robot(s['rb']),
        'set_strategy': lambda: e.set_strategy(e.NO_PARENTS),
        'render': lambda: e.render(np.asarray(Q_B, float), 6),
        'coverage': lambda: e.coverage(cand[:12], 6),
        'small eval': lambda: e.eval(cand[:2], 6, eng.LOSS_DEPTH),
        'lookup_build': lambda: e.lookup_build(cand[:40], 6, s['crop']),
        'larger upload': lambda: e.eval(np.concatenate([cand, cand[:160] + 1e-3]), 6, eng.LOSS_DEPTH),      # 480 rows: the buffers grow
    }


@pytest.mark.parametrize('what', ['set_camera, same values', 'set_robot', 'set_strategy', 'render', 'coverage', 'small eval', 'lookup_build',
                                  'larger upload'])
def test_what_drops_the_kept_geometry(scene, fresh_b, what):
    s = scene
    e, loss = s['e'], eng.LOSS_DEPTH
    e.set_strategy(0)
    give_target(e, s['B'])
    e.eval(s['cand'], 6, loss)
    before = e.geometry_cache_stats()
    e.eval(s['cand'], 6, loss)
    assert delta(e, before) == (1, 0), "not kept in the first place"
    _drops(s)[what]()
    if what in ('set_camera, same values', 'set_robot'):
        give_target(e, s['B'])                             # a new camera or robot may take the target with it
    mark = e.geometry_cache_stats()
    got = e.eval(s['cand'], 6, loss, want_sums=True)
    assert delta(e, mark) == (0, 1), f"{what}: the next pass ran on the kept geometry"
    assert_same(got, fresh_b[loss], what)
    assert_same(e.eval(s['cand'], 6, loss, want_sums=True), fresh_b[loss], f"{what}: the pass after")
    assert delta(e, mark) == (1, 1)
    e.set_strategy(0)


def test_another_n_render_and_another_crop_miss(scene, fresh_b):
    s = scene
    e = s['e']
    e.set_strategy(0)
    give_target(e, s['B'])
    e.upload_candidates(s['cand'])
    f = new_engine(s, s['B'])
    f.upload_candidates(s['cand'])
    before = e.geometry_cache_stats()
    crop2 = [s['crop'][0] + 7, s['crop'][1], s['crop'][2], s['crop'][3] - 9]
    steps = [(6, eng.LOSS_LOOKUP, s['crop']), (6, eng.LOSS_LOOKUP, s['crop']), (6, eng.LOSS_LOOKUP, crop2), (6, eng.LOSS_LOOKUP, crop2),
             (4, eng.LOSS_DEPTH, None), (4, eng.LOSS_DEPTH, None), (6, eng.LOSS_DEPTH, None), (6, eng.LOSS_FULL, None)]
    want_hits = [0, 1, 1, 2, 2, 3, 3, 4]                   # the loss alone is no part of the key: DEPTH -> FULL at the same frame hits
    for (n, loss, cr), hits in zip(steps, want_hits):
        e.eval_resident(n, loss, cr)
        got = e.download(want_err=True, want_sums=True)
        assert delta(e, before)[0] == hits, (n, loss, cr)
        f.set_strategy(f.NO_GEOMETRY_CACHE)
        f.eval_resident(n, loss, cr)
        assert_same(got, f.download(want_err=True, want_sums=True), f"n_render {n} loss {loss} crop {cr}")
    assert_same(got, fresh_b[eng.LOSS_FULL], "FULL on DEPTH's geometry")
    f.close()


def test_eval_views_drops_the_kept_geometry(scene, fresh_b):
    s = scene
    e, loss = s['e'], eng.LOSS_DEPTH
    e.set_strategy(0)
    give_target(e, s['B'])
    e.eval(s['cand'], 6, loss)
    e.eval(s['cand'], 6, loss)
    qs = np.asarray([Q_A, Q_B], float)
    e.set_frames(qs, np.stack([s['A']['tq'], s['B']['tq']]), np.stack([s['A']['full'], s['B']['full']]))
    e.eval_views(np.stack([s['PV']] * 150), 6, loss)       # 300 rows of the per-candidate buffers
    mark = e.geometry_cache_stats()
    got = e.eval(s['cand'], 6, loss, want_sums=True)       # equal rows, but they are no longer resident: uploaded and built again
    assert delta(e, mark) == (0, 1)
    assert_same(got, fresh_b[loss], "after rope_eval_views")


# ---------------------------------------------------------------- 5. the kernels that clip
def test_hit_equals_miss_under_a_near_camera():
    pose, q0 = NEAR
    s = make_scene(pose, q0, [0.15, -0.1, 0.2, 0, 0, 0])
    e = s['e']
    from test_gpu_instantiations import beyond_reach, cut_triangles
    assert not beyond_reach(s['rb'], s['PV']), "the camera is out of the robot's reach: the plain kernels would be chosen"
    assert sum(cut_triangles(s['o'], q) for q in s['cand'][::40]) > 0, "the near camera cuts no triangles of the sampled rows"
    for loss in LOSSES:
        cr = crop_of(s, loss)
        e.set_strategy(e.NO_GEOMETRY_CACHE)
        give_target(e, s['B'])
        miss = e.eval(s['cand'], 6, loss, crop=cr, want_sums=True)
        e.set_strategy(0)
        give_target(e, s['A'])
        e.eval(s['cand'], 6, loss, crop=cr)
        give_target(e, s['B'])
        before = e.geometry_cache_stats()
        hit = e.eval(s['cand'], 6, loss, crop=cr, want_sums=True)
        assert delta(e, before) == (1, 0)
        assert_same(hit, miss, f"near camera, loss {loss}")
    rows = np.arange(3, 320, 45)
    t = s['B']
    _, sums_ref = s['o'].eval(s['cand'][rows], eng.LOSS_TSWEEP, 6, t['tq'], t['full'], None, t['flags'], threads=8, want_sums=True)
    assert np.array_equal(hit[1][rows], sums_ref)
    e.close()
