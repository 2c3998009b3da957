"""GPU: a fixed grid's kept fragments (rope_ctx::frags, csrc/rope_fragstore.h, csrc/rope_abi.hip) — after a pass has run on kept
geometry, the context also keeps, per row, the 4-sample groups where the row's own links beat its shared layer, and later passes
score by streaming them (fragment_score_kernel) instead of drawing the own links again.  Such a pass gives the bits of a pass that
builds everything; the store holds exactly the groups the oracle's id image says; the budget refuses; and whatever drops the kept
geometry drops the store.

The shape is test_gpu_geometry_cache's: 160x120 (2 x 2 partial tiles), 320 rows = 64 layers of 5 — the building pass draws the rows
in five chunks of 64 (the scratch is no larger than the layer buffer).  All comparisons are exact.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rope_s3d_amd import build, engine as eng
from rope_s3d_amd.constants import ZFAR, ZNEAR

from test_gpu_geometry_cache import (LOSSES, NEAR, Q_A, Q_B, ROOT, assert_same, crop_of, give_target, grid, make_scene, new_engine,
                                     resident)

pytestmark = pytest.mark.gpu

TILE_W, TILE_H, N_SHARED = 128, 96, 3


@pytest.fixture(scope='module')
def scene():
    return make_scene(None, Q_A, Q_B)


def fresh_results(s):
    """Per (loss, target): a context that keeps nothing — computed once, shared, left alone."""
    out = {}
    e = new_engine(s)
    e.set_strategy(e.NO_GEOMETRY_CACHE)
    for name in 'AB':
        give_target(e, s[name])
        for loss in LOSSES:
            out[loss, name] = e.eval(s['cand'], 6, loss, crop=crop_of(s, loss), want_sums=True)
    assert e.fragment_store_stats() == (0, 0, 0, 0)
    e.close()
    return out


@pytest.fixture(scope='module')
def fresh(scene):
    return fresh_results(scene)


def stats_delta(e, before):
    now = e.fragment_store_stats()
    return now[0] - before[0], now[1] - before[1]


def three_passes_then_b(s, e, want, what):
    """passes 1 (miss), 2 (first hit: builds, then scores from the store) and 3 (served) on A, then B after set_target — per loss,
    each from a context without kept geometry"""
    for loss in LOSSES:
        cr = crop_of(s, loss)
        e.set_strategy(0)                                     # drops geometry and store: the next pass builds everything
        give_target(e, s['A'])
        e.upload_candidates(s['cand'])
        f0, g0 = e.fragment_store_stats(), e.geometry_cache_stats()
        assert f0[2:] == (0, 0), "set_strategy left a store behind"
        assert_same(resident(e, loss, cr), want[loss, 'A'], f"{what}, loss {loss}: pass 1")
        assert stats_delta(e, f0) == (0, 0)
        assert_same(resident(e, loss, cr), want[loss, 'A'], f"{what}, loss {loss}: pass 2, which builds the store")
        assert stats_delta(e, f0) == (1, 1)
        built = e.fragment_store_stats()
        assert built[3] > 0 and built[2] == 36 * built[3] + 8 * (320 * 4 + 1)
        assert_same(resident(e, loss, cr), want[loss, 'A'], f"{what}, loss {loss}: pass 3, served")
        give_target(e, s['B'])
        assert_same(resident(e, loss, cr), want[loss, 'B'], f"{what}, loss {loss}: target B from A's store")
        assert stats_delta(e, f0) == (1, 3)
        assert e.fragment_store_stats()[2:] == built[2:]
        g1 = e.geometry_cache_stats()
        assert (g1[0] - g0[0], g1[1] - g0[1]) == (3, 1), "the geometry cache's counts changed their meaning"


# ---------------------------------------------------------------- 1. served passes give the bits of passes that build everything
def test_every_loss_builds_once_and_serves(scene, fresh):
    three_passes_then_b(scene, scene['e'], fresh, "plain kernels")


def test_one_store_serves_every_loss(scene, fresh):
    s, e = scene, scene['e']
    e.set_strategy(0)
    give_target(e, s['B'])
    e.upload_candidates(s['cand'])
    f0 = e.fragment_store_stats()
    for k, loss in enumerate([eng.LOSS_DEPTH, eng.LOSS_DEPTH, eng.LOSS_FULL, eng.LOSS_TSWEEP, eng.LOSS_DEPTH]):      # one frame, one key
        assert_same(resident(e, loss, None), fresh[loss, 'B'], f"pass {k}, loss {loss}")
    assert stats_delta(e, f0) == (1, 4)
    assert_same(resident(e, eng.LOSS_LOOKUP, s['crop']), fresh[eng.LOSS_LOOKUP, 'B'], "the crop is part of the key: built anew")
    assert stats_delta(e, f0) == (1, 4)
    assert_same(resident(e, eng.LOSS_LOOKUP, s['crop']), fresh[eng.LOSS_LOOKUP, 'B'], "LOOKUP from its own store")
    assert stats_delta(e, f0) == (2, 5)


# ---------------------------------------------------------------- 2. the kernels that clip draw the store
def test_every_loss_under_a_near_camera():
    pose, q0 = NEAR
    s = make_scene(pose, q0, [0.15, -0.1, 0.2, 0, 0, 0])
    from test_gpu_instantiations import beyond_reach, cut_triangles
    assert not beyond_reach(s['rb'], s['PV']), "the camera is out of the robot's reach: the plain kernels would be chosen"
    assert sum(cut_triangles(s['o'], q) for q in s['cand'][::40]) > 0, "the near camera cuts no triangles of the sampled rows"
    three_passes_then_b(s, s['e'], fresh_results(s), "near camera")
    s['e'].close()


# ---------------------------------------------------------------- 3. what the store holds
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    build.build()
    csrc = os.path.dirname(build.LIB_PATH)
    out = str(tmp_path_factory.mktemp('fragstore_shim') / 'libfragstore_shim.so')
    subprocess.check_call([build.shutil.which('hipcc') or '/opt/rocm/bin/hipcc'] + build.HIPCC_FLAGS +
                          [os.path.join(ROOT, 'tests', 'fragstore_shim.hip'), '-L' + csrc, '-lrope_hip', '-Wl,-rpath,' + csrc, '-o', out])
    eng.load_library()
    lib = C.CDLL(out)
    lib.shim_fragment_shape.argtypes = [C.c_void_p, C.c_void_p]
    lib.shim_fragment_read.argtypes = [C.c_void_p] * 5
    lib.shim_force_unweighted.argtypes = [C.c_void_p]
    lib.shim_fragment_score_repeat.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def read_store(shim, e):
    shape = np.zeros(7, np.int64)
    assert shim.shim_fragment_shape(e._ctx, shape.ctypes.data) == 0
    valid, rows, tiles, groups, declined, n_shared, tiles_x = (int(x) for x in shape)
    assert valid and not declined and n_shared == N_SHARED
    offs = np.zeros(rows * tiles + 1, np.uint64)
    where = np.zeros(max(groups, 1), np.uint32)
    fin, base = np.zeros((max(groups, 1), 4), np.uint32), np.zeros((max(groups, 1), 4), np.uint32)
    assert shim.shim_fragment_read(e._ctx, offs.ctypes.data, where.ctypes.data, fin.ctypes.data, base.ctypes.data) == 0
    return dict(rows=rows, tiles=tiles, tiles_x=tiles_x, groups=groups, offs=offs.astype(np.int64), where=where, fin=fin, base=base)


def groups_of_ids(ids, tiles_x):
    """(tile, group) of every 4-sample group of the id image that holds an own link (N_SHARED <= id < 255), in the store's order"""
    H, W = ids.shape
    own = (ids >= N_SHARED) & (ids != 255)
    out = []
    for r, c in zip(*np.nonzero(own)):
        tile = (r // TILE_H) * tiles_x + c // TILE_W
        out.append((int(tile), int(((r % TILE_H) * TILE_W + c % TILE_W) // 4)))
    return sorted(set(out))


def hidden_pose(o, q0):
    """(S, L) near which links 3-5 leave the 160x120 frame for every U of the grid — searched on the CPU with the oracle"""
    u = q0[2] + np.linspace(-.3, .3, 5)
    for S in np.linspace(-3.1, 3.1, 9):                       # (the rows are test input, not poses the arm can take)
        for L in np.linspace(-3.0, 3.0, 13):
            qs = [np.array([S, L, uu, q0[3], q0[4], q0[5]], float) for uu in u]
            if all(not ((ids >= N_SHARED) & (ids != 255)).any() for _, ids in (o.render(q, 6) for q in qs)):
                return S, L
    return None


def test_store_holds_the_groups_of_the_oracles_id_image(scene, shim):
    s, o = scene, scene['o']
    e = new_engine(s, s['A'])
    cand = s['cand'].copy()
    sl = hidden_pose(o, np.asarray(Q_A, float))
    assert sl is not None, "no pose of the search hides links 3-5: the empty row would go untested"
    cand[315:320, 0], cand[315:320, 1] = sl                  # the last layer: five rows whose own links are nowhere in the frame
    for _ in range(2):
        e.eval(cand, 6, eng.LOSS_DEPTH)
    assert e.fragment_store_stats()[:2] == (1, 1)
    st = read_store(shim, e)
    assert st['rows'] == 320 and st['tiles'] == 4 and st['offs'][-1] == st['groups'] == e.fragment_store_stats()[3]
    assert (np.diff(st['offs']) >= 0).all()
    for row in (0, 7, 63, 64, 161, 255, 314, 317, 319):      # both ends of chunks of 64, and two rows of the hidden layer
        lo, hi = st['offs'][row * 4], st['offs'][(row + 1) * 4]
        w = st['where'][lo:hi]
        got = [(int(x >> 12), int(x & 0xFFF)) for x in w]
        assert got == sorted(set(got)), f"row {row}: list not ordered by tile, then group"
        for t in range(4):                                    # every tile's slice holds that tile's groups
            a, b = st['offs'][row * 4 + t], st['offs'][row * 4 + t + 1]
            assert ((st['where'][a:b] >> 12) == t).all()
        _, ids = o.render(cand[row], 6)
        want = groups_of_ids(ids, st['tiles_x'])
        assert got == want, f"row {row}: {len(got)} groups stored, the oracle's image has {len(want)}"
        if row >= 315:
            assert not got
        else:
            assert got, f"row {row} shows none of its own links: pick another"
        fin, base = st['fin'][lo:hi], st['base'][lo:hi]
        assert (fin <= base).all() and (fin < base).any(axis=1).all(), f"row {row}: a stored group in which no own key beats the base"
        # the finished keys carry the ids of the oracle's image
        for (tile, g), keys in list(zip(got, fin))[::17]:
            r, c = (tile // st['tiles_x']) * TILE_H + (4 * g) // TILE_W, (tile % st['tiles_x']) * TILE_W + (4 * g) % TILE_W
            for j in range(4):
                if c + j < ids.shape[1] and r < ids.shape[0]:
                    assert (255 if keys[j] == 0xFFFFFFFF else int(keys[j] & 0xFF)) == int(ids[r, c + j]), (row, tile, g, j)
    # and the pass that was scored from it agrees with a context that keeps nothing
    f = new_engine(s, s['A'])
    f.set_strategy(f.NO_GEOMETRY_CACHE)
    assert_same(e.eval(cand, 6, eng.LOSS_FULL, want_sums=True), f.eval(cand, 6, eng.LOSS_FULL, want_sums=True), "grid with a hidden layer")
    assert e.fragment_store_stats()[:2] == (1, 2)
    f.close()
    e.close()


def test_unweighted_queue_draws_the_same_store(scene, fresh, shim):
    """Frames of more than 256 tiles keep no pair weights: the building launch then takes one queue segment from the start of the
    item buffer.  The same 320 rows under that layout: the same store contents, the same bits from it."""
    s = scene
    w = new_engine(s, s['B'])
    for _ in range(2):
        w.eval(s['cand'], 6, eng.LOSS_DEPTH)
    want = read_store(shim, w)
    e = new_engine(s, s['B'])
    e.eval(s['cand'], 6, eng.LOSS_DEPTH)                      # allocates the per-candidate buffers
    assert shim.shim_force_unweighted(e._ctx) == 0
    for loss in LOSSES:
        for k in range(3):                                    # miss (the layout changed under it), build, served
            assert_same(e.eval(s['cand'], 6, loss, crop=crop_of(s, loss), want_sums=True), fresh[loss, 'B'], f"unweighted, loss {loss}, pass {k}")
    assert e.fragment_store_stats()[:2] == (3, 9)             # DEPTH's store served FULL; LOOKUP's crop built its own; TSWEEP built the frame's again
    for k in range(2):
        e.eval(s['cand'], 6, eng.LOSS_DEPTH)
    got = read_store(shim, e)
    assert got['groups'] == want['groups'] > 0 and e.fragment_store_pairs() == w.fragment_store_pairs() > 0
    for name in ('offs', 'where', 'fin', 'base'):
        assert np.array_equal(got[name], want[name]), f"unweighted: {name} differs from the weighted build's"
    w.close()
    e.close()


# ---------------------------------------------------------------- 3b. rows of any length
@pytest.mark.parametrize('loss', [eng.LOSS_FULL, eng.LOSS_DEPTH, eng.LOSS_TSWEEP])
def test_a_thread_that_meets_thousands_of_groups(scene, shim, loss):
    """The full loss keeps its per-link counts in 12-bit fields (score_pixel) that score_tile, at 16 samples a thread, cannot fill.
    A thread of fragment_score_kernel meets a row's groups / 256 rounds of four samples: a 4K frame gives it thousands.  A synthetic
    store in which every thread meets the same group r times must give r times the sums of once, modulo 2^64 — for r around and far
    beyond 4096 / 4 rounds.  (Once is what every other test of this file holds to the oracle.)"""
    s = scene
    e = new_engine(s, s['B'])
    one = np.zeros(eng.SUM_WORDS, np.uint64)
    assert shim.shim_fragment_score_repeat(e._ctx, loss, 1, one.ctypes.data) == 0
    assert one[1:5].all(), "the synthetic groups add nothing to the sums: the test would show nothing"
    if loss == eng.LOSS_FULL:       # link 5's two counts: 256 x 4 samples, of which the target's corner holds link 5 in few if any
        assert one[5 + 3 * 5] >= 512 and one[5 + 3 * 5 + 1] >= 512, "too few mismatches for a field to fill up"
    for r in (1000, 1001, 1023, 1024, 1025, 2001, 4100):
        got = np.zeros(eng.SUM_WORDS, np.uint64)
        assert shim.shim_fragment_score_repeat(e._ctx, loss, r, got.ctypes.data) == 0
        with np.errstate(over='ignore'):
            want = one * np.uint64(r)
        assert np.array_equal(got, want), f"{r} rounds: words {np.nonzero(got != want)[0]} differ"
    e.close()


# ---------------------------------------------------------------- 4. the budget
def test_budget_below_the_count_keeps_nothing(scene, fresh):
    s = scene
    e = new_engine(s, s['B'])
    e.set_fragment_budget(0.02)                               # 20 KiB: the offsets alone are 10 KiB, the groups far more
    for k in range(4):
        assert_same(e.eval(s['cand'], 6, eng.LOSS_DEPTH, want_sums=True), fresh[eng.LOSS_DEPTH, 'B'], f"budget too small, pass {k}")
    assert e.fragment_store_stats() == (0, 0, 0, 0)
    assert e.geometry_cache_stats() == (3, 1)
    e.set_fragment_budget()                                   # the default: the next hit counts again, and keeps
    assert_same(e.eval(s['cand'], 6, eng.LOSS_DEPTH, want_sums=True), fresh[eng.LOSS_DEPTH, 'B'], "default budget")
    builds, served, nbytes, groups = e.fragment_store_stats()
    assert (builds, served) == (1, 1) and groups > 0
    e.set_fragment_budget(nbytes / 2 ** 20)                   # exactly what it takes fits; one byte less does not
    e.eval(s['cand'], 6, eng.LOSS_DEPTH)
    assert e.fragment_store_stats() == (2, 2, nbytes, groups)
    e.set_fragment_budget((nbytes - 1) / 2 ** 20)
    assert_same(e.eval(s['cand'], 6, eng.LOSS_DEPTH, want_sums=True), fresh[eng.LOSS_DEPTH, 'B'], "one byte short")
    assert e.fragment_store_stats() == (2, 2, 0, 0)
    e.close()


# ---------------------------------------------------------------- 5. what drops the kept geometry drops the store
def _drops(s, e):
    other = s['cand'] + 1e-3
    return {
        'other rows': lambda: e.eval(other, 6, eng.LOSS_DEPTH),
        'set_camera, same values': lambda: e.set_camera(s['PV'], s['W'], s['H'], ZNEAR, ZFAR),
        'set_robot': lambda: e.set_robot(s['rb']),
        'set_strategy': lambda: e.set_strategy(e.NO_PARENTS),
        'small eval': lambda: e.eval(s['cand'][:2], 6, eng.LOSS_DEPTH),
        'eval_views': lambda: (e.set_frames(np.asarray([Q_A, Q_B], float), np.stack([s['A']['tq'], s['B']['tq']]),
                                            np.stack([s['A']['full'], s['B']['full']])),
                               e.eval_views(np.stack([s['PV']] * 150), 6, eng.LOSS_DEPTH)),
    }


@pytest.mark.parametrize('what', ['other rows', 'set_camera, same values', 'set_robot', 'set_strategy', 'small eval', 'eval_views'])
def test_what_drops_the_geometry_drops_the_store(scene, fresh, what):
    s, e, loss = scene, scene['e'], eng.LOSS_DEPTH
    e.set_strategy(0)
    give_target(e, s['B'])
    for _ in range(3):
        e.eval(s['cand'], 6, loss)
    f0 = e.fragment_store_stats()
    assert f0[3] > 0, "no store in the first place"
    _drops(s, e)[what]()
    if what in ('set_camera, same values', 'set_robot'):
        give_target(e, s['B'])
    if what != 'other rows':                                  # (those rows have had one pass: no store of theirs either)
        assert e.fragment_store_stats()[2:] == (0, 0), f"{what}: the store is still held"
    mark = e.fragment_store_stats()
    assert_same(e.eval(s['cand'], 6, loss, want_sums=True), fresh[loss, 'B'], f"{what}: the pass that builds the geometry again")
    assert stats_delta(e, mark) == (0, 0) and e.fragment_store_stats()[2:] == (0, 0)
    assert_same(e.eval(s['cand'], 6, loss, want_sums=True), fresh[loss, 'B'], f"{what}: the hit that builds the store again")
    assert stats_delta(e, mark) == (1, 1)
    assert_same(e.eval(s['cand'], 6, loss, want_sums=True), fresh[loss, 'B'], f"{what}: served from the new store")
    assert stats_delta(e, mark) == (1, 2) and e.fragment_store_stats()[2:] == f0[2:]
    e.set_strategy(0)


# ---------------------------------------------------------------- 6. off
def test_strategy_128_scores_as_before_and_the_cache_flag_implies_it(scene, fresh):
    s, e = scene, scene['e']
    for flags, hits in ((e.NO_KEPT_FRAGMENTS, 3), (e.NO_GEOMETRY_CACHE, 0), (e.NO_QUEUE, 3)):      # NO_QUEUE: the build is a queue launch
        e.set_strategy(flags)
        give_target(e, s['B'])
        f0, g0 = e.fragment_store_stats(), e.geometry_cache_stats()
        for k in range(4):
            assert_same(e.eval(s['cand'], 6, eng.LOSS_FULL, want_sums=True), fresh[eng.LOSS_FULL, 'B'], f"strategy {flags}, pass {k}")
        assert stats_delta(e, f0) == (0, 0) and e.fragment_store_stats()[2:] == (0, 0)
        g1 = e.geometry_cache_stats()
        assert (g1[0] - g0[0], g1[1] - g0[1]) == (hits, 4 - hits)
    e.set_strategy(0)
    with pytest.raises(eng.EngineError):
        e.set_strategy(256)
