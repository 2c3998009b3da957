"""The first and the last kernels of every evaluation pass (rope_kernels.hip: fk_mvp, bounds, fk_bounds; finalize_only,
finalize_frames, finalize_argmin), the raster queue's builder (score_queue) and a kept grid's clearing (clear_pass), each launched on
its own through tests/geometry_shim.hip on inputs the test supplies — bit for bit against tests/geometry_ref.py (box_exact,
finalize_ref, queue_ref, clear_pass_ref) and the oracle's link matrices, and by inequality only against the float64 projection
(box_bounds64, whose slack is derived there).  tests/test_geometry_refs.py shows on the CPU that the inputs reach the
edges they are named for and that they tell the references from deliberately wrong ones.

Every output buffer lies between guard bytes and starts out as 0xA5 bytes (table_child.Out)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import geometry_ref as R
import helpers
import table_child as K

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
PARITY_POSES = [[0, 0, 0, 0, 0, 0], [0.3, 0.4, 0.5, 0, 0, 0], [-0.7, -0.9, 2.2, 0, 0, 0], [1.5, 1.2, -0.8, 0.5, -0.7, 0.3],
                [0.8, 0.1, 1.0, -2.0, 1.5, 3.0]]                                  # tests/test_gpu_parity.py's
NEAR_CAMERAS = [([0.3, -0.12, 0.77, 0, 0.2, 0.3], [0, 0, 0, 0, 0, 0]), ([0.2, -0.1, 0.6, 0.3, 0.1, -0.4], [0.5, 0.4, 0.6, 0.2, 0.3, 0.1])]  # test_clipping_kernels_...'s


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    from rope_s3d_amd import build
    csrc = os.path.dirname(build.LIB_PATH)
    out = str(tmp_path_factory.mktemp('geometry_shim') / 'libgeometry_shim.so')
    subprocess.check_call([build.shutil.which('hipcc') or '/opt/rocm/bin/hipcc'] + build.HIPCC_FLAGS +
                          [os.path.join(ROOT, 'tests', 'geometry_shim.hip'), '-L' + csrc, '-lrope_hip', '-Wl,-rpath,' + csrc, '-o', out])
    torch.cuda.init()                                   # one HIP runtime in the process: torch's, loaded first
    lib = C.CDLL(out)
    vp, i32 = C.c_void_p, C.c_int
    lib.shim_constant.argtypes = [i32]
    lib.shim_fk.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]
    lib.shim_bounds.argtypes = [i32] * 4 + [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    lib.shim_fk_bounds.argtypes = [i32] * 4 + [vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.shim_finalize.argtypes = [vp, vp, i32, i32, i32, C.c_double, vp, vp, vp]
    lib.shim_finalize_frames.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_double, vp, vp]
    lib.shim_score_queue.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, C.c_ulonglong, vp, vp, vp]
    lib.shim_clear_pass.argtypes = [vp, i32, vp, vp]
    k = R.constants()
    for i, name in enumerate(R.SHIM_CONSTANTS):          # what the references read out of the headers is what the library was built with
        assert lib.shim_constant(i) == k[name], (name, lib.shim_constant(i), k[name])
    assert lib.shim_constant(len(R.SHIM_CONSTANTS)) == -1
    return lib


def ptr(t):
    return t.data_ptr() if t is not None else None


def filled(name, n, dtype, host=None):
    """An Out of n elements; with `host`, holding its values instead of guard bytes."""
    o = K.Out(name, n, dtype)
    if host is not None:
        raw = np.ascontiguousarray(host, dtype).reshape(-1).view(np.uint8)
        assert raw.size == o.nbytes
        o.t[K.PAD:K.PAD + o.nbytes] = torch.from_numpy(raw.copy()).cuda()
    return o


def guard_words(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, K.GUARD, np.uint8).view(dtype)


def run_fk(shim, rb, cand, n_render, PV, view_of, fp, extra_rows=3):
    """launch_fk on buffers of len(cand) + extra_rows rows -> dict of host arrays, one row per allocated row."""
    k = R.constants()
    n, rows = len(cand), len(cand) + extra_rows
    words, n_tiles = R.mask_words_of(fp), fp[2] * fp[3]
    d_cand, d_jf, d_ja, d_pv = K.dev(np.asarray(cand, np.float64)), K.dev(rb.joint_fixed.astype(np.float64)), K.dev(rb.joint_axes.astype(np.float64)), K.dev(np.asarray(PV, np.float64))
    d_view = K.dev(np.asarray(view_of, np.int32)) if view_of is not None else None
    o = dict(mvp=K.Out('mvp', rows * k['MAX_LINKS'] * 16, np.float32), sums=K.Out('sums', rows * k['SUM_WORDS'], np.uint64),
             mask_lo=K.Out('mask_lo', rows * words, np.uint32), mask_hi=K.Out('mask_hi', rows * words, np.uint32),
             counters=K.Out('queue_counters', 2 * k['QUEUE_COUNTERS'] + 4, np.int32), tris=K.Out('tile_tris', rows * n_tiles, np.uint32),
             tris_lo=K.Out('tile_tris_lo', rows * n_tiles, np.uint32))
    rc = shim.shim_fk(ptr(d_cand), n, n_render, ptr(d_jf), ptr(d_ja), ptr(d_pv), ptr(d_view), o['mvp'].ptr, o['sums'].ptr, o['mask_lo'].ptr,
                      o['mask_hi'].ptr, words, o['counters'].ptr, o['tris'].ptr, o['tris_lo'].ptr, n_tiles, None)
    assert rc == 0, rc
    h = {key: v.host() for key, v in o.items()}
    return dict(mvp=h['mvp'].reshape(rows, k['MAX_LINKS'], 16), sums=h['sums'].reshape(rows, -1), mask_lo=h['mask_lo'].reshape(rows, words),
                mask_hi=h['mask_hi'].reshape(rows, words), counters=h['counters'], tris=h['tris'].reshape(rows, n_tiles),
                tris_lo=h['tris_lo'].reshape(rows, n_tiles))


def run_bounds(shim, fp, header, aabb, mvp, n_render, n_shared, lo_first=0, layers=None, weights=True):
    """launch_bounds on cleared masks and weights (what launch_fk leaves) -> boxes (C, M, 4), mask_lo, mask_hi (C, words), tris, tris_lo
    (C, n_tiles) or None."""
    n, M = len(mvp), len(header)
    words, n_tiles = R.mask_words_of(fp), fp[2] * fp[3]
    assert words <= R.constants()['MAX_MASK_WORDS'] and n_tiles <= R.constants()['QUEUE_WEIGHT_TILES'] and M <= R.constants()['MAX_MESHLETS']
    d_h, d_a, d_m = K.dev(header.astype(np.uint32)), K.dev(aabb.astype(np.float32)), K.dev(np.asarray(mvp, np.float32))
    d_of, d_rep = (K.dev(np.array(layers[0], np.int32)), K.dev(np.array(layers[1], np.int32))) if layers else (None, None)
    boxes = K.Out('bounds', n * M * 4, np.int16)
    lo, hi = filled('mask_lo', n * words, np.uint32, np.zeros(n * words)), filled('mask_hi', n * words, np.uint32, np.zeros(n * words))
    tris = filled('tile_tris', n * n_tiles, np.uint32, np.zeros(n * n_tiles)) if weights else None
    tris_lo = filled('tile_tris_lo', n * n_tiles, np.uint32, np.zeros(n * n_tiles)) if weights else None
    rc = shim.shim_bounds(*fp, ptr(d_h), ptr(d_a), M, n, n_render, n_shared, ptr(d_m), boxes.ptr, lo.ptr, hi.ptr, words, ptr(d_of), ptr(d_rep),
                          tris.ptr if weights else None, tris_lo.ptr if weights else None, lo_first, None)
    assert rc == 0, rc
    return (boxes.host().reshape(n, M, 4), lo.host().reshape(n, words), hi.host().reshape(n, words),
            tris.host().reshape(n, n_tiles) if weights else None, tris_lo.host().reshape(n, n_tiles) if weights else None)


def run_fk_bounds(shim, rb, fp, header, aabb, cand, n_render, n_shared, PV, view_of=None):
    k = R.constants()
    n, M = len(cand), len(header)
    words = R.mask_words_of(fp)
    assert words <= k['MAX_MASK_WORDS'] and M <= k['MAX_MESHLETS']
    keep = [K.dev(np.asarray(cand, np.float64)), K.dev(rb.joint_fixed.astype(np.float64)), K.dev(rb.joint_axes.astype(np.float64)),
            K.dev(np.asarray(PV, np.float64)), K.dev(header.astype(np.uint32)), K.dev(aabb.astype(np.float32))]
    d_view = K.dev(np.asarray(view_of, np.int32)) if view_of is not None else None
    mvp, boxes = K.Out('mvp', n * k['MAX_LINKS'] * 16, np.float32), K.Out('bounds', n * M * 4, np.int16)
    sums, lo, hi = K.Out('sums', n * k['SUM_WORDS'], np.uint64), K.Out('mask_lo', n * words, np.uint32), K.Out('mask_hi', n * words, np.uint32)
    rc = shim.shim_fk_bounds(*fp, ptr(keep[4]), ptr(keep[5]), M, ptr(keep[0]), n, n_render, n_shared, ptr(keep[1]), ptr(keep[2]), ptr(keep[3]),
                             ptr(d_view), mvp.ptr, boxes.ptr, sums.ptr, lo.ptr, hi.ptr, words, None)
    assert rc == 0, rc
    return (mvp.host().reshape(n, k['MAX_LINKS'], 16), boxes.host().reshape(n, M, 4), sums.host().reshape(n, -1), lo.host().reshape(n, words),
            hi.host().reshape(n, words))


def first_difference(got, want, what, names=None):
    """'' when equal, else the first few differing elements by index with both values."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    return '' if not len(bad) else f"{what}: {len(bad)} differ, first " + '; '.join(
        f"{tuple(int(v) for v in i)}{' [' + names[int(i[0])] + ']' if names else ''}: got {got[tuple(i)]!r}, want {want[tuple(i)]!r}" for i in bad[:4])


# ------------------------------------------------------------------------------------------------ launch_fk
@pytest.fixture(scope='module')
def robot_scene():
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color')
    _, PV2 = helpers.camera('640_480_color', pose=NEAR_CAMERAS[0][0])
    return rb, intr, PV, PV2, helpers.make_oracle(rb, intr, PV), helpers.make_oracle(rb, intr, PV2)


def some_poses(rb, n, seed):
    lim = rb.joint_limits
    q = np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (n, 6))
    q[:len(PARITY_POSES)] = PARITY_POSES[:n]
    return q


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_fk_clears_its_rows_and_nothing_else(shim, robot_scene, n):
    rb, intr, PV = robot_scene[:3]
    k = R.constants()
    fp = R.frame(640, 480)
    got = run_fk(shim, rb, some_poses(rb, n, 1), 6, PV, None, fp)
    for key in ('sums', 'mask_lo', 'mask_hi', 'tris', 'tris_lo'):
        rows = np.flatnonzero(got[key][:n].any(axis=1))
        assert not len(rows), f"{key}: rows {rows[:5]} of {n} not cleared, e.g. {got[key][rows[0]][:4]}"
        rest = got[key][n:]
        assert (rest == guard_words(1, rest.dtype)[0]).all(), f"{key}: written past row {n} (or past mask_words / n_tiles of the last row)"
    assert not got['counters'][:2 * k['QUEUE_COUNTERS']].any(), got['counters']
    assert (got['counters'][2 * k['QUEUE_COUNTERS']:] == guard_words(1, np.int32)[0]).all(), got['counters']
    assert (got['mvp'][n:].view(np.uint32) == guard_words(1, np.uint32)[0]).all(), "link matrices written past the last candidate"


@pytest.mark.parametrize('n_render', [4, 6])
@pytest.mark.parametrize('views', [False, True])
def test_fk_matrices_equal_the_oracle(shim, robot_scene, n_render, views):
    rb, intr, PV, PV2, o1, o2 = robot_scene
    k = R.constants()
    q = some_poses(rb, 9, 2)
    view_of = (np.arange(len(q)) % 2).astype(np.int32) if views else None         # two views, interleaved
    got = run_fk(shim, rb, q, n_render, np.stack([PV, PV2]) if views else PV, view_of, R.frame(640, 480))
    for i in range(len(q)):
        want = (o2 if views and view_of[i] else o1).mvp(q[i], n_render)
        msg = first_difference(got['mvp'][i, :n_render].view(np.uint32), want.view(np.uint32), f"candidate {i} (link, element)")
        assert not msg, msg
    assert (got['mvp'][:, n_render:].view(np.uint32) == guard_words(1, np.uint32)[0]).all(), "matrices of links that are not rendered were written"


# ------------------------------------------------------------------------------------------------ launch_bounds
def check_against_exact(g, boxes, lo, hi, tris, tris_lo, who):
    for c in range(g['C']):
        w = g['want'][c]
        msgs = [first_difference(boxes[c], w['boxes'], f"{who} candidate {c} box (meshlet, word)", g['names']),
                first_difference(lo[c], w['mask_lo'], f"{who} candidate {c} mask_lo word"), first_difference(hi[c], w['mask_hi'], f"{who} candidate {c} mask_hi word")]
        if tris is not None:
            msgs += [first_difference(tris[c], w['tris'], f"{who} candidate {c} tile_tris tile"), first_difference(tris_lo[c], w['tris_lo'], f"{who} candidate {c} tile_tris_lo tile")]
        assert not any(msgs), '\n'.join(m for m in msgs if m)


@pytest.mark.parametrize('case', R.GEOMETRY_CASES, ids=lambda c: '-'.join(str(int(v)) for v in c))
def test_bounds_equal_box_exact(shim, case):
    g = R.geometry_case(*case)
    layers = (R.LAYER_OF[:g['C']], R.LAYER_REP) if g['layers'] else None
    got = run_bounds(shim, g['fp'], g['header'], g['aabb'], g['mvp'], g['n_render'], g['n_shared'], g['lo_first'], layers)
    check_against_exact(g, *got, 'launch_bounds')
    for c in range(g['C']):                             # and the promises in float64 hold for what the kernel stored
        skip = g['layers'] and g['n_shared'] > 0 and R.LAYER_REP[R.LAYER_OF[c]] != c
        bad = R.check_boxes(g['fp'], got[0][c], g['b64'][c], f"candidate {c} ", (g['header'][:, 7] < g['n_shared']) if skip else None)
        assert not bad, '\n'.join(bad[:8])
    no_weights = run_bounds(shim, g['fp'], g['header'], g['aabb'], g['mvp'], g['n_render'], g['n_shared'], g['lo_first'], layers, weights=False)
    check_against_exact(g, *no_weights, 'launch_bounds without weights')


# ------------------------------------------------------------------------------------------------ launch_fk_bounds, the real robot
def robot_candidates(rb):
    """(camera pose, candidates) of the parity poses under the default camera and of the two near-camera scenes."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    out = [(DEFAULT_CAMERA_POSE, 1, np.array(PARITY_POSES, np.float64))]
    for pose, q0 in NEAR_CAMERAS:
        out.append((pose, 2, np.array([q0, np.array(q0) + [0.2, -0.15, 0.3, 0, 0, 0], np.array(q0) + [-0.25, 0.2, -0.4, 0, 0, 0]], np.float64)))
    return out


@pytest.mark.parametrize('scene', [0, 1, 2])
@pytest.mark.parametrize('n_render,n_shared', [(6, 3), (4, 0)])
def test_fk_bounds_equal_fk_then_bounds_and_hold_every_vertex_of_the_real_robot(shim, scene, n_render, n_shared):
    rb = helpers.robot()
    pose, ds, cand = robot_candidates(rb)[scene]
    intr, PV = helpers.camera('640_480_color', ds=ds, pose=pose)
    fp = R.frame(intr.width, intr.height)
    header, aabb, verts = R.robot_tables(rb)
    assert len(header) > 1024                           # the 1024-thread stride of fk_bounds_kernel wraps
    fk = run_fk(shim, rb, cand, n_render, PV, None, fp, extra_rows=0)
    boxes, lo, hi, _, _ = run_bounds(shim, fp, header, aabb, fk['mvp'], n_render, n_shared)
    mvp1, boxes1, sums1, lo1, hi1 = run_fk_bounds(shim, rb, fp, header, aabb, cand, n_render, n_shared, PV)
    msgs = [first_difference(mvp1[:, :n_render].view(np.uint32), fk['mvp'][:, :n_render].view(np.uint32), 'fk_bounds against fk: matrix (candidate, link, element)'),
            first_difference(boxes1, boxes, 'fk_bounds against bounds: box (candidate, meshlet, word)'),
            first_difference(lo1, lo, 'fk_bounds against bounds: mask_lo (candidate, word)'), first_difference(hi1, hi, 'fk_bounds against bounds: mask_hi (candidate, word)')]
    assert not any(msgs), '\n'.join(m for m in msgs if m)
    assert not sums1.any(), "fk_bounds does not clear the sums"
    o = helpers.make_oracle(rb, intr, PV)
    seen_near = on_screen = 0
    for c in range(len(cand)):
        assert np.array_equal(fk['mvp'][c, :n_render].view(np.uint32), o.mvp(cand[c], n_render).view(np.uint32)), c
        want = R.box_exact(fp, header, aabb, fk['mvp'][c], n_render, n_shared)
        msgs = [first_difference(boxes[c], want['boxes'], f"candidate {c} box (meshlet, word)"), first_difference(lo[c], want['mask_lo'], f"candidate {c} mask_lo word"),
                first_difference(hi[c], want['mask_hi'], f"candidate {c} mask_hi word")]
        assert not any(msgs), '\n'.join(m for m in msgs if m)
        bad = R.check_boxes(fp, boxes[c], R.box_bounds64(fp, header, aabb, fk['mvp'][c], n_render), f"candidate {c} ")
        bad += R.check_masks(fp, boxes[c], header, n_shared, lo[c], hi[c], f"candidate {c} ")
        more, seen = R.check_vertices(fp, boxes[c], header, verts, fk['mvp'][c], n_render, n_shared, lo[c], hi[c], f"candidate {c} ")
        assert not bad + more, '\n'.join((bad + more)[:8])
        seen_near, on_screen = seen_near + seen['near'], on_screen + seen['on_screen']
    assert scene == 0 or seen_near, "the near-camera scenes put no vertex behind the near plane"
    assert scene != 0 or on_screen > 1000 * len(cand), "the default camera sees the robot"


@pytest.mark.parametrize('case', [c for c in R.GEOMETRY_CASES if c[2] in (1, 257, 1025)][:4], ids=lambda c: '-'.join(str(int(v)) for v in c))
def test_fk_bounds_on_synthetic_tables_with_two_views(shim, robot_scene, case):
    """The synthetic tables under the real robot's link matrices (whatever they put on screen), candidates of two views interleaved:
    the fused kernel against the two separate ones."""
    rb, intr, PV, PV2 = robot_scene[:4]
    W, H, M, n, n_render, n_shared = case[:6]
    fp = R.frame(W, H)
    _, header, aabb = R.meshlet_table(W, H, M)
    cand = some_poses(rb, 3, 4)
    view_of = np.array([1, 0, 1], np.int32)
    fk = run_fk(shim, rb, cand, n_render, np.stack([PV, PV2]), view_of, fp, extra_rows=0)
    boxes, lo, hi, _, _ = run_bounds(shim, fp, header, aabb, fk['mvp'], n_render, n_shared)
    mvp1, boxes1, sums1, lo1, hi1 = run_fk_bounds(shim, rb, fp, header, aabb, cand, n_render, n_shared, np.stack([PV, PV2]), view_of)
    msgs = [first_difference(mvp1[:, :n_render].view(np.uint32), fk['mvp'][:, :n_render].view(np.uint32), 'matrix (candidate, link, element)'),
            first_difference(boxes1, boxes, 'box (candidate, meshlet, word)'), first_difference(lo1, lo, 'mask_lo (candidate, word)'),
            first_difference(hi1, hi, 'mask_hi (candidate, word)')]
    assert not any(msgs), '\n'.join(m for m in msgs if m)
    assert not sums1.any()


# ------------------------------------------------------------------------------------------------ finalize
def run_finalize(shim, f):
    k = R.constants()
    sums = filled('sums', f['C'] * k['SUM_WORDS'], np.uint64, f['sums'])
    d_total = K.dev(f['total'])
    err = K.Out('err', f['C'] + 2, np.float64)
    flags = np.ascontiguousarray(f['flags'], np.uint8)
    rc = shim.shim_finalize(sums.ptr, ptr(d_total), f['C'], f['loss'], f['n_render'], f['n_pix'], flags.ctypes.data_as(C.c_void_p), err.ptr, None)
    assert rc == 0, rc
    return err.host(), sums.host().reshape(f['C'], -1)


@pytest.mark.parametrize('n_rows', R.finalize_sizes()[0])
def test_finalize_errors_words_and_argmin(shim, n_rows):
    ran = 0
    for args in R.finalize_cases():
        if args[0] != n_rows:
            continue
        f = R.finalize_case(*args)
        err, words = run_finalize(shim, f)
        msgs = [first_difference(R.bits(err[:n_rows]), R.bits(f['err']), f"{f['name']} error bits of row"),
                first_difference(words, f['words'], f"{f['name']} sums written back (row, word)")]
        assert not any(msgs), '\n'.join(m for m in msgs if m)
        assert err[n_rows + 1] == f['best'] and R.bits(err[n_rows]) == R.bits(f['err'][f['best']]), \
            (f['name'], 'best index', err[n_rows + 1], 'want', f['best'], 'best error', err[n_rows], 'want', f['err'][f['best']])
        ran += 1
    assert ran >= 8


@pytest.mark.parametrize('n_rows', R.FRAME_SIZES)
def test_finalize_frames_rows_of_mixed_frames(shim, n_rows):
    k = R.constants()
    for loss, n_render in ((k['LOSS_FULL'], 6), (k['LOSS_FULL'], 4), (k['LOSS_DEPTH'], 6), (k['LOSS_LOOKUP'], 6), (k['LOSS_TSWEEP'], 6)):
        f = R.finalize_frames_case(n_rows, loss, n_render)
        sums = filled('sums', n_rows * k['SUM_WORDS'], np.uint64, f['sums'])
        d_totals, d_of, d_flags = K.dev(f['totals']), K.dev(f['frame_of']), K.dev(f['flags'])
        err = K.Out('err', n_rows, np.float64)
        rc = shim.shim_finalize_frames(sums.ptr, ptr(d_totals), ptr(d_of), ptr(d_flags), n_rows, loss, n_render, f['n_pix'], err.ptr, None)
        assert rc == 0, rc
        msgs = [first_difference(R.bits(err.host()), R.bits(f['err']), f"loss {loss} n_render {n_render}: error bits of row"),
                first_difference(sums.host().reshape(n_rows, -1), f['words'], f"loss {loss} n_render {n_render}: sums written back (row, word)")]
        assert not any(msgs), '\n'.join(m for m in msgs if m)


# ------------------------------------------------------------------------------------------------ launch_score_queue
@pytest.mark.parametrize('size', R.QUEUE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize('form', R.QUEUE_FORMS, ids=lambda f: f.replace(' ', '-'))
def test_score_queue_equals_the_reference(shim, form, size):
    k = R.constants()
    n_cls, n_ctr = k['QUEUE_CLASSES'], k['QUEUE_COUNTERS']
    c = R.queue_case(form, *size)
    rows, n_tiles, segment, want = c['rows'], c['n_tiles'], c['segment'], c['want']
    assert c['words'] <= k['MAX_MASK_WORDS'] and n_tiles <= k['QUEUE_WEIGHT_TILES'] and rows <= 65535 and max(want['counts']) <= (segment or c['n_items'])
    d = {key: (K.dev(c[key]) if c[key] is not None else None) for key in ('mask_lo', 'mask_hi', 'weights', 'layer_of', 'layer_rep', 'cand_of_row')}
    layer_sums = filled('layer_sums', c['layer_sums'].size, np.uint64, c['layer_sums']) if c['layer_sums'] is not None else None
    sums = filled('sums', c['sums'].size, np.uint64, c['sums'])
    items = K.Out('items', c['n_items'], np.uint32)
    counters = K.Out('counters', n_ctr + 4, np.int32)
    counters.t[K.PAD:K.PAD + 4 * n_ctr] = 0
    rc = shim.shim_score_queue(ptr(d['mask_lo']), ptr(d['mask_hi']), c['words'], ptr(d['layer_of']), ptr(d['layer_rep']),
                               layer_sums.ptr if layer_sums else None, ptr(d['cand_of_row']), sums.ptr, rows, n_tiles, items.ptr, segment, counters.ptr,
                               ptr(d['weights']), None)
    assert rc == 0, rc
    got_ctr, got_items, got_sums = counters.host(), items.host(), sums.host().reshape(c['sums'].shape)
    guard = guard_words(1, np.uint32)[0]
    assert got_ctr[2:n_ctr].tolist() == want['counts'], (got_ctr, want['counts'])
    assert not got_ctr[:2].any() and (got_ctr[n_ctr:] == guard_words(1, np.int32)[0]).all(), got_ctr
    written = np.zeros(len(got_items), bool)
    for cls, (n, ref) in enumerate(zip(want['counts'], want['items'])):
        seg = got_items[cls * segment:cls * segment + n]
        written[cls * segment:cls * segment + n] = True
        msg = first_difference(np.sort(seg), np.array(ref, np.uint32), f"class {cls} of {want['counts']}, sorted items (row | tile << 16)")
        assert not msg, msg
    stray = np.flatnonzero(~written & (got_items != guard))
    assert not len(stray), f"item words written past the counts {want['counts']} (segment {segment}): {stray[:8]} hold {got_items[stray[:8]]}"
    msg = first_difference(got_sums, want['sums'], 'sums (row, word)')
    assert not msg, msg
    assert np.array_equal(got_sums[rows:], c['sums'][rows:]) and (c['base'] == 'layers' or np.array_equal(got_sums, c['sums']))
    if layer_sums:
        assert np.array_equal(layer_sums.host(), c['layer_sums'].reshape(-1)), "the layers' stored sums were written"


# ------------------------------------------------------------------------------------------------ launch_clear_pass
@pytest.mark.parametrize('with_counters', [True, False])
@pytest.mark.parametrize('n', R.CLEAR_SIZES)
def test_clear_pass_clears_its_words_and_nothing_else(shim, n, with_counters):
    k = R.constants()
    n_words, n_ctr = k['SUM_WORDS'], 2 * k['QUEUE_COUNTERS']
    sums, counters = K.Out('sums', (n + 2) * n_words, np.uint64), K.Out('queue_counters', n_ctr + 4, np.int32)
    before = sums.host(), counters.host()
    rc = shim.shim_clear_pass(sums.ptr, n, counters.ptr if with_counters else None, None)
    assert rc == 0, rc
    want_sums, want_ctr = R.clear_pass_ref(before[0], n, before[1] if with_counters else None)
    got_sums, got_ctr = sums.host(), counters.host()
    msg = first_difference(got_sums, want_sums, f"sums word (cleared: the first {n * n_words})")
    assert not msg, msg
    assert not got_sums[:n * n_words].any() and (got_sums[n * n_words:] == guard_words(1, np.uint64)[0]).all()
    msg = first_difference(got_ctr, want_ctr if with_counters else before[1], 'queue counter')
    assert not msg, msg
    assert (got_ctr[n_ctr:] == guard_words(1, np.int32)[0]).all() and (not got_ctr[:n_ctr].any() if with_counters else (got_ctr == guard_words(1, np.int32)[0]).all())
