"""GPU: the loss pass — score_pixel / score_tile and every kernel that calls them — against tests/loss_ref.py on targets built
for its edges (tests/test_loss_refs.py holds the reference and the builders to the oracle on the CPU).

The image of a sampled row is the engine's own rope_render of it; its 23 words come from sums_ref, its error from
geometry_ref.finalize_ref on those words, and the CPU oracle's sums are compared as well.  All other rows are compared between
launch forms.  Every form is one call (two where a pass on kept geometry needs the pass before it); nothing is repeated.

Forms 1-3 run against the target with the all-masks tile, so there tile (0, 0) holds one tq value and the tq edge values are
met in the other touched tiles; forms 4-10 also use the targets without it.
"""
import numpy as np
import pytest

from oracle import camera_ref, oracle as orc
from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR

import geometry_ref as G
import helpers
import loss_ref as R
from test_gpu_geometry_cache import grid
from test_loss_refs import Q0, SIZES, crops_of, edge_targets, rows_about

pytestmark = pytest.mark.gpu

SMALL = (2, 200, 400, 800)             # rows without shared layers: split over 8, 4, 2 and 1 row bands at four tiles (rope_abi.hip)
PICK_SMALL = [0, 1, 57, 199, 200, 333, 399, 512, 700, 799]
PICK_GRID = list(range(7, 320, 37))    # nine rows of the 8 x 8 x 5 grid
LOSSES = (eng.LOSS_DEPTH, eng.LOSS_FULL, eng.LOSS_LOOKUP, eng.LOSS_TSWEEP)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope='module', params=SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def scene(request):
    W, H = request.param
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=4)
    e = eng.Engine(0)
    e.set_robot(rb)
    e.set_camera(PV, W, H, ZNEAR, ZFAR)
    o = orc.Oracle(rb.verts, rb.faces, rb.vtx_off, rb.tri_off, rb.joint_fixed, rb.joint_axes, PV, W, H)
    small = np.concatenate([rows_about(Q0, 4, 7), rows_about(Q0, 796, 8)])      # the first four: the rows the targets are built from
    big = grid(Q0)
    targets = edge_targets([e.render(q, 6) for q in small[:4]], W, H)
    return dict(W=W, H=H, rb=rb, PV=PV, P=intr.gl_projection(ZNEAR, ZFAR), e=e, o=o, small=small, big=big, targets=targets, images={}, refs={})


def image(s, q, n):
    key = (tuple(np.asarray(q, float).tolist()), n)
    if key not in s['images']:
        s['images'][key] = s['e'].render(q, n)
    return s['images'][key]


def reference(s, q, n, loss, ti, crop=None):
    """(23 words, error bits) of row q against target ti — computed once, shared, left alone"""
    key = (tuple(np.asarray(q, float).tolist()), n, loss, ti, tuple(crop) if crop is not None else None)
    if key not in s['refs']:
        t = s['targets'][ti]
        d, ids = image(s, q, n)
        words = R.sums_ref(d, ids, loss, n, t['tq'], t['t32'], t['planes'], crop)
        err, _ = G.finalize_ref(np.array(words, np.uint64), np.zeros(23, np.uint64), loss, n, R.n_pix_of(loss, s['W'], s['H'], crop), t['flags'])
        s['refs'][key] = (np.array(words, np.uint64), _bits(err)[0])
    return s['refs'][key]


def give(e, t):
    e.set_target(t['tq'], t['t32'], t['flags'])
    e.set_target_tsweep(None)


def check_rows(s, cand, pick, n, loss, ti, crop, got, what):
    err, sums, bi, be = got
    t, o = s['targets'][ti], s['o']
    _, o_sums = o.eval(cand[pick], loss, n, t['tq'], t['t32'], crop, t['flags'], threads=8, want_sums=True)
    for j, k in enumerate(pick):
        words, ebits = reference(s, cand[k], n, loss, ti, crop)
        assert np.array_equal(o_sums[j], words), f"{what}: oracle and reference differ on row {k}"
        assert np.array_equal(sums[k], words), f"{what}: row {k}: {[(w, int(sums[k][w]), int(words[w])) for w in range(23) if sums[k][w] != words[w]]}"
        assert _bits(err[k:k + 1])[0] == ebits, f"{what}: error of row {k}"
    assert bi == G.argmin(err) and _bits(be)[0] == _bits(err[bi:bi + 1])[0], f"{what}: argmin"


def same(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: sums differ between launch forms"
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[2] == b[2], f"{what}: errors or argmin differ between launch forms"


# ---------------------------------------------------------------- forms 1-3: batches that are split, or scored in one launch
@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('rows', SMALL)
def test_small_batches(scene, rows, loss):
    """Default: raster_score_kernel<., SPLIT[_GEO]> + score_gtile_kernel over 8 / 4 / 2 / 1 row bands; NO_SPLIT: MODE_SCORE in
    raster_score_kernel; SEPARATE_GEOMETRY: the split after a geometry launch of its own.  Target 1 carries the all-masks tile."""
    s = scene
    e, cand = s['e'], s['small'][:rows]
    pick = [k for k in PICK_SMALL if k < rows]
    n = 6 if rows != 200 else 3
    give(e, s['targets'][1])
    for crop in (crops_of(s['W'], s['H']) if loss == eng.LOSS_LOOKUP else [None]):
        e.set_strategy(0)
        base = e.eval(cand, n, loss, crop=crop, want_sums=True)
        for flag in (e.NO_SPLIT, e.SEPARATE_GEOMETRY):
            e.set_strategy(flag)
            same(base, e.eval(cand, n, loss, crop=crop, want_sums=True), f"{rows} rows loss {loss} crop {crop} strategy {flag}")
        e.set_strategy(0)
        check_rows(s, cand, pick, n, loss, 1, crop, base, f"{rows} rows loss {loss} crop {crop}")


# ---------------------------------------------------------------- forms 4-8: a grid with shared layers
@pytest.mark.parametrize('loss', LOSSES)
def test_grid_with_layers(scene, loss):
    """320 rows under 64 (S, L) pairs: the layer queue and the scoring queue; NO_QUEUE; NO_LAYERS | NO_QUEUE; CLIP_KERNELS; and
    the same grid again after rope_set_target with another edge target — layer_sums_kernel on kept geometry, empty_tile_kernel
    for the new target."""
    s = scene
    e, cand = s['e'], s['big']
    for crop in (crops_of(s['W'], s['H']) if loss == eng.LOSS_LOOKUP else [None]):
        give(e, s['targets'][0])
        e.set_strategy(0)
        base = e.eval(cand, 6, loss, crop=crop, want_sums=True)
        for flag in (e.NO_QUEUE, e.NO_LAYERS | e.NO_QUEUE, e.CLIP_KERNELS):
            e.set_strategy(flag)
            same(base, e.eval(cand, 6, loss, crop=crop, want_sums=True), f"grid loss {loss} crop {crop} strategy {flag}")
        e.set_strategy(0)
        check_rows(s, cand, PICK_GRID, 6, loss, 0, crop, base, f"grid loss {loss} crop {crop}")
        e.eval(cand, 6, loss, crop=crop)                             # builds and keeps the geometry (set_strategy dropped it)
        give(e, s['targets'][1])
        before = e.geometry_cache_stats()
        hit = e.eval(cand, 6, loss, crop=crop, want_sums=True)
        after = e.geometry_cache_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (1, 0), "the pass after rope_set_target did not run on the kept geometry"
        check_rows(s, cand, PICK_GRID, 6, loss, 1, crop, hit, f"kept geometry, loss {loss} crop {crop}")
        e.set_strategy(e.NO_GEOMETRY_CACHE)                          # every row of the hit against a pass that builds everything
        try:
            same(hit, e.eval(cand, 6, loss, crop=crop, want_sums=True), f"kept geometry against a miss, loss {loss} crop {crop}")
        finally:
            e.set_strategy(0)


# ---------------------------------------------------------------- form 9: three frames, three edge targets
@pytest.mark.parametrize('loss', LOSSES)
def test_eval_targets(scene, loss):
    s = scene
    e, ts = s['e'], s['targets']
    cand = np.concatenate([s['big'], s['small'][:10]])
    frame_of = (np.arange(len(cand)) % 3).astype(np.int32)          # interleaved
    pick = PICK_GRID + [320, 321, 325, 329]
    e.set_strategy(0)
    e.set_targets(np.stack([t['tq'] for t in ts]), np.stack([t['t32'] for t in ts]), np.stack([t['flags'] for t in ts]))
    for crop in (crops_of(s['W'], s['H']) if loss == eng.LOSS_LOOKUP else [None]):
        err = e.eval_targets(cand, frame_of, 6, loss, crop)
        for k in pick:
            assert _bits(err[k:k + 1])[0] == reference(s, cand[k], 6, loss, int(frame_of[k]), crop)[1], f"row {k} frame {frame_of[k]} loss {loss} crop {crop}"


# ---------------------------------------------------------------- form 10: the camera-pose path
@pytest.mark.parametrize('K', [2, 342])     # 6 rows: split; 1026 rows: raster_queue_kernel
def test_eval_views(scene, K):
    s = scene
    e, o, ts, P = s['e'], s['o'], s['targets'], s['P']
    rng = np.random.default_rng(19)
    qs = s['small'][:3]
    poses = np.array(DEFAULT_CAMERA_POSE, float) + rng.uniform(-1, 1, (K, 6)) * np.array([.05, .05, .05, .03, .03, .03])
    PV = np.stack([P @ camera_ref.view_of_pose(p) for p in poses])
    views = sorted({0, 1, K - 1})
    imgs = {}
    for k in views:
        d, ids = e.render_batch(qs, 6, PV=np.stack([PV[k]] * 3))
        imgs[k] = [(d[f], ids[f]) for f in range(3)]
    e.set_strategy(0)
    e.set_frames(qs, np.stack([t['tq'] for t in ts]), np.stack([t['t32'] for t in ts]), np.stack([t['planes'] for t in ts]))
    try:
        for loss in (eng.LOSS_DEPTH, eng.LOSS_TSWEEP, eng.LOSS_CAMFULL):
            got = e.eval_views(PV, 6, loss)
            for k in views:
                o.PV = np.ascontiguousarray(PV[k])
                for f, t in enumerate(ts):
                    d, ids = imgs[k][f]
                    words = np.array(R.sums_ref(d, ids, loss, 6, t['tq'], t['t32'], t['planes']), np.uint64)
                    key = o.raster_key(qs[f], 6)
                    want = camera_ref.camfull_sums(*o.resolve(key), t['tq'], t['planes']) if loss == eng.LOSS_CAMFULL else o.sums(key, loss, 6, t['tq'], t['t32'])
                    assert np.array_equal(want, words), f"view {k} frame {f} loss {loss}: oracle and reference differ"
                    assert np.array_equal(got[k, f], words), f"view {k} frame {f} loss {loss}: engine and reference differ"
    finally:
        o.PV = np.ascontiguousarray(s['PV'])


# ---------------------------------------------------------------- the stored table against the live LOOKUP, on an edge target
def test_stored_table(scene):
    """rope_lookup_build + rope_lookup_score (crop_total_kernel, the table's score kernels) take the same float differences as
    score_pixel does for ROPE_LOSS_LOOKUP: against an edge target the table's scores are the live errors' bits on every row, and
    the reference's on the sampled ones — floats of 2^20 and more over undrawn samples included."""
    s = scene
    e, cand = s['e'], s['big']
    e.set_strategy(0)
    give(e, s['targets'][0])
    for crop in crops_of(s['W'], s['H']):
        e.lookup_build(cand, 6, crop)
        scores, bi, be = e.lookup_score(want_scores=True)
        live = e.eval(cand, 6, eng.LOSS_LOOKUP, crop=crop)
        assert np.array_equal(_bits(scores), _bits(live[0])) and bi == live[2] and _bits(be)[0] == _bits(live[3])[0], f"crop {crop}"
        for k in PICK_GRID:
            assert _bits(scores[k:k + 1])[0] == reference(s, cand[k], 6, eng.LOSS_LOOKUP, 0, crop)[1], f"row {k} crop {crop}"
