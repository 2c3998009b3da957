"""CPU: tests/loss_ref.py held to the oracle, on the targets tests/test_gpu_loss_edges.py gives the engine.

sums_ref (one loop over the pixels, from the contract) equals the oracle's sums word for word on the edge targets; the
builders place every kind of value in every tile on drawn and on undrawn samples; the packed count fields of score_tile are wide
enough for the all-masks tile at every launch form; six deliberately wrong variants of sums_ref are told from the right one.
"""
import math

import numpy as np
import pytest

from oracle import camera_ref, oracle as orc

import helpers
import loss_ref as R

Q0 = np.array([0.4, 0.3, 0.8, 0, 0, 0])
SIZES = [(160, 120), (158, 118)]                        # 2 x 2 tiles of 128 x 96, partial on both edges; the second: W % 4 != 0
ALL_MASKS_TILE = (0, 0)


def crops_of(W, H):
    """c0 % 4 = 0, 1, 2, 3 and a crop of one column; borders on the image's last row and column and on the tile seams"""
    return [[18, 108, 16, 152], [3, H - 1, 13, W - 1], [0, 95, 2, 127], [96, H - 2, 127, W - 2], [10, 110, 129, 129]]


def rows_about(q0, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(q0, float) + rng.uniform(-.3, .3, (n, 6)) * np.array([1, 1, 1, .5, .5, .5])


def edge_targets(renders, W, H):
    """Three different edge targets from the renders of the sampled rows: the second carries the all-masks tile"""
    crops = crops_of(W, H)
    out = []
    for seed, tile in ((0, None), (4, ALL_MASKS_TILE), (11, None)):
        tq, c_tq = R.build_tq(renders, seed, tile)
        t32, c_f = R.build_t32(renders, seed, crops)
        planes, c_l = R.build_link_planes(renders, seed)
        out.append(dict(tq=tq, t32=t32, planes=planes, flags=np.array([3] * 6 + [0, 0], np.uint8), counts={**c_tq, **c_f, **c_l}, tile=tile))
    return out


@pytest.fixture(scope='module', params=SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def scene(request):
    W, H = request.param
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=4)
    o = orc.Oracle(rb.verts, rb.faces, rb.vtx_off, rb.tri_off, rb.joint_fixed, rb.joint_axes, PV, W, H)
    cand = rows_about(Q0, 4, 7)
    keys = {n: [o.raster_key(q, n) for q in cand] for n in (3, 6)}
    renders = {n: [o.resolve(k) for k in keys[n]] for n in (3, 6)}
    return dict(W=W, H=H, o=o, cand=cand, keys=keys, renders=renders, targets=edge_targets(renders[6], W, H))


# ------------------------------------------------------------------------------------------------ pixel maths
def test_q32_from_bits_is_the_float64_product_truncated():
    vals = list(R.FLOAT_VALUES.values()) + [np.float32(v) for v in (1, 1.5, 100, 2.0 ** -149, 2.0 ** -126, 2.0 ** 31, 0.1)]
    rng = np.random.default_rng(0)
    vals += list(rng.integers(0, 0x4F800000, 2000).astype(np.uint32).view(np.float32))      # every float in [0, 2^32)
    for v in vals:
        assert R.q32(v) == int(float(v) * 4294967296.0), v               # float32 * 2^32 is exact in float64 below 2^32
    assert R.q32(R.FLOAT_VALUES['below 2^32']) == (1 << 64) - (1 << 40) and R.q32(np.float32(2.0 ** -33)) == 0


def test_camfull_root_is_the_rounded_float64_root_truncated():
    """The contract's root is the float64 one (np.abs(diff) ** .5 of the reference, the oracle's np.sqrt, the kernel's sqrt):
    round_sqrt_f64 rebuilds it from integers and equals math.sqrt; truncated after scaling it equals isqrt(dq << 32) except
    where the rounding lands on the multiple of 2^-16 just above the root — there it is one more.  dq = 2^30 + 1 is such a
    value (its root is 2^15 + 2^-16 - 2^-48...), so isqrt alone would not be the contract."""
    edges = {d for k in range(40) for d in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 < d < 1 << 39}
    edges |= {n * n + d for n in (1, 2, 3, 255, 65535, 65536, 741454) for d in (-1, 0, 1) if 0 < n * n + d < 1 << 39}
    rng = np.random.default_rng(1)
    sample = sorted(edges) + [int(v) for v in rng.integers(1, 1 << 39, 20000)]
    lifted = []
    for dq in sample:
        sig, ex = R.round_sqrt_f64(dq)
        assert math.ldexp(sig, ex) == math.sqrt(dq)
        got, floor_ = R.sqrt_q32(dq), R.sqrt_q32_exact(dq)
        assert got == int(math.sqrt(dq) * 65536.0) and floor_ <= got <= floor_ + 1
        if got != floor_:
            assert got * got > dq << 32 and (got - 1) * (got - 1) <= dq << 32      # the float is the integer just above the root
            lifted.append(dq)
    assert (1 << 30) + 1 in lifted and all(d > 1 << 20 for d in lifted)
    assert len(lifted) < 1e-4 * len(sample) + 8


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_sums(s, k, n, loss, t, crop=None):
    o = s['o']
    if loss == R.LOSS_CAMFULL:
        d, ids = s['renders'][n][k]
        return [int(v) for v in camera_ref.camfull_sums(d, ids, t['tq'], t['planes'])]
    return [int(v) for v in o.sums(s['keys'][n][k], loss, n, t['tq'], t['t32'], crop)]


@pytest.mark.parametrize('n_render', [3, 6])
def test_reference_equals_oracle(scene, n_render):
    s = scene
    W, H = s['W'], s['H']
    for ti, t in enumerate(s['targets']):
        for k in range(len(s['cand']) if ti == 0 else 2):
            d, ids = s['renders'][n_render][k]
            for loss in (R.LOSS_DEPTH, R.LOSS_FULL, R.LOSS_TSWEEP, R.LOSS_CAMFULL):
                got = R.sums_ref(d, ids, loss, n_render, t['tq'], t['t32'], t['planes'])
                want = oracle_sums(s, k, n_render, loss, t)
                if loss == R.LOSS_CAMFULL:
                    # camfull_sums has no n_render: the words of the links that are not rendered are not the contract's
                    want[R.SUM_LINK0 + 3 * n_render:] = [0] * (3 * (6 - n_render))
                assert got == want, f"target {ti} row {k} loss {loss}"
            for crop in crops_of(W, H):
                got = R.sums_ref(d, ids, R.LOSS_LOOKUP, n_render, t32=t['t32'], crop=crop)
                assert got == oracle_sums(s, k, n_render, R.LOSS_LOOKUP, t, crop), f"target {ti} row {k} crop {crop}"


# ------------------------------------------------------------------------------------------------ placement
def test_every_kind_on_drawn_and_undrawn_samples_of_every_tile(scene):
    s = scene
    W, H = s['W'], s['H']
    for t in s['targets']:
        c = t['counts']
        touched = [tile for tile, n in c['named'].items() if n['drawn'] > 0]
        assert len(touched) >= 3, "the sampled rows stay inside one or two tiles"
        for tile in touched:
            named = c['named'][tile]
            assert named['undrawn'] > 0
            for what in ('depth', 'mask', 'float'):
                if what != 'float' and tile == t['tile']:
                    continue                                     # the all-masks tile holds one value
                for kind, (on, off) in c[what]['tiles'][tile].items():
                    assert on >= 1 and off >= 1, f"{what} kind {kind} in tile {tile}: {on} drawn, {off} undrawn"
            for l in range(6):
                for kind, (on, off) in c['tiles'][l]['tiles'][tile].items():
                    assert on >= 1 and off >= 1, f"link {l} kind {kind} in tile {tile}: {on} drawn, {off} undrawn"
            if tile != t['tile']:
                assert min(named['mask, T = 0']) >= 1 and named['mask of another link'] >= 1 and named['mask, nothing drawn'] >= 1
        for l in range(6):                                       # every combination with "this link drawn here"; link 0 on empty pixels
            assert all(on >= 1 and off >= 1 for on, off in c['link'][l].values()), f"link {l}: {c['link'][l]}"
        for what, names in (('depth', R.DEPTH_KINDS), ('mask', range(64)), ('float', R.FLOAT_KINDS)):
            for line, kinds in c[what]['lines'].items():
                short = line in ('crop 4 top', 'crop 4 bottom')  # the one-column crop: its top and bottom are one sample each
                if t['tile'] is None or what == 'float':
                    assert short or kinds == set(names), f"{what} kinds along {line}: {sorted(set(names) - kinds)} missing"
        tile = t['tile']
        if tile is not None:
            sub = t['tq'][tile[0] * 96:(tile[0] + 1) * 96, tile[1] * 128:(tile[1] + 1) * 128]
            assert sub.shape == (96, 128) and (sub == np.uint64(R.T_MAX | (0x3E << 40))).all()


# ------------------------------------------------------------------------------------------------ field widths
def test_packed_count_fields_hold_the_all_masks_tile():
    """Every sample of the all-masks tile mismatches on every link, in the tile and (masks without a render) in its base: a
    thread's count per link is the number of samples it meets.  768 threads over a whole tile (raster_tile, layer_sums_kernel,
    empty_tile_kernel) and 256 threads over 96 / bands rows (score_gtile_kernel) must stay below the 10-bit fields of
    ROPE_LOSS_CAMFULL, so below the 12-bit ones of ROPE_LOSS_FULL too.  The mapping, the thread counts, the block widths 2 / 4 / 4
    and the band counts are restated here from rope_lossmath.h, rope_kernels.hip and rope_abi.hip: this is arithmetic on a copy, no guard on the
    kernels — whoever changes the mapping there has to change it in loss_ref.py as well for the test to say anything."""
    live = np.ones((R.TILE_H, R.TILE_W), bool)
    most = {'raster_tile': R.samples_per_thread(768, 0, 95, 2, live), 'layer_sums': R.samples_per_thread(768, 0, 95, 4, live),
            'empty_tile': R.samples_per_thread_plain(768, live)}
    for bands in R.band_counts():
        rows = R.TILE_H // bands
        most[f'gtile/{bands}'] = max(R.samples_per_thread(256, b * rows, b * rows + rows - 1, 4, live) for b in range(bands))
    assert most['raster_tile'] == most['layer_sums'] == most['empty_tile'] == 16 and most['gtile/1'] == 48 and most['gtile/8'] == 8
    assert all(v < 1024 for v in most.values()), most


# ------------------------------------------------------------------------------------------------ wrong from right
def test_six_wrong_variants_are_told_from_the_right_sums(scene):
    s = scene
    t = s['targets'][1]                                          # the one with the all-masks tile
    d, ids = s['renders'][6][0]
    crop = crops_of(s['W'], s['H'])[1]
    cases = {'ab term dropped': (R.LOSS_DEPTH, {}), 'depth masked to 38 bits': (R.LOSS_DEPTH, {}), '9-bit link fields': (R.LOSS_FULL, {}),
             'T = 0 mask pixels skipped': (R.LOSS_FULL, {}), 'link 0 as the other links': (R.LOSS_CAMFULL, {}),
             "crop's last column ignored": (R.LOSS_LOOKUP, {'crop': crop})}
    assert set(cases) == set(R.WRONG)
    for wrong, (loss, kw) in cases.items():
        right = R.sums_ref(d, ids, loss, 6, t['tq'], t['t32'], t['planes'], **kw)
        assert R.sums_ref(d, ids, loss, 6, t['tq'], t['t32'], t['planes'], wrong=(wrong,), **kw) != right, wrong
