"""tests/geometry_ref.py on the CPU: the exact float32 fma, every input builder reaches the edge it is named for, box_exact keeps the
promises of box_bounds64 on every input, and the inputs tell box_exact / finalize_ref / argmin / queue_ref / clear_pass_ref from
deliberately wrong versions of themselves.  tests/test_gpu_geometry_kernels.py then holds the kernels to the same references on the same inputs."""
import numpy as np
import pytest

import geometry_ref as R
import helpers

F32 = np.float32
K = R.constants()
CASE_IDS = ['-'.join(str(int(v)) for v in c) for c in R.GEOMETRY_CASES]


def test_fmaf_rounds_once():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(400).astype(F32), rng.standard_normal(400).astype(F32)
    c = (-(a.astype(np.float64) * b)).astype(F32) * F32(1 + 2.0 ** -12)          # cancellation: the low bits of the product decide
    a = np.concatenate([a, F32([1 + 2.0 ** -12, 1 + 2.0 ** -12, 3.0e-20, 1.0e-30])])
    b = np.concatenate([b, F32([1 + 2.0 ** -12, 1 + 2.0 ** -12, 2.0e-20, 1.0e-10])])
    c = np.concatenate([c, F32([2.0 ** -60, -2.0 ** -60, 1.0e-45, 1.0e-45])])     # a float32 tie that a 53-bit sum cannot see past; subnormals
    got = R.fmaf(a, b, c)
    want = np.array([R.fmaf_fraction(x, y, z) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    twice = (a.astype(np.float64) * b + c).astype(F32)
    assert twice[400] != want[400] and twice[401] == want[401], "the adversarial operands do not tell one rounding from two"


def test_constants_come_from_the_headers():
    assert K['SUM_WORDS'] == R.SUM_LINK0 + 3 * K['MAX_LINKS'] and K['TILE_W'] > 0 and K['TILE_H'] > 0
    sizes, seams = R.finalize_sizes()
    assert len(seams) == 3 and all(s in sizes and s + 1 in sizes for s in seams) and {1, 255, 256, 257, 1025} <= set(sizes)


@pytest.mark.parametrize('W,H', [(128, 96), (160, 120), (640, 480), (1280, 720)])
def test_edge_rows_reach_their_edges(W, H):
    fp = R.frame(W, H)
    TW, TH, px = K['TILE_W'], K['TILE_H'], F32(K['COMPACT_PX'])
    assert fp[2:] == {(128, 96): (1, 1), (160, 120): (2, 2), (640, 480): (5, 5), (1280, 720): (10, 8)}[(W, H)] or (TW, TH) != (128, 96)
    rows = R.edge_rows(W, H)
    hdr = np.zeros((len(rows), 8), np.uint32)
    hdr[:, 6] = 1 << 16
    hdr[:, 7] = [link for _, link, _ in rows]
    rec = R.box_exact(fp, hdr, np.stack([r for _, _, r in rows]), R.link_matrices(fp, 0), 6, 3)
    seen = set()
    tile_of = lambda x, y: ((H - 1 - y) // TH) * fp[2] + x // TW
    for m, (name, link, _) in enumerate(rows):
        x0, x1, y0, y1, compact, near = R.unpack(rec['boxes'][m])
        where = (name, (x0, x1, y0, y1), compact, near)
        word = name.split()
        if name.startswith('x1 on the last column before seam'):
            s = int(word[-1]); assert x1 == s - 1 and tile_of(x1, y0) + 1 == tile_of(s, y0), where
            if tile_of(s, y0) % 32 == 0:
                seen.add(f'word seam {tile_of(s, y0) // 32}')
                assert rec['boxes'][m + 1][1] == s, where                  # its neighbour, one past, sets bit 0 of the next word
        elif name.startswith('x1 one past seam'):
            assert x1 == int(word[-1]), where
        elif name.startswith('x0 on seam'):
            assert x0 == int(word[-1]), where
        elif name.startswith('x0 one before seam'):
            assert x0 == int(word[-1]) - 1, where
        elif name.startswith('y0 on the lowest row above seam'):
            s = int(word[-1]); assert y0 == s and (H - 1 - s) % TH == TH - 1, where
        elif name.startswith('y0 one below seam'):
            s = int(word[-1]); assert y0 == s - 1 and (H - 1 - y0) // TH == (H - 1 - s) // TH + 1, where
        elif name.startswith('y1 on the highest row below seam'):
            assert y1 == int(word[-1]) - 1, where
        elif name.startswith('y1 one above seam'):
            assert y1 == int(word[-1]), where
        elif name.startswith('clamped at column 0'):
            assert x0 == 0 and rec['sxlo'][m] < 0, where
        elif name.startswith('clamped at column W'):
            assert x1 == W - 1 and rec['sxhi'][m] > W, where
        elif name.startswith('clamped at row 0'):
            assert y0 == 0 and rec['sylo'][m] < 0, where
        elif name.startswith('clamped at row H'):
            assert y1 == H - 1 and rec['syhi'][m] > H, where
        elif name.startswith('off the') or name.startswith('every corner behind') or name == 'every corner at w = 1e-4f exactly':
            assert tuple(rec['boxes'][m]) == R.EMPTY_BOX, where
            assert rec['front'][m] == name.startswith('off the'), where
        elif name.startswith('on column 0 by the margin'):
            assert (x0, x1) == (0, 0) and rec['sxhi'][m] < -0.5, where
        elif name.startswith('on column W - 1 by the margin'):
            assert x1 == W - 1 and x0 <= W - 1 and rec['sxlo'][m] > W, where
        elif name == 'the whole frame and more':
            assert (x0, x1, y0, y1, compact, near) == (0, W - 1, 0, H - 1, False, False), where
        elif name.startswith('extent exactly COMPACT_PX'):
            ex, ey = rec['sxhi'][m] - rec['sxlo'][m], rec['syhi'][m] - rec['sylo'][m]
            assert compact and (ex == px or 'in y' in name) and (ey == px or 'in x' in name) and max(ex, ey) == px, where + (ex, ey)
            seen.add('exact inside')
        elif name.startswith('extent COMPACT_PX + 5'):
            assert not compact and x0 <= x1, where
        elif name.startswith('compact '):
            which = dict((n, w) for n, _, w in R.compact_rows(W, H))[name]
            ex, ey = rec['sxhi'][m] - rec['sxlo'][m], rec['syhi'][m] - rec['sylo'][m]
            over = np.nextafter(px, F32(np.inf))
            for e, w, half in ((ex, which[0], W // 2), (ey, which[1], H // 2)):
                if w == 0:
                    assert px - half * 2.0 ** -22 <= e <= px and (e == px or half & (half - 1)), where + (e,)
                elif w == 1:
                    assert px < e <= px + half * 2.0 ** -22 and (e == over or half & (half - 1)), where + (e,)
                else:
                    assert e < px, where
            assert compact == (1 not in which) and x0 <= x1, where
            seen.add(name)
        elif name.startswith('near: last inside'):
            assert near and not rec['behind'][m] and (x0, x1, y0, y1) == (0, W - 1, 0, H - 1) and not compact, where
            assert rows[m + 1][0] == 'near: first outside the margin' and rows[m + 1][2][2] == np.nextafter(rows[m][2][2], F32(1)), where
        elif name.startswith('near: first outside'):
            assert not near and not rec['behind'][m] and (x0, x1, y0, y1) != (0, W - 1, 0, H - 1) and x0 <= x1, where
        elif name == 'deep, well inside the near margin':
            assert near and not rec['behind'][m] and (x0, x1, y0, y1) == (0, W - 1, 0, H - 1), where
        elif name == 'straddles the eye plane and the near plane':
            assert rec['behind'][m] and rec['front'][m] and near and not compact and (x0, x1, y0, y1) == (0, W - 1, 0, H - 1), where
        elif name == 'straddles the eye plane alone':
            assert rec['behind'][m] and rec['front'][m] and not near and not compact and (x0, x1, y0, y1) == (0, W - 1, 0, H - 1), where
        elif name == 'every corner at the float above w = 1e-4f':
            assert rec['front'][m] and not rec['behind'][m], where
        elif name in ('plain', 'deep, clear of both planes', 'clear of the eye plane, no near plane'):
            assert x0 <= x1 and not near and not rec['behind'][m] and (x0, x1, y0, y1) != (0, W - 1, 0, H - 1), where
        elif name.startswith('off the left by the margin') or name.startswith('off the right by the margin'):
            assert tuple(rec['boxes'][m]) == R.EMPTY_BOX and rec['front'][m], where
        else:
            raise AssertionError(f"no check for the edge {name!r}")
    assert {'compact x at', 'compact x over', 'compact y at', 'compact y over', 'compact both at'} <= seen
    if (W, H) == (640, 480):
        assert 'exact inside' in seen
    if (W, H) == (1280, 720):
        assert {'word seam 1', 'word seam 2'} <= seen and R.mask_words_of(fp) == 3
    # the y flip matters: H is not a multiple of TILE_H, so the tile rows counted from the bottom are other rows
    assert H % TH == 0 or any((H - 1 - y) // TH != y // TH for y in range(H))


@pytest.mark.parametrize('case', R.GEOMETRY_CASES, ids=CASE_IDS)
def test_box_exact_keeps_the_promises_of_box_bounds64(case):
    g = R.geometry_case(*case)
    classes = set()
    for c in range(g['C']):
        skip = g['layers'] and g['n_shared'] > 0 and R.LAYER_REP[R.LAYER_OF[c]] != c
        not_drawn = (g['header'][:, 7] < g['n_shared']) if skip else None
        bad = R.check_boxes(g['fp'], g['want'][c]['boxes'], g['b64'][c], f"candidate {c} ", not_drawn)
        bad += R.check_masks(g['fp'], g['want'][c]['boxes'], g['header'], g['n_shared'], g['want'][c]['mask_lo'], g['want'][c]['mask_hi'], f"candidate {c} ")
        assert not bad, '\n'.join(bad[:8])
        assert float(np.max(g['b64'][c]['slack'])) < 0.01, "the derived slack is far below the half pixel the margins leave"
        classes |= set(g['b64'][c]['cls'].tolist())
        if skip:                                        # candidate 1: no shared-link box, no mask_lo, no shared weight
            w = g['want'][c]
            assert not w['mask_lo'].any() and not w['tris_lo'].any() and (w['boxes'][g['header'][:, 7] < g['n_shared']] == R.EMPTY_BOX).all()
            assert g['want'][0]['mask_lo'].any()
    if case[2] > 200 and case[4] == 6:
        assert {'plain', 'near', 'behind', 'none in front'} <= classes, classes
    if case[4] == 4:
        assert 'unrendered' in classes


def test_cases_cover_the_counts_and_arguments():
    cases = R.GEOMETRY_CASES
    assert {c[:2] for c in cases} == {(128, 96), (160, 120), (640, 480), (1280, 720)}
    assert {c[2] for c in cases} == {1, 255, 256, 257, 1025} and {c[3] for c in cases} == {1, 3} and {c[4] for c in cases} == {4, 6}
    assert {c[5] for c in cases} == {0, 3, 6} and {c[6] for c in cases} == {0, 2} and {c[7] for c in cases} == {False, True}
    for c in cases:
        g = R.geometry_case(*c)
        if 0 < c[5] < 6 and c[2] > 200:
            assert any(w['tris'].any() and w['tris_lo'].any() and w['mask_lo'].any() and w['mask_hi'].any() for w in g['want']), c
        if c[6] == 2 and c[5] == 3 and c[2] > 200:          # lo_first = 2 drops links 0 and 1 from the shared weights
            other = R.box_exact(g['fp'], g['header'], g['aabb'], g['mvp'][0], c[4], c[5], 0)
            assert not np.array_equal(other['tris_lo'], g['want'][0]['tris_lo']) and np.array_equal(other['tris'], g['want'][0]['tris'])


@pytest.mark.parametrize('wrong', R.WRONG_BOX)
def test_inputs_tell_box_exact_from_a_wrong_one(wrong):
    hits = []
    for case in R.GEOMETRY_CASES:
        g = R.geometry_case(*case)
        for c in range(g['C']):
            skip = g['layers'] and g['n_shared'] > 0 and R.LAYER_REP[R.LAYER_OF[c]] != c
            other = R.box_exact(g['fp'], g['header'], g['aabb'], g['mvp'][c], g['n_render'], g['n_shared'], g['lo_first'], skip, wrong=(wrong,))
            if not R.same_boxes(other, g['want'][c]):
                hits.append(case)
    assert len(set(hits)) >= 2, (wrong, hits)


def test_a_wrong_box_breaks_a_promise():
    """check_boxes is not vacuous: a dropped near margin, a box that is too loose and a compact bit on a large meshlet each break a
    promise of box_bounds64 on the committed inputs.  (A margin of 0.5 for 1.5 does not: the spare pixel is there for rounding and
    snapping, which these inequalities already allow for — only box_exact, bit for bit, tells the two apart.)"""
    g = R.geometry_case(*R.GEOMETRY_CASES[1])
    for wrong in ('near margin dropped',):
        other = R.box_exact(g['fp'], g['header'], g['aabb'], g['mvp'][0], g['n_render'], g['n_shared'], g['lo_first'], wrong=(wrong,))
        assert R.check_boxes(g['fp'], other['boxes'], g['b64'][0]), wrong
    loose = g['want'][0]['boxes'].copy()
    m = int(np.flatnonzero(g['b64'][0]['cls'] == 'plain')[0])
    loose[m] = (0, g['fp'][0] - 1, 0, g['fp'][1] - 1)
    assert any('tight' in b for b in R.check_boxes(g['fp'], loose, g['b64'][0]))
    big = int(np.flatnonzero((g['b64'][0]['cls'] == 'plain') & ~g['want'][0]['compact'] & g['want'][0]['live'])[0])
    flagged = g['want'][0]['boxes'].copy()
    flagged[big, 0] |= 0x4000
    assert any('bit 14' in b for b in R.check_boxes(g['fp'], flagged, g['b64'][0])) or g['names'][big].startswith('compact')


def test_real_robot_vertices_lie_inside_box_exact():
    """The vertex properties on the CPU, with box_exact standing in for the kernel, at a parity pose under the default camera and at
    a near-camera scene; boxes cut in half and a missing mask bit are noticed."""
    rb = helpers.robot()
    header, aabb, verts = R.robot_tables(rb)
    for pose, ds, q, want_near in ((None, 1, [0.3, 0.4, 0.5, 0, 0, 0], False), ([0.3, -0.12, 0.77, 0, 0.2, 0.3], 2, [0, 0, 0, 0, 0, 0], True)):
        intr, PV = helpers.camera('640_480_color', ds=ds, pose=pose) if pose else helpers.camera('640_480_color')
        fp = R.frame(intr.width, intr.height)
        mvp = helpers.make_oracle(rb, intr, PV).mvp(q, 6)
        rec = R.box_exact(fp, header, aabb, mvp, 6, 3)
        bad = R.check_boxes(fp, rec['boxes'], R.box_bounds64(fp, header, aabb, mvp, 6)) + R.check_masks(fp, rec['boxes'], header, 3, rec['mask_lo'], rec['mask_hi'])
        more, seen = R.check_vertices(fp, rec['boxes'], header, verts, mvp, 6, 3, rec['mask_lo'], rec['mask_hi'])
        assert not bad + more, '\n'.join((bad + more)[:8])
        assert seen['on_screen'] > 1000 and bool(seen['near']) == want_near, seen
        shrunk = rec['boxes'].copy()                    # boxes cut to their left halves, masks without the first set bit: both noticed
        shrunk[:, 1] = (shrunk[:, 1] + (shrunk[:, 0] & 0x1FFF)) // 2
        assert any('outside box' in b for b in R.check_vertices(fp, shrunk, header, verts, mvp, 6, 3, rec['mask_lo'], rec['mask_hi'])[0])
        fewer = rec['mask_hi'].copy()
        w = int(np.flatnonzero(fewer)[0])
        fewer[w] &= fewer[w] - np.uint32(1)
        assert any('missing in mask_hi' in b for b in R.check_vertices(fp, rec['boxes'], header, verts, mvp, 6, 3, rec['mask_lo'], fewer)[0])


# ------------------------------------------------------------------------------------------------ finalize
def test_finalize_cases_reach_their_edges():
    sizes, _ = R.finalize_sizes()
    cases = R.finalize_cases()
    assert {c[0] for c in cases} == set(sizes) and {c[1] for c in cases} == {K['LOSS_DEPTH'], K['LOSS_FULL'], K['LOSS_LOOKUP'], K['LOSS_TSWEEP']}
    assert {c[4] for c in cases} == set(R.PLACEMENTS) and {c[2] for c in cases} == {4, 6}
    assert {c[3] for c in cases if c[1] == K['LOSS_FULL']} == set(R.FLAG_SETS)
    assert {tuple(v) for v in R.FLAG_SETS.values()} >= {(0,) * 8} and {b for v in R.FLAG_SETS.values() for b in v} == {0, 1, 3}
    for args in cases:
        f = R.finalize_case(*args)
        C, loss, n_render, _, placement = args
        final = np.array([[v for v in r] for r in f['final']], dtype=object)
        assert f['wraps'] > 0 and (f['sums'].astype(object) + f['total'].astype(object) >= 2 ** 64).any(), args     # sums negative modulo 2^64
        if f['placed'] is not None:
            assert f['best'] == f['placed'] == R.argmin(f['err']), args
            ties = np.flatnonzero(f['err'] == f['err'][f['best']])
            assert len(ties) >= len(f['placed_at']), args
            if placement == 'minimum last':
                assert f['best'] == C - 1
            if placement == 'tie across the first wave seam' and C > 64:
                assert {63, 64} <= set(ties.tolist())
        if placement == 'nan first':
            assert np.isnan(f['err'][0]) and (C == 1 or f['best'] > 0)
        if placement == 'nan last':
            assert np.isnan(f['err'][C - 1])
        if placement == 'all nan':
            assert np.isnan(f['err']).all() and f['best'] == 0
        if placement == 'all rows wrap':
            assert f['wraps'] == C * K['SUM_WORDS'] and (f['sums'] > np.uint64(2 ** 63)).all()
        if placement == 'count 0 with s1 > 0':
            assert final[C // 2, R.SUM_CNT] == 0 and np.isinf(f['err'][C // 2])
        if placement == 'nan first' or placement == 'all nan':
            assert final[0, R.SUM_CNT] == 0 and final[0, R.SUM_S1] == 0          # 0 / 0
        if placement == 'link count 0 with flag 3':
            assert f['flags'][3] == 3 and final[0, R.SUM_LINK0 + 10] == 0 and np.isfinite(f['err'][0])
        if placement == 'negative variance':
            s = [int(v) for v in final[0]]
            m1 = (np.float64(float(s[R.SUM_S1])) * 2.0 ** -32) / f['n_pix']
            S2 = (np.float64(float(s[R.SUM_AA])) * 2.0 ** 40 + np.float64(float(s[R.SUM_AB])) * 2.0 ** 21) + np.float64(float(s[R.SUM_BB]))
            assert (S2 * 2.0 ** -64) / f['n_pix'] - m1 * m1 < 0.0 and (loss == K['LOSS_FULL'] or f['err'][0] == 0.0)
        if loss == K['LOSS_FULL'] and n_render < 6:
            assert not f['words'][:, R.SUM_LINK0 + 3 * n_render:].any() and f['sums'][:, R.SUM_LINK0 + 3 * n_render:].all()
        if loss != K['LOSS_FULL']:
            assert not f['words'][:, R.SUM_LINK0:].any()
    for C in R.FRAME_SIZES:
        f = R.finalize_frames_case(C, K['LOSS_FULL'], 6)
        assert len({tuple(t) for t in f['totals'].tolist()}) == 3 and len({tuple(t) for t in f['flags'].tolist()}) == 3
        assert C < 3 or (set(f['frame_of'].tolist()) == {0, 1, 2} and (np.diff(f['frame_of'][:3]) != 0).all())


def test_inputs_tell_finalize_ref_and_argmin_from_wrong_ones():
    hit = {w: 0 for w in R.WRONG_FINALIZE + ('last index wins a tie',)}
    for args in R.finalize_cases():
        if args[0] > 300:
            continue
        f = R.finalize_case(*args)
        for wrong in R.WRONG_FINALIZE:
            err, words = R.finalize_ref(f['sums'], f['total'], f['loss'], f['n_render'], f['n_pix'], f['flags'], wrong=(wrong,))
            hit[wrong] += not (np.array_equal(R.bits(err), R.bits(f['err'])) and np.array_equal(words, f['words']))
        hit['last index wins a tie'] += R.argmin_last(f['err']) != f['best']
    assert all(v >= 3 for v in hit.values()), hit
    assert R.argmin([np.nan, 2.0, 1.0, 1.0, np.nan]) == 2 and R.argmin([np.nan, np.nan]) == 0 and R.argmin([np.inf, np.inf]) == 0 and R.argmin([0.0, -0.0]) == 0


# ------------------------------------------------------------------------------------------------ the raster queue's builder
def test_queue_weight_table_lies_on_every_class_border():
    top, n = K['QUEUE_TOP_LOG2'], K['QUEUE_CLASSES']
    table = R.queue_weight_table()
    assert {0, 1, 1 << 31, 0xFFFFFFFF} <= set(table) and all(0 <= t < 1 << 32 for t in table)
    for e in range(top - n, top + 2):
        assert {(1 << e) - 1, 1 << e, (1 << e) + 1} <= set(table)
        below, at, above = (R.queue_class(t) for t in ((1 << e) - 1, 1 << e, (1 << e) + 1))
        assert at == above == min(max(top - e, 0), n - 1) and below == min(max(top - e + 1, 0), n - 1), e
    assert {R.queue_class(t) for t in table} == set(range(n))
    assert R.queue_class(0) == R.queue_class(1) == n - 1 and R.queue_class(1 << 31) == R.queue_class(0xFFFFFFFF) == 0
    assert R.queue_class((1 << top) - 1) == 1 and R.queue_class(1 << top) == 0 and R.queue_class((1 << (top - n + 2)) - 1) == n - 1
    assert R.queue_class(1 << (top - n + 2)) == n - 2                         # the last border that is not a clamp


def _bits(mask_row, n_tiles):
    return [(int(mask_row[t >> 5]) >> (t & 31)) & 1 for t in range(n_tiles)]


@pytest.mark.parametrize('form', R.QUEUE_FORMS)
def test_queue_cases_reach_their_edges(form):
    n_cls, table = K['QUEUE_CLASSES'], R.queue_weight_table()
    assert {r for r, _ in R.QUEUE_SIZES} == {1, 7, 8, 9, 257, 65535} and {(t + 31) // 32 for _, t in R.QUEUE_SIZES} == {1, 2, 3, 8}
    assert {(r, t) for r, t in R.QUEUE_SIZES if r < 65535} == {(r, t) for r in (1, 7, 8, 9, 257) for t in (1, 4, 32, 33, 80, 256)} and (65535, 4) in R.QUEUE_SIZES
    seen_classes = set()
    for rows, n_tiles in R.QUEUE_SIZES:
        c = R.queue_case(form, rows, n_tiles)
        want, words = c['want'], c['words']
        who = (form, rows, n_tiles)
        # the contract: no mask bit at or past n_tiles, a segment holds every pair of the launch, a row fits an item's 16 bits
        for m in (c['mask_lo'], c['mask_hi']):
            assert m.shape == (c['n_cands'], words) and m.dtype == np.uint32
            if n_tiles % 32:
                assert not (m[:, -1] >> np.uint32(n_tiles % 32)).any(), who
        assert words == (n_tiles + 31) // 32 and n_tiles <= K['QUEUE_WEIGHT_TILES'] and rows <= 65535
        assert c['segment'] == (rows * words * 32 if c['weights'] is not None else 0) and c['n_items'] == max(c['segment'] * n_cls, rows * words * 32)
        assert sum(want['counts']) <= rows * n_tiles and all(n <= max(c['segment'], rows * words * 32) for n in want['counts'])
        if rows == 65535:                               # the last row an item's 16 bits are asked to name (rope_abi.hip: C <= 65535)
            assert any(i & 0xFFFF == rows - 1 for v in want['items'] for i in v), (who, 'the last row is not queued')
        assert all(i & 0xFFFF < rows and i >> 16 < n_tiles for v in want['items'] for i in v)
        assert c['sums'].all() and c['sums'].shape == (rows + R.QUEUE_SPARE_ROWS, K['SUM_WORDS'])
        assert np.array_equal(want['sums'][rows:], c['sums'][rows:])
        if c['weights'] is None:
            assert not any(want['counts'][:-1]) and (want['counts'][-1] > 0 or rows * n_tiles == 1), who
        else:
            at = (lambda i: c['cand_of_row'][i & 0xFFFF]) if c['base'] == 'for_layers' else (lambda i: i & 0xFFFF)
            weight = lambda i: int(c['weights'][at(i), i >> 16])
            assert all(R.queue_class(weight(i)) == cls for cls, v in enumerate(want['items']) for i in v)
            seen_classes |= {cls for cls, n in enumerate(want['counts']) if n}
            if sum(want['counts']) >= len(table):       # every weight of the table is queued: every class, both clamps, bit 31
                assert {weight(i) for v in want['items'] for i in v} == set(table), who
                assert all(want['counts']), who
                assert {1 << 31, 0xFFFFFFFF} <= {weight(i) for i in want['items'][0]}, who
                assert 0 in {weight(i) for i in want['items'][-1]}, who
            assert (rows, n_tiles) != (65535, 4) or sum(want['counts']) >= len(table)
        if c['base'] == 'for_layers':
            assert c['cand_of_row'][0] != 0 and len(set(c['cand_of_row'].tolist())) == rows and c['n_cands'] > rows
            assert np.array_equal(want['sums'], c['sums']), who
            if rows >= 7:                               # rows and representatives weigh differently: the classes say which was read
                assert any(R.queue_class(int(c['weights'][i & 0xFFFF, i >> 16])) != cls for cls, v in enumerate(want['items']) for i in v)
        if c['base'] == 'plain':
            assert np.array_equal(want['sums'], c['sums']), who
        if c['base'] != 'layers':
            continue
        of, rep, ls = c['layer_of'], c['layer_rep'], c['layer_sums']
        own = [i for i in range(rows) if rep[of[i]] == i]
        assert own and len(own) == len(rep) and not np.delete(c['mask_lo'], own, axis=0).any(), who
        only = lambda i: [l & ~h & 1 for l, h in zip(_bits(c['mask_lo'][rep[of[i]]], n_tiles), _bits(c['mask_hi'][i], n_tiles))]
        w = c['wrapped']
        tiles = [t for t, b in enumerate(only(w)) if b]
        start, added = int(c['sums'][w, R.SUM_S1]), [int(ls[of[w], t, R.SUM_S1]) for t in tiles]
        assert start > 0 and R.M64 in added and start + sum(added) >= 1 << 64, (who, 'no wrap')
        assert int(want['sums'][w, R.SUM_S1]) == (start + sum(added)) % (1 << 64) != sum(added) % (1 << 64)         # an add, and no store
        if rows >= 7:
            z, cov = c['zero_layer'], c['covered']
            assert z is not None and not ls[z].any() and any(only(int(rep[z]))) and np.array_equal(want['sums'][rep[z]], c['sums'][rep[z]]), who
            assert cov is not None and not any(only(cov)) and c['mask_lo'][rep[of[cov]]].any() and np.array_equal(want['sums'][cov], c['sums'][cov]), who
            assert any(rep[of[i]] != i and any(only(i)) for i in range(min(rows, 300))), who
        if rows >= 7 and words >= 2:
            s = c['span']
            assert s is not None and only(s)[0] and only(s)[32], (who, 'no layer-only tile in a mask word past the first')
            assert (want['sums'][s] != c['sums'][s]).any()
    if form.startswith('unweighted'):
        assert not seen_classes
    else:
        assert seen_classes == set(range(n_cls))


@pytest.mark.parametrize('wrong', R.WRONG_QUEUE)
def test_inputs_tell_queue_ref_from_a_wrong_one(wrong):
    hits = []
    for form in R.QUEUE_FORMS:
        for rows, n_tiles in R.QUEUE_SIZES:
            if rows > 300:
                continue
            c = R.queue_case(form, rows, n_tiles)
            if not R.same_queue(R.queue_ref(*c['args'], wrong=(wrong,)), c['want']):
                hits.append((form, rows, n_tiles))
    assert len(hits) >= 2, (wrong, hits)
    forms = {h[0] for h in hits}
    if wrong.startswith('class one'):                   # without weights there is no class to get wrong
        assert forms == {'plain', 'layers', 'for_layers'}, forms
    if wrong in ('lo of the row itself', 'layer_sums by candidate', 'store for add', 'hi | lo queued with layers'):
        assert forms == {'layers', 'unweighted layers'}, forms


def test_clear_sizes_and_wrong_clears():
    n_ctr, n_words = 2 * K['QUEUE_COUNTERS'], K['SUM_WORDS']
    words = [C * n_words for C in R.CLEAR_SIZES]
    assert {1, 11, 12, 256, 257} <= set(R.CLEAR_SIZES)
    assert min(words) < n_ctr < max(words) and any(0 < w <= 256 for w in words) and any(256 < w <= 512 for w in words) and any(w > 512 for w in words)
    assert 11 * n_words <= 256 < 12 * n_words or n_words != 23
    hit = {w: 0 for w in R.WRONG_CLEAR}
    for C in R.CLEAR_SIZES:
        sums = np.full((C + 2) * n_words, 0xA5A5A5A5A5A5A5A5, np.uint64)
        for counters in (np.full(n_ctr + 4, 0x25A5A5A5, np.int32), None):
            s, q = R.clear_pass_ref(sums, C, counters)
            assert not s[:C * n_words].any() and (s[C * n_words:] == sums[0]).all() and (sums == sums[0]).all()
            assert (q is None) if counters is None else (not q[:n_ctr].any() and (q[n_ctr:] == counters[0]).all())
            for wrong in R.WRONG_CLEAR:
                s2, q2 = R.clear_pass_ref(sums, C, counters, wrong=(wrong,))
                hit[wrong] += not (np.array_equal(s, s2) and ((q is None and q2 is None) or (q is not None and q2 is not None and np.array_equal(q, q2))))
    assert all(v >= 1 for v in hit.values()), hit
