"""The scenes of tests/raster_ref.py, on the CPU: every builder reaches the edge it is named for (the assertion states the edge,
from the kernel's own rules restated in Python); the C oracle equals the exact rasteriser on every scene — coverage, link on
every pixel, 24-bit depth within the per-pixel bound B of DESIGN.md §6; the inputs keep different links' surfaces 2^-16 apart
outside the deliberate ties; and the scenes tell the exact rules from eight deliberately wrong ones.  No scene leaves a pixel
out of any comparison.  Scene 'nearplane' (triangles cut at the near plane) is held to the oracle only, on the GPU: the exact rasteriser does not cut;
here its builder is shown to reach every class of cut and both drop cases."""
import numpy as np
import pytest

import raster_ref as rr

NAMES = [n for n in rr.SCENES if n not in rr.CUT_SCENES]       # the exact rasteriser does not cut: 'nearplane' is held to the oracle only
TIES = {'depth'}                   # the only scene with two links on bit-identical planes
MAX_RATIO = 0.3                    # measured: the largest |d24_oracle - d24_exact| / B over all scenes is 2/7 (scene 'depth')
_exact = {}


def exact(name):
    if name not in _exact:
        sc = rr.scene(name)
        st = {}
        m = sc.model
        ids, d24, gap = rr.render_exact(m.verts, m.faces, m.vtx_off, m.tri_off, sc.mats, sc.W, sc.H, stats=st)
        _exact[name] = (sc, ids, d24, gap, st)
    return _exact[name]


def walks(name):
    """Every (tile, walk, w, h, items) of every front-facing drawn triangle of the scene, per meshlet order."""
    sc, *_, st = exact(name)
    return [c for (_, _, a, b, c_) in st['tri'] for c in rr.classify((a, b, c_), sc.W, sc.H)]


@pytest.mark.parametrize('name', NAMES)
def test_oracle_equals_the_exact_rasteriser(name):
    """Identical coverage, identical link on every pixel, |d24_oracle - d24_exact| <= B per pixel (rr.d24_bound: derived from the
    float32 roundings of plane_from and the two fmaf; the largest over the triangles that cover the pixel, since the oracle's
    nearest may be another triangle of the same surface than the exact one's)."""
    sc, ids, d24, gap, st = exact(name)
    key = rr.make_oracle(sc).raster_key(sc.rows[0], 6)
    o_ids = np.where(key == 0xFFFFFFFF, 255, key & 0xFF).astype(np.uint8)
    assert (ids != 255).any()
    assert np.array_equal(ids != 255, o_ids != 255), f"{name}: coverage differs on {((ids != 255) != (o_ids != 255)).sum()} px"
    assert np.array_equal(ids, o_ids), f"{name}: link differs on {(ids != o_ids).sum()} px"
    cov = ids != 255
    err = np.abs((key >> 8).astype(np.int64) - d24.astype(np.int64))[cov]
    B = st['bound'][cov]
    print(f"{name}: max |d24 err| {err.max()}, max B {B.max()}, max err/B {(err / B).max():.3f}")
    assert (err <= B).all(), f"{name}: {(err > B).sum()} px beyond the bound"
    assert (err / B).max() <= MAX_RATIO, f"{name}: err/B {(err / B).max()} above the pinned ratio"


@pytest.mark.parametrize('name', NAMES)
def test_surfaces_of_different_links_stay_apart(name):
    """A condition on the INPUTS: wherever two links cover a pixel their surfaces are 2^-16 apart in window depth, so the exact
    reference has no near-tie and nothing is excluded; in scene 'depth' the tied planes are bit-identical (gap exactly 0)."""
    sc, ids, d24, gap, st = exact(name)
    cov = ids != 255
    tied = gap == 0.0
    assert tied.any() == (name in TIES), name
    assert (gap[cov & ~tied] >= 2.0 ** -16).all(), f"{name}: {gap[cov & ~tied].min()}"


def test_boxes_reach_every_size_and_every_walk():
    """(a) every clamped box size 1..6 x 1..6; 4x4 (one lane) against 5x4 and 4x5 (rows, columns); h == w above 4 (rows)."""
    got = {(w, h): walk for (_, walk, w, h, _) in walks('boxes')}
    for w in range(1, 7):
        for h in range(1, 7):
            assert got[(w, h)] == ('small' if w <= 4 and h <= 4 else 'cols' if h > w else 'rows'), (w, h)
    assert got[(4, 4)] == 'small' and got[(5, 4)] == 'rows' and got[(4, 5)] == 'cols' and got[(5, 5)] == 'rows' and got[(6, 6)] == 'rows'
    sc = rr.scene('boxes')
    tiles = {t for (t, *_) in walks('boxes')}
    assert tiles == set(range(6)), "a box in every tile, the partial last row included"
    assert max((h.view(np.uint32)[6] & 0xFFFF) for h in sc.model.meshlets.header) == 63


def test_edges_reach_the_coefficient_limit_and_the_K_clamp():
    """(c) a coefficient of exactly 2^22 - 1 (fast walk) and of 2^22 (raster_exact), as A and as B; A == 0, B == 0 and |A| == 1
    in boxes that go through clip_span; unclamped K beyond +-2^30 on both sides."""
    sc, ids, d24, gap, st = exact('edges')
    A, B, K, walk_of = set(), set(), [], {}
    for (_, _, a, b, c) in st['tri']:
        cl = rr.classify((a, b, c), sc.W, sc.H)
        for (p, q) in ((a, b), (b, c), (c, a)):
            for t, (col0, vy0, *_) in enumerate(rr.tile_frames(sc.W, sc.H)):
                if any(x[0] == t for x in cl):
                    Ak, Bk, Kk = rr.edge_K(p[0], p[1], q[0], q[1], col0, vy0)
                    walk = [x[1] for x in cl if x[0] == t][0]
                    walk_of.setdefault((abs(Ak), 'A'), set()).add(walk)
                    walk_of.setdefault((abs(Bk), 'B'), set()).add(walk)
                    if walk != 'exact':
                        K.append(Kk)
    L = rr.EDGE_COEF_LIMIT
    assert walk_of[(L - 1, 'A')] <= {'rows', 'cols'} and walk_of[(L - 1, 'B')] <= {'rows', 'cols'}
    assert walk_of[(L, 'A')] == {'exact'} and walk_of[(L, 'B')] == {'exact'}
    for k in ((0, 'A'), (0, 'B'), (1, 'A')):
        assert walk_of[k] & {'rows', 'cols'}, k
    assert max(K) > rr.EDGE_K_LIMIT and min(K) < -rr.EDGE_K_LIMIT, (min(K), max(K))
    # the clamp cuts only half-spaces that are constant over the tile: |A| 127 + |B| 95 stays below 2^30 for coefficients below 2^22
    assert (L - 1) * (rr.TILE_W - 1 + rr.TILE_H - 1) < rr.EDGE_K_LIMIT


def test_edges_reach_every_case_of_clip_span():
    """(c) the row and column items of scene 'edges', through clip_span's own arithmetic restated: A == 0 with n > 0 (an empty
    line) and with n <= 0, |A| == 1, a quotient above TILE_W + 2 and one below -3 that the clamp of floor_div_pos cuts, and K
    clamped at +-2^30."""
    sc, *_, st = exact('edges')
    got = set()
    for (_, _, a, b, c) in st['tri']:
        got |= rr.span_cases((a, b, c), sc.W, sc.H)
    assert got >= {'A0_n_pos', 'A0_n_nonpos', 'A1', 'cut_hi', 'cut_lo', 'K_clamped'}, got


def test_corner_scene_splits_a_box_every_way():
    """(a) the 6x6 box at every position relative to a tile corner: the four tiles around each corner see it cut to i x j,
    (6 - i) x j, i x (6 - j) and (6 - i) x (6 - j) for every i, j in 1..5."""
    sc, ids, *_, st = exact('corners')
    per_box = {}
    for (_, _, a, b, c) in st['tri']:
        cl = rr.classify((a, b, c), sc.W, sc.H)
        key = (min(a[0], b[0], c[0]), min(a[1], b[1], c[1]))
        per_box.setdefault(key, set()).update((w, h) for (_, _, w, h, _) in cl)
    splits = {frozenset(v) for v in per_box.values()}
    assert len(per_box) == 25
    assert splits == {frozenset({(i, j), (6 - i, j), (i, 6 - j), (6 - i, 6 - j)}) for i in range(1, 6) for j in range(1, 6)}
    assert (ids != 255).sum() == 25 * 36


def test_compact_scene_lists_both_kinds_in_one_tile():
    """(b) what can be said without the GPU about the mixed batch: tile 0 lists 24 compact and 24 non-compact meshlets (more
    meshlets than the workgroup has waves, so a wave draws several and its batch of 64 carries survivors of both kinds unless
    every wave happens to draw one kind only), and tile 3 lists compact ones only."""
    sc = rr.scene('compact')
    frames = rr.tile_frames(sc.W, sc.H)

    def tiles_of(tris):
        xs, ys = [v[0] / 256.0 for t in tris for v in t], [v[1] / 256.0 for t in tris for v in t]
        return {t for t, (_, _, wx0, wx1, wy0, wy1) in enumerate(frames) if max(xs) >= wx0 and min(xs) <= wx1 + 1 and max(ys) >= wy0 and min(ys) <= wy1 + 1}
    lists = {t: [sum(t in tiles_of(tr) for tr in sc.edges[kind]) for kind in ('compact', 'loose')] for t in range(len(frames))}
    assert lists[0][0] >= 24 and lists[0][1] == 24 and lists[0][0] + lists[0][1] > 12
    assert lists[3][0] >= 1 and lists[3][1] == 0


@pytest.mark.parametrize('n_tri,items', [(63, 6048), (64, 6144), (65, 6240)])
def test_queue_scene_fills_the_row_item_queue(n_tri, items):
    """(d) every triangle survives the cull, takes the row walk over the whole 128x96 tile and queues 96 items: 64 of them 6144
    items in 96 chunks of 64, the last word of the kernel's per-wave chunk-mask array (TILE_H words)."""
    w = walks(f'queue{n_tri}')
    assert len(w) == n_tri and all(x == (0, 'rows', 128, 96, 96) for x in w)
    assert sum(x[4] for x in w) == items
    first_batch = sum(x[4] for x in w[:64])
    assert first_batch <= 64 * rr.TILE_H and (first_batch + 63) // 64 <= rr.TILE_H
    if n_tri >= 64:
        assert first_batch == 6144 and (first_batch + 63) // 64 == 96
    sc = rr.scene(f'queue{n_tri}')
    assert len(sc.meshlet_tris[2]) == 1 and len(sc.meshlet_tris[2][0]) == n_tri, "all of them in ONE meshlet"
    _, ids, *_ = exact(f'queue{n_tri}')
    assert (ids == 2).all()


def test_shared_scene_draws_every_sample_exactly_once():
    """(e) at least 8 samples exactly on an edge of each ownership class — left, top, right, bottom and the four diagonals — and
    every sample of the fans and the strip drawn by exactly one triangle."""
    sc, ids, d24, gap, st = exact('shared')
    for k in ('left', 'right', 'top', 'bottom', 'down_leftwards', 'down_rightwards', 'up_leftwards', 'up_rightwards'):
        assert st['zero'].get(k, 0) >= 8, (k, st['zero'])
    assert set(np.unique(st['count'])) == {0, 1}
    top, bottom = sc.H - 1 - 101, sc.H - 1 - 100
    assert st['count'][top, 20:60].all() and st['count'][top, 60] == 0 and st['count'][bottom, 20:61].sum() == 0, \
        "the strip's top and left edges own their samples, its bottom and right edges do not"
    for (X, Y, r) in ((60, 200, 2), (127, 160, 3), (128, 63, 2), (200, 30, 5)):       # the fans: a square of 2r x 2r samples
        sq = st['count'][sc.H - 1 - (Y + r):sc.H - 1 - (Y - r), X - r:X + r]      # rows Y-r+1 .. Y+r: the top edge owns, the bottom does not
        assert sq.shape == (2 * r, 2 * r) and sq.all(), (X, Y)
    assert len(set(ids[top, 20:60])) >= 3 and (ids[top, 20:59] != ids[top, 21:60]).all(), "neighbouring samples of the strip belong to different links"


def test_depth_scene_reaches_both_ends_of_the_24_bits():
    """(f) d24 of 0 and of D24_MAX - 1 are drawn, the plane at exactly 1.0 is not; the lower of two links on one plane wins."""
    sc, ids, d24, gap, st = exact('depth')
    row = sc.H - 1 - 8
    assert ids[row, 10] == 0 and d24[row, 10] == 0
    assert ids[row, 36] == 1 and d24[row, 36] == rr.D24 - 1
    assert ids[row, 60] == 255
    assert ids[sc.H - 1 - 12, 90] == 3 and d24[sc.H - 1 - 12, 90] == rr.D24 - 1
    assert ids[sc.H - 1 - 20, 90] == 255
    assert (gap == 0).sum() > 400 and set(ids[gap == 0]) == {1}
    assert (ids[sc.H - 1 - 59:sc.H - 1 - 10, 150] == 4).sum() >= 20, "the sliver draws a column"
    assert len(set(ids[sc.H - 1 - 125:sc.H - 1 - 85, 20:140].ravel()) - {255}) == 6, "every link of the stack shows"


def test_compact_scene_sits_on_both_sides_of_the_threshold():
    """(b) meshlet_box's own extent: 60 - 1/256 px of vertices still pass as compact (<= 60 with the outward-rounded box), 60 px do
    not; tile-relative vertex coordinates reach 187 px (47 936 / 256) to the right of a tile and 60 px to the left of one."""
    sc = rr.scene('compact')
    b = rr.SceneBuilder('x', sc.W, sc.H)
    for kind, ok in (('compact', True), ('loose', False)):
        for tris in sc.edges[kind]:
            ex = rr.meshlet_extent_px([b.model_vertex(v) for t in tris for v in t], sc.PV, sc.W, sc.H)
            assert (max(ex) <= rr.COMPACT_PX) == ok, (kind, ex)
            assert abs(max(ex) - 60.0) < 0.01
    assert len(sc.edges['compact']) == 27 and len(sc.edges['loose']) == 24
    xs = [v[0] for tris in sc.edges['compact'] for t in tris for v in t]
    assert max(xs) - 0 >= 187 * 256 and any(128 * 256 - 60 * 256 <= x < 128 * 256 - 59 * 256 for x in xs)


def test_limit_scenes_reach_the_meshlet_limits():
    """(g) 64 vertices and 128 triangles in one meshlet, 65 triangles, a single one, a vertex without a window position inside a
    drawn meshlet; 2048 single-triangle meshlets all in one tile."""
    sc = rr.scene('limits_full')
    nv = [int(h[6]) & 0xFFFF for h in sc.model.meshlets.header]
    nt = [int(h[6]) >> 16 for h in sc.model.meshlets.header]
    assert (64, 128) in zip(nv, nt) and 65 in nt and 1 in nt
    sv = rr.shade_links(sc.model.verts, sc.model.vtx_off, sc.mats, sc.W, sc.H, 6)
    assert sum(v is None for v in sv[5]) == 1 and (exact('limits_full')[1] == 5).any()
    sc = rr.scene('limits_many')
    assert len(sc.model.meshlets.header) == rr.MAX_MESHLETS and (sc.W, sc.H) == (rr.TILE_W, rr.TILE_H)
    assert all(int(h[6]) >> 16 == 1 for h in sc.model.meshlets.header)
    assert (exact('limits_many')[4]['count'] > 0).sum() >= rr.MAX_MESHLETS, "every one of them draws"


def test_size_scenes_reach_the_image_borders():
    """Tile geometry: an image lower than a tile (vy0 < 0), narrower than two, of a width that is no multiple of 4; the last
    column and row are drawn by rectangles that end there, and one triangle covers every tile."""
    for name, (W, H) in (('sizes_131x37', (131, 37)), ('sizes_160x120', (160, 120)), ('sizes_256x256', (256, 256)), ('sizes_100x37', (100, 37))):
        sc, ids, *_ = exact(name)
        assert (sc.W, sc.H) == (W, H) and (ids != 255).all()
        assert ids[0, W - 1] != 0 and ids[H - 1, 0] != 0 and ids[H - 1, W - 1] == 0
        assert {t for (t, *_) in walks(name)} == set(range(len(rr.tile_frames(W, H))))
    assert 131 % 4 and rr.tile_frames(131, 37)[0][1] < 0
    (col0, vy0, wx0, wx1, wy0, wy1), = rr.tile_frames(100, 37)
    assert wx1 < rr.TILE_W - 1 and vy0 < 0, "an image narrower and lower than its one tile"


def test_nearplane_scene_reaches_every_cut_and_both_drops():
    """(h) Held to the oracle only (the exact rasteriser does not cut triangles).  Each of the six classes — one or two vertices
    behind the near plane, the odd vertex in each of the three places — occurs, on a link of its own, and each of those triangles
    alone draws through the oracle; the two dropped triangles (a cut vertex 2 * 10^6 px out; a vertex beyond the far plane beside
    one behind the near plane) draw nothing."""
    sc = rr.scene('nearplane')
    assert sorted((n, place) for (_, n, place) in sc.edges['classes']) == [(n, p) for n in (1, 2) for p in range(3)]
    assert sorted(l for (l, _, _) in sc.edges['classes']) == list(range(6))
    for i, (link, n_behind, place) in enumerate(sc.edges['classes']):
        alone = rr.scene_nearplane(only=i)
        tri, = alone.meshlet_tris[link]
        cls = [rr.clip_class(v) for v in tri[0]]
        assert cls.count('behind') == n_behind and 'bad' not in cls
        assert (cls.index('behind') if n_behind == 1 else cls.index('ok')) == place
        ids = rr.make_oracle(alone).render(alone.rows[0], 6)[1]
        assert set(np.unique(ids)) == {link, 255} and (ids == link).sum() > 1000, (i, (ids == link).sum())
    far_px, far_plane = sc.edges['drops']
    assert [rr.clip_class(v) for v in far_px] == ['ok', 'ok', 'behind']
    assert abs(rr.cut_vertex_px(far_px[0], far_px[2], sc.W, sc.H)[0]) > 1.5e6 and abs(rr.cut_vertex_px(far_px[1], far_px[2], sc.W, sc.H)[0]) > 1.5e6
    assert [rr.clip_class(v) for v in far_plane] == ['ok', 'bad', 'behind']
    drops = rr.scene_nearplane(only='drops')
    assert (rr.make_oracle(drops).render(drops.rows[0], 6)[1] == 255).all()
    ids = rr.make_oracle(sc).render(sc.rows[0], 6)[1]
    assert set(np.unique(ids)) == {0, 1, 2, 3, 4, 5, 255}


CAUGHT_BY = {'topleft_inverted': 'shared', 'owns_dy_positive': 'shared', 'centre_256p': 'boxes', 'lequal': 'depth', 'tie_high': 'depth',
             'front_cw': 'shared', 'box_no_offset': 'shared', 'snap_trunc': 'sizes_160x120'}


@pytest.mark.parametrize('wrong', rr.WRONG)
def test_scenes_tell_the_exact_rules_from_wrong_ones(wrong):
    """Each deliberately wrong rule changes the image of the scene named for it."""
    name = CAUGHT_BY[wrong]
    sc, ids, d24, *_ = exact(name)
    m = sc.model
    w_ids, w_d24, _ = rr.render_exact(m.verts, m.faces, m.vtx_off, m.tri_off, sc.mats, sc.W, sc.H, wrong=wrong)
    assert not (np.array_equal(ids, w_ids) and np.array_equal(d24, w_d24)), f"{wrong} goes unnoticed on {name}"
    assert set(CAUGHT_BY) == set(rr.WRONG)
