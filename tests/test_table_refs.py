"""CPU: tests/table_ref.py is what it claims to be.  Its dense restatement of the lookup score gives the oracle's bits on rendered
rows at one crop per cw % 4 (that entitles it to stand in for the kernels' contract in tests/test_gpu_table_kernels.py), and every
input builder reaches the edge it is named for."""
import numpy as np
import pytest

from oracle import oracle as orc

import helpers
import table_ref as R

# the 160 x 120 camera: crops r0, r1, c0, c1 of tests/test_gpu_lookup_edges.py, by what they are there for
ENGINE_CROPS = {'cw%4==0': [30, 119, 40, 139], 'cw%4==1': [25, 110, 36, 136], 'cw%4==2': [40, 119, 50, 151], 'cw%4==3': [20, 100, 60, 122],
                'one column': [20, 119, 90, 90], 'one row': [100, 100, 0, 159], 'empty corner': [0, 2, 0, 2], 'whole image': [0, 119, 0, 159],
                'some poses miss': [20, 60, 124, 150]}
TARGET_ROW = 13


def engine_rows(limits):
    """slu_grid(limits, 3) and row TARGET_ROW twice more: three rows that tie."""
    grid = helpers.slu_grid(limits, 3)
    return np.concatenate([grid, grid[[TARGET_ROW, TARGET_ROW]]])


@pytest.fixture(scope='module')
def scene():
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=4)
    o = helpers.make_oracle(rb, intr, PV)
    cand = engine_rows(rb.joint_limits)
    dense = np.stack([np.sqrt(o.render(q)[0]) for q in cand])               # a table row: the square root of the metric depth
    d, ids = o.render([0.35, 0.45, 0.9, 0, 0, 0])
    tq, t32, flags, *_ = helpers.synthetic_target(d, ids)
    return o, cand, dense, tq, t32, flags


@pytest.mark.parametrize('name', ['cw%4==0', 'cw%4==1', 'cw%4==2', 'cw%4==3', 'one column', 'some poses miss'])
def test_reference_scores_have_the_oracles_bits(scene, name):
    o, cand, dense, tq, t32, flags = scene
    r0, r1, c0, c1 = ENGINE_CROPS[name]
    assert (c1 - c0 + 1) % 4 == {'cw%4==0': 0, 'cw%4==1': 1, 'cw%4==2': 2, 'cw%4==3': 3, 'one column': 1, 'some poses miss': 3}[name]
    want, want_sums = o.eval(cand, orc.LOSS_LOOKUP, 6, tq, t32, ENGINE_CROPS[name], flags, threads=4, want_sums=True)
    T = t32[r0:r1 + 1, c0:c1 + 1]
    got_sums = np.array([R.sums(T, D[r0:r1 + 1, c0:c1 + 1]) for D in dense], np.uint64)
    assert np.array_equal(got_sums, want_sums[:, 1:5])
    got = np.array([R.score_of(s, T.size) for s in got_sums.tolist()])
    assert np.array_equal(R.bits(got), R.bits(want))
    assert R.argmin(want) == int(np.argmin(want))


def test_engine_crops_are_what_they_are_named(scene):
    o, cand, dense, *_ = scene
    assert dense.shape[1:] == (120, 160)
    drawn = {k: np.array([(D[r0:r1 + 1, c0:c1 + 1] != 0).any() for D in dense]) for k, (r0, r1, c0, c1) in ENGINE_CROPS.items()}
    assert not drawn['empty corner'].any()
    assert drawn['some poses miss'].any() and not drawn['some poses miss'].all() and drawn['some poses miss'][TARGET_ROW]
    for k in ('cw%4==0', 'cw%4==1', 'cw%4==2', 'cw%4==3', 'one column', 'one row', 'whole image'):
        assert drawn[k].all(), k
    assert np.array_equal(dense[TARGET_ROW], dense[27]) and np.array_equal(dense[TARGET_ROW], dense[28])


# ------------------------------------------------------------------------------------------------ the builders
def test_q32_and_special_values():
    assert R.q32(R.B_ONES) == [0xFFFFF, 0xFFFFFF, (1 << 23) | 0xFFFFF]
    assert all(v & 0xFFFFF == 0xFFFFF for v in R.q32(R.B_ONES))
    assert R.q32(R.SUBNORMALS + R.BELOW_Q32) == [0, 0, 0, 0] and all(v > 0 for v in R.SUBNORMALS + R.BELOW_Q32)
    assert all(0 < v < np.finfo(np.float32).tiny for v in R.SUBNORMALS) and all(v >= np.finfo(np.float32).tiny for v in R.BELOW_Q32)
    assert R.q32([np.float32(1.0), np.float32(127.5), np.float32(-0.0)]) == [1 << 32, 255 << 31, 0]
    # the epilogue: four equal samples have no spread, two different ones have the spread written out by hand
    assert R.score_of(R.sums(np.full(4, 0.5, np.float32), np.zeros(4, np.float32)), 4) == 0.0
    assert R.score_of(R.sums(np.array([1, 0], np.float32), np.zeros(2, np.float32)), 2) == 0.5 * 0.5
    assert R.sums(np.float32([3.0]), np.float32([1.0]))[0] == 2 << 32


def test_every_crop_case_reaches_its_edge():
    assert {cw % 4 for cw, _ in R.CROP_SHAPES} == {0, 1, 2, 3} and {1, 2, 3} <= {cw for cw, _ in R.CROP_SHAPES} and {ch for _, ch in R.CROP_SHAPES} >= {1, 2, 17}
    n_groups = {(cw + 3) // 4 * ch for cw, ch in R.CROP_LONG}
    assert n_groups == {255, 256, 257, 513}
    seen, negative_delta, classes = set(), 0, set()
    for cw, ch in R.CROP_SHAPES:
        cases = R.crop_cases(cw, ch)
        assert [c['W'] - cw for c in cases] == [0, 3, 9]
        for c in cases:
            seen.add(c['name'])
            assert (c['cw'], c['ch']) == (cw, ch) and c['T'].shape == (ch, cw)
            inside = np.zeros(c['plane'].shape, bool)
            inside[c['r0']:c['r1'] + 1, c['c0']:c['c1'] + 1] = True
            assert np.isnan(c['plane'][~inside]).all() and np.isfinite(c['plane'][inside]).all()         # NaN everywhere outside the crop
            assert (c['T'] >= 0).all() and (c['T'] < 128).all() and not np.signbit(c['T']).any()
            if c['name'] == 'whole':
                assert c['plane'].shape == (ch, cw)
            if c['name'] == 'right':
                assert c['c0'] % 4 == 3 and c['c1'] == c['W'] - 1
            if c['name'] == 'left':
                assert c['c0'] == 0 and c['r0'] == 0 and c['c1'] < c['W'] - 1
            if c['name'] == 'inner':
                assert c['c0'] % 4 == 1 and 0 < c['r0'] and c['r1'] < c['H'] - 1 and c['c1'] < c['W'] - 1
            rows, gw = c['rows'], (cw + 3) // 4
            count = [len(g[0]) for g in c['groups']]
            assert rows.shape == (7, ch, cw) and (np.abs(rows) < 128).all()
            assert count[0] == 0 and not rows[0].any()                                                # the empty row
            assert count[1] == gw * ch and (rows[1] != 0).all()                                       # fully dense
            assert count[2] == 1 and c['groups'][2][0][0] == 0                                        # only the first group
            assert count[3] == 1 and c['groups'][3][0][0] == 4 * (gw * ch - 1)                        # only the last group ...
            if cw % 4:
                assert (c['groups'][3][1][0, cw % 4:] == 0).all() and c['groups'][3][1][0, cw % 4 - 1] != 0       # ... its tail past the crop reads 0
            assert count[4] == (gw * ch + 1) // 2 and (c['groups'][4][0] % 8 == 0).all()              # every other group
            assert count[5] == 0 and np.signbit(rows[5]).all() and (rows[5].view(np.uint32) == 0x80000000).all()      # only -0.0: no group
            assert np.array_equal(rows[6].view(np.uint32), rows[1].view(np.uint32))                   # the duplicate
            assert R.bits(c['scores'][6]) == R.bits(c['scores'][1]) and R.bits(c['scores'][5]) == R.bits(c['scores'][0])
            if gw * ch > 1:                                                                           # a group of only -0.0 inside a row that has groups
                pad = np.zeros((ch, 4 * gw), np.float32)
                pad[:, :cw] = rows[4]
                odd = pad.reshape(-1, 4)[1::2]
                assert (odd == 0).all() and np.signbit(odd[:, 0]).all()
            if cw >= 2:                                                                               # -0.0 inside a kept group keeps its bits
                assert (c['groups'][4][1][0, 1:2].view(np.uint32) == 0x80000000).all()
            negative_delta += R.delta_s1(c['T'], rows[1]) < 0
            # which classes of value pairs this case holds
            dq = np.array(R.q32(np.abs(c['T'] - rows[1])) + R.q32(np.abs(c['T'] - rows[4])) + R.q32(c['T']), object)
            both = np.concatenate([c['T'].ravel(), c['T'].ravel(), c['T'].ravel()]), np.concatenate([rows[1].ravel(), rows[4].ravel(), np.zeros(cw * ch, np.float32)])
            tiny = np.finfo(np.float32).tiny
            classes |= {'b all ones'} if any(v & 0xFFFFF == 0xFFFFF for v in dq) else set()
            classes |= {'dq == 0 of a difference'} if ((dq == 0) & (both[0] != both[1])).any() else set()
            classes |= {'T == D'} if ((both[0] == both[1]) & (both[0] != 0)).any() else set()
            classes |= {'zero target'} if (c['T'] == 0).any() else set()
            classes |= {'subnormal target'} if ((c['T'] > 0) & (c['T'] < tiny)).any() else set()
            classes |= {'subnormal row value'} if ((np.abs(rows) > 0) & (np.abs(rows) < tiny)).any() else set()
            classes |= {'a above 2^18'} if any(v >> 38 for v in dq) else set()
    assert seen == {'whole', 'right', 'left', 'inner'}
    assert negative_delta > len(R.CROP_SHAPES)              # a delta sum below zero before the total is added back, in most cases
    assert classes == {'b all ones', 'dq == 0 of a difference', 'T == D', 'zero target', 'subnormal target', 'subnormal row value', 'a above 2^18'}
    big = R.crop_cases(36, 57)[0]
    assert len(big['groups'][1][0]) == 513 > 512 and len(big['groups'][4][0]) == 257 > 256


def test_empty_table_case_holds_no_group():
    c = R.empty_table_case()
    assert all(len(g[0]) == 0 for g in c['groups']) and np.signbit(c['rows'][1::2]).all() and not np.signbit(c['rows'][::2]).any()
    assert len(set(R.bits(c['scores']).tolist())) == 1 and c['best'] == 0 and c['scores'][0] > 0


def test_frames_case():
    fc = R.frames_case()
    crops = fc['crops']
    assert crops.shape == (130, 8, 24) and R.FRAMES_GEOM[4] % 4 == 1
    assert len({c.tobytes() for c in crops}) == 130                                         # mutually different
    assert len({R.bits(s).tobytes() for s in fc['scores']}) == 130
    assert R.delta_s1(crops[0], fc['rows'][1]) < 0 and len(R.groups(fc['rows'][1])[0]) == 48
    assert [len(R.groups(D)[0]) for D in fc['rows']] == [0, 48, 1, 1, 24, 0, 48]
    assert R.FRAME_COUNTS == (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 129, 130)
    place = {}
    for n in R.FRAME_COUNTS:
        idx = R.frames_of_batch(n)
        assert len(set(idx.tolist())) == n                                                  # no frame twice in a batch
        for at, f in enumerate(idx.tolist()):
            place.setdefault(f, set()).add(at)
    assert all(len(p) > 1 for f, p in place.items() if f in R.frames_of_batch(100))         # the same frame at other indices of other batches
    assert set(R.TABLE_VARIANTS) == {(f, l) for f in (2, 4, 8) for l in (8, 16, 64)} and set(R.CHILD_FRAME_COUNTS) <= set(R.FRAME_COUNTS)
    # the frame counts against the launch's chunks (launch_table_score_frames: 4 x F x 64 / LANES frames per workgroup)
    for F, L in R.TABLE_VARIANTS:
        per_wg, per_wave = 4 * F * (64 // L), min(F, 4 if L == 8 else 8) * (64 // L)
        cut = [n for n in R.CHILD_FRAME_COUNTS if -(-n // max(1, -(-n // per_wg))) % per_wave]
        assert cut, (F, L)                                                                  # a chunk that cuts a wave's lane groups


def test_argmin_cases_sit_where_they_say():
    assert R.ARGMIN_SIZES == (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
    assert [R.block_of(C) for C in (64, 65, 256, 257, 1024, 1025, 4097)] == [64, 256, 256, 1024, 1024, 1024, 1024]
    names = set()
    for C in R.ARGMIN_SIZES:
        B = R.block_of(C)
        for name, idx in R.tie_places(C):
            names.add(name)
            assert all(0 <= i < C for i in idx) and list(idx) == sorted(idx)
            if name == 'wave':
                assert idx == (63, 64)
            if name == 'stride':
                assert idx[1] // B == idx[0] // B + 1 and idx[1] % B < idx[0] % B and idx[0] % 64 != idx[1] % 64
            if name == 'thread':
                assert len({i % B for i in idx}) == 1 and len(idx) >= 2
            rows, want = R.tie_table(C, idx)
            assert all(np.array_equal(rows[i], R.tie_pool()['best']) for i in idx)
            assert np.flatnonzero(want == want.min()).tolist() == list(idx) and R.argmin(want) == idx[0]      # the tie sits exactly there
        for name, v, want in R.argmin_sets_cases(C):
            names.add(name)
            assert len(v) == C and R.argmin(v) == want, (C, name)
            finite = v[~np.isnan(v)]
            if len(finite):
                assert v[want] == finite.min() and not (v[:want] == v[want]).any()
            if name == 'nan_before_min':
                assert np.isnan(v[:want]).all() and want > 0
            if name == 'all_inf':
                assert np.isinf(v).all() and want == 0
    assert names == {'first', 'last', 'ends', 'wave', 'stride', 'thread', 'nan_before_min', 'nan_first_min_last', 'all_nan', 'inf_but_one',
                     'all_inf', 'nan_then_inf'}
    pool = R.tie_pool()
    assert 0 < pool['best_score'] < pool['scores'].min() and len(set(pool['scores'].tolist())) == len(pool['scores'])
    assert R.score(pool['T'], pool['best']) == pool['best_score'] and R.score(pool['T'], pool['rows'][5]) == pool['scores'][5]
    assert [R.argmin(v) for v in ([np.nan, 2.0, 1.0, 1.0], [np.nan, np.nan], [np.inf, np.inf], [np.nan, np.inf], [3.0])] == [2, 0, 0, 1, 0]
