"""The stored lookup table's kernels (rope_table.hip: crop_total, table_count, table_fill, table_score,
table_score_frames<F, LANES>; rope_kernels.hip: argmin_sets and the ROPE_LOSS_LOOKUP branch of finalize) on tables and targets the test supplies,
through tests/table_shim.hip — bit for bit against the dense reference of tests/table_ref.py, which tests/test_table_refs.py
holds to the oracle on the CPU and whose builders it shows to reach the edges they are named for.  The engine only ever feeds
these kernels rows the robot happens to draw, at crops with cw % 4 == 1; here: every cw % 4, cw < 4, one crop row, the whole image,
rows without groups, rows of -0.0, rows of more than 256 and 512 groups, frame counts on either side of every chunk and wave
boundary, every compiled <F, LANES>, and ties at chosen places on either side of every workgroup size of the argmin.

Every output buffer lies between guard bytes (table_child.Out) and the target planes are NaN outside the crop."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import table_child as K
import table_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
S1, BB = 1, 4                                          # the words of a row's sums the lookup score uses: S1, AA, AB, BB


@pytest.fixture(scope='module')
def shim_path(tmp_path_factory):
    from rope_s3d_amd import build
    csrc = os.path.dirname(build.LIB_PATH)
    out = str(tmp_path_factory.mktemp('table_shim') / 'libtable_shim.so')
    subprocess.check_call([build.shutil.which('hipcc') or '/opt/rocm/bin/hipcc'] + build.HIPCC_FLAGS +
                          [os.path.join(ROOT, 'tests', 'table_shim.hip'), '-L' + csrc, '-lrope_hip', '-Wl,-rpath,' + csrc, '-o', out])
    return out


@pytest.fixture(scope='module')
def shim(shim_path):
    lib = K.load_shim(shim_path)
    assert lib.shim_sum_words() == 23
    return lib


def check_compaction(tbl, case):
    """counts and the slices of goff / gval equal the reference's ordered groups row by row; the rows' ranges are disjoint and tile
    [0, used) — in whatever order the rows reserved them."""
    ranges = []
    for k, (goff, gval) in enumerate(case['groups']):
        n, o = int(tbl['h_counts'][k]), int(tbl['h_offs'][k])
        where = (case['name'], case['cw'], case['ch'], R.ROW_NAMES[k])
        assert n == len(goff), where
        assert n or o == 0, where
        assert np.array_equal(tbl['h_goff'][o:o + n], goff), where
        assert np.array_equal(tbl['h_gval'][o:o + n].view(np.uint32), gval.view(np.uint32)), where
        if n:
            ranges.append((o, o + n))
    ranges.sort()
    assert [a for a, _ in ranges] == [0] * bool(ranges) + [b for _, b in ranges[:-1]], ranges
    assert tbl['used'] == (ranges[-1][1] if ranges else 0)


def check_single_frame(shim, tbl, case):
    geom = [case[k] for k in ('W', 'H', 'r0', 'r1', 'c0', 'c1')]
    sums, scores, best_score, best = K.score_one(shim, tbl, geom, case['plane'], 23)
    where = (case['name'], case['cw'], case['ch'])
    assert np.array_equal(sums[:, S1:BB + 1], case['sums']), where
    assert not sums[:, :S1].any() and not sums[:, BB + 1:].any(), where
    assert np.array_equal(R.bits(scores), R.bits(case['scores'])), where
    assert best == case['best'] and R.bits(best_score) == R.bits(case['scores'][case['best']]), where


@pytest.mark.parametrize('cw,ch', R.CROP_SHAPES)
def test_compaction_and_single_frame_scores(shim, cw, ch):
    for case in R.crop_cases(cw, ch):
        tbl = K.build_table(shim, case['rows'])
        check_compaction(tbl, case)
        check_single_frame(shim, tbl, case)


def test_table_without_a_single_group(shim):
    case = R.empty_table_case()
    tbl = K.build_table(shim, case['rows'])
    assert tbl['used'] == 0 and not tbl['h_counts'].any() and not tbl['h_offs'].any()
    assert (tbl['goff'].host().view(np.uint8) == K.GUARD).all() and (tbl['gval'].host().view(np.uint8) == K.GUARD).all()     # one element each, untouched
    check_compaction(tbl, case)
    check_single_frame(shim, tbl, case)
    assert len(set(R.bits(case['scores']).tolist())) == 1 and case['best'] == 0
    planes = np.stack([case['plane']] * 3)
    scores, best = K.score_frames(shim, tbl, [case[k] for k in ('W', 'H', 'r0', 'r1', 'c0', 'c1')], planes, 23)
    assert np.array_equal(R.bits(scores), R.bits(np.stack([case['scores']] * 3)))
    assert np.array_equal(R.bits(best), R.bits(np.stack([[case['scores'][0], 0.0]] * 3)))


# ------------------------------------------------------------------------------------------------ many frames
@pytest.fixture(scope='module')
def frames_table(shim):
    return K.build_table(shim, R.frames_case()['rows'])


def check_frames(n, scores, best):
    fc = R.frames_case()
    idx = R.frames_of_batch(n)
    bad = np.argwhere(R.bits(scores) != R.bits(fc['scores'][idx]))
    assert not len(bad), (n, bad[:6])
    want = np.stack([fc['scores'][idx, fc['best'][idx]], fc['best'][idx].astype(np.float64)], axis=1)
    assert np.array_equal(R.bits(best), R.bits(want)), n


@pytest.mark.parametrize('n', R.FRAME_COUNTS)
def test_frames_scores_and_best(shim, frames_table, n):
    fc = R.frames_case()
    scores, best = K.score_frames(shim, frames_table, R.FRAMES_GEOM, fc['planes'][R.frames_of_batch(n)], 23)
    check_frames(n, scores, best)


def test_a_frame_scores_the_same_at_any_index_of_any_batch(shim, frames_table):
    fc = R.frames_case()
    seen = {}
    for n in (9, 33, 65, 130):
        idx = R.frames_of_batch(n)
        scores, best = K.score_frames(shim, frames_table, R.FRAMES_GEOM, fc['planes'][idx], 23)
        for at, f in enumerate(idx.tolist()):
            got = (R.bits(scores[at]).tobytes(), R.bits(best[at]).tobytes())
            assert seen.setdefault(f, (got, n, at))[0] == got, (f, n, at, seen[f][1:])
    assert len(seen) == R.N_FRAMES and all(sum(f in R.frames_of_batch(n) for n in (9, 33, 65, 130)) >= 2 for f in R.frames_of_batch(65).tolist())


# One child at a time, each a fresh process (the variant is read once per process).  A child's wall time on an MI355X has not been
# measured yet (each test prints it): importing numpy and torch alone takes 2.4 s on a machine without a GPU, opening the device
# and loading the library's code objects a few seconds more, the seven launches themselves milliseconds.  The limit is some
# twenty times that estimate; replace the estimate with the printed figure after the first run.
CHILD_TIMEOUT = 180
_child_fault = []


@pytest.mark.parametrize('frames,lanes', R.TABLE_VARIANTS)
def test_every_frames_lanes_instantiation(shim_path, tmp_path, frames, lanes):
    if _child_fault:
        pytest.fail(f"not started: an earlier variant ended by {_child_fault[0]}")
    fc = R.frames_case()
    src, dst = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(src, shim=shim_path, rows=fc['rows'], planes=fc['planes'], geom=np.array(R.FRAMES_GEOM),
             **{f'batch_{n}': R.frames_of_batch(n) for n in R.CHILD_FRAME_COUNTS})
    env = dict(os.environ, ROPE_TABLE_FRAMES=str(frames), ROPE_TABLE_LANES=str(lanes))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'table_child.py'), src, dst], env=env, timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _child_fault.append(f"the time limit at <{frames}, {lanes}>")
        pytest.fail(f"<{frames}, {lanes}>: no answer within {CHILD_TIMEOUT} s")
    print(f"<{frames}, {lanes}>: child took {time.perf_counter() - t0:.1f} s")
    if r.returncode < 0 or r.returncode in (134, 139):
        _child_fault.append(f"signal / abort ({r.returncode}) at <{frames}, {lanes}>")
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    with np.load(dst) as z:
        for n in R.CHILD_FRAME_COUNTS:
            check_frames(n, z[f'scores_{n}'], z[f'best_{n}'])


# ------------------------------------------------------------------------------------------------ argmin
@pytest.mark.parametrize('n_values', R.ARGMIN_SIZES)
def test_argmin_sets_first_index_of_the_smallest(shim, n_values):
    cases = R.argmin_sets_cases(n_values)
    for lo in range(0, len(cases), 3):
        trio = (cases[lo:lo + 3] + cases[:3])[:3]                       # three sets per launch
        err = K.dev(np.stack([v for _, v, _ in trio]))
        best = K.Out('best', 6, np.float64)
        assert shim.shim_argmin_sets(err.data_ptr(), n_values, 3, best.ptr, None) == 0
        got = best.host().reshape(3, 2)
        for (name, v, want), (score, index) in zip(trio, got):
            assert want == R.argmin(v), name                            # the builder's answer is the reference rule's
            assert index == want and R.bits(score) == R.bits(v[want]), (n_values, name, index, want)


@pytest.mark.parametrize('n_rows', R.ARGMIN_SIZES)
def test_finalize_argmin_on_tables_whose_scores_tie(shim, n_rows):
    pool = R.tie_pool()
    for name, idx in R.tie_places(n_rows):
        rows, want = R.tie_table(n_rows, idx)
        tbl = K.build_table(shim, rows)
        assert tbl['used'] == 2 * n_rows                                # every row dense: two groups
        sums, scores, best_score, best = K.score_one(shim, tbl, R.TIE_GEOM, pool['plane'], 23)
        assert np.array_equal(R.bits(scores), R.bits(want)), (n_rows, name)
        assert best == idx[0] == R.argmin(want) and R.bits(best_score) == R.bits(want[idx[0]]), (n_rows, name, best)
