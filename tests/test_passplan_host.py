"""The rules that choose a pass's launches (csrc/rope_passplan.h) without a GPU.  Every launch structure gives the same bits, so no
GPU test can tell a right plan from a wrong one: tests/passplan_main.cpp — a program of its own, built under AddressSanitizer and
UBSan — prints plan_pass() for rows of inputs, and tests/passplan_ref.py, written from the host code the header replaced, must
agree on every field of every row.  The pinned rows are the batches the GPU tests are built around."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from rope_s3d_amd import build

import passplan_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
CSRC = os.path.join(ROOT, 'rope_s3d_amd', 'csrc')
COL = {k: i for i, k in enumerate(R.INPUTS)}
OUT = {k: i for i, k in enumerate(R.OUTPUTS)}

ROWS_C = (1, 2, 7, 8, 26, 48, 49, 63, 64, 85, 86, 170, 171, 256, 257, 682, 683, 1024, 1025, 2048, 2049, 4096, 32768, 65535)
TILES = (1, 2, 3, 4, 5, 6, 12, 20, 25, 60, 256, 257)
# each tunable at its default, at rope_create's clamps (split_target and layer_min_wg have a lower one only, score_target none) and between
TUNABLES = dict(split_target=(512, 1, 100, 4096), split_min=(8, 1, 64, 20), split_min_many=(3, 1, 64, 20), split_cap=(64, 1, 7),
                score_target=(6144, 1, 1000, 100000), geo_rows=(48, 0, 256, 100), layer_min_wg=(64, 0, 10, 1000))


def table(**columns):
    """The full product of the given columns' values, every other input at its default -> (n, 20)."""
    names = list(columns)
    grid = np.array(list(itertools.product(*(columns[k] for k in names))), np.int64).reshape(-1, len(names))
    rows = np.tile(np.array([R.DEFAULTS[k] for k in R.INPUTS], np.int64), (len(grid), 1))
    for j, k in enumerate(names):
        rows[:, COL[k]] = grid[:, j]
    return rows


def layerings(C):
    """(n_layers, n_parents) pairs for C rows: none shared, the border of the 4x rule on both sides, everything shared — at both levels"""
    out = set()
    for nl in (C, C // 4, C // 4 + 1, 1):
        if 1 <= nl <= C:
            out.update((nl, n_par) for n_par in (nl, nl // 4, nl // 4 + 1, 1) if 1 <= n_par <= nl)
    return sorted(out)


def sweep():
    shapes = np.array([(C, t, nl, n_par) for C in ROWS_C for t in TILES for nl, n_par in layerings(C)], np.int64)
    main = np.repeat(table(strategy=[0])[:1], len(shapes) * 256, axis=0)
    for j, k in enumerate(('C', 'n_tiles', 'n_layers', 'n_parents')):
        main[:, COL[k]] = np.repeat(shapes[:, j], 256)
    main[:, COL['strategy']] = np.tile(np.arange(256), len(shapes))
    # the remaining inputs one at a time, each with every strategy, on batches of every kind: split with and without its own
    # geometry, layered small and large, large without layers
    few = [(2, 2, 2, 2), (26, 4, 26, 26), (64, 4, 64, 64), (200, 25, 50, 10), (320, 4, 64, 8), (768, 9, 64, 64), (1040, 4, 1040, 1040), (4096, 25, 256, 16)]
    rest = []
    for C, t, nl, n_par in few:
        base = dict(C=[C], n_tiles=[t], n_layers=[nl], n_parents=[n_par], strategy=range(256))
        rest.append(table(kind=range(3), frame_index=(0, 1), **base))
        rest.append(table(loss=range(5), kind=range(3), **base))
        for k, values in (('q_weighted', (0, 1)), ('clip', (0, 1)), ('skip', (0, 1)), ('n_cu', (8, 256, 304)), ('n_render', (1, 2, 3, 6))):
            rest.append(table(**{k: values}, **base))
        for k, values in TUNABLES.items():
            rest.append(table(**{k: values}, **base))
    # the tunables against every shape as well (strategy 0 and NO_LAYERS: the split's arithmetic is where they enter)
    for k, values in TUNABLES.items():
        rest.append(table(C=ROWS_C, n_tiles=TILES, strategy=(0, R.NO_LAYERS), **{k: values}))
    return np.concatenate([main] + rest)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('passplan') / 'passplan_main')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-fno-sanitize-recover=undefined',
                           '-g', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'passplan_main.cpp'), '-o', exe])

    def run(rows):
        rows = np.ascontiguousarray(rows, np.int64)
        text = '\n'.join(' '.join(map(str, r)) for r in rows.tolist()) + '\n'
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        return np.array(r.stdout.split(), np.int64).reshape(len(rows), len(R.OUTPUTS))
    return run


def test_header_is_plain_cxx_and_part_of_the_build_id():
    assert 'rope_passplan.h' in build._DEPS
    with open(os.path.join(CSRC, 'rope_passplan.h')) as f:
        src = f.read()
    assert not re.search(r'#include\s*[<"](hip/|rope_)', src), "rope_passplan.h must build without HIP and without the context"
    # the one project header it takes is the public C header, which includes <stdint.h> alone
    assert re.findall(r'#include\s*"([^"]+)"', src) == ['../../include/rope_s3d.h']
    with open(os.path.join(ROOT, 'include', 'rope_s3d.h')) as f:
        assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read()) == ['stdint.h']


def test_the_rules_live_in_the_header_alone():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.cpp')):
            with open(os.path.join(CSRC, name)) as f:
                src = f.read()
            assert not re.search(r'busy_tiles|want_layers|layers_pay|want_parents|use_parents|\*\s*4\s*<=', src), name


def test_plan_equals_the_reference_on_the_sweep(program):
    rows = sweep()
    want = R.enqueue_eval(rows)
    # the sweep is not vacuous (of the reference alone: nothing here depends on the header)
    for k in ('layers', 'parents', 'layer_queue', 'weighted', 'own_geometry', 'fused_geometry', 'cache_scope', 'cacheable', 'fragment_scope', 'clip'):
        assert set(np.unique(want[:, OUT[k]])) == {0, 1}, f"{k} is not seen both ways"
    assert set(np.unique(want[:, OUT['scoring']])) == {R.SCORE_GTILE, R.SCORE_QUEUE, R.SCORE_PLAIN}
    default_cap = rows[:, COL['split_cap']] == R.DEFAULTS['split_cap']
    splits = set(np.unique(want[default_cap, OUT['split']]))
    assert {1, R.DEFAULTS['split_cap']} <= splits and any(1 < s < R.DEFAULTS['split_cap'] for s in splits)
    assert {1, 8} <= set(np.unique(want[:, OUT['slices']]))
    assert set(np.unique(want[:, OUT['n_shared']])) == {0, 1, 2, 3} and set(np.unique(want[:, OUT['lo_first']])) == {0, 2}
    got = program(rows)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (f"{len(bad)} of {len(rows)} rows differ; the first: inputs {dict(zip(R.INPUTS, rows[bad[0]].tolist()))}\n"
                           f"plan_pass  {dict(zip(R.OUTPUTS, got[bad[0]].tolist()))}\nreference  {dict(zip(R.OUTPUTS, want[bad[0]].tolist()))}")


# The batches the GPU tests are built around, on an MI355X (256 CUs): 160x120 is 2 x 2 tiles of 128 x 96, 320x240 is 3 x 3.
GRID = dict(C=320, n_tiles=4, n_layers=64, n_parents=8)               # tests/test_gpu_geometry_cache.py, tests/test_gpu_kept_fragments.py: 8 x 8 x 5
PINNED = [
    # tests/test_gpu_instantiations.py test_eval_views ('far' / 'near' / 'mixed', 260): 1040 (view, frame) rows at four tiles score through the queue
    (dict(C=1040, n_tiles=4, n_layers=1040, kind=R.EVAL_VIEWS, loss=R.LOSS_CAMFULL), dict(scoring=R.SCORE_QUEUE, split=1, layers=0, fused_geometry=0)),
    # the border of that rule at four tiles (busy_tiles 2): 1024 rows are still split, 1025 are not
    (dict(C=1024, n_tiles=4, n_layers=1024), dict(scoring=R.SCORE_GTILE, split=3)),
    (dict(C=1025, n_tiles=4, n_layers=1025), dict(scoring=R.SCORE_QUEUE, split=1)),
    # tests/test_gpu_instantiations.py test_eval_far_queue_and_layer_queue under NO_LAYERS: 768 rows at 320x240 (busy_tiles 3) are past 682
    (dict(C=682, n_tiles=9, n_layers=682), dict(scoring=R.SCORE_GTILE, split=3)),
    (dict(C=683, n_tiles=9, n_layers=683), dict(scoring=R.SCORE_QUEUE, split=1)),
    (dict(C=768, n_tiles=9, n_layers=64, n_parents=64, strategy=R.NO_LAYERS), dict(scoring=R.SCORE_QUEUE, split=1, layers=0)),
    (dict(C=768, n_tiles=9, n_layers=64, n_parents=64, strategy=R.NO_LAYERS | R.NO_QUEUE), dict(scoring=R.SCORE_PLAIN, split=1, layers=0)),
    # the same test under strategy 0, and test_stored_table_near: layers through the layer queue, then the scoring queue
    (dict(C=768, n_tiles=9, n_layers=64, n_parents=64, loss=R.LOSS_LOOKUP), dict(layers=1, n_shared=3, layer_queue=1, weighted=1, parents=0, scoring=R.SCORE_QUEUE)),
    (dict(C=768, n_tiles=9, n_layers=64, n_parents=64, strategy=R.NO_QUEUE), dict(layers=1, layer_queue=0, scoring=R.SCORE_PLAIN)),
    # tests/test_gpu_instantiations.py test_eval_targets_near: 864 rows of three frames, layers inside every frame, both queues, CLIP
    (dict(C=864, n_tiles=9, n_layers=72, n_parents=72, kind=R.EVAL_TARGETS, frame_index=1, clip=1),
     dict(layers=1, layer_queue=1, scoring=R.SCORE_QUEUE, clip=1, cache_scope=0)),
    # the layer queue's border: at most 256 tiles (q_weighted, ensure_capacity) and rows x busy_tiles <= 512 x CUs
    (dict(C=1541, n_tiles=256, n_layers=16, n_parents=16), dict(layers=1, layer_queue=1, weighted=1)),           # 1541 x 85 = 130 985 <= 131 072
    (dict(C=1543, n_tiles=256, n_layers=16, n_parents=16), dict(layers=1, layer_queue=0, weighted=0)),           # 1543 x 85 = 131 155
    (dict(C=1541, n_tiles=257, n_layers=16, n_parents=16, q_weighted=0), dict(layers=1, layer_queue=0, weighted=0)),
    # tests/test_gpu_instantiations.py test_eval_views ('near' / 'mixed', 12): 256 rows or fewer are split (48 x 2 pairs: the floor of 8 shares)
    (dict(C=48, n_tiles=4, n_layers=48, kind=R.EVAL_VIEWS, clip=1), dict(scoring=R.SCORE_GTILE, split=8, own_geometry=0, fused_geometry=1, clip=1)),
    (dict(C=256, n_tiles=4, n_layers=256), dict(scoring=R.SCORE_GTILE, split=3, fused_geometry=1)),
    (dict(C=257, n_tiles=4, n_layers=257), dict(scoring=R.SCORE_GTILE, split=3, fused_geometry=0)),
    # tests/test_gpu_geometry_cache.py test_hit_equals_miss_fresh_context_and_oracle, tests/test_gpu_kept_fragments.py
    # test_every_loss_builds_once_and_serves: the grid is kept and its fragments serve
    (dict(GRID), dict(layers=1, n_shared=3, layer_queue=1, weighted=1, parents=0, cache_scope=1, cacheable=1, fragment_scope=1, scoring=R.SCORE_QUEUE)),
    # tests/test_gpu_geometry_cache.py "hit under NO_QUEUE": the second sharing level draws the layers, kept; tests/test_gpu_kept_fragments.py
    # test_strategy_128_scores_as_before_and_the_cache_flag_implies_it: hits without a store
    (dict(GRID, strategy=R.NO_QUEUE), dict(layers=1, parents=1, lo_first=2, layer_queue=0, cacheable=1, fragment_scope=0, scoring=R.SCORE_PLAIN)),
    (dict(GRID, strategy=R.NO_KEPT_FRAGMENTS), dict(cacheable=1, fragment_scope=0)),
    (dict(GRID, strategy=R.NO_GEOMETRY_CACHE), dict(cache_scope=1, cacheable=0, fragment_scope=0)),
    # tests/test_gpu_kept_fragments.py test_unweighted_queue_draws_the_same_store: no weights, the store all the same
    (dict(GRID, q_weighted=0), dict(weighted=0, layer_queue=0, parents=1, cacheable=1, fragment_scope=1)),
]


@pytest.mark.parametrize('case', range(len(PINNED)))
def test_pinned_batches(program, case):
    inputs, fields = PINNED[case]
    row = table(**{k: [v] for k, v in inputs.items()})
    for plan in (program(row)[0], R.enqueue_eval(row)[0]):
        got = {k: int(plan[OUT[k]]) for k in fields}
        assert got == fields, (inputs, got)
