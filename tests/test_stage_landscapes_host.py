"""The stage machine (csrc/rope_predict.cpp) against the sequential restatement of the reference (oracle/predictor_ref.py) on
scripted error landscapes (tests/stage_landscapes.py): no renderer, so a whole prediction costs milliseconds, thousands of
trajectories are compared instead of the handful that rendered frames give, and a landscape can be built for one named decision.

(a) fuzz: seeded landscapes and stage lists, every stage's angles bit for bit, the scored poses in the reference's order;
(b) directed: one hand-built landscape per branch label, which the reference must report having taken (predict_reference's `events`);
(c) reach: over (a) and (b) every label is seen, or is listed below with the reason it cannot be;
(d) lockstep: rope_predict_batch at B in {1, 2, 7, 16}, each frame on its own landscape, against rope_predict frame by frame;
(e) the same once through the stored-table entry points, and the n_frames rule — also as a sanitised program of its own
    (tests/predict_table_main.cpp)."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

import stage_landscapes as SL

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
CSRC = os.path.join(ROOT, 'rope_s3d_amd', 'csrc')
# one seed is one landscape, one stage list and three predictions (the reference, speculate 1 and 3)
N_SEEDS = int(os.environ.get('ROPE_STAGE_FUZZ_SEEDS', '600'))
# labels with no run, each with its reason; the reach test requires that such a label is indeed never seen.  No label of the
# stage machine's own decisions is unreachable.
UNREACHABLE = {'isweep.spline_tie': "kept out on purpose, not unreachable: equal samples make the spline's argmin rounding noise of two "
                                      "different solvers (stage_landscapes' docstring); fuzz seeds that reach it draw again"}

reached = collections.Counter()          # label -> runs of the reference that reported it, over (a) and (b)


def _count(events):
    reached.update(set(events))


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('landscapes') / 'libpredict_shim.so')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-fPIC', '-shared', os.path.join(CSRC, 'rope_predict.cpp'),
                           os.path.join(ROOT, 'tests', 'native_shim.cpp'), '-o', out])
    return SL.declare(C.CDLL(out))


def _same_as_reference(shim, case, speculates=(1, 3)):
    """-> the reference's events.  Every stage's angles, the evaluation count, and at speculate 1 every scored pose in order."""
    trace, evaluated, n_eval, events = case.reference()              # a landscape on which this raises is a defect of the landscape
    for speculate in speculates:
        rc, got, n, logged, scored = SL.run_native(shim, case, speculate)
        assert rc == 0, (case.name, shim.shim_last_error())
        assert len(trace) == len(case.stages) == len(got)
        for k, (kind, ang) in enumerate(trace):
            assert SL.same_bits(got[k], ang), (case.name, speculate, k, kind, got[k], ang, case.stages)
        # on_eval sees every batch scored after the lookup grid, in order, with the index and links drawn of its stage
        n_lookup = len(case.grid) * sum(st[0] == 'lookup' for st in case.stages)
        assert len(logged) == len(scored) and all(SL.same_bits(rows, sent) for (_, _, rows), sent in zip(logged, scored))
        assert all(n_render == case.stages[k][1] and case.stages[k][0] != 'lookup' for k, n_render, _ in logged)
        assert n == n_lookup + sum(len(rows) for rows in scored)
        if speculate == 1:
            # the serial order asks for exactly the reference's renders, minus the lower-limit render SFlip throws away
            shown = SL.shown_rows(case, logged)
            assert len(shown) == len(evaluated) == n_eval - n_lookup, (case.name, len(shown), len(evaluated))
            for i, ((n_got, q_got), (n_ref, q_ref)) in enumerate(zip(shown, evaluated)):
                assert n_got == n_ref and SL.same_bits(q_got, q_ref), (case.name, i, n_got, q_got, n_ref, q_ref)
    return events


def test_fuzz_single_frame_equals_the_reference(shim):
    """(a): no seed is skipped; the first failing seed is reported with its stage list."""
    variants = collections.Counter()
    for seed in range(N_SEEDS):
        case = SL.fuzz_case(seed)
        variants[case.f.variant] += 1
        _count(_same_as_reference(shim, case))
    assert N_SEEDS < 60 or len(variants) == 5, variants              # every variant of the family took part


DIRECTED = SL.directed()


@pytest.mark.parametrize('name,labels,case', DIRECTED, ids=[d[0].replace(' ', '_') for d in DIRECTED])
def test_directed_landscape_reaches_its_branch_and_agrees(shim, name, labels, case):
    """(b): the assertion on `events` keeps a case from silently ceasing to reach the branch it was built for."""
    _, _, _, events = case.reference()
    for label in labels:
        assert label in events, (name, label, sorted(set(events)))
    _count(_same_as_reference(shim, case))


def test_every_label_has_a_directed_case():
    built_for = {label for _, labels, _ in DIRECTED for label in labels}
    assert built_for | set(UNREACHABLE) == set(SL.ALL_LABELS), set(SL.ALL_LABELS) - built_for


def test_one_division_takes_the_start(shim):
    """np.linspace(lo, hi, 1) is [lo]: a one-division TensorSweep over the whole range ends on the LOWER limit."""
    case = dict((d[0], d[2]) for d in DIRECTED)['one division, whole range']
    rc, got, _, _, _ = SL.run_native(shim, case, 3)
    assert rc == 0 and got[-1][2] == SL.LIMITS[2, 0]


def test_reach(shim):
    """(c): runs after (a) and (b) in file order and reads what they counted; on its own it counts the directed cases itself."""
    if not reached:
        for _, _, case in DIRECTED:
            _count(case.reference()[3])
    fuzzed = sum(reached.values()) > len(DIRECTED) * 8
    lines = ['label                      runs that reached it']
    for label in SL.ALL_LABELS:
        lines.append(f'{label:26s} {reached[label]:6d}' + (f'   unreachable: {UNREACHABLE[label]}' if label in UNREACHABLE else ''))
    print('\n'.join(lines))
    if os.environ.get('ROPE_STAGE_REACH_OUT') and fuzzed:
        with open(os.environ['ROPE_STAGE_REACH_OUT'], 'w') as fh:
            fh.write(f'predict_reference branch labels over {N_SEEDS} fuzz seeds and {len(DIRECTED)} directed cases '
                     '(tests/test_stage_landscapes_host.py)\n' + '\n'.join(lines) + '\n')
    for label in SL.ALL_LABELS:
        assert (reached[label] == 0) == (label in UNREACHABLE), (label, reached[label])


def _lockstep_cases(B, seed):
    """B landscapes under ONE stage list, grid and pose (a batch shares them): the variants mixed, one frame all NaN."""
    rng = np.random.default_rng([seed, B])
    stages = [('lookup',), ('sflip', 4), ('descent', 4, 10, 'SL', [0.05, 0.05, 0.1, 0.5, 0.5, 0.5], 0.5, 0.1), ('tsweep', 6, 1, 'U', 0.5),
              ('isweep', 6, 5, 'U', None), ('sflip', 6), ('tsweep', 4, 3, 'SL', 0.2), ('descent', 6, 12, 'SLU', [None] * 6, 0.5, 0.0075)]
    grid = SL.LIMITS[:, 0] + (SL.LIMITS[:, 1] - SL.LIMITS[:, 0]) * rng.uniform(0, 1, (6, 6))
    grid[:, 3:] = 0
    cases = []
    for f in range(B):
        fn = SL.landscape(rng)
        if f == B // 2 and B > 1:
            look = fn
            fn = lambda a, n, loss, look=look: look(a, n, loss) if loss == orc.LOSS_LOOKUP else SL.NAN       # a frame without depth
            fn.variant = 'all_nan'
        cases.append(SL.Case(fn, stages, grid, SL.TILTED, name=f'lockstep {B}/{f} ({fn.variant})'))
    return cases


@pytest.mark.parametrize('B,use_table', [(1, False), (2, False), (7, False), (16, False), (7, True)])
def test_lockstep_equals_frame_by_frame(shim, B, use_table):
    """(d), and (e) once: traces, angles and the total n_evals of rope_predict_batch equal rope_predict's per frame, bit for bit."""
    cases = _lockstep_cases(B, 11)
    for speculate in (3, 1):
        rc, trace, n, batches = SL.run_native_batch(shim, cases, speculate, use_table)
        assert rc == 0, shim.shim_last_error()
        assert any(frames == B for _, frames in batches)             # a step really carries the rows of all B frames
        total, left_at = 0, set()
        for f, case in enumerate(cases):
            rc, one, n1, logged, _ = SL.run_native(shim, case, speculate, use_table)
            assert rc == 0, shim.shim_last_error()
            assert SL.same_bits(one, trace[f]), (B, speculate, f, case.name)
            total += n1
            left_at.add(sum(1 for k, _, _ in logged if k == 2))      # batches this frame took part in during the first Descent
        assert n == total
        assert B < 7 or len(left_at) > 1, left_at                    # frames leave Descent at different iterations
    if B > 1:                                                        # and the frames are told apart: the all-NaN frame differs from its neighbours
        assert not SL.same_bits(trace[B // 2], trace[0])


def test_batch_refuses_a_frame_count_other_than_the_resident_one(shim):
    cases = _lockstep_cases(4, 3)
    for use_table in (True, False):
        for n_frames in (3, 5):
            rc, _, n, batches = SL.run_native_batch(shim, cases, 3, use_table, n_frames=n_frames, resident=4)
            assert rc == -1 and not batches and n == 0
            msg = shim.shim_last_error().decode()
            assert str(n_frames) in msg and '4' in msg and 'resident' in msg, msg
    assert SL.run_native_batch(shim, cases, 3, True, n_frames=4, resident=4)[0] == 0


def test_n_frames_rule_as_a_sanitised_program(tmp_path):
    """tests/predict_table_main.cpp: a program of its own under AddressSanitizer + UBSan, no Python in the process."""
    exe = str(tmp_path / 'predict_table_main')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                           '-fno-sanitize-recover=undefined', '-g', os.path.join(ROOT, 'tests', 'predict_table_main.cpp'),
                           os.path.join(CSRC, 'rope_predict.cpp'), os.path.join(ROOT, 'tests', 'native_shim.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok' and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
