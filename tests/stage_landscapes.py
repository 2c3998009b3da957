"""Scripted error landscapes for the stage machine (csrc/rope_predict.cpp), no GPU and no renderer.

The stage machine only ever sees numbers: the errors of the poses it asks for.  Here those numbers come from a plain function
f(angles, n_render, loss) instead of a render, given to BOTH sides: to oracle/predictor_ref.predict_reference through a duck-typed
stand-in for the CPU oracle (the three methods it uses), and to rope_predict / rope_predict_batch through the callbacks of
tests/native_shim.cpp.  An evaluation costs microseconds, so thousands of whole predictions fit where one rendered prediction did,
and a landscape can be built to reach one named branch (DIRECTED).

What the landscapes keep away from, and why:
  - the Lookup score and a TensorSweep's scores along ONE sweep are never partly NaN: the reference takes tf.argmin of both
    (predict.py:169, 369), the restatement np.argmin (the first NaN), the engine the first smallest number (DESIGN.md keeps that
    deviation); all NaN, or none, is where the three agree.  So the NaN band of LOSS_TSWEEP lies on the last joint, and no generated
    TensorSweep sweeps that joint (Descent still walks it into and out of the band).
  - a Descent stage always has a joint: without one the reference reads over_err before any assignment (predict.py:222).
  - grids lie inside the limits: a sweep about an angle beyond them has lo > hi, which interp1d refuses.
  - an InterpolativeSweep whose spline has a second point within 1e-9 of its minimum ('isweep.spline_tie': all samples equal, or
    two samples that tie for the smallest, which quantised landscapes produce).  The argmin over the spline — the pose rendered
    next — is then the rounding noise of scipy's banded B-spline solve on one side and of the library's elimination on second
    derivatives on the other (the one piece of rope_predict.cpp that is not a transcription; both are good to ~1e-13).  Neither is
    right, so no test can hold one to the other there.  A fuzz seed whose reference run reports it draws again (fuzz_case: same
    seed, next attempt; FLAT_REDRAWS counts them) — no seed is skipped, and ties and plateaus everywhere else stay in.
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from oracle import predictor_ref
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
from rope_s3d_amd.engine import (STAGE_DESCENT, STAGE_ISWEEP, STAGE_LOOKUP, STAGE_SFLIP, STAGE_TSWEEP, EvalHook, PredictArgs, StageDesc)
from rope_s3d_amd.prediction.predict import preview_rows

NAN = float('nan')
LETTERS = 'SLURBT'
TILTED = [0.1, -1.6, 0.8, 0.05, 0.08, -0.1]          # SFlip's axis mixes cam[4] and cam[5] (predict.py:245); the default pose gives 0
POSES = (list(DEFAULT_CAMERA_POSE), TILTED)
# joint limits in binary fractions, so that "a start exactly one step from a limit" is exact; asymmetric where the robot's are
LIMITS = np.array([[-3.0, 3.0], [-1.125, 2.5], [-2.375, 4.5], [-3.25, 3.25], [-2.25, 2.25], [-6.25, 6.25]])
INC = np.array([.005] * 6)
KIND = {'lookup': STAGE_LOOKUP, 'descent': STAGE_DESCENT, 'sflip': STAGE_SFLIP, 'isweep': STAGE_ISWEEP, 'tsweep': STAGE_TSWEEP}
ALL_LABELS = tuple(f'{k}.{l}' for k, ls in predictor_ref.EVENT_LABELS.items() for l in ls)
_NAMES = ['link%d' % i for i in range(6)]
_BLUE = {n: 10 * (i + 1) for i, n in enumerate(_NAMES)}
_CROP = np.array([0, 1, 0, 1], np.int32)
_PLANE = np.zeros((2, 2))

EvalCb = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32))
TargetsCb = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double))
TableCb = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int32), C.c_int)


class ScriptedOracle:
    """What predict_reference asks of an Oracle, answered from f: the 'raster key' is the pose itself."""

    def __init__(self, f):
        self.f = f

    def raster_key(self, q, n):
        return np.array(q, np.float64)

    def sums(self, key, loss, n, tq=None, t32=None, crop=None):
        return key

    def finalize(self, sums, loss, n, n_pix, link_flags):
        return self.f(sums, n, loss)


def engine_argmin(err):
    """finalize_argmin_kernel's rule: the first smallest number, a NaN never wins, all NaN -> row 0"""
    ok = ~np.isnan(err)
    return int(np.flatnonzero(ok)[np.argmin(err[ok])]) if ok.any() else 0


class Case:
    """One prediction: a landscape, a stage list (predictor_ref's tuples), a lookup grid inside the limits, a camera pose."""

    def __init__(self, f, stages, grid, pose=POSES[0], inc=INC, name=''):
        self.f, self.stages, self.pose, self.name = f, list(stages), list(pose), name
        self.grid = np.ascontiguousarray(np.atleast_2d(np.asarray(grid, np.float64)))
        self.inc = np.asarray(inc, np.float64)
        assert ((LIMITS[:, 0] <= self.grid) & (self.grid <= LIMITS[:, 1])).all(), name

    def errors(self, rows, n_render, loss):
        return np.array([self.f(r, n_render, loss) for r in rows], np.float64)

    def reference(self):
        """-> (trace [(kind, angles)], evaluated [(n_render, pose)], n_evals, events); computed once"""
        if getattr(self, '_ref', None) is None:
            self._ref = self._reference()
        return self._ref

    def _reference(self):
        evaluated, events = [], []
        _, trace, n = predictor_ref.predict_reference(ScriptedOracle(self.f), _PLANE, _PLANE, _NAMES, _BLUE, LIMITS, self.pose, self.grid, _CROP,
                                                      min_ang_inc=self.inc, stages=self.stages, evaluated=evaluated, events=events)
        return trace, evaluated, n, events

    def native_stages(self):
        return native_stages(self.stages)


def native_stages(stages):
    """predictor_ref's stage tuples as the rope_stage records of the same list"""
    out = []
    for st in stages:
        d = StageDesc(KIND[st[0]], 6 if st[0] == 'lookup' else st[1], 0, 0)
        d.init_rate[:] = [NAN] * 6
        d.rate_reduction, d.early_stop, d.range = 0.5, 0.01, NAN
        if st[0] == 'descent':
            _, _, d.count, letters, init, d.rate_reduction, d.early_stop = st
            d.init_rate[:] = [NAN if r is None else r for r in init]
        elif st[0] in ('isweep', 'tsweep'):
            _, _, d.count, letters, rng = st
            d.range = NAN if rng is None else rng
        if st[0] in ('descent', 'isweep', 'tsweep'):
            d.joints = sum(1 << LETTERS.index(c) for c in letters)
        out.append(d)
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def declare(lib):
    lib.rope_predict.argtypes = [C.c_void_p, C.POINTER(PredictArgs), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.rope_predict_batch.argtypes = [C.c_void_p, C.POINTER(PredictArgs), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.shim_last_error.restype = C.c_char_p
    lib.shim_set_targets_callback.argtypes = [C.c_void_p]
    lib.shim_set_table_callbacks.argtypes = [C.c_void_p, C.c_void_p]
    lib.shim_set_resident.argtypes = [C.c_int]
    return lib


def run_native(lib, case, speculate, use_table=False):
    """rope_predict on the shim -> (rc, trace (n_stages, 6), n_evals, logged on_eval batches [(stage, n_render, rows)], scored rows)"""
    scored = []

    @EvalCb
    def answer(cand, n, n_render, loss, crop_p, err_out, best_idx):
        rows = np.ctypeslib.as_array(cand, (n, 6)).copy()
        err = case.errors(rows, n_render, loss)
        if loss != orc.LOSS_LOOKUP:
            scored.append(rows)
        if err_out:
            np.ctypeslib.as_array(err_out, (n,))[:] = err
        if best_idx:
            best_idx[0] = engine_argmin(err)
        return 0

    @TableCb
    def table(best_idx, n):
        best_idx[0] = engine_argmin(case.errors(case.grid, 6, orc.LOSS_LOOKUP))
        return 0
    logged = []

    @EvalHook
    def on_eval(user, stage, n_render, rows, n):
        logged.append((stage, n_render, np.ctypeslib.as_array(rows, (n, 6)).copy()))
    lib.shim_set_callback(answer)
    lib.shim_set_table_callbacks(C.cast(table, C.c_void_p) if use_table else None, None)
    stages = case.native_stages()
    arr = (StageDesc * len(stages))(*stages)
    cam = np.asarray(case.pose, np.float64)
    args = PredictArgs(arr, len(arr), speculate, _p(LIMITS), _p(cam), _p(case.inc), _p(case.grid), len(case.grid), int(use_table), _p(_CROP), None, on_eval)
    out, trace, n = np.full(6, 7.0), np.full((len(arr), 6), 7.0), C.c_int64()
    rc = lib.rope_predict(C.c_void_p(1), C.byref(args), _p(out), _p(trace), C.byref(n))
    lib.shim_set_callback(None)
    lib.shim_set_table_callbacks(None, None)
    assert rc != 0 or same_bits(out, trace[-1])
    return rc, trace, n.value, logged, scored


def run_native_batch(lib, cases, speculate, use_table=False, n_frames=None, resident=None):
    """rope_predict_batch on the shim, frame f on cases[f]'s landscape; the stage list, grid, pose and increments are cases[0]'s
    -> (rc, trace (B, n_stages, 6), n_evals, batches [(rows, frames in it)])"""
    B = len(cases) if n_frames is None else n_frames
    batches = []

    @TargetsCb
    def answer(cand, frame_of, n, n_render, loss, crop_p, err_out):
        rows = np.ctypeslib.as_array(cand, (n, 6)).copy()
        fo = np.ctypeslib.as_array(frame_of, (n,)).copy()
        if fo.min() < 0 or fo.max() >= len(cases):
            return -1
        batches.append((n, len(set(fo.tolist()))))
        np.ctypeslib.as_array(err_out, (n,))[:] = [cases[f].f(r, n_render, loss) for f, r in zip(fo, rows)]
        return 0

    @TableCb
    def table(best_idx, n):                       # one entry per RESIDENT target, as rope_lookup_score_targets writes them
        for f in range(n):
            best_idx[f] = engine_argmin(cases[f].errors(cases[0].grid, 6, orc.LOSS_LOOKUP))
        return 0
    lib.shim_set_targets_callback(C.cast(answer, C.c_void_p))
    lib.shim_set_table_callbacks(None, C.cast(table, C.c_void_p) if use_table else None)
    lib.shim_set_resident(len(cases) if resident is None else resident)
    first = cases[0]
    stages = first.native_stages()
    arr = (StageDesc * len(stages))(*stages)
    cam = np.asarray(first.pose, np.float64)
    args = PredictArgs(arr, len(arr), speculate, _p(LIMITS), _p(cam), _p(first.inc), _p(first.grid), len(first.grid), int(use_table), _p(_CROP))
    out, trace, n = np.full((B, 6), 7.0), np.full((B, len(arr), 6), 7.0), C.c_int64()
    rc = lib.rope_predict_batch(C.c_void_p(1), C.byref(args), B, _p(out), _p(trace), C.byref(n))
    lib.shim_set_targets_callback(None)
    lib.shim_set_table_callbacks(None, None)
    lib.shim_set_resident(0)
    assert rc != 0 or same_bits(out, trace[:, -1])
    return rc, trace, n.value, batches


def same_bits(a, b):
    """bit for bit, NaN as NaN (a NaN's payload and sign are nobody's decision)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def shown_rows(case, logged):
    """the on_eval batches as the poses the reference renders (predict.preview_rows puts SFlip's discarded lower endpoint back)"""
    return [(n_render, q) for k, n_render, rows in logged for q in preview_rows(case.stages[k][0] == 'sflip', rows, LIMITS)]


# ---------------------------------------------------------------------------------------------------------------- landscapes

def landscape(rng):
    """A weighted quadratic about a centre that may lie beyond the limits, plus a ripple; then one of: as is, quantised to 2^-k
    (ties and plateaus), exactly zero on a band, NaN on a band (LOSS_FULL: any joint; LOSS_TSWEEP: the last joint)."""
    span = LIMITS[:, 1] - LIMITS[:, 0]
    centre = LIMITS[:, 0] + span * rng.uniform(-0.25, 1.25, 6)
    weight = rng.uniform(0.05, 2.0, 6) * (rng.random(6) < 0.8)
    amp, freq, phase = rng.uniform(0, 0.3), rng.uniform(0.5, 12.0, 6), rng.uniform(0, 6.28, 6)
    look_centre = LIMITS[:, 0] + span * rng.uniform(0, 1, 6)
    variant = ('plain', 'quant', 'quant', 'zero', 'nan', 'nan_quant')[int(rng.integers(6))]
    k = int(rng.integers(12))
    band_j = int(rng.integers(6))
    band_lo = LIMITS[band_j, 0] + span[band_j] * rng.uniform(0, 0.8)
    band_hi = band_lo + span[band_j] * rng.uniform(0.02, 0.4)
    t_lo = LIMITS[5, 0] + span[5] * rng.uniform(0, 0.8)
    t_hi = t_lo + span[5] * rng.uniform(0.05, 0.5)
    scale = float(2 ** k)

    def f(a, n_render, loss):
        a = np.asarray(a, np.float64)
        if loss == orc.LOSS_LOOKUP:
            return float(np.sum((a - look_centre) ** 2))
        v = float(np.sum(weight * (a - centre) ** 2) + amp * np.sum(np.cos(freq * a + phase)) + 0.125 * n_render)
        if loss == orc.LOSS_TSWEEP:
            v = -v * 0.5
            if variant.startswith('nan') and t_lo < a[5] < t_hi:
                return NAN
        elif variant.startswith('nan') and band_lo < a[band_j] < band_hi:
            return NAN
        if variant == 'zero' and band_lo < a[band_j] < band_hi:
            return 0.0
        if 'quant' in variant:
            v = float(np.floor(v * scale) / scale)
        return v
    f.variant = variant
    return f


def _shipped(which):
    return [tuple(st) for st in predictor_ref.STAGES[which]]


def stage_list(rng):
    """The two shipped lists, the shipped lists with a TensorSweep inserted, or a random list."""
    def tsweep():
        return ('tsweep', int(rng.integers(1, 7)), int(rng.integers(1, 5)), LETTERS[:int(rng.integers(1, 6))][-int(rng.integers(1, 3)):],
                (None, 0.001, 0.2, 10.0)[int(rng.integers(4))])
    pick = int(rng.integers(8))
    if pick < 2:
        return _shipped(('SL', 'SLU')[pick])
    if pick < 4:
        stages = _shipped(('SL', 'SLU')[pick - 2])
        stages.insert(int(rng.integers(1, len(stages) + 1)), tsweep())
        return stages
    stages = [('lookup',)] if rng.random() < 0.85 else []
    for _ in range(int(rng.integers(2, 7))):
        kind = ('descent', 'descent', 'sflip', 'isweep', 'tsweep')[int(rng.integers(5))]
        n = int(rng.integers(1, 7))
        if kind == 'descent':
            init = [None if rng.random() < 0.5 else float(rng.choice([0.005, 0.05, 0.1, 0.5, 1.0])) for _ in range(6)]
            stages.append(('descent', n, int(rng.integers(0, 12)), LETTERS[:int(rng.integers(1, 7))], init, 1.0, 0.0))
        elif kind == 'sflip':
            stages.append(('sflip', n))
        elif kind == 'isweep':
            stages.append(('isweep', n, int(rng.integers(4, 9)), LETTERS[int(rng.integers(6))], (None, 0.001, 0.1, 10.0)[int(rng.integers(4))]))
        else:
            stages.append(tsweep())
    return stages


FLAT_REDRAWS = [0]


def fuzz_case(seed):
    """The case of a seed: the first attempt whose reference run keeps off 'isweep.spline_tie' (see the module's docstring)."""
    for attempt in range(64):
        case = _fuzz_draw(seed, attempt)
        if 'isweep.spline_tie' not in case.reference()[3]:
            return case
        FLAT_REDRAWS[0] += 1
    raise AssertionError(f'seed {seed}: no attempt without a tie in a sweep\'s spline')


def _fuzz_draw(seed, attempt):
    rng = np.random.default_rng([seed, attempt, 0x57A6E])
    f = landscape(rng)
    grid = LIMITS[:, 0] + (LIMITS[:, 1] - LIMITS[:, 0]) * rng.uniform(0, 1, (int(rng.integers(1, 9)), 6))
    grid[:, 3:] *= rng.random() < 0.5
    if rng.random() < 0.3:                                  # rows on a limit, and on S == 0
        j = int(rng.integers(3))
        grid[0, j] = LIMITS[j, int(rng.integers(2))]
        grid[-1, 0] = 0.0
    return Case(f, stage_list(rng), grid, POSES[seed % 2], name=f'seed {seed} ({f.variant})')


# ------------------------------------------------------------------------------------------------------------------ directed

def _quad(centre, weight=(1, 1, 1, 1, 1, 1)):
    c, w = np.asarray(centre, float), np.asarray(weight, float)
    return lambda a, n, loss: float(np.sum(w * (np.asarray(a) - c) ** 2))


def _const(v):
    return lambda a, n, loss: v


def _descent(letters, count, init=None, redux=0.5, early=0.0, n=4):
    return ('descent', n, count, letters, list(init or [None] * 6), redux, early)


def directed():
    """[(name, labels the reference must report, Case)], each built by hand for its labels."""
    L = LIMITS
    look = ('lookup',)
    half = [0.5] * 6
    ulp_up = float(np.nextafter(0.005, 1.0))
    nan_in = lambda j, lo, hi, g: (lambda a, n, loss: NAN if lo < a[j] < hi else g(a, n, loss))
    only = lambda loss_kind, v, g: (lambda a, n, loss: v if loss == loss_kind else g(a, n, loss))
    out = []

    def add(name, labels, f, stages, start, pose=POSES[0], inc=INC):
        out.append((name, tuple(labels), Case(f, stages, [start], pose, inc, name)))

    # ---- Descent
    add('init rates given', ['descent.init_rate_set', 'descent.ran_out'], _quad([1, 1, 1, 0, 0, 0]), [look, _descent('SL', 2, half)], [0.25, 0.25, 0, 0, 0, 0])
    add('start within a step of the zero history', ['descent.lr_cut'], _quad([1, 0, 0, 0, 0, 0]), [look, _descent('S', 3, [0.05] + [None] * 5)], [0.03125, 0, 0, 0, 0, 0])
    add('start on the lower limit', ['descent.under_outside', 'descent.step_over'], _quad([0] * 6), [look, _descent('S', 2, half)], [L[0, 0], 0, 0, 0, 0, 0])
    add('start on the upper limit', ['descent.over_outside', 'descent.step_under'], _quad([0] * 6), [look, _descent('L', 2, half)], [0, L[1, 1], 0, 0, 0, 0])
    # 2.0 + 0.5 is the limit 2.5 itself: the render happens (<=), the step lands on the limit, and the next one is outside
    add('a step lands exactly on a limit', ['descent.step_over', 'descent.over_outside'], _quad([0, 9, 0, 0, 0, 0]), [look, _descent('L', 3, half, redux=1.0)],
        [0, 2.0, 0, 0, 0, 0])
    add('constant landscape: every comparison ties', ['descent.step_tie', 'descent.break_still'], _const(1.5), [look, _descent('SLU', 10, half)], [1, 1, 1, 0, 0, 0])
    add('symmetric about the start: a tie between two renders', ['descent.step_tie'], _quad([1, 1, 1, 0, 0, 0]), [look, _descent('SLU', 4, half)], [1, 1, 1, 0, 0, 0])
    add('error flat to one part in a thousand: the early stop', ['descent.break_err'], lambda a, n, loss: 1.0 + 0.001 * a[0],
        [look, _descent('S', 10, [0.05] + [None] * 5, redux=0.5, early=0.1)], [1, 0, 0, 0, 0, 0])
    add('an error history that starts at zero', ['descent.break_still'], _const(0.0), [look, _descent('SL', 10, half, early=0.1)], [1, 1, 0, 0, 0, 0])
    add('both neighbours outside: the history gets inf', ['descent.under_outside', 'descent.over_outside', 'descent.step_tie'], _quad([0] * 6),
        [look, _descent('B', 3, [None] * 4 + [4.0, None], redux=1.0, early=0.1)], [0, 0, 0, 0, 1.0, 0])
    # from the zero pose one step of exactly min_ang_inc: the spread over the (zero) history EQUALS it
    add('spread equal to min_ang_inc', ['descent.break_spread'], lambda a, n, loss: 10.0 - a[0], [_descent('S', 5, [0.005] + [None] * 5, redux=1.0)], [0] * 6)
    add('spread one ulp above min_ang_inc: np.isclose', ['descent.break_spread'], lambda a, n, loss: 10.0 - a[0], [_descent('S', 5, [ulp_up] + [None] * 5, redux=1.0)], [0] * 6)
    # np.isclose's band is atol + rtol |inc| = 1e-8 + 1e-5 * 0.005 = 6e-8 wide
    add('spread just inside np.isclose', ['descent.break_spread'], lambda a, n, loss: 10.0 - a[0], [_descent('S', 5, [0.005 + 5.9e-8] + [None] * 5, redux=1.0)], [0] * 6)
    add('spread just beyond np.isclose', ['descent.step_over', 'descent.ran_out'], lambda a, n, loss: 10.0 - a[0],
        [_descent('S', 2, [0.005 + 6.1e-8] + [None] * 5, redux=1.0)], [0] * 6)
    add('no iterations', ['descent.ran_out'], _quad([0] * 6), [look, _descent('SLURBT', 0, half)], [1, 1, 1, 1, 1, 1])
    # ---- SFlip (default pose: the axis is 0 and the flip is S -> -S; TILTED: axis about -0.096)
    add('S of zero: sign(0)', ['sflip.sign0', 'sflip.inside_kept'], _quad([0] * 6), [look, ('sflip', 4)], [0, 1, 1, 0, 0, 0])
    add('S of zero, tilted camera', ['sflip.sign0'], _quad([0] * 6), [look, ('sflip', 4)], [0, 1, 1, 0, 0, 0], TILTED)
    add('the flipped pose is better', ['sflip.inside_taken'], _quad([-1, 0, 0, 0, 0, 0]), [look, ('sflip', 4)], [1, 0, 0, 0, 0, 0])
    add('the flipped pose is worse', ['sflip.inside_kept'], _quad([1, 0, 0, 0, 0, 0]), [look, ('sflip', 4)], [1, 0, 0, 0, 0, 0])
    add('the flipped pose ties', ['sflip.inside_kept'], _const(2.0), [look, ('sflip', 4)], [1, 0, 0, 0, 0, 0])
    add('flipped beyond the lower limit', ['sflip.outside', 'sflip.endpoint_kept'], _quad([2.9375, 0, 0, 0, 0, 0]), [look, ('sflip', 4)], [2.9375, 0, 0, 0, 0, 0], TILTED)
    add('flipped beyond the upper limit, the endpoint wins', ['sflip.outside', 'sflip.endpoint_taken'], _quad([3, 0, 0, 0, 0, 0]), [look, ('sflip', 4)],
        [-2.9375, 0, 0, 0, 0, 0], [0, -1.5, .75, 0, 0, -0.1])
    add('flipped within 0.15 of the lower limit', ['sflip.close', 'sflip.inside_kept', 'sflip.endpoint_kept'], _quad([2.875, 0, 0, 0, 0, 0]), [look, ('sflip', 4)],
        [2.875, 0, 0, 0, 0, 0])
    add('flipped within 0.15 of the upper limit', ['sflip.close', 'sflip.endpoint_taken'], _quad([3, 0, 0, 0, 0, 0]), [look, ('sflip', 4)], [-2.875, 0, 0, 0, 0, 0])
    # an accepted flip IS temp, and the endpoint loop writes the upper limit into it whatever the comparison says (predict.py:270-277)
    add('an accepted flip is moved to the upper limit', ['sflip.close', 'sflip.inside_taken', 'sflip.endpoint_kept'], _quad([-2.875, 0, 0, 0, 0, 0]),
        [look, ('sflip', 4)], [2.875, 0, 0, 0, 0, 0])
    add('the flip lands exactly on the limit', ['sflip.close', 'sflip.inside_taken'], _quad([-3, 0, 0, 0, 0, 0]), [look, ('sflip', 4)], [3.0, 0, 0, 0, 0, 0])
    # ---- InterpolativeSweep
    add('nothing beats the start', ['isweep.which0', 'isweep.whole_range'], _quad([0, 0, 1, 0, 0, 0]), [look, ('isweep', 6, 5, 'U', None)], [0, 0, 1, 0, 0, 0])
    add('minimum at the sweep end', ['isweep.which1'], lambda a, n, loss: 10.0 - a[2], [look, ('isweep', 6, 4, 'U', 0.125)], [0, 0, 1, 0, 0, 0])
    add('minimum between the samples', ['isweep.which2'], _quad([0, 0, 1.0625, 0, 0, 0]), [look, ('isweep', 6, 4, 'U', 0.5)], [0, 0, 1.25, 0, 0, 0])
    add('range clipped below only', ['isweep.clip_lo', 'isweep.which2'], _quad([0, 0, -2.3, 0, 0, 0]), [look, ('isweep', 6, 5, 'U', 0.125)], [0, 0, -2.3125, 0, 0, 0])
    add('range clipped above only', ['isweep.clip_hi'], _quad([0, 2.48, 0, 0, 0, 0]), [look, ('isweep', 6, 5, 'L', 0.125)], [0, 2.4375, 0, 0, 0, 0])
    add('range wider than the limits', ['isweep.clip_lo', 'isweep.clip_hi'], _quad([1, 0, 0, 0, 0, 0]), [look, ('isweep', 4, 8, 'S', 10.0)], [0.5, 0, 0, 0, 0, 0])
    add('range smaller than min_ang_inc', ['isweep.which2'], _quad([0, 0, 1.00047, 0, 0, 0]), [look, ('isweep', 6, 4, 'U', 0.001)], [0, 0, 1, 0, 0, 0])
    add('a NaN among the samples', ['isweep.nan_spline'], nan_in(2, 1.05, 1.2, _quad([0, 0, 1, 0, 0, 0])), [look, ('isweep', 6, 6, 'U', 0.25)], [0, 0, 1, 0, 0, 0])
    add('all NaN', ['isweep.nan_spline', 'isweep.which0'], _const(NAN), [look, ('isweep', 6, 4, 'SLU', 0.25)], [0.5, 0.5, 1, 0, 0, 0])
    # ---- TensorSweep
    add('one division, whole range', ['tsweep.one_division', 'tsweep.whole_range'], _quad([0, 0, 1, 0, 0, 0]), [look, ('tsweep', 6, 1, 'U', None)], [0, 0, 1, 0, 0, 0])
    add('one division, clipped above', ['tsweep.one_division', 'tsweep.clip_hi'], _quad([0, 0, 1, 0, 0, 0]), [look, ('tsweep', 6, 1, 'SL', 0.25), ('sflip', 4)],
        [0.5, 2.375, 1, 0, 0, 0])
    add('two divisions clipped below', ['tsweep.clip_lo'], _quad([-3, 0, 0, 0, 0, 0]), [look, ('tsweep', 4, 2, 'S', 0.25)], [-2.875, 0, 0, 0, 0, 0])
    add('minimum at the sweep end', ['tsweep.whole_range'], lambda a, n, loss: -a[1], [look, ('tsweep', 4, 4, 'L', None)], [0, 0, 0, 0, 0, 0])
    add('every score NaN', ['tsweep.all_nan'], only(orc.LOSS_TSWEEP, NAN, _quad([0] * 6)), [look, ('tsweep', 6, 3, 'LU', 0.5), _descent('S', 2, half)], [1, 1, 1, 0, 0, 0])
    add('every score ties', ['tsweep.clip_lo', 'tsweep.clip_hi'], _const(-1.0), [look, ('tsweep', 6, 4, 'R', 10.0)], [0, 0, 0, 1, 0, 0])
    return out
