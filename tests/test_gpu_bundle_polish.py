"""GPU: the native camera and bundle polish (csrc/rope_bundle_polish.hip) against the plain-loop restatement of its contract
(tests/bundle_polish_ref.py) — the pool, both steps and both variances bit for bit on fabricated words, rope_refine_bundle byte for
byte against the restatement's loop driven through the step exports and the engine's own renders and equations, its determinism,
what every entry refuses, BundleRefiner(native=True) against the host loop, and the switches of calibrate.py and the camera
predictors.  No tolerance enters the bit-for-bit cases: both sides do one IEEE operation per written operation."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR
from rope_s3d_amd.projection import Intrinsics, camera_matrix

import bundle_polish_ref as br
import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
E_ARG = -1
GARBAGE = float(np.frombuffer(b'\x5a' * 8, np.float64)[0])
CLIP = 2.0 ** -5
FRAME_COUNTS = (1, 2, 64, 65, 130)                      # one workgroup, its edge, a second and a third
SLOT_MASKS = (0, 4095, 0b111111000111, 0b000100000000, 0b000000000101, 0b010101101010)
# BundleRefiner(native=True) against the host loop on the frames below: the largest differences an MI355X gave
# (profiles/bundle_native.txt), per unknown; the assertion stands at 100 times these — other LAPACK builds round in other orders —
# and never above 1e-3 of the unknown's smallest finite formal sigma on those frames
RECORDED = {'frame': dict(pose=1.12e-16, angles=2.23e-16, sigma=5.09e-16), 'offset': dict(pose=6.94e-17, angles=5.56e-17, offsets=5.30e-17, sigma=3.42e-14)}


def same(a, b) -> bool:
    """the same bits, NaN compared as NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope='module')
def scene():
    """The engine at 160 x 120 with the robot under the golden set's camera."""
    intr, PV = helpers.camera('640_480_color', 4)
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    yield e, intr
    e.close()


# ---------------------------------------------------------------------------------------------- the kernels on fabricated words
@pytest.mark.parametrize('n, dead', [(n, False) for n in FRAME_COUNTS] + [(2, True), (65, True)])
def test_pool_steps_and_variances_bit_for_bit(scene, n, dead):
    """dead: no frame has camera columns, so kc is empty"""
    e, _ = scene
    words = br.fabricated_batch(n, camera_dead=dead)
    rng = np.random.default_rng(n)
    q, pose, off = rng.uniform(-1.5, 1.5, (n, 6)), rng.uniform(-1, 1, 6), rng.uniform(-.01, .01, 6)
    pooled = br.pool(words)
    assert same(host(e.bundle_pool(words)), pooled)
    clipped = False
    for jm, cm in br.MASKS:
        for lam in (0.0, 1e-3):
            t_q, t_pose = e.bundle_schur_step(words, pooled, q, pose, lam, jm, cm, br.LIMITS)
            w_q, w_pose = br.schur_step(words, pooled, q, pose, lam, jm, cm, br.LIMITS)
            assert same(host(t_q), w_q) and same(host(t_pose), w_pose), (n, dead, jm, cm, lam, np.argwhere(host(t_q) != w_q)[:4])
            clipped = clipped or bool(((w_q == br.LIMITS[:, 0]) | (w_q == br.LIMITS[:, 1])).any())
        v_q, v_pose = e.bundle_schur_variance(words, pooled, jm, cm)
        x_q, x_pose = br.schur_variance(words, pooled, jm, cm)
        assert same(host(v_q), x_q) and same(host(v_pose), x_pose), (n, dead, jm, cm)
    assert clipped
    few = br.fabricated_batch(n, camera_dead=dead, inliers=1.0)             # pooled inliers below p + 1
    v_q, v_pose = e.bundle_schur_variance(few, br.pool(few), 63, 63)
    x_q, x_pose = br.schur_variance(few, br.pool(few), 63, 63)
    assert same(host(v_q), x_q) and same(host(v_pose), x_pose) and np.isinf(x_q).all() and np.isinf(x_pose).all()
    for sm in SLOT_MASKS:
        for lam in (0.0, 1e-3):
            got = e.bundle_columns_step(pooled, lam, sm, pose, off, q, br.LIMITS)
            want = br.columns_step(pooled, lam, sm, pose, off, q, br.LIMITS)
            assert all(same(host(g), w) for g, w in zip(got, want)), (n, dead, sm, lam)
        assert same(host(e.bundle_columns_variance(pooled, sm)), br.columns_variance(pooled, sm)), (n, dead, sm)
    # the edges are reached: a frame that leaves the sums, finite and infinite variances, a dead camera
    x_q, x_pose = br.schur_variance(words, pooled, 63, 63)
    if n >= 65:                                         # (at n = 65 the last frame, without camera columns, stands at 64)
        assert np.isinf(x_q[63]).all() and np.isinf(x_q[64]).all() == (n > 65) and np.isfinite(x_q[1]).all() and np.isfinite(x_pose).all() != dead


# ---------------------------------------------------------------------------------------------- the loop
def _frames(e, intr, n, seed=1):
    """n frames of the golden set's poses (its three, their mean, and S / L / U shifted copies), rendered under the true camera as
    depth frames with holes; the start: the camera within 5 mm and 4 mrad, S, L and U within 0.0075 rad (tests/test_gpu_bundle.py)."""
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'camera_160x120.npz'))
    rng = np.random.default_rng(seed)
    slu = np.array([1, 1, 1, 0, 0, 0])
    base = np.asarray(gold['joint_poses'], np.float64)
    poses = [base[0], base[1], base[2], base.mean(axis=0)]
    while len(poses) < n:
        poses.append(base[len(poses) % 3] + rng.uniform(-.3, .3, 6) * slu)
    truth = np.stack(poses[:n])
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])
    start_pose = true_pose + rng.uniform(-1, 1, 6) * np.array([.005, .005, .005, .004, .004, .004])
    start = truth + rng.uniform(-.0075, .0075, (n, 6)) * slu
    T = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (n, 1, 1)))[0].clone()
    T[:, ::7, ::5] = 0.0
    return truth, true_pose, start, start_pose, T.contiguous()


CASES = {'frame': ('frame', 0b000111, 63), 'offset': ('offset', 0b000111, 63), 'camera': ('frame', 0, 63)}
KEYS = ('pose', 'angles', 'offsets', 'var_pose', 'var_joints', 'frame_cost', 'words')


def _restated(e, intr, mode, jm, cm, pose, start, T, limits, iterations, damping):
    """bundle_polish_ref.refine driven through the step exports and the engine's own render and equations call"""
    n = len(start)
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)

    def equations(p, q):
        Rwc, tc, tw = eng.camera_twists(p)
        rd, ri = e.render_batch_device(np.ascontiguousarray(q), 6, np.tile(camera_matrix(p, intr)[None], (n, 1, 1)))
        axes = e.joint_axes_device(q, Rwc, tc) if jm else None
        words = e.bundle_normal_equations(rd, ri, T, axes, np.tile(tw[None], (n, 1, 1)) if cm else None, 6, CLIP, intr4)
        return words, host(e.bundle_pool(words))

    def step(words, pooled, q, q0, p, off, lam):
        if mode == 'frame':
            t_q, t_pose = e.bundle_schur_step(words, pooled, q, p, lam, jm, cm, limits)
            return host(t_pose), off, host(t_q)
        t_pose, t_off, t_q = e.bundle_columns_step(pooled, lam, jm | (cm << 6), p, off, q0, limits)
        return host(t_pose), host(t_off), host(t_q)

    def variance(words, pooled):
        if mode == 'frame':
            v_q, v_pose = e.bundle_schur_variance(words, pooled, jm, cm)
            return host(v_pose), host(v_q)
        v = host(e.bundle_columns_variance(pooled, jm | (cm << 6)))
        return v[6:].copy(), v[:6].copy()

    return br.refine(mode, pose, start, equations, step, variance, iterations, damping)


def _native(e, intr, mode, jm, cm, pose, start, T, limits, iterations, damping):
    return e.refine_bundle(mode, pose, start, T, (intr.fx, intr.fy, intr.cx, intr.cy), ZNEAR, ZFAR, jm, cm, limits, CLIP, iterations, damping,
                           want_words=True)


def _hold(got, want):
    for k in KEYS:
        assert same(got[k], want[k]), (k, got[k], want[k])
    assert got['steps'] == want['steps'] and same(np.array([got['cost_before'], got['cost_after'], got['inliers']]), want['costs'])


@pytest.mark.parametrize('iterations, damping', [(0, 1e-3), (1, 0.0), (5, 1e-3)])
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('n', [3, 8])
def test_refine_bundle_returns_the_bytes_of_the_restated_loop(scene, n, case, iterations, damping):
    e, intr = scene
    mode, jm, cm = CASES[case]
    limits = np.asarray(helpers.robot().joint_limits, np.float64)
    truth, true_pose, start, start_pose, T = _frames(e, intr, n)
    got = _native(e, intr, mode, jm, cm, start_pose, start, T, limits, iterations, damping)
    want = _restated(e, intr, mode, jm, cm, start_pose, start, T, limits, iterations, damping)
    print(case, n, iterations, damping, 'steps', got['steps'], 'trial costs', want['trial_costs'])
    _hold(got, want)
    assert got['cost_after'] <= got['cost_before'] and 0 <= got['steps'] <= iterations
    assert np.array_equal(got['angles'][:, 3:], start[:, 3:]) and (jm or np.array_equal(got['angles'], start))
    if iterations == 5:
        assert got['steps'] >= 1 and got['cost_after'] < got['cost_before']
        again = _native(e, intr, mode, jm, cm, start_pose, start, T, limits, iterations, damping)      # twice the same bytes
        for k in KEYS:
            assert same(again[k], got[k]), k


def test_refine_bundle_on_a_tiny_frame():
    e = eng.Engine(0)
    try:
        e.set_robot(helpers.robot())
        intr = Intrinsics('640_480_color')
        intr.downscale(80)
        assert (intr.width, intr.height) == (8, 6)
        e.set_camera(camera_matrix(DEFAULT_CAMERA_POSE, intr, ZNEAR, ZFAR), intr.width, intr.height, ZNEAR, ZFAR)
        limits = np.asarray(helpers.robot().joint_limits, np.float64)
        _, _, start, start_pose, T = _frames(e, intr, 1)
        for mode, jm, cm in CASES.values():
            _hold(_native(e, intr, mode, jm, cm, start_pose, start, T, limits, 5, 1e-3),
                  _restated(e, intr, mode, jm, cm, start_pose, start, T, limits, 5, 1e-3))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- against the host loop
@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_native_refiner_against_the_host_loop(scene, mode):
    """BundleRefiner(native=True) and BundleRefiner() on the same 8 frames.  The conditions: the accept / reject sequence (read off
    runs of 1 .. 5 rounds: every run is a prefix of the next) and steps_taken are equal, and no decision of the loop is a near
    tie (the margin between a trial's cost and the cost held is above 1e-6 of the cost, as tests/test_gpu_bundle.py asks of its
    seeds).  The differences are printed; RECORDED keeps what an MI355X gave."""
    from rope_s3d_amd.prediction.refinement import BundleRefiner
    e, intr = scene
    limits = np.asarray(helpers.robot().joint_limits, np.float64)
    truth, true_pose, start, start_pose, T = _frames(e, intr, 8)
    want = _restated(e, intr, mode, 0b111, 63, start_pose, start, T, limits, 5, 1e-3)
    held, margins = want['trial_costs'][0], []
    for c in want['trial_costs'][1:]:
        margins.append(abs(c - held) / held)
        held = min(held, c)
    print(mode, 'native trial costs', want['trial_costs'], 'relative margins', margins)
    assert min(margins) > 1e-6, "choose another seed: a decision of the loop is a near tie"
    seq = {True: [], False: []}
    for native in (False, True):
        for k in range(1, 6):
            r = BundleRefiner(e, intr, joints=mode, iterations=k, native=native).refine(start_pose, start, T)
            seq[native].append((r.steps_taken, r.cost_after))
    print(mode, 'host (steps, cost) after 1 .. 5 rounds', seq[False], 'native', seq[True])
    assert [s for s, _ in seq[True]] == [s for s, _ in seq[False]]
    a = BundleRefiner(e, intr, joints=mode).refine(start_pose, start, T)
    b = BundleRefiner(e, intr, joints=mode, native=True).refine(start_pose, start, T)
    assert b.steps_taken == a.steps_taken >= 1 and b.inliers == a.inliers and b.cost_after <= b.cost_before
    sig_a = a.sigma_angles[:, :3] if mode == 'frame' else a.sigma_offsets[:3]
    sig_b = b.sigma_angles[:, :3] if mode == 'frame' else b.sigma_offsets[:3]
    diff = dict(pose=np.abs(b.pose - a.pose), angles=np.abs(b.angles - a.angles)[:, :3].max(axis=0),
                sigma=np.concatenate([np.abs(b.sigma_pose - a.sigma_pose), np.abs(sig_b - sig_a).reshape(-1, 3).max(axis=0)]))
    floor = dict(pose=a.sigma_pose, angles=sig_a.reshape(-1, 3).min(axis=0), sigma=np.concatenate([a.sigma_pose, sig_a.reshape(-1, 3).min(axis=0)]))
    if mode == 'offset':
        diff['offsets'], floor['offsets'] = np.abs(b.offsets - a.offsets)[:3], a.sigma_offsets[:3]
    for k in diff:
        print(f"{mode}: |native - host| {k} {diff[k]}  smallest formal sigma {floor[k]}")
        assert np.isfinite(floor[k]).all()
        bound = 1e-3 * floor[k] if RECORDED[mode][k] is None else np.minimum(100.0 * RECORDED[mode][k], 1e-3 * floor[k])
        assert (diff[k] <= bound).all(), (k, diff[k], bound)
    assert type(b.steps_taken) is type(a.steps_taken) and b.frame_cost.shape == a.frame_cost.shape == (8,)
    if mode == 'frame':
        assert np.isnan(b.offsets).all() and b.sigma_offsets is None and np.isnan(b.sigma_angles[:, 3:]).all()
    else:
        assert b.sigma_angles is None and not b.offsets[3:].any() and np.isnan(b.sigma_offsets[3:]).all()
    with pytest.raises(ValueError):
        BundleRefiner(e, intr, silhouette=1.0, native=True)


# ---------------------------------------------------------------------------------------------- what the entries refuse
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _untouched(t):
    return bool((t.cpu().numpy().view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all())


def test_kernel_entries_refuse_and_leave_the_outputs_alone():
    lib = eng.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 4
    words = br.fabricated_batch(n)
    bad_lim = br.LIMITS.copy()
    bad_lim[2] = bad_lim[2, ::-1]
    nan_lim = br.LIMITS.copy()
    nan_lim[0, 1] = np.nan

    def run(entry, ins, outs, ints, case):
        """ins / outs: device tensors by position; ints: {position: value}; the call's arguments are assembled in `order`"""
        fresh = [torch.full(o, GARBAGE, dtype=torch.float64, device='cuda') for o in outs]
        tensors = ins + fresh
        ptr = lambda k: None if case.get('null') == k else C.c_void_p(tensors[k].data_ptr() + (4 if case.get('odd') == k else 0))
        lim = case.get('limits', br.LIMITS)
        lim_p = None if lim is None else np.ascontiguousarray(lim, np.float64).ctypes.data_as(C.c_void_p)
        rc = entry(ptr, {k: case.get(name, v) for k, (name, v) in ints.items()}, lim_p, stream)
        torch.cuda.synchronize()
        assert rc == E_ARG and all(_untouched(t) for t in fresh), (entry, case)

    work = torch.empty(lib.rope_bundle_schur_workspace(n) // 8, dtype=torch.float64, device='cuda')
    common = [dict(n=0), dict(n=-1)]
    limit_cases = [dict(limits=bad_lim), dict(limits=nan_lim), dict(limits=None)]
    # rope_bundle_pool: 0 words, 1 pooled
    for case in common + [dict(null=0), dict(null=1), dict(odd=0), dict(odd=1)]:
        run(lambda p, i, l, s: lib.rope_bundle_pool(p(0), i[0], p(1), s), [_dev(words)], [(96,)], {0: ('n', n)}, case)
    # rope_bundle_schur_step: 0 words, 1 pooled, 2 q, 3 pose, 4 lam, 5 work | 6 trial_q, 7 trial_pose
    ins = [_dev(words), _dev(br.pool(words)), _dev(np.zeros((n, 6))), _dev(np.zeros(6)), _dev(np.zeros(1)), work]
    for case in common + [dict(jm=-1), dict(jm=64), dict(cm=-1), dict(cm=64)] + limit_cases + [dict(null=k) for k in range(8)] + \
            [dict(odd=k) for k in range(8)]:
        run(lambda p, i, l, s: lib.rope_bundle_schur_step(p(0), p(1), p(2), p(3), p(4), i[0], i[1], i[2], l, p(5), p(6), p(7), s), ins,
            [(n + 1, 6), (7,)], {0: ('n', n), 1: ('jm', 7), 2: ('cm', 63)}, case)
    # rope_bundle_schur_variance: 0 words, 1 pooled, 2 work | 3 var_q, 4 var_pose
    ins = [_dev(words), _dev(br.pool(words)), work]
    for case in common + [dict(jm=-1), dict(jm=64), dict(cm=-1), dict(cm=64)] + [dict(null=k) for k in range(5)] + [dict(odd=k) for k in range(5)]:
        run(lambda p, i, l, s: lib.rope_bundle_schur_variance(p(0), p(1), i[0], i[1], i[2], p(2), p(3), p(4), s), ins, [(n + 1, 6), (7,)],
            {0: ('n', n), 1: ('jm', 7), 2: ('cm', 63)}, case)
    # rope_bundle_columns_step: 0 pooled, 1 lam, 2 pose, 3 off, 4 q0 | 5 trial_pose, 6 trial_off, 7 trial_q
    ins = [_dev(br.pool(words)), _dev(np.zeros(1)), _dev(np.zeros(6)), _dev(np.zeros(6)), _dev(np.zeros((n, 6)))]
    for case in common + [dict(sm=-1), dict(sm=4096)] + limit_cases + [dict(null=k) for k in range(8)] + [dict(odd=k) for k in range(8)]:
        run(lambda p, i, l, s: lib.rope_bundle_columns_step(p(0), p(1), i[1], p(2), p(3), p(4), i[0], l, p(5), p(6), p(7), s), ins,
            [(7,), (7,), (n + 1, 6)], {0: ('n', n), 1: ('sm', 4095)}, case)
    # rope_bundle_columns_variance: 0 pooled | 1 var
    for case in [dict(sm=-1), dict(sm=4096), dict(null=0), dict(null=1), dict(odd=0), dict(odd=1)]:
        run(lambda p, i, l, s: lib.rope_bundle_columns_variance(p(0), i[0], p(1), s), [_dev(br.pool(words))], [(13,)], {0: ('sm', 4095)}, case)
    # rope_camera_twists: host pointers
    pose, out = np.zeros(6), [np.full(9, GARBAGE), np.full(3, GARBAGE), np.full(36, GARBAGE)]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = pose.copy()
    bad[4] = np.inf
    for args in ((None, vp(out[0]), vp(out[1]), vp(out[2])), (vp(pose), None, vp(out[1]), vp(out[2])), (vp(pose), vp(out[0]), None, vp(out[2])),
                 (vp(pose), vp(out[0]), vp(out[1]), None), (vp(bad), vp(out[0]), vp(out[1]), vp(out[2]))):
        assert lib.rope_camera_twists(*args) == E_ARG and all((o.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all() for o in out)


def test_refine_bundle_refuses_and_leaves_the_outputs_alone(scene):
    e, intr = scene
    lib = eng.load_library()
    limits = np.ascontiguousarray(helpers.robot().joint_limits, np.float64)
    _, _, start, start_pose, T = _frames(e, intr, 2)
    bad_lim = limits.copy()
    bad_lim[1] = bad_lim[1, ::-1]
    nan_q = start.copy()
    nan_q[1, 2] = np.nan
    work = torch.empty(e.refine_bundle_workspace(2) // 8 + 1, dtype=torch.float64, device='cuda')
    bare = eng.Engine(0)                                            # neither robot nor camera
    no_camera = eng.Engine(0)
    no_camera.set_robot(helpers.robot())
    base = dict(ctx=e._ctx, mode=0, pose=np.ascontiguousarray(start_pose), q=start, depth=T.data_ptr(), n=2, fx=float(intr.fx), znear=ZNEAR, zfar=ZFAR,
                jm=7, cm=63, limits=limits, clip=CLIP, iterations=2, damping=1e-3, work=work.data_ptr())
    cases = [dict(n=0), dict(n=-1), dict(n=65536), dict(mode=2), dict(mode=-1), dict(jm=-1), dict(jm=64), dict(cm=-1), dict(cm=64), dict(jm=0, cm=0),
             dict(limits=bad_lim), dict(limits=None), dict(clip=0.0), dict(clip=float('nan')), dict(iterations=-1), dict(damping=-1.0),
             dict(damping=float('nan')), dict(damping=float('inf')), dict(work=None), dict(work=work.data_ptr() + 4), dict(depth=None),
             dict(depth=T.data_ptr() + 2), dict(q=nan_q), dict(q=None), dict(pose=None), dict(fx=0.0), dict(fx=float('inf')), dict(znear=0.0),
             dict(zfar=ZNEAR), dict(ctx=bare._ctx), dict(ctx=no_camera._ctx)] + [dict(null_out=k) for k in range(8)]
    try:
        for case in cases:
            a = dict(base)
            a.update(case)
            outs = [np.full(6, GARBAGE), np.full((2, 6), GARBAGE), np.full(6, GARBAGE), np.full(6, GARBAGE), np.full((2, 6), GARBAGE), np.full(3, GARBAGE),
                    np.full(1, 0x5a5a5a5a, np.int32), np.full(2, GARBAGE), np.full((2, 96), GARBAGE)]
            keep = [o.copy() for o in outs]
            vp = lambda x: None if x is None else (C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))
            qa = None if a['q'] is None else np.ascontiguousarray(a['q'])
            ptrs = [None if a.get('null_out') == k else vp(o) for k, o in enumerate(outs)]
            rc = lib.rope_refine_bundle(a['ctx'], a['mode'], vp(a['pose']), vp(qa), vp(a['depth']), a['n'], a['fx'], float(intr.fy), float(intr.cx),
                                        float(intr.cy), a['znear'], a['zfar'], a['jm'], a['cm'], vp(a['limits']), a['clip'], a['iterations'], a['damping'],
                                        vp(a['work']), *ptrs)
            assert rc == E_ARG and all(o.tobytes() == k.tobytes() for o, k in zip(outs, keep)), case
    finally:
        bare.close()
        no_camera.close()
    assert eng.Engine.refine_bundle_workspace(e, 0) == 0 and e.refine_bundle_workspace(2) > 0
    # and the engine's wrapper says so before the library is asked
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
    for kw in (dict(mode='both'), dict(jm=64), dict(jm=0, cm=0), dict(iterations=-1), dict(damping=-1.0)):
        a = dict(mode='frame', jm=7, cm=63, iterations=2, damping=1e-3)
        a.update(kw)
        with pytest.raises(ValueError):
            e.refine_bundle(a['mode'], start_pose, start, T, intr4, ZNEAR, ZFAR, a['jm'], a['cm'], limits, CLIP, a['iterations'], a['damping'])
    with pytest.raises(ValueError):
        e.refine_bundle('frame', start_pose, start, T[:1], intr4, ZNEAR, ZFAR, 7, 63, limits, CLIP, 2, 1e-3)


# ---------------------------------------------------------------------------------------------- the switches
def test_calibrate_native_returns_what_the_host_run_returns(tmp_path):
    """calibrate.py on a synthetic set of 8 frames, 'offset' mode: the set plants no encoder error, so the offsets come back near
    0 on both paths, the same steps taken, and every offset and pose parameter within 1e-3 of its formal sigma of the host run's."""
    reps = {}
    for native in (False, True):
        out = tmp_path / f'{native}.json'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'calibrate.py'), 'synthetic:8', '-frames', '8', '-joints', 'offset', '-ds_factor', '8',
                            '-iterations', '3', '-json', str(out)] + (['-native'] if native else []), cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        reps[native] = json.loads(out.read_text())
    a, b = reps[False], reps[True]
    print('host', a['offsets'], a['pose'], 'native', b['offsets'], b['pose'])
    assert b['native'] is True and a['native'] is False and b['steps_taken'] == a['steps_taken'] and b['inliers'] == a['inliers']
    for k in ('offsets', 'pose'):
        sig = np.array(a['sigma_' + k], float)
        d = np.abs(np.array(b[k], float) - np.array(a[k], float))
        live = np.isfinite(sig)
        assert (d[live] <= 1e-3 * sig[live]).all() and not d[~live].any(), (k, d, sig)
    assert np.abs(np.array(b['offsets'][:3])).max() < 1e-3


def test_predictor_switch_bundle_native_and_the_default_alone():
    from rope_s3d_amd import ModellessCameraPredictor
    from rope_s3d_amd.prediction.refinement import BundleRefineResult, BundleRefiner
    from rope_s3d_amd.simulation.render import Renderer
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])
    r = Renderer('seg', true_pose, '640_480_color')
    lim = r.robot.joint_limits
    qs = np.random.default_rng(9).uniform(lim[:, 0] * .5, lim[:, 1] * .5, (4, 6)) * np.array([1, 1, 1, 0, 0, 0])
    colors, depths = [], []
    for q in qs:
        r.setJointAngles(q)
        c, d = r.render()
        colors.append(c); depths.append(np.asarray(d, np.float64))
    r.engine.close()
    start = true_pose + np.array([.004, -.003, .003, .002, -.002, .002])

    def run(refine):
        p = ModellessCameraPredictor(start, 4, base_intrinsics='640_480_color', refine=refine)
        p.stages = [('descent', 6, 0.5, .001, [True] * 6, [0.002] * 6)]
        return p, p.run(np.stack(colors), np.stack(depths), qs)

    off, before = run(False)
    host_p, host_pose = run('bundle')
    nat_p, nat_pose = run('bundle+native')
    try:
        res = nat_p.last_refinement
        assert nat_p.refine == 'bundle+native' and nat_p._refiner.native and isinstance(res, BundleRefineResult) and np.array_equal(nat_pose, res.pose)
        assert res.steps_taken == host_p.last_refinement.steps_taken and res.cost_after <= res.cost_before and res.angles.shape == (4, 6)
        assert (np.abs(nat_pose - host_pose) <= 1e-3 * host_p.last_refinement.sigma_pose).all()
        # the default paths: the switch off leaves the stages' pose, 'bundle' is the host loop's bytes
        assert off.last_refinement is None and not host_p._refiner.native
        by_hand = BundleRefiner(host_p.renderer, host_p.renderer.intrinsics).refine(before, qs, np.asarray(host_p._tgt_depths, np.float32))
        assert host_pose.tobytes() == by_hand.pose.tobytes() and host_p.last_refinement.sigma_pose.tobytes() == by_hand.sigma_pose.tobytes()
    finally:
        for p in (off, host_p, nat_p):
            p.engine.close()
