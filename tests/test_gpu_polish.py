"""GPU: the native polish (csrc/rope_polish.hip) against the plain-loop restatement of its contract (tests/polish_ref.py) — the
step, the variances and the joint axes bit for bit, rope_refine_poses byte for byte against the restatement's loop driven with the
engine's own renders and equations, its determinism, what every entry refuses, PoseRefiner(native=True) against the host loop,
and the Predictor's switch.  No tolerance enters the bit-for-bit cases: both sides do one IEEE operation per written operation."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR
from rope_s3d_amd.projection import Intrinsics, camera_matrix

import helpers
import polish_ref as pr
from test_polish_refs import TILTED_POSE, axes_poses

pytestmark = pytest.mark.gpu

E_ARG = -1
GARBAGE = float(np.frombuffer(b'\x5a' * 8, np.float64)[0])
FRAME_COUNTS = (1, 63, 64, 65, 257)
CLIP = 2.0 ** -5


def same(a, b) -> bool:
    """the same bits, NaN compared as NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _intrinsics(preset, ds):
    intr = Intrinsics(preset)
    intr.downscale(ds)
    return intr


@pytest.fixture(scope='module')
def scene():
    """The engine with the robot (mh5l) at 160 x 90 under a tilted camera."""
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    intr = _intrinsics('1280_720_color', 8)
    e.set_camera(camera_matrix(TILTED_FRAME_POSE, intr, ZNEAR, ZFAR), intr.width, intr.height, ZNEAR, ZFAR)
    yield e, intr
    e.close()


TILTED_FRAME_POSE = np.asarray(DEFAULT_CAMERA_POSE, np.float64) + np.array([0.02, -0.03, 0.01, 0.02, -0.015, 0.01])


def _table_frames(n):
    table = pr.system_table()
    rows = [table[f % len(table)] for f in range(n)]
    return (np.stack([r[1] for r in rows]), np.array([r[2] for r in rows]), np.stack([r[3] for r in rows]))


@pytest.mark.parametrize('n', FRAME_COUNTS)
def test_step_and_variance_bit_for_bit(scene, n):
    e, _ = scene
    words, lam, q = _table_frames(n)
    for mask in pr.MASKS:
        got = e.levenberg_step(words, q, lam, mask, pr.LIMITS).cpu().numpy()
        assert same(got, pr.levenberg_step(words, q, lam, mask, pr.LIMITS)), (n, mask)
        var = e.formal_variance(words, mask).cpu().numpy()
        want = pr.formal_variance(words, mask)
        assert same(var, want), (n, mask, np.argwhere(~((var == want) | (np.isnan(var) & np.isnan(want))))[:4])
        assert np.isnan(var[:, [j for j in range(6) if not (mask >> j) & 1]]).all()
    # the table reaches every path: steps taken and refused, finite and infinite variances
    moved = (e.levenberg_step(words, q, lam, 63, pr.LIMITS).cpu().numpy() != q).any(axis=1)
    if n >= 20:
        assert moved.any() and not moved.all() and np.isinf(var).any() and np.isfinite(var).any()


@pytest.mark.parametrize('n', FRAME_COUNTS)
def test_axes_bit_for_bit(scene, n):
    e, _ = scene
    rb = helpers.robot()
    poses = axes_poses(np.asarray(rb.joint_limits, np.float64))
    q = poses[np.arange(n) % len(poses)]
    Rwc, tc = pr.camera_axes(TILTED_POSE)
    got = e.joint_axes_device(q, Rwc, tc).cpu().numpy()
    want = pr.joint_axes(poses, rb.joint_fixed, rb.joint_axes, Rwc, tc)[np.arange(n) % len(poses)]
    assert same(got, want), np.abs(got - want).max()


# ---------------------------------------------------------------------------------------------- the loop
def _frames(e, n, seed):
    """n poses of the robot, their renders as depth frames with holes, and starts 0.01 .. 0.02 rad off on S, L and U."""
    rng = np.random.default_rng(seed)
    lim = np.asarray(helpers.robot().joint_limits, np.float64)
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
    off = rng.uniform(.01, .02, (n, 6)) * rng.choice([-1.0, 1.0], (n, 6)) * np.array([1, 1, 1, 0, 0, 0])
    T = e.render_batch_device(truth, min(e.n_links, 6))[0].clone()
    T[:, ::7, ::5] = 0.0
    return truth, truth + off, T.contiguous()


def _reference_loop(e, intr, pose, start, T, mask, iterations, damping):
    rb = helpers.robot()
    Rwc, tc = pr.camera_axes(pose)
    n_links = min(e.n_links, 6)
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)

    def equations(q):
        rd, ri = e.render_batch_device(q, n_links)
        return e.pose_normal_equations(rd, ri, T, pr.joint_axes(q, rb.joint_fixed, rb.joint_axes, Rwc, tc), n_links, CLIP, intr4)

    return pr.refine(start, equations, mask, np.asarray(rb.joint_limits, np.float64), iterations, damping)


KEYS = ('angles', 'var', 'cost_before', 'cost_after', 'steps', 'inliers', 'words')


def _native(e, intr, pose, start, T, mask, iterations, damping):
    return e.refine_poses(start, T, pose, (intr.fx, intr.fy, intr.cx, intr.cy), mask, helpers.robot().joint_limits, CLIP, iterations, damping,
                          want_words=True)


@pytest.mark.parametrize('iterations, damping', [(0, 1e-3), (1, 0.0), (1, 1e-3), (5, 0.0), (5, 1e-3)])
def test_refine_poses_returns_the_bytes_of_the_restated_loop(scene, iterations, damping):
    e, intr = scene
    truth, start, T = _frames(e, 5, 31)
    got = _native(e, intr, TILTED_FRAME_POSE, start, T, 0b111, iterations, damping)
    want = _reference_loop(e, intr, TILTED_FRAME_POSE, start, T, 0b111, iterations, damping)
    for k in KEYS:
        assert same(got[k], want[k]), (k, got[k], want[k])
    assert (got['cost_after'] <= got['cost_before']).all() and (got['steps'] <= iterations).all()
    if iterations == 5:
        assert (got['steps'] >= 1).all() and np.abs(got['angles'] - truth)[:, :3].max() < np.abs(start - truth)[:, :3].max()
        # in one call, or 2 + 3 in two; and twice the same
        parts = [_native(e, intr, TILTED_FRAME_POSE, start[a:b], T[a:b].contiguous(), 0b111, iterations, damping) for a, b in ((0, 2), (2, 5))]
        again = _native(e, intr, TILTED_FRAME_POSE, start, T, 0b111, iterations, damping)
        for k in KEYS:
            assert same(np.concatenate([p[k] for p in parts]), got[k]), k
            assert same(again[k], got[k]), k


def test_refine_poses_on_a_tiny_frame():
    e = eng.Engine(0)
    try:
        e.set_robot(helpers.robot())
        intr = _intrinsics('640_480_color', 20)                 # 32 x 24
        assert (intr.width, intr.height) == (32, 24)
        e.set_camera(camera_matrix(DEFAULT_CAMERA_POSE, intr, ZNEAR, ZFAR), intr.width, intr.height, ZNEAR, ZFAR)
        _, start, T = _frames(e, 1, 4)
        pose = np.asarray(DEFAULT_CAMERA_POSE, np.float64)
        got = _native(e, intr, pose, start, T, 0b111111, 5, 1e-3)
        want = _reference_loop(e, intr, pose, start, T, 0b111111, 5, 1e-3)
        for k in KEYS:
            assert same(got[k], want[k]), (k, got[k], want[k])
    finally:
        e.close()


def test_native_refiner_against_the_host_loop(scene):
    """PoseRefiner(native=True) and PoseRefiner() on the same frames: the same accepted steps, no worse a cost, and every angle
    within the host loop's own formal sigma of the host loop's answer.  Measured (profiles/polish_native.txt): the largest angle
    difference is at the rounding of the solve."""
    from rope_s3d_amd.prediction.refinement import PoseRefiner
    e, intr = scene
    _, start, T = _frames(e, 5, 31)
    host = PoseRefiner(e, TILTED_FRAME_POSE, intr, 'SLU').refine(start, T)
    nat = PoseRefiner(e, TILTED_FRAME_POSE, intr, 'SLU', native=True).refine(start, T)
    print('steps', host.steps_taken, nat.steps_taken, 'largest angle difference', np.abs(host.angles - nat.angles).max(),
          'largest sigma difference', np.nanmax(np.abs(host.sigma - nat.sigma)), 'cost', host.cost_after, nat.cost_after)
    assert (nat.cost_after <= nat.cost_before).all()
    assert np.array_equal(nat.steps_taken, host.steps_taken), (host.cost_after, nat.cost_after)
    assert (np.abs(nat.angles - host.angles)[:, :3] <= host.sigma[:, :3]).all()
    assert np.array_equal(nat.angles[:, 3:], start[:, 3:]) and np.isnan(nat.sigma[:, 3:]).all() and np.isfinite(nat.sigma[:, :3]).all()
    assert nat.steps_taken.dtype == host.steps_taken.dtype and np.array_equal(nat.inliers, host.inliers)
    empty = PoseRefiner(e, TILTED_FRAME_POSE, intr, 'SLU', native=True).refine(np.zeros((0, 6)), T[:0])
    assert len(empty) == 0 and empty.sigma.shape == (0, 6)


# ---------------------------------------------------------------------------------------------- what the entries refuse
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t, null=False, odd=False):
    return None if null else C.c_void_p(t.data_ptr() + (4 if odd else 0))


def test_step_and_variance_refuse_and_leave_the_output_alone():
    lib = eng.load_library()
    words, lam, q = _table_frames(8)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad_limits = []
    for k, v in ((0, np.nan), (3, np.inf), (4, -np.inf)):
        L = pr.LIMITS.copy().reshape(-1)
        L[k] = v
        bad_limits.append(L)
    L = pr.LIMITS.copy()
    L[2] = L[2, ::-1]
    bad_limits.append(L.reshape(-1))
    cases = [dict(n=0), dict(n=-1), dict(mask=-1), dict(mask=64)] + [dict(null=k) for k in range(5)] + [dict(odd=k) for k in (0, 1, 2, 4)] + \
        [dict(limits=L) for L in bad_limits]
    for case in cases:
        t = [_dev(words), _dev(q), _dev(lam), None, torch.full((9, 6), GARBAGE, dtype=torch.float64, device='cuda')]
        lim = np.ascontiguousarray(case.get('limits', pr.LIMITS), np.float64)
        ptrs = [_ptr(x, case.get('null') == k, case.get('odd') == k) if x is not None else None for k, x in enumerate(t)]
        ptrs[3] = None if case.get('null') == 3 else lim.ctypes.data_as(C.c_void_p)
        rc = lib.rope_levenberg_step(ptrs[0], ptrs[1], ptrs[2], case.get('n', 8), case.get('mask', 7), ptrs[3], ptrs[4], stream)
        torch.cuda.synchronize()
        assert rc == E_ARG and (t[4].cpu().numpy().view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case
    for case in [dict(n=0), dict(n=-1), dict(mask=-1), dict(mask=64), dict(null=0), dict(null=1), dict(odd=0), dict(odd=1)]:
        t = [_dev(words), torch.full((9, 6), GARBAGE, dtype=torch.float64, device='cuda')]
        ptrs = [_ptr(x, case.get('null') == k, case.get('odd') == k) for k, x in enumerate(t)]
        rc = lib.rope_formal_variance(ptrs[0], case.get('n', 8), case.get('mask', 7), ptrs[1], stream)
        torch.cuda.synchronize()
        assert rc == E_ARG and (t[1].cpu().numpy().view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case


def test_joint_axes_and_refine_poses_refuse_and_leave_the_outputs_alone(scene):
    e, intr = scene
    lib = eng.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Rwc, tc = pr.camera_axes(TILTED_POSE)
    Rwc = np.ascontiguousarray(Rwc)
    q = _dev(np.zeros((4, 6)))
    for case in [dict(n=0), dict(n=-1), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(odd=0), dict(odd=3), dict(nan=True)]:
        out = torch.full((5, 6, 6), GARBAGE, dtype=torch.float64, device='cuda')
        R = Rwc.copy()
        if case.get('nan'):
            R[1, 1] = np.nan
        ptrs = [_ptr(q, case.get('null') == 0, case.get('odd') == 0), None if case.get('null') == 1 else R.ctypes.data_as(C.c_void_p),
                None if case.get('null') == 2 else tc.ctypes.data_as(C.c_void_p), _ptr(out, case.get('null') == 3, case.get('odd') == 3)]
        rc = lib.rope_joint_axes(e._ctx, ptrs[0], case.get('n', 4), ptrs[1], ptrs[2], ptrs[3], stream)
        torch.cuda.synchronize()
        assert rc == E_ARG and (out.cpu().numpy().view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case

    _, start, T = _frames(e, 2, 31)
    lim = np.ascontiguousarray(helpers.robot().joint_limits, np.float64)
    bad_lim = lim.copy()
    bad_lim[1] = bad_lim[1, ::-1]
    nan_q = start.copy()
    nan_q[1, 2] = np.nan
    work = torch.empty(e.refine_workspace(2) // 8 + 1, dtype=torch.float64, device='cuda')
    pose = np.ascontiguousarray(TILTED_FRAME_POSE)
    base = dict(q=start, n=2, mask=7, limits=lim, clip=CLIP, iterations=2, damping=1e-3, work=work.data_ptr(), depth=T.data_ptr(), pose=pose)
    cases = [dict(n=0), dict(n=-1), dict(mask=-1), dict(mask=64), dict(limits=bad_lim), dict(limits=None), dict(clip=0.0), dict(clip=float('nan')),
             dict(iterations=-1), dict(damping=-1.0), dict(damping=float('nan')), dict(damping=float('inf')), dict(work=None),
             dict(work=work.data_ptr() + 4), dict(depth=None), dict(depth=T.data_ptr() + 2), dict(q=nan_q), dict(q=None), dict(pose=None),
             dict(fx=0.0), dict(fx=float('inf'))]
    for case in cases:
        a = dict(base)
        a.update(case)
        outs = [np.full((2, 6), GARBAGE), np.full((2, 6), GARBAGE), np.full(2, GARBAGE), np.full(2, GARBAGE), np.full(2, 0x5a5a5a5a, np.int32),
                np.full(2, GARBAGE), np.full((2, 32), GARBAGE)]
        keep = [o.copy() for o in outs]
        vp = lambda x: None if x is None else (C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))
        qa = None if a['q'] is None else np.ascontiguousarray(a['q'])
        rc = lib.rope_refine_poses(e._ctx, vp(qa), vp(a['depth']), a['n'], vp(a['pose']), a.get('fx', float(intr.fx)), float(intr.fy), float(intr.cx),
                                   float(intr.cy), a['mask'], vp(a['limits']), a['clip'], a['iterations'], a['damping'], vp(a['work']),
                                   *[vp(o) for o in outs])
        assert rc == E_ARG and all(o.tobytes() == k.tobytes() for o, k in zip(outs, keep)), case
    # and the engine's wrapper says so before the library is asked
    for kw in (dict(active_mask=64), dict(iterations=-1), dict(damping=-1.0)):
        args = dict(active_mask=7, iterations=2, damping=1e-3)
        args.update(kw)
        with pytest.raises(ValueError):
            e.refine_poses(start, T, pose, (intr.fx, intr.fy, intr.cx, intr.cy), args['active_mask'], lim, CLIP, args['iterations'], args['damping'])
    with pytest.raises(ValueError):
        e.refine_poses(start, T[:1], pose, (intr.fx, intr.fy, intr.cx, intr.cy), 7, lim, CLIP, 2, 1e-3)


# ---------------------------------------------------------------------------------------------- the callers
def test_predictor_native_switch_polishes_and_leaves_the_default_alone():
    from rope_s3d_amd import Predictor
    from rope_s3d_amd.prediction.synthetic import SyntheticPredictor
    synth = SyntheticPredictor(DEFAULT_CAMERA_POSE, '640_480_color', 4, 'SLU', noise=False, seed=11, lookup_divisions=4)
    p = synth.predictor
    lim = helpers.robot().joint_limits
    colors, depths = [], []
    for seed in range(8):
        q = np.random.default_rng(50 + seed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
        synth.renderer.setJointAngles(q)
        c, d = synth.renderer.render()
        colors.append(c); depths.append(d)
    before = p.run_many(colors, depths)
    assert p.refine is False and p.last_refinement is None
    on = Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', color_dict=p.color_dict, lookup_divisions=4, refine='native')
    assert on.refine is True and on.refine_native
    polished = on.run_many(colors, depths)
    res = on.last_refinement
    assert on._refiner.native and len(res) == 8 and np.array_equal(res.angles, polished)
    assert np.isfinite(res.sigma[:, :3]).all() and np.isnan(res.sigma[:, 3:]).all() and (res.cost_after <= res.cost_before).all()
    assert np.array_equal(polished[res.steps_taken == 0], before[res.steps_taken == 0]) and np.array_equal(polished[:, 3:], before[:, 3:])
    assert p.run_many(colors, depths).tobytes() == before.tobytes() and p.last_refinement is None
