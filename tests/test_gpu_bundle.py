"""GPU: rope_bundle_normal_equations (csrc/rope_bundle.hip; Engine.bundle_normal_equations) against the numpy restatement of its
contract (tests/bundle_ref.py) and against the two shipped 6-column kernels on the same planes — counts equal, every float sum
within the worst case of a reordered float64 summation — its determinism, what it refuses, BundleRefiner end to end in both modes
against bundle_ref's loops on the engine's own renders, the 'bundle' switch of the two camera predictors, calibrate.py, and the
host loop the refiners share against the restated loops on the words of the same engine calls, byte for byte.

The bound is tests/test_gpu_refine.py's: a sum of n float64 terms added in any order differs from the exact sum by at most
(n - 1) eps sum|terms| to first order, eps = 2^-52; two orders differ by at most twice that, and the terms themselves are the
same bits on both sides.  4 n eps sum|terms| covers it with the second-order terms; n is the pixel count of the frame."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import bundle_ref as bref
import camera_refine_ref as cref
import helpers
import refine_ref
from refine_ref import CLIP, HAND_INTR, HAND_LINKS, hand_planes
from test_bundle_refs import hand_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
E_ARG = -1
EPS = 2.0 ** -52
GARBAGE = float(np.frombuffer(b'\x5a' * 8, np.float64)[0])
COMBOS = ((0, 6), (6, 0), (1, 1), (3, 6), (6, 6))          # (n_joints, n_cols)


def _call(R, ids, T, joints, twists, n_links, intr, clip=CLIP, null=None, odd=None, n_frames=None, hw=None, n_joints=None, n_cols=None):
    """The C entry point on an out buffer filled with garbage -> (rc, out (N, 96) float64).  Pointers by position: 0 render, 1 ids,
    2 frames, 3 joints, 4 twists, 5 out, 6 work."""
    N, H, W = R.shape
    lib = eng.load_library()
    joints = np.zeros((N, 0, 6)) if joints is None else np.asarray(joints, np.float64)
    twists = np.zeros((N, 0, 6)) if twists is None else np.asarray(twists, np.float64)
    pad = lambda a: a if a.size else np.zeros((N, 1, 6))                                 # something to point at when a count is overridden
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (R, ids, T, pad(joints), pad(twists))]
    out = torch.full((N, 96), GARBAGE, dtype=torch.float64, device='cuda')
    work = torch.full((max(1, lib.rope_bundle_normal_workspace(N, H, W) // 8) + 1,), GARBAGE, dtype=torch.float64, device='cuda')
    ptrs = [x.data_ptr() for x in t] + [out.data_ptr(), work.data_ptr()]
    if odd is not None:
        ptrs[odd] += 2
    ptrs = [C.c_void_p(p) for p in ptrs]
    nj = joints.shape[1] if n_joints is None else n_joints
    nc = twists.shape[1] if n_cols is None else n_cols
    if joints.shape[1] == 0 and n_joints is None:
        ptrs[3] = None                                                                   # a pointer whose count is 0 may be null
    if twists.shape[1] == 0 and n_cols is None:
        ptrs[4] = None
    if null is not None:
        ptrs[null] = None
    H, W = hw if hw is not None else (H, W)
    rc = lib.rope_bundle_normal_equations(ptrs[0], ptrs[1], ptrs[2], N if n_frames is None else n_frames, H, W, n_links, *[float(v) for v in intr],
                                          ptrs[3], nj, ptrs[4], nc, clip, ptrs[5], ptrs[6], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert work[-1].item() == GARBAGE                                                    # nothing written past the workspace
    return rc, out.cpu().numpy()


def _hold(got, R, ids, T, joints, twists, n_links, intr, clip=CLIP):
    want, mag = bref.normal_equations(R, ids, T, n_links, intr, joints, twists, clip)
    n = R.shape[1] * R.shape[2]
    nj = 0 if joints is None else np.asarray(joints).shape[1]
    nc = 0 if twists is None else np.asarray(twists).shape[1]
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 2, 94, 95]], want[:, [0, 2, 94, 95]]), (got[:, [0, 2]], want[:, [0, 2]])
    err, bound = np.abs(got - want), 4 * n * EPS * mag
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{R.shape}, {nj} joints, {nc} columns: largest |kernel - reference| {err.max():.3e}; nearest to its bound at word {worst}: "
          f"{err[worst]:.3e} of {bound[worst]:.3e}")
    assert (err <= bound).all(), (worst, err[worst], bound[worst])
    dead = [c for c in range(12) if (c < 6 and c >= nj) or (c >= 6 and c - 6 >= nc)]
    for f in range(len(got)):                                       # the slots that are not given: exactly zero
        A, g = bref.unpack(got[f])
        assert not g[dead].any() and not A[dead].any() and not A[:, dead].any()
    return want


def _columns(rng, N, nj, nc):
    joints = np.concatenate([rng.uniform(-1, 1, (N, nj, 3)), rng.uniform(-.5, .5, (N, nj, 2)), rng.uniform(1.5, 2.5, (N, nj, 1))], axis=2) if nj else None
    return joints, (rng.uniform(-1, 1, (N, nc, 6)) if nc else None)


def test_kernel_agrees_with_the_reference_on_hand_built_planes_tiny_frames_and_chunk_edges():
    rng = np.random.default_rng(5)
    # the frame worked by hand: the base carries the camera's columns, every word exact
    Rf, If, Tf, jf, twf, intrf, words = hand_frame()
    rc, got = _call(Rf, If, Tf, jf, twf, 2, intrf)
    assert rc == 0 and np.array_equal(got[0], words), np.flatnonzero(got[0] != words)
    # the hand planes: NaN, inf, 0, 128 and negative depths, ids 4 and 255, an island, a grazing pixel
    R, ids, T, _ = hand_planes()
    for nj, nc in COMBOS:
        joints, tw = _columns(rng, 3, nj, nc)
        rc, got = _call(R, ids, T, joints, tw, HAND_LINKS, HAND_INTR)
        assert rc == 0
        want = _hold(got, R, ids, T, joints, tw, HAND_LINKS, HAND_INTR)
        assert want[1, 0] == refine_ref.HAND_FLAT_WORDS[0] and want[1, 1] == refine_ref.HAND_FLAT_WORDS[1] == got[1, 1] and (want[:, 2] > 0).all()
    # 1 x 1, 1 x W, H x 1: no pixel has a normal, the BOTH sums stay
    for H, W in ((1, 1), (1, 7), (9, 1)):
        R1 = rng.uniform(1.5, 2.5, (2, H, W)).astype(np.float32)
        T1 = (R1 + rng.uniform(-0.04, 0.04, R1.shape)).astype(np.float32)
        I1 = np.zeros((2, H, W), np.uint8)
        I1[1, 0, 0] = 255
        joints, tw = _columns(rng, 2, 3, 6)
        rc, got = _call(R1, I1, T1, joints, tw, HAND_LINKS, HAND_INTR)
        assert rc == 0
        want = _hold(got, R1, I1, T1, joints, tw, HAND_LINKS, HAND_INTR)
        assert want[0, 0] == H * W and want[1, 0] == H * W - 1 and not want[:, 2].any() and want[0, 1] > 0
    # one pixel below, at and above a workgroup's 2048, and 47 x 45 = 2115: links 0 .. 2 in stripes, so base pixels carry inliers
    n = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    for Hh, Ww in ((23, 89), (32, 64), (3, 683), (47, 45)):
        intr = (150.0, 150.0, Ww / 2 - 0.25, Hh / 2)
        R3 = np.stack([refine_ref.tilted_depth(Hh, Ww, intr, n, c) for c in (1.8, 2.3)]).astype(np.float32)
        I3 = (np.arange(Ww)[None, None, :] * 3 // Ww + np.zeros((2, Hh, 1))).astype(np.uint8)
        I3[1, Hh - 1:] = 255
        T3 = (R3 + rng.uniform(-0.04, 0.04, R3.shape)).astype(np.float32)
        T3[0, Hh - 1, Ww - 5:] = 0.0
        for nj, nc in COMBOS if (Hh, Ww) == (47, 45) else ((3, 6), (6, 6)):
            joints, tw = _columns(rng, 2, nj, nc)
            rc, got = _call(R3, I3, T3, joints, tw, 3, intr)
            assert rc == 0
            want = _hold(got, R3, I3, T3, joints, tw, 3, intr)
            assert (want[:, 2] > 1000).all()
        parts = [_call(R3[a:b], I3[a:b], T3[a:b], joints[a:b], tw[a:b], 3, intr)[1] for a, b in ((0, 1), (1, 2))]
        assert np.concatenate(parts).tobytes() == got.tobytes()


def _robot_scene():
    """The engine at 160 x 120 with the robot; four poses: the three of the golden set and their mean."""
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'camera_160x120.npz'))
    intr, PV = helpers.camera('640_480_color', 4)
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    from rope_s3d_amd.constants import ZFAR, ZNEAR
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    q = np.asarray(gold['joint_poses'], np.float64)
    return e, intr, np.concatenate([q, q.mean(axis=0, keepdims=True)])


def test_kernel_on_renders_of_the_robot_against_the_reference_and_the_two_shipped_kernels():
    """4 frames at 160 x 120 = 19 200 pixels: ten workgroups a frame, the last one partial.  Frames: the renders under the true
    camera with 10 % holes and a NaN block; renders: under a camera a few mm and mrad away and angles a few mrad away."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import BundleRefiner, camera_twists
    from rope_s3d_amd.projection import camera_matrix
    e, intr, truth = _robot_scene()
    try:
        T_t, _ = e.render_batch_device(truth, 6)
        T = T_t.cpu().numpy()
        rng = np.random.default_rng(3)
        T[rng.random(T.shape) < 0.1] = 0.0
        T[:, 40:50, 60:80] = np.nan
        pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.004, -.003, .005, .003, -.002, .004])
        q = truth + rng.uniform(-.005, .005, truth.shape)
        rd, ri = e.render_batch_device(q, 6, np.tile(camera_matrix(pose, intr)[None], (4, 1, 1)))
        twists = np.tile(camera_twists(pose)[None], (4, 1, 1))
        joints = BundleRefiner(e, intr).joint_axes(pose, q)
        intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
        Tt = torch.from_numpy(T).cuda()
        Rn, In = rd.cpu().numpy(), ri.cpu().numpy()
        got = e.bundle_normal_equations(rd, ri, Tt, joints, twists, 6, CLIP, intr4)
        want = _hold(got, Rn, In, T, joints, twists, 6, intr4)
        A, g = bref.unpack(got[0])
        live = [0, 1, 2, 3, 4] + list(range(6, 12))                      # joint 5 moves a link that is not drawn: its slot stays 0
        assert (want[:, 2] > 500).all() and (np.diag(A)[live] > 0).all() and A[5, 5] == 0 and np.abs(A[:5, 6:]).min() > 0
        for nj, nc in ((3, 6), (6, 0), (0, 6)):
            part = e.bundle_normal_equations(rd, ri, Tt, joints[:, :nj] if nj else None, twists[:, :nc] if nc else None, 6, CLIP, intr4)
            _hold(part, Rn, In, T, joints[:, :nj] if nj else None, twists[:, :nc] if nc else None, 6, intr4)
        # the shipped kernels on the same planes: [0] .. [3] and the camera block are the camera call's, the joint block the pose call's
        n = 160 * 120
        _, mag = bref.normal_equations(Rn, In, T, 6, intr4, joints, twists)
        cam = e.camera_normal_equations(rd, ri, Tt, twists, 6, CLIP, intr4)
        jnt = e.pose_normal_equations(rd, ri, Tt, joints, 6, CLIP, intr4)
        for f in range(4):
            assert np.array_equal(got[f, [0, 2]], cam[f, [0, 2]]) and jnt[f, 2] < got[f, 2]
            Ab, gb = bref.unpack(got[f])
            Mb, mb = bref.unpack(mag[f])
            (Ac, gc), (Aj, gj) = refine_ref.unpack(cam[f]), refine_ref.unpack(jnt[f])
            assert (np.abs(got[f, :4] - cam[f, :4]) <= 4 * n * EPS * mag[f, :4]).all()
            assert (np.abs(Ab[6:, 6:] - Ac) <= 4 * n * EPS * Mb[6:, 6:]).all() and (np.abs(gb[6:] - gc) <= 4 * n * EPS * mb[6:]).all()
            assert (np.abs(Ab[:6, :6] - Aj) <= 4 * n * EPS * Mb[:6, :6]).all() and (np.abs(gb[:6] - gj) <= 4 * n * EPS * mb[:6]).all()
        # determinism: twice the same bytes; one call of 4 frames is two calls of 2, byte for byte
        again = e.bundle_normal_equations(rd, ri, Tt, joints, twists, 6, CLIP, intr4)
        assert again.tobytes() == got.tobytes()
        parts = [e.bundle_normal_equations(rd[a:b].contiguous(), ri[a:b].contiguous(), Tt[a:b].contiguous(), joints[a:b], twists[a:b], 6, CLIP, intr4)
                 for a, b in ((0, 2), (2, 4))]
        assert np.concatenate(parts).tobytes() == got.tobytes()
        assert e.bundle_normal_equations(rd[:0], ri[:0], Tt[:0], joints[:0], twists[:0], 6, CLIP, intr4).shape == (0, 96)
        for bad in ((rd.double(), ri, Tt), (rd, ri.int(), Tt), (rd, ri, Tt[:2]), (rd.cpu(), ri, Tt)):
            with pytest.raises(ValueError):
                e.bundle_normal_equations(*bad, joints, twists, 6, CLIP, intr4)
        for bad in (twists.astype(np.float32), twists[:2], twists[:, :, :5]):
            with pytest.raises(ValueError):
                e.bundle_normal_equations(rd, ri, Tt, joints, torch.from_numpy(bad), 6, CLIP, intr4)
        with pytest.raises(ValueError):
            e.bundle_normal_equations(rd, ri, Tt, None, None, 6, CLIP, intr4)
        with pytest.raises(ValueError):
            e.bundle_normal_equations(rd, ri, Tt, joints, twists, 6, -1.0, intr4)
    finally:
        e.close()


def test_argument_errors_return_their_code_and_leave_the_output_alone():
    R, ids, T, _ = hand_planes()
    joints, tw = _columns(np.random.default_rng(2), 3, 2, 2)
    cases = [dict(n_frames=0), dict(n_frames=-1), dict(hw=(0, 23)), dict(hw=(20, 0)), dict(hw=(4097, 4096)), dict(n_links=0), dict(n_links=7),
             dict(n_joints=-1), dict(n_joints=7), dict(n_cols=-1), dict(n_cols=7), dict(n_joints=0, n_cols=0), dict(clip=0.0), dict(clip=-CLIP),
             dict(clip=float('nan')), dict(clip=float('inf'))]
    cases += [dict(null=k) for k in range(7)] + [dict(odd=k) for k in (0, 2, 3, 4, 5, 6)]
    for case in cases:
        kw = dict(n_links=HAND_LINKS, clip=CLIP)
        kw.update(case)
        n_links = kw.pop('n_links')
        rc, got = _call(R, ids, T, joints, tw, n_links, HAND_INTR, **kw)
        assert rc == E_ARG and (got.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case
    # a null pointer with a count of 0 is no error
    rc, got = _call(R, ids, T, None, tw, HAND_LINKS, HAND_INTR)
    assert rc == 0 and not np.isnan(got).any()


# ---------------------------------------------------------------------------------------------- the refiner
E2E_SEED = {'frame': 1, 'offset': 1}
TRUE_POSE_OFFSET = np.array([.06, -.05, .04, .01, -.015, .02])
DESCENT_STEP = 0.0075                               # rad: where the Predictor's last Descent stops halving (stages.py, early_stop)
PLANTED = np.array([.004, -.003, .005, 0, 0, 0])    # rad: the encoder zero offsets of the 'offset' scene


def e2e_scene(renderer, mode, seed):
    """8 random S / L / U poses and the true camera; the start: the camera within 5 mm and 4 mrad, and the angles either within one
    Descent step each ('frame') or all off by the same PLANTED offsets ('offset')."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    rng = np.random.default_rng(seed)
    lim = renderer.robot.joint_limits
    slu = np.array([1, 1, 1, 0, 0, 0])
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (8, 6)) * slu
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + TRUE_POSE_OFFSET
    start_pose = true_pose + rng.uniform(-1, 1, 6) * np.array([.005, .005, .005, .004, .004, .004])
    start = truth + rng.uniform(-DESCENT_STEP, DESCENT_STEP, (8, 6)) * slu if mode == 'frame' else truth - PLANTED
    return truth, true_pose, start, start_pose


def reference_run(renderer, mode, truth, true_pose, start, start_pose, iterations=5):
    """bundle_ref.refine on the engine's own renders -> (its result, the frames T as a device tensor)."""
    from rope_s3d_amd.prediction.refinement import BundleRefiner, camera_twists
    from rope_s3d_amd.projection import camera_matrix
    intr, e = renderer.intrinsics, renderer.engine
    N = len(truth)
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
    T_t = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (N, 1, 1)))[0]
    T = T_t.cpu().numpy()
    axes_of = BundleRefiner(renderer, intr).joint_axes               # PoseRefiner.joint_axes' host arithmetic (tests/test_refine_refs.py holds it)

    def equations(p, q):
        d, i = e.render_batch_device(np.ascontiguousarray(q), 6, np.tile(camera_matrix(p, intr)[None], (N, 1, 1)))
        return bref.normal_equations(d.cpu().numpy(), i.cpu().numpy(), T, 6, intr4, axes_of(p, q), np.tile(camera_twists(p)[None], (N, 1, 1)), CLIP)[0]

    limits = np.asarray(renderer.robot.joint_limits, np.float64)
    return bref.refine(start_pose, start, equations, limits, mode, (0, 1, 2), tuple(range(6)), iterations, 1e-3), T_t


def seed_conditions(want):
    """The conditions on a seed, evaluated by the reference alone -> (no near tie, all sigmas finite, a step accepted)."""
    sig = np.concatenate([want['sigma_pose'], (want['sigma_angles'][:, :3] if 'sigma_angles' in want else want['sigma_offsets'][:3]).reshape(-1)])
    return (bool((want['margins'] > 1e-6 * want['costs'][:-1]).all()), bool(np.isfinite(sig).all()), want['steps_taken'] >= 1)


def origin_rms(pose, angles, true_pose, truth):
    """RMS displacement, in camera axes, of the six link origins over the frames between (pose, angles) and (true_pose, truth)."""
    from rope_s3d_amd.projection import camera_pose_matrix
    from rope_s3d_amd.simulation.kinematics import ForwardKinematics
    fk = ForwardKinematics()
    (Ra, ta), (Rb, tb) = cref.Rwc_t(pose, camera_pose_matrix), cref.Rwc_t(true_pose, camera_pose_matrix)
    Xa = np.stack([fk.calc(a)[:6, :3, 3] for a in angles]).reshape(-1, 3)
    Xb = np.stack([fk.calc(a)[:6, :3, 3] for a in truth]).reshape(-1, 3)
    d = (Xa - ta) @ Ra.T - (Xb - tb) @ Rb.T
    return float(np.sqrt((d * d).sum(axis=1).mean()))


@pytest.fixture(scope='module')
def renderer():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.simulation.render import Renderer
    r = Renderer('seg', DEFAULT_CAMERA_POSE, '640_480_color', intrinsic_ds_factor=4)
    yield r
    r.engine.close()


@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_bundle_refiner_walks_the_reference_loop_on_the_engines_renders(renderer, mode):
    """8 frames at 160 x 120.  BundleRefiner and bundle_ref.refine see the same renders (the engine's) and differ in the order of
    the kernel's sums alone.  The conditions on E2E_SEED need the engine's renders and are checked here on the reference alone."""
    from rope_s3d_amd.prediction.refinement import BundleRefineResult, BundleRefiner
    truth, true_pose, start, start_pose = e2e_scene(renderer, mode, E2E_SEED[mode])
    want, T_t = reference_run(renderer, mode, truth, true_pose, start, start_pose)
    no_tie, finite, stepped = seed_conditions(want)
    assert no_tie, "choose another E2E_SEED: a decision of the loop is a near tie"
    assert finite and stepped, "choose another E2E_SEED: a sigma of the reference is not finite, or it accepted no step"
    got = BundleRefiner(renderer, renderer.intrinsics, joints=mode).refine(start_pose, start, T_t)
    assert isinstance(got, BundleRefineResult)
    rms0, rms1 = origin_rms(start_pose, start, true_pose, truth), origin_rms(got.pose, got.angles, true_pose, truth)
    print(mode, 'steps', got.steps_taken, 'cost', got.cost_before, '->', got.cost_after, 'max pose difference', np.abs(got.pose - want['pose']).max(),
          'max angle difference', np.abs(got.angles - want['angles']).max(), 'sigma_pose', got.sigma_pose)
    print(f"{mode}: pose error start {np.abs(start_pose - true_pose)} refined {np.abs(got.pose - true_pose)}")
    print(f"{mode}: mean |angle error| on S, L, U: start {np.abs(start - truth)[:, :3].mean():.6e} refined {np.abs(got.angles - truth)[:, :3].mean():.6e} rad")
    print(f"{mode}: RMS displacement of the link origins against the truth: start {rms0:.6e} m, refined {rms1:.6e} m")
    assert got.steps_taken == want['steps_taken'] and got.inliers == want['inliers']
    assert np.abs(got.pose - want['pose']).max() <= 1e-9 and np.abs(got.angles - want['angles']).max() <= 1e-9
    assert got.cost_after <= got.cost_before and got.frame_cost.shape == (8,) and np.isfinite(got.sigma_pose).all()
    assert np.array_equal(got.angles[:, 3:], start[:, 3:])
    assert rms1 < rms0
    if mode == 'frame':
        assert np.isnan(got.offsets).all() and got.sigma_offsets is None
        assert np.isfinite(got.sigma_angles[:, :3]).all() and np.isnan(got.sigma_angles[:, 3:]).all()
    else:
        print('offsets', got.offsets, 'planted', PLANTED, 'sigma_offsets', got.sigma_offsets)
        assert got.sigma_angles is None and np.abs(got.offsets - want['offsets']).max() <= 1e-9
        assert np.isfinite(got.sigma_offsets[:3]).all() and np.isnan(got.sigma_offsets[3:]).all() and not got.offsets[3:].any()
        assert (np.abs(got.offsets[:3] - PLANTED[:3]) < np.abs(PLANTED[:3])).all()          # each comes back closer than it started (at 0)
        assert np.array_equal(got.angles, np.clip(start + got.offsets, renderer.robot.joint_limits[:, 0], renderer.robot.joint_limits[:, 1]))


# ---------------------------------------------------------------------------------------------- the public interface
@pytest.mark.parametrize('mode', ['modelless', 'segmented'])
def test_predictor_switch_bundle_and_the_two_old_settings(mode):
    from rope_s3d_amd import CameraPredictor, ModellessCameraPredictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import BundleRefineResult, CameraPoseRefiner, CameraRefineResult
    from rope_s3d_amd.segmentation import ColorSegmenter
    from rope_s3d_amd.simulation.render import Renderer
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + TRUE_POSE_OFFSET
    r = Renderer('seg', true_pose, '640_480_color')
    lim = r.robot.joint_limits
    qs = np.random.default_rng(9).uniform(lim[:, 0] * .5, lim[:, 1] * .5, (4, 6)) * np.array([1, 1, 1, 0, 0, 0])
    colors, depths = [], []
    for q in qs:
        r.setJointAngles(q)
        c, d = r.render()
        colors.append(c); depths.append(np.asarray(d, np.float64))
    names = ['BG'] + list(r.robot.link_names[:6])
    r.engine.close()
    start = true_pose + np.array([.004, -.003, .003, .002, -.002, .002])
    stages = [('descent', 6, 0.5, .001, [True] * 6, [0.002] * 6)]

    def make(**kw):
        if mode == 'modelless':
            p = ModellessCameraPredictor(start, 4, base_intrinsics='640_480_color', **kw)
        else:
            p = CameraPredictor(start, 4, base_intrinsics='640_480_color', segmenter=ColorSegmenter(names), **kw)
        p.stages = list(stages)
        return p

    off = make(refine=False)
    before = off.run(np.stack(colors), np.stack(depths), qs)
    assert off.refine is False and off.last_refinement is None
    on = make(refine=True)
    polished = on.run(np.stack(colors), np.stack(depths), qs)
    assert on.refine is True and isinstance(on.last_refinement, CameraRefineResult)
    assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(on.trace, off.trace)) and len(on.trace) == len(off.trace)
    by_hand = CameraPoseRefiner(on.renderer, on.renderer.intrinsics).refine(before, qs, np.asarray(on._tgt_depths, np.float32))
    assert polished.tobytes() == by_hand.pose.tobytes() and on.last_refinement.sigma.tobytes() == by_hand.sigma.tobytes()
    bundle = make(refine='bundle')
    qs_in = qs.copy()
    both = bundle.run(np.stack(colors), np.stack(depths), qs_in)
    res = bundle.last_refinement
    assert bundle.refine == 'bundle' and isinstance(res, BundleRefineResult) and np.array_equal(both, res.pose)
    assert np.array_equal(qs_in, qs) and res.angles.shape == (4, 6) and res.sigma_angles.shape == (4, 6) and res.frame_cost.shape == (4,)
    assert res.cost_after <= res.cost_before and np.isnan(res.offsets).all()
    assert all(a[1].tobytes() == b[1].tobytes() for a, b in zip(bundle.trace, off.trace))
    print(mode, 'stages', before, 'camera polish', polished, 'bundle', both, 'steps', res.steps_taken, 'cost', res.cost_before, '->', res.cost_after)
    if res.steps_taken == 0:
        assert np.array_equal(both, before)
    with pytest.raises(ValueError):
        make(refine='both')
    for p in (off, on, bundle):
        p.engine.close()


@pytest.mark.parametrize('joints', ['frame', 'offset', 'fixed'])
def test_calibrate_runs_on_a_synthetic_set(tmp_path, joints):
    out = tmp_path / f'{joints}.json'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'calibrate.py'), 'synthetic:8', '-frames', '8', '-joints', joints, '-ds_factor', '8',
                        '-iterations', '2', '-json', str(out)], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(out.read_text())
    assert rep['joints'] == joints and rep['frames'] == 8 and len(rep['pose']) == 6 and len(rep['sigma_pose']) == 6
    assert rep['cost_after'] <= rep['cost_before'] and len(rep['frame_cost']) == 8 and len(rep['worst_frames']) >= 1
    assert 0 <= rep['steps_taken'] <= 2 and rep['inliers'] > 0
    if joints == 'offset':
        assert len(rep['offsets']) == 6 and len(rep['sigma_offsets']) == 6
    if joints == 'frame':
        assert len(rep['angle_change_max']) == 6 and len(rep['angle_change_rms']) == 6 and len(rep['sigma_angles']) == 8


# ---------------------------------------------------------------------------------------------- the shared host loop, byte for byte
def _silhouette_loop(pose, angles, equations, limits, mode, active_j, active_c, weight, clip, radius, iterations=5, damping=1e-3):
    """BundleRefiner(silhouette=weight)'s loop restated on bundle_ref's solves.  equations(pose, angles) -> (depth words (N, 96) or
    None, outline words (N, 96)).  A step is judged by c_d / clip^2 + weight c_s / R'^2 and solved on the sum of the two terms' words,
    each divided by its pixel count and truncation; the sigmas add the terms' information, each over its own s^2."""
    p, q0 = np.array(pose, np.float64).reshape(6), np.array(angles, np.float64).reshape(-1, 6)
    active_j, active_c = list(active_j), list(active_c)
    slots = active_j + [6 + k for k in active_c]
    far = np.sqrt(radius * radius + 1.0) - 0.5
    norm_d, norm_s = clip * clip, far * far
    nan = float('nan')

    def look(p, q):
        w_d, w_s = equations(p, q)
        p_d, p_s = None if w_d is None else bref.pool(w_d), bref.pool(w_s)
        c_s = p_s[1] / p_s[0] if p_s[0] > 0 else np.inf
        if p_d is None:
            return w_d, w_s, p_d, p_s, nan, float(c_s), float(weight * (c_s / norm_s))
        c_d = p_d[1] / p_d[0] if p_d[0] > 0 else np.inf
        return w_d, w_s, p_d, p_s, float(c_d), float(c_s), float(c_d / norm_d + weight * (c_s / norm_s))

    q, off, lam, steps = q0.copy(), np.zeros(6), float(damping), 0
    w_d, w_s, p_d, p_s, cd, cs, cost = look(p, q)
    cd0, cs0 = cd, cs
    for _ in range(iterations):
        a_d = 1.0 / (p_d[0] * norm_d) if p_d is not None and p_d[0] > 0 else 0.0
        a_s = weight / (p_s[0] * norm_s) if p_s[0] > 0 else 0.0
        words = np.zeros_like(w_s)
        words[:, 4:94] = a_s * w_s[:, 4:94] if w_d is None else a_d * w_d[:, 4:94] + a_s * w_s[:, 4:94]
        if mode == 'frame':
            dq, dc = bref.schur_step(words, active_j, active_c, lam)
            t_p, t_off, t_q = p + dc, off, np.clip(q + dq, limits[:, 0], limits[:, 1])
        else:
            d = bref.columns_step(bref.pool(words), slots, lam)
            t_p, t_off = p + d[6:], off + d[:6]
            t_q = np.clip(q0 + t_off, limits[:, 0], limits[:, 1])
        trial = look(t_p, t_q)
        if trial[6] < cost:
            p, off, q = t_p, t_off, t_q
            w_d, w_s, p_d, p_s, cd, cs, cost = trial
            steps += 1
        else:
            lam *= 10.0
    terms = [(w, pl) for w, pl in ((w_d, p_d), (w_s, p_s)) if w is not None]
    if mode == 'frame':
        frames, kc, _, _ = bref.arrow_blocks(sum(w for w, _ in terms), active_j, active_c)
        n_live = len(kc) + sum(len(fr[0]) for fr in frames)
    else:
        A, _ = bref.unpack(sum(pl for _, pl in terms))
        n_live = sum(1 for c in slots if A[c, c] > 0)
    info = np.zeros_like(w_s)
    for w, pl in terms:
        if n_live > 0 and pl[2] >= n_live + 1 and pl[3] > 0:
            info[:, 4:94] += w[:, 4:94] / (pl[3] / (pl[2] - n_live))
    if info.any():
        info[0, 2], info[0, 3] = n_live + 1.0, 1.0
    out = dict(pose=p, angles=q, cost_before=cd0, cost_after=cd, steps_taken=steps, inliers=0.0 if p_d is None else float(p_d[2]),
               frame_cost=np.full(len(q), np.nan) if w_d is None else np.array([bref.mean_cost(w) for w in w_d]),
               cost_silhouette_before=cs0, cost_silhouette_after=cs, inliers_silhouette=float(p_s[2]))
    if mode == 'frame':
        sq, sc = bref.schur_sigma(info, active_j, active_c)
        out.update(offsets=np.full(6, np.nan), sigma_pose=sc, sigma_angles=sq, sigma_offsets=None)
    else:
        s = bref.columns_sigma(bref.pool(info), slots)
        out.update(offsets=np.where(np.isin(np.arange(6), active_j), off, 0.0), sigma_pose=s[6:], sigma_angles=None, sigma_offsets=s[:6])
    return out


def _same_fields(got, want, fields):
    for k in fields:
        g, w = getattr(got, k), want[k]
        if w is None:
            assert g is None, k
            continue
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (k, g, w)


@pytest.fixture(scope='module')
def small_scene():
    """Three frames of 47 x 45 = 2115 pixels — two passes of a workgroup's 256 x 8 and a ragged last row, the shape of
    tests/test_gpu_neq_terms.py's three-frame case — of the robot under a camera 5 mm / 4 mrad from the start."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR
    from rope_s3d_amd.projection import Intrinsics, camera_matrix
    intr = Intrinsics('640_480_color')
    intr.resolution, intr.f, intr.pp = [47, 45], [v * 47 / 640 for v in intr.f], [23.25, 22.75]
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    e.set_camera(camera_matrix(DEFAULT_CAMERA_POSE, intr, ZNEAR, ZFAR), intr.width, intr.height, ZNEAR, ZFAR)
    rng = np.random.default_rng(31)
    lim, slu = np.asarray(helpers.robot().joint_limits, np.float64), np.array([1, 1, 1, 0, 0, 0])
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (3, 6)) * slu
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + TRUE_POSE_OFFSET
    start_pose = true_pose + rng.uniform(-1, 1, 6) * np.array([.005, .005, .005, .004, .004, .004])
    start = truth + rng.uniform(-DESCENT_STEP, DESCENT_STEP, (3, 6)) * slu
    T, ti = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (3, 1, 1)))
    yield e, intr, lim, truth, start, start_pose, T.clone(), (ti < 6).clone()
    e.close()


@pytest.mark.parametrize('case', ['camera', 'frame', 'offset', 'silhouette', 'silhouette alone'])
def test_the_refiners_walk_the_restated_loops_byte_for_byte_on_the_same_engine(small_scene, case):
    """CameraPoseRefiner and BundleRefiner against camera_refine_ref.refine, bundle_ref.refine and _silhouette_loop, every side
    with the words of the SAME engine calls: the host loops add nothing of their own, so no tolerance enters."""
    from rope_s3d_amd.prediction import refinement as rf
    from rope_s3d_amd.projection import camera_matrix, camera_pose_matrix
    e, intr, lim, truth, start, start_pose, T, mask = small_scene
    assert tuple(T.shape) == (3, 45, 47)
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
    sd2 = e.mask_distance(mask.to(torch.uint8).contiguous(), 8)

    def words(p, q, depth=True, outline=False):
        q = np.ascontiguousarray(q, np.float64)
        rd, ri = e.render_batch_device(q, 6, np.tile(camera_matrix(p, intr)[None], (3, 1, 1)))
        axes = rf.joint_axes_camera(rf.ForwardKinematics(), *cref.Rwc_t(p, camera_pose_matrix), q)
        tw = np.tile(rf.camera_twists(p)[None], (3, 1, 1))
        if case == 'camera':
            return e.camera_normal_equations(rd, ri, T, tw, 6, CLIP, intr4)
        w_d = e.bundle_normal_equations(rd, ri, T, axes[:, :3], tw, 6, CLIP, intr4) if depth else None
        return (w_d, e.silhouette_normal_equations(rd, ri, sd2, axes[:, :3], tw, 6, 8, intr4)) if outline else w_d

    plain = ('pose', 'cost_before', 'cost_after', 'steps_taken', 'inliers', 'frame_cost')
    if case == 'camera':
        want = cref.refine(start_pose, lambda p: words(p, truth))
        got = rf.CameraPoseRefiner(e, intr).refine(start_pose, truth, T)
        _same_fields(got, want, plain + ('sigma',))
    elif case in ('frame', 'offset'):
        want = bref.refine(start_pose, start, words, lim, case)
        want.setdefault('sigma_angles'), want.setdefault('sigma_offsets')
        got = rf.BundleRefiner(e, intr, joints=case).refine(start_pose, start, T)
        _same_fields(got, want, plain + ('angles', 'offsets', 'sigma_pose', 'sigma_angles', 'sigma_offsets'))
        assert np.isnan(got.cost_silhouette_before) and np.isnan(got.cost_silhouette_after) and got.inliers_silhouette == 0
    else:
        depth = case == 'silhouette'
        for mode in ('frame', 'offset'):
            want = _silhouette_loop(start_pose, start, lambda p, q: words(p, q, depth, True), lim, mode, (0, 1, 2), range(6), 1.0, CLIP, 8)
            got = rf.BundleRefiner(e, intr, joints=mode, silhouette=1.0).refine(start_pose, start, T if depth else None, mask)
            _same_fields(got, want, plain + ('angles', 'offsets', 'sigma_pose', 'sigma_angles', 'sigma_offsets', 'cost_silhouette_before',
                                             'cost_silhouette_after', 'inliers_silhouette'))
            assert want['inliers_silhouette'] > 0 and (want['inliers'] > 0) == depth
    print(case, 'steps', got.steps_taken, 'cost', got.cost_before, '->', got.cost_after)
    assert want['inliers'] > 0 or case == 'silhouette alone'
