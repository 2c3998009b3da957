"""GPU: rope_camera_normal_equations (csrc/rope_refine.hip; Engine.camera_normal_equations) against the numpy restatement of its
contract (tests/camera_refine_ref.py) — counts equal, every float sum within the worst case of a reordered float64 summation — its
determinism, what it refuses, CameraPoseRefiner end to end against camera_refine_ref's pooled loop on the engine's own renders, and
the switch of the two camera predictors.

The bound is tests/test_gpu_refine.py's: a sum of n float64 terms added in any order differs from the exact sum by at most
(n - 1) eps sum|terms| to first order, eps = 2^-52 being twice the unit roundoff; two orders differ by at most twice that, and the
terms themselves are the same bits on both sides (one IEEE operation per written operation).  4 n eps sum|terms| covers it with
the second-order terms; n is the pixel count of the frame.  No measured number enters."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import camera_refine_ref as cref
import helpers
import refine_ref
from refine_ref import CLIP, HAND_INTR, HAND_LINKS, hand_planes

pytestmark = pytest.mark.gpu

E_ARG = -1
EPS = 2.0 ** -52
GARBAGE = float(np.frombuffer(b'\x5a' * 8, np.float64)[0])


def _call(R, ids, T, twists, n_links, intr, clip=CLIP, null=None, odd=None, n_frames=None, hw=None, n_cols=None):
    """The C entry point on an out buffer filled with garbage -> (rc, out (N, 32) float64)."""
    N, H, W = R.shape
    lib = eng.load_library()
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (R, ids, T, np.asarray(twists, np.float64))]
    out = torch.full((N, 32), GARBAGE, dtype=torch.float64, device='cuda')
    work = torch.full((max(1, lib.rope_pose_normal_workspace(N, H, W) // 8) + 1,), GARBAGE, dtype=torch.float64, device='cuda')
    ptrs = [x.data_ptr() for x in t] + [out.data_ptr(), work.data_ptr()]
    if odd is not None:
        ptrs[odd] += 2
    ptrs = [C.c_void_p(p) for p in ptrs]
    if null is not None:
        ptrs[null] = None
    H, W = hw if hw is not None else (H, W)
    rc = lib.rope_camera_normal_equations(ptrs[0], ptrs[1], ptrs[2], N if n_frames is None else n_frames, H, W, n_links, *[float(v) for v in intr],
                                          ptrs[3], np.asarray(twists).shape[1] if n_cols is None else n_cols, clip, ptrs[4], ptrs[5],
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _hold(got, R, ids, T, twists, n_links, intr, clip=CLIP):
    want, mag = cref.normal_equations(R, ids, T, n_links, intr, twists, clip)
    n = R.shape[1] * R.shape[2]
    n_cols = np.asarray(twists).shape[1]
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 2, 31]], want[:, [0, 2, 31]]), (got[:, [0, 2]], want[:, [0, 2]])
    err, bound = np.abs(got - want), 4 * n * EPS * mag
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{R.shape}, {n_cols} columns: largest |kernel - reference| {err.max():.3e}; nearest to its bound at word {worst}: {err[worst]:.3e} of {bound[worst]:.3e}")
    assert (err <= bound).all(), (worst, err[worst], bound[worst])
    A = np.zeros((6, 6))
    for f in range(len(got)):                                       # columns from n_cols on: exactly zero
        A[np.triu_indices(6)] = got[f, 10:31]
        assert not got[f, 4 + n_cols:10].any() and not A[n_cols:].any() and not A[:, n_cols:].any()
    return want


def _twists(rng, N, n_cols):
    return rng.uniform(-1, 1, (N, n_cols, 6))


def test_kernel_agrees_with_the_reference_on_the_hand_built_planes_and_tiny_frames():
    R, ids, T, _ = hand_planes()
    rng = np.random.default_rng(5)
    for n_cols in (1, 3, 6):
        tw = _twists(rng, 3, n_cols)
        rc, got = _call(R, ids, T, tw, HAND_LINKS, HAND_INTR)
        assert rc == 0
        want = _hold(got, R, ids, T, tw, HAND_LINKS, HAND_INTR)
        assert want[1, 0] == refine_ref.HAND_FLAT_WORDS[0] and want[1, 1] == refine_ref.HAND_FLAT_WORDS[1] == got[1, 1]
        assert (want[:, 2] > 0).all() and (want[:, 10] > 0).all()
    # the flat frame worked by hand: link 0 carries the system, every word exact
    Rf, If, Tf, twf, words = cref.flat_frame()
    rc, got = _call(Rf, If, Tf, twf, 2, HAND_INTR)
    assert rc == 0 and np.array_equal(got[0], words), (got[0], words)
    # 1 x 1: no neighbour at all; 1 x 7: one row, differences along x only: no pixel has a normal, the BOTH sums stay
    for H, W in ((1, 1), (1, 7)):
        R1 = rng.uniform(1.5, 2.5, (2, H, W)).astype(np.float32)
        T1 = (R1 + rng.uniform(-0.04, 0.04, R1.shape)).astype(np.float32)
        I1 = np.zeros((2, H, W), np.uint8)
        I1[1, 0, 0] = 255
        tw = _twists(rng, 2, 3)
        rc, got = _call(R1, I1, T1, tw, HAND_LINKS, HAND_INTR)
        assert rc == 0
        want = _hold(got, R1, I1, T1, tw, HAND_LINKS, HAND_INTR)
        assert want[0, 0] == H * W and want[1, 0] == H * W - 1 and not want[:, 2].any() and want[0, 1] > 0
    # three frames of 47 x 45 = 2115 pixels: a second workgroup with 67 of its 2048 pixels in the frame
    Hh, Ww = 47, 45
    n = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    R3 = np.stack([refine_ref.tilted_depth(Hh, Ww, (150.0, 150.0, 22.25, 23.5), n, c) for c in (1.8, 2.0, 2.3)]).astype(np.float32)
    I3 = (np.arange(Ww)[None, None, :] // 16 + np.zeros((3, Hh, 1))).astype(np.uint8)          # links 0, 1, 2 in stripes
    I3[2, 40:] = 255
    T3 = (R3 + rng.uniform(-0.04, 0.04, R3.shape)).astype(np.float32)
    T3[0, 46, 40:] = 0.0
    for n_cols in (1, 3, 6):
        tw = _twists(rng, 3, n_cols)
        rc, got = _call(R3, I3, T3, tw, 3, (150.0, 150.0, 22.25, 23.5))
        assert rc == 0
        want = _hold(got, R3, I3, T3, tw, 3, (150.0, 150.0, 22.25, 23.5))
        assert (want[:, 2] > 1000).all()
    parts = [_call(R3[a:b], I3[a:b], T3[a:b], tw[a:b], 3, (150.0, 150.0, 22.25, 23.5))[1] for a, b in ((0, 1), (1, 3))]
    assert np.concatenate(parts).tobytes() == got.tobytes()


@pytest.mark.parametrize('Hh,Ww', [(23, 89), (32, 64), (3, 683)])
def test_kernel_at_the_chunk_edges_and_cut_into_calls(Hh, Ww):
    """2047, 2048 and 2049 pixels: the last pass one thread short, a full workgroup, a second workgroup for one pixel; frames
    built as test_gpu_bundle's, links 0 .. 2 in stripes.  Three frames cut as [0:1], [1:3]: the gather kernel's last workgroup
    holds one frame of its two."""
    rng = np.random.default_rng(Hh)
    n = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    intr = (150.0, 150.0, Ww / 2 - 0.25, Hh / 2)
    R3 = np.stack([refine_ref.tilted_depth(Hh, Ww, intr, n, c) for c in (1.8, 2.0, 2.3)]).astype(np.float32)
    I3 = (np.arange(Ww)[None, None, :] * 3 // Ww + np.zeros((3, Hh, 1))).astype(np.uint8)
    I3[1, Hh - 1:] = 255
    T3 = (R3 + rng.uniform(-0.04, 0.04, R3.shape)).astype(np.float32)
    T3[0, Hh - 1, Ww - 5:] = 0.0
    for n_cols in (3, 6):
        tw = _twists(rng, 3, n_cols)
        rc, got = _call(R3, I3, T3, tw, 3, intr)
        assert rc == 0
        want = _hold(got, R3, I3, T3, tw, 3, intr)
        assert (want[:, 2] > 1000).all()
    parts = [_call(R3[a:b], I3[a:b], T3[a:b], tw[a:b], 3, intr)[1] for a, b in ((0, 1), (1, 3))]
    assert np.concatenate(parts).tobytes() == got.tobytes()


def _robot_scene():
    """The engine at 160 x 120 with the robot and the three poses of the golden set."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'camera_160x120.npz'))
    intr, PV = helpers.camera('640_480_color', 4)
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    from rope_s3d_amd.constants import ZFAR, ZNEAR
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    return e, intr, gold['joint_poses']


def test_kernel_agrees_with_the_reference_on_renders_of_the_robot():
    """160 x 120 = 19 200 pixels: ten workgroups a frame, the last one partial.  Frames: the renders under the true camera with
    10 % holes and a NaN block; renders: under a camera a few mm and mrad away, through PV."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import camera_twists
    from rope_s3d_amd.projection import camera_matrix
    e, intr, truth = _robot_scene()
    try:
        T_t, _ = e.render_batch_device(truth, 6)
        T = T_t.cpu().numpy()
        rng = np.random.default_rng(3)
        T[rng.random(T.shape) < 0.1] = 0.0                                   # holes
        T[:, 40:50, 60:80] = np.nan
        pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.004, -.003, .005, .003, -.002, .004])
        rd, ri = e.render_batch_device(truth, 6, np.tile(camera_matrix(pose, intr)[None], (3, 1, 1)))
        twists = np.tile(camera_twists(pose)[None], (3, 1, 1))
        intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
        Tt = torch.from_numpy(T).cuda()
        got = e.camera_normal_equations(rd, ri, Tt, twists, 6, CLIP, intr4)
        want = _hold(got, rd.cpu().numpy(), ri.cpu().numpy(), T, twists, 6, intr4)
        assert (want[:, 2] > 500).all() and (np.diag(refine_ref.unpack(want[0])[0]) > 0).all()
        # the base counts here: more inliers than under the joints' MOVING rule, which leaves link 0 out
        joints_rule = refine_ref.normal_equations(rd.cpu().numpy(), ri.cpu().numpy(), T, 6, intr4, np.zeros((3, 6, 6)))[0]
        assert (want[:, 2] > joints_rule[:, 2]).all()
        # determinism: twice the same bytes; frames [0:3] in one call are [0:1] and [1:3], byte for byte
        again = e.camera_normal_equations(rd, ri, Tt, twists, 6, CLIP, intr4)
        assert again.tobytes() == got.tobytes()
        parts = [e.camera_normal_equations(rd[a:b].contiguous(), ri[a:b].contiguous(), Tt[a:b].contiguous(), twists[a:b], 6, CLIP, intr4)
                 for a, b in ((0, 1), (1, 3))]
        assert np.concatenate(parts).tobytes() == got.tobytes()
        assert e.camera_normal_equations(rd[:0], ri[:0], Tt[:0], twists[:0], 6, CLIP, intr4).shape == (0, 32)
        for bad in ((rd.double(), ri, Tt), (rd, ri.int(), Tt), (rd, ri, Tt[:2]), (rd.cpu(), ri, Tt)):
            with pytest.raises(ValueError):
                e.camera_normal_equations(*bad, twists, 6, CLIP, intr4)
        for bad in (twists.astype(np.float32), twists[:2], twists[:, :, :5], torch.from_numpy(twists).float()):
            with pytest.raises(ValueError):
                e.camera_normal_equations(rd, ri, Tt, bad if isinstance(bad, torch.Tensor) else torch.from_numpy(bad), 6, CLIP, intr4)
        with pytest.raises(ValueError):
            e.camera_normal_equations(rd, ri, Tt, twists, 6, -1.0, intr4)
    finally:
        e.close()


def test_argument_errors_return_their_code_and_leave_the_output_alone():
    R, ids, T, _ = hand_planes()
    tw = _twists(np.random.default_rng(2), 3, 2)
    cases = [dict(n_frames=0), dict(n_frames=-1), dict(hw=(0, 23)), dict(hw=(20, 0)), dict(hw=(4097, 4096)), dict(n_links=0), dict(n_links=7),
             dict(n_cols=0), dict(n_cols=7), dict(clip=0.0), dict(clip=-CLIP), dict(clip=float('nan')), dict(clip=float('inf'))]
    cases += [dict(null=k) for k in range(6)] + [dict(odd=k) for k in (0, 2, 3, 4, 5)]
    for case in cases:
        kw = dict(n_links=HAND_LINKS, clip=CLIP)
        kw.update(case)
        n_links = kw.pop('n_links')
        rc, got = _call(R, ids, T, tw, n_links, HAND_INTR, **kw)
        assert rc == E_ARG and (got.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case


# ---------------------------------------------------------------------------------------------- the refiner
E2E_SEED = 1
TRUE_POSE_OFFSET = np.array([.06, -.05, .04, .01, -.015, .02])


def e2e_scene(renderer, seed):
    """8 random S / L / U poses, the true camera and a start within 5 mm and 4 mrad of it: the search's lattice is 1 mm / 2 mrad,
    this is the regime the polish is for."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    rng = np.random.default_rng(seed)
    lim = renderer.robot.joint_limits
    angles = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (8, 6)) * np.array([1, 1, 1, 0, 0, 0])
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + TRUE_POSE_OFFSET
    start = true_pose + rng.uniform(-1, 1, 6) * np.array([.005, .005, .005, .004, .004, .004])
    return angles, true_pose, start


def reference_run(renderer, angles, true_pose, start, active=tuple(range(6)), iterations=5):
    """camera_refine_ref.refine on the engine's own renders -> (its result, the frames T as a device tensor)."""
    from rope_s3d_amd.prediction.refinement import camera_twists
    from rope_s3d_amd.projection import camera_matrix
    intr, e = renderer.intrinsics, renderer.engine
    N = len(angles)
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
    T_t = e.render_batch_device(angles, 6, np.tile(camera_matrix(true_pose, intr)[None], (N, 1, 1)))[0]
    T = T_t.cpu().numpy()

    def equations(p):
        d, i = e.render_batch_device(angles, 6, np.tile(camera_matrix(p, intr)[None], (N, 1, 1)))
        return cref.normal_equations(d.cpu().numpy(), i.cpu().numpy(), T, 6, intr4, np.tile(camera_twists(p)[None], (N, 1, 1)), CLIP)[0]

    return cref.refine(start, equations, active, iterations, 1e-3), T_t


def seed_conditions(want):
    """The conditions on the seed, evaluated by the reference alone -> (no near tie, all sigmas finite, a step accepted)."""
    return (bool((want['margins'] > 1e-6 * want['costs'][:-1]).all()), bool(np.isfinite(want['sigma']).all()), want['steps_taken'] >= 1)


def _origin_rms(pose, true_pose, angles):
    """RMS displacement, in camera axes, of the six link origins over the frames between the cameras `pose` and `true_pose`."""
    from rope_s3d_amd.projection import camera_pose_matrix
    from rope_s3d_amd.simulation.kinematics import ForwardKinematics
    fk = ForwardKinematics()
    X = np.stack([fk.calc(a)[:6, :3, 3] for a in angles]).reshape(-1, 3)
    (Ra, ta), (Rb, tb) = cref.Rwc_t(pose, camera_pose_matrix), cref.Rwc_t(true_pose, camera_pose_matrix)
    d = (X - ta) @ Ra.T - (X - tb) @ Rb.T
    return float(np.sqrt((d * d).sum(axis=1).mean()))


@pytest.fixture(scope='module')
def renderer():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.simulation.render import Renderer
    r = Renderer('seg', DEFAULT_CAMERA_POSE, '640_480_color', intrinsic_ds_factor=4)
    yield r
    r.engine.close()


def test_camera_refiner_walks_the_reference_loop_on_the_engines_renders(renderer):
    """8 frames at 160 x 120.  CameraPoseRefiner and camera_refine_ref.refine see the same renders (the engine's) and differ in the
    order of the kernel's sums alone.  The conditions on E2E_SEED need the engine's renders: they cannot be checked without a GPU."""
    from rope_s3d_amd.prediction.refinement import CameraPoseRefiner
    angles, true_pose, start = e2e_scene(renderer, E2E_SEED)
    want, T_t = reference_run(renderer, angles, true_pose, start)
    no_tie, finite, stepped = seed_conditions(want)
    assert no_tie, "choose another E2E_SEED: a decision of the loop is a near tie"
    assert finite and stepped, "choose another E2E_SEED: a sigma of the reference is not finite, or it accepted no step"
    got = CameraPoseRefiner(renderer, renderer.intrinsics).refine(start, angles, T_t)
    rms0, rms1 = _origin_rms(start, true_pose, angles), _origin_rms(got.pose, true_pose, angles)
    print('steps', got.steps_taken, 'cost', got.cost_before, '->', got.cost_after, 'max pose difference', np.abs(got.pose - want['pose']).max(),
          'sigma', got.sigma, 'frame cost', got.frame_cost)
    print(f"RMS displacement of the link origins against the true camera: start {rms0:.6e} m, refined {rms1:.6e} m")
    assert got.steps_taken == want['steps_taken'] and got.inliers == want['inliers']
    assert np.abs(got.pose - want['pose']).max() <= 1e-9
    assert got.cost_after <= got.cost_before and np.isfinite(got.sigma).all() and got.frame_cost.shape == (8,)
    assert rms1 < rms0


def test_do_params_leaves_the_other_parameters_alone(renderer):
    from rope_s3d_amd.prediction.refinement import CameraPoseRefiner
    angles, true_pose, start = e2e_scene(renderer, E2E_SEED)
    want, T_t = reference_run(renderer, angles, true_pose, start, (0, 1, 2), 2)
    got = CameraPoseRefiner(renderer, renderer.intrinsics, [True, True, True, False, False, False], iterations=2).refine(start, angles, T_t)
    assert np.array_equal(got.pose[3:], start[3:]) and np.isnan(got.sigma[3:]).all() and not np.isnan(got.sigma[:3]).any()
    assert got.cost_after <= got.cost_before and got.steps_taken <= 2
    assert np.array_equal(np.isnan(want['sigma']), np.isnan(got.sigma))


@pytest.mark.parametrize('mode', ['modelless', 'segmented'])
def test_predictor_switch_polishes_and_leaves_the_default_alone(mode):
    from rope_s3d_amd import CameraPredictor, ModellessCameraPredictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
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

    plain = make()
    assert plain.refine is False
    before = plain.run(np.stack(colors), np.stack(depths), qs)
    assert plain.last_refinement is None
    off = make(refine=False)
    assert off.run(np.stack(colors), np.stack(depths), qs).tobytes() == before.tobytes() and off.last_refinement is None
    assert len(off.trace) == len(plain.trace) and all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(off.trace, plain.trace))
    on = make(refine=True)
    polished = on.run(np.stack(colors), np.stack(depths), qs)
    res = on.last_refinement
    assert res is not None and np.array_equal(polished, res.pose) and res.cost_after <= res.cost_before
    assert all(a[1].tobytes() == b[1].tobytes() for a, b in zip(on.trace, plain.trace)) and res.sigma.shape == (6,) and res.frame_cost.shape == (4,)
    print(mode, 'stages', before, 'polished', polished, 'steps', res.steps_taken, 'cost', res.cost_before, '->', res.cost_after, 'sigma', res.sigma)
    if res.steps_taken == 0:
        assert np.array_equal(polished, before)
    for p in (plain, off, on):
        p.engine.close()
