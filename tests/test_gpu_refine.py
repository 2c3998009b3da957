"""GPU: rope_pose_normal_equations (csrc/rope_refine.hip; Engine.pose_normal_equations) against the numpy restatement of its contract
(tests/refine_ref.py) — counts equal, every float sum within the worst case of a reordered float64 summation — its determinism,
what it refuses, PoseRefiner end to end against refine_ref's loop on the engine's own renders, and the Predictor's switch.

The bound.  A sum of n float64 terms added in any order differs from the exact sum by at most (n - 1) eps sum|terms| to first
order, eps = 2^-52 being twice the unit roundoff; two orders differ by at most twice that, and the terms themselves are the same
bits on both sides (one IEEE operation per written operation; tests/test_gpu_neq_terms.py holds the kernels to that on frames
of one and two inliers, exactly).  4 n eps sum|terms| covers it with the second-order terms; n is the pixel count of the frame.
No measured number enters."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import helpers
import refine_ref
from refine_ref import CLIP, HAND_INTR, HAND_JOINTS, HAND_LINKS, hand_planes

pytestmark = pytest.mark.gpu

E_ARG = -1
EPS = 2.0 ** -52
GARBAGE = float(np.frombuffer(b'\x5a' * 8, np.float64)[0])


def _call(R, ids, T, joints, n_links, intr, clip=CLIP, out=None, null=None, odd=None, n_frames=None, hw=None, n_joints=None):
    """The C entry point on an out buffer filled with garbage (or the one given) -> (rc, out (N, 32) float64)."""
    N, H, W = R.shape
    lib = eng.load_library()
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (R, ids, T, np.asarray(joints, np.float64))]
    if out is None:
        out = torch.full((N, 32), GARBAGE, dtype=torch.float64, device='cuda')
    work = torch.full((max(1, lib.rope_pose_normal_workspace(N, H, W) // 8) + 1,), GARBAGE, dtype=torch.float64, device='cuda')
    ptrs = [x.data_ptr() for x in t] + [out.data_ptr(), work.data_ptr()]
    if odd is not None:
        ptrs[odd] += 2
    ptrs = [C.c_void_p(p) for p in ptrs]
    if null is not None:
        ptrs[null] = None
    H, W = hw if hw is not None else (H, W)
    rc = lib.rope_pose_normal_equations(ptrs[0], ptrs[1], ptrs[2], N if n_frames is None else n_frames, H, W, n_links, *[float(v) for v in intr],
                                        ptrs[3], np.asarray(joints).shape[1] if n_joints is None else n_joints, clip, ptrs[4], ptrs[5],
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _hold(got, R, ids, T, joints, n_links, intr, clip=CLIP):
    want, mag = refine_ref.normal_equations(R, ids, T, n_links, intr, joints, clip)
    n = R.shape[1] * R.shape[2]
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 2, 31]], want[:, [0, 2, 31]]), (got[:, [0, 2]], want[:, [0, 2]])
    err, bound = np.abs(got - want), 4 * n * EPS * mag
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{R.shape}: largest |kernel - reference| {err.max():.3e}; nearest to its bound at word {worst}: {err[worst]:.3e} of {bound[worst]:.3e}")
    assert (err <= bound).all(), (worst, err[worst], bound[worst])
    return want


def _robot_scene():
    """The engine at 160 x 120 with the robot, three poses of the golden set, frames = the renders of the truth with holes cut in."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'camera_160x120.npz'))
    intr, PV = helpers.camera('640_480_color', 4)
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    from rope_s3d_amd.constants import ZFAR, ZNEAR
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    return e, intr, gold['joint_poses']


def test_kernel_agrees_with_the_reference_on_the_hand_built_planes_and_tiny_frames():
    R, ids, T, joints = hand_planes()
    rc, got = _call(R, ids, T, joints, HAND_LINKS, HAND_INTR)
    assert rc == 0
    want = _hold(got, R, ids, T, joints, HAND_LINKS, HAND_INTR)
    for w, v in refine_ref.HAND_FLAT_WORDS.items():
        assert got[1, w] == v == want[1, w]
    # 1 x 1: no neighbour at all; 1 x 7: one row, differences along x only: no pixel has a normal, the BOTH sums stay
    rng = np.random.default_rng(7)
    for H, W in ((1, 1), (1, 7)):
        R1 = rng.uniform(1.5, 2.5, (2, H, W)).astype(np.float32)
        T1 = (R1 + rng.uniform(-0.04, 0.04, R1.shape)).astype(np.float32)
        I1 = np.ones((2, H, W), np.uint8)
        I1[1, 0, 0] = 255
        rc, got = _call(R1, I1, T1, joints[:2], HAND_LINKS, HAND_INTR)
        assert rc == 0
        want = _hold(got, R1, I1, T1, joints[:2], HAND_LINKS, HAND_INTR)
        assert want[0, 0] == H * W and want[1, 0] == H * W - 1 and not want[:, 2].any() and want[0, 1] > 0


def _axes(rng, N, n_joints):
    """Generic joint axes and points about the planes' depth (test_gpu_bundle's `_columns`)."""
    return np.concatenate([rng.uniform(-1, 1, (N, n_joints, 3)), rng.uniform(-.5, .5, (N, n_joints, 2)), rng.uniform(1.5, 2.5, (N, n_joints, 1))], axis=2)


@pytest.mark.parametrize('n_links,n_joints', [(HAND_LINKS, 1), (HAND_LINKS, 3), (HAND_LINKS, 4), (2, 6), (3, 6)])
def test_hand_planes_at_the_other_counts_of_joints_and_links(n_links, n_joints):
    """`j < n_joints && j < id` and MOVING's `id <= n_joints` have an edge at every count; the other tests run 2 joints on 4 links
    and 6 on 6.  Here: fewer joints than moving links (1, 3), as many joints as ids below n_links + 1 (4: link 3 moves too), and
    joints beyond the drawn links (n_links 2 and 3 with 6 joints: the planes' links 2 .. 4 are not rendered)."""
    R, ids, T, _ = hand_planes()
    joints = _axes(np.random.default_rng(10 * n_links + n_joints), 3, n_joints)
    rc, got = _call(R, ids, T, joints, n_links, HAND_INTR)
    assert rc == 0
    want = _hold(got, R, ids, T, joints, n_links, HAND_INTR)
    top = min(n_joints, n_links - 1)                                 # the last link that is drawn and moves
    assert (want[:2, 2] > 0).all() and (want[:2, 10] > 0).all()
    live = [4 + j for j in range(min(top, 2))]                       # frame 0 has links 1 and 2
    assert want[0, live].all() and not got[0, 4 + min(top, 2):10].any() and not got[:, 4 + top:10].any()
    if n_links == HAND_LINKS and n_joints == 1:
        more = refine_ref.normal_equations(R, ids, T, n_links, HAND_INTR, _axes(np.random.default_rng(1), 3, 2))[0]
        assert more[0, 2] > want[0, 2]                               # a second joint moves frame 0's link 2 as well


def _chunk_edge_frames(Hh, Ww, rng):
    """Three frames a pixel below, at or above a workgroup's 2048, built as test_gpu_bundle's: links 0 .. 2 in stripes."""
    n = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    intr = (150.0, 150.0, Ww / 2 - 0.25, Hh / 2)
    R3 = np.stack([refine_ref.tilted_depth(Hh, Ww, intr, n, c) for c in (1.8, 2.0, 2.3)]).astype(np.float32)
    I3 = (np.arange(Ww)[None, None, :] * 3 // Ww + np.zeros((3, Hh, 1))).astype(np.uint8)
    I3[1, Hh - 1:] = 255
    T3 = (R3 + rng.uniform(-0.04, 0.04, R3.shape)).astype(np.float32)
    T3[0, Hh - 1, Ww - 5:] = 0.0
    return R3, I3, T3, intr


@pytest.mark.parametrize('Hh,Ww', [(23, 89), (32, 64), (3, 683)])
def test_kernel_at_the_chunk_edges_and_cut_into_calls(Hh, Ww):
    """2047, 2048 and 2049 pixels: the last pass one thread short, a full workgroup, a second workgroup for one pixel.  Three
    frames cut as [0:1], [1:3]: the gather kernel's last workgroup holds one frame of its two."""
    rng = np.random.default_rng(Hh)
    R3, I3, T3, intr = _chunk_edge_frames(Hh, Ww, rng)
    for n_joints in (2, 6):
        joints = _axes(rng, 3, n_joints)
        rc, got = _call(R3, I3, T3, joints, 3, intr)
        assert rc == 0
        want = _hold(got, R3, I3, T3, joints, 3, intr)
        assert (want[:, 2] > 500).all()                              # two of three stripes move, about 0.78 of them within the clip
    parts = [_call(R3[a:b], I3[a:b], T3[a:b], joints[a:b], 3, intr)[1] for a, b in ((0, 1), (1, 3))]
    assert np.concatenate(parts).tobytes() == got.tobytes()


def test_kernel_agrees_with_the_reference_on_renders_of_the_robot():
    from rope_s3d_amd.prediction.refinement import PoseRefiner
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    e, intr, truth = _robot_scene()
    try:
        ref = PoseRefiner(e, DEFAULT_CAMERA_POSE, intr, 'SLURBT')
        T_t, _ = e.render_batch_device(truth, 6)
        T = T_t.cpu().numpy()
        rng = np.random.default_rng(3)
        T[rng.random(T.shape) < 0.1] = 0.0                                   # holes
        T[:, 40:50, 60:80] = np.nan
        q = truth + np.array([.01, -.01, .01, 0, 0, 0])
        rd, ri = e.render_batch_device(q, 6)
        joints = ref.joint_axes(q)
        intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
        got = e.pose_normal_equations(rd, ri, torch.from_numpy(T).cuda(), joints, 6, CLIP, intr4)
        want = _hold(got, rd.cpu().numpy(), ri.cpu().numpy(), T, joints, 6, intr4)
        assert (want[:, 2] > 500).all() and (want[:, 10] > 0).all() and (want[:, 30] == 0).all()      # link 6 is never drawn: no T column
        # determinism: twice the same bytes; frames [0:3] in one call are [0:1] and [1:3], byte for byte
        again = e.pose_normal_equations(rd, ri, torch.from_numpy(T).cuda(), joints, 6, CLIP, intr4)
        assert again.tobytes() == got.tobytes()
        Tt = torch.from_numpy(T).cuda()
        parts = [e.pose_normal_equations(rd[a:b].contiguous(), ri[a:b].contiguous(), Tt[a:b].contiguous(), joints[a:b], 6, CLIP, intr4)
                 for a, b in ((0, 1), (1, 3))]
        assert np.concatenate(parts).tobytes() == got.tobytes()
        assert e.pose_normal_equations(rd[:0], ri[:0], Tt[:0], joints[:0], 6, CLIP, intr4).shape == (0, 32)
        for bad in ((rd.double(), ri, Tt), (rd, ri.int(), Tt), (rd, ri, Tt[:2]), (rd.cpu(), ri, Tt)):
            with pytest.raises(ValueError):
                e.pose_normal_equations(*bad, joints, 6, CLIP, intr4)
        with pytest.raises(ValueError):
            e.pose_normal_equations(rd, ri, Tt, joints, 6, -1.0, intr4)
    finally:
        e.close()


def test_hand_planes_give_the_same_bytes_twice_and_in_parts():
    R, ids, T, joints = hand_planes()
    rc, one = _call(R, ids, T, joints, HAND_LINKS, HAND_INTR)
    rc2, two = _call(R, ids, T, joints, HAND_LINKS, HAND_INTR)
    assert rc == 0 == rc2 and one.tobytes() == two.tobytes()
    parts = [_call(R[a:b], ids[a:b], T[a:b], joints[a:b], HAND_LINKS, HAND_INTR)[1] for a, b in ((0, 1), (1, 3))]
    assert np.concatenate(parts).tobytes() == one.tobytes()


def test_argument_errors_return_their_code_and_leave_the_output_alone():
    R, ids, T, joints = hand_planes()
    cases = [dict(n_frames=0), dict(n_frames=-1), dict(hw=(0, 23)), dict(hw=(20, 0)), dict(hw=(4097, 4096)), dict(n_links=0), dict(n_links=7),
             dict(n_joints=0), dict(n_joints=7), dict(clip=0.0), dict(clip=-CLIP), dict(clip=float('nan')), dict(clip=float('inf'))]
    cases += [dict(null=k) for k in range(6)] + [dict(odd=k) for k in (0, 2, 3, 4, 5)]
    for case in cases:
        kw = dict(n_links=HAND_LINKS, clip=CLIP)
        kw.update(case)
        n_links = kw.pop('n_links')
        rc, got = _call(R, ids, T, joints, n_links, HAND_INTR, **kw)
        assert rc == E_ARG and (got.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case


@pytest.fixture(scope='module')
def synth():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.synthetic import SyntheticPredictor
    return SyntheticPredictor(DEFAULT_CAMERA_POSE, '640_480_color', 4, 'SLU', noise=False, seed=11, lookup_divisions=4)


E2E_SEED = 20


def test_pose_refiner_walks_the_reference_loop_on_the_engines_renders(synth):
    """8 synthetic frames at 160 x 120; the start is the truth moved by up to 0.02 rad on S, L and U.  PoseRefiner and
    refine_ref.refine see the same renders (the engine's) and differ in the order of the kernel's sums alone."""
    from rope_s3d_amd.prediction.refinement import PoseRefiner
    p = synth.predictor
    rng = np.random.default_rng(E2E_SEED)
    lim = p.u_reader.joint_limits
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (8, 6)) * np.array([1, 1, 1, 0, 0, 0])
    start = truth + rng.uniform(-.02, .02, (8, 6)) * np.array([1, 1, 1, 0, 0, 0])
    ref = PoseRefiner(p.renderer, p.camera_pose, p.intrinsics, 'SLU')
    p.renderer.setMaxParts(None)
    T = p.renderer.render_ids_batch_device(truth)[0]
    got = ref.refine(start, T)
    intr4 = (p.intrinsics.fx, p.intrinsics.fy, p.intrinsics.cx, p.intrinsics.cy)

    def render(q):
        d, i = p.renderer.render_ids_batch_device(q)
        return d.cpu().numpy(), i.cpu().numpy()

    want = refine_ref.refine(start, refine_ref.equations_of(render, T.cpu().numpy(), 6, intr4, ref.joint_axes, CLIP), lim, (0, 1, 2), 5, 1e-3)
    # the condition on the seed: no accept / reject decision of the reference within the summation's reach of a tie
    assert (want['margins'] > 1e-6 * want['costs'][:-1]).all(), "choose another E2E_SEED: a decision of the loop is a near tie"
    print('steps', got.steps_taken, 'cost', got.cost_before, '->', got.cost_after, 'max angle difference', np.abs(got.angles - want['angles']).max())
    assert np.array_equal(got.steps_taken, want['steps_taken']) and (got.steps_taken >= 1).all()
    assert np.abs(got.angles - want['angles']).max() <= 1e-9
    assert (got.cost_after <= got.cost_before).all() and np.isfinite(got.sigma[:, :3]).all() and np.isnan(got.sigma[:, 3:]).all()
    assert np.array_equal(got.angles[:, 3:], start[:, 3:]) and np.array_equal(got.inliers, want['inliers'])
    assert np.abs(got.angles - truth)[:, :3].max() < np.abs(start - truth)[:, :3].max()


def test_predictor_switch_polishes_and_leaves_the_default_alone(synth):
    from rope_s3d_amd import Predictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    p = synth.predictor
    lim = helpers.robot().joint_limits
    colors, depths = [], []
    for seed in range(8):
        q = np.random.default_rng(50 + seed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
        synth.renderer.setJointAngles(q)
        c, d = synth.renderer.render()
        colors.append(c); depths.append(d)
    assert p.refine is False
    before = p.run_many(colors, depths)
    assert p.last_refinement is None
    off = Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', color_dict=p.color_dict, lookup_divisions=4, refine=False)
    assert off.run_many(colors, depths).tobytes() == before.tobytes() and off.last_refinement is None
    on = Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', color_dict=p.color_dict, lookup_divisions=4, refine=True)
    polished = on.run_many(colors, depths)
    res = on.last_refinement
    assert len(res) == 8 and res.sigma.shape == (8, 6) and np.array_equal(res.angles, polished)
    assert (res.cost_after <= res.cost_before).all() and np.isnan(res.sigma[:, 3:]).all() and not np.isnan(res.sigma[:, :3]).any()
    assert np.array_equal(polished[res.steps_taken == 0], before[res.steps_taken == 0]) and np.array_equal(polished[:, 3:], before[:, 3:])
    # frame after frame: the same polish, one entry per frame again
    serial = on.run_many(colors, depths, batch=1)
    assert len(on.last_refinement) == 8 and np.array_equal(serial, polished)
    one = on.run(colors[2], depths[2])
    assert len(on.last_refinement) == 1 and np.array_equal(one, polished[2])
