"""GPU: rope_mask_distance and rope_silhouette_normal_equations (csrc/rope_silhouette.hip) against the restatement of their
contracts (tests/silhouette_ref.py) — the field bit for bit, the counts of the normal equations exactly and every float sum within
the worst case of a reordered float64 summation — their determinism, what they refuse, and BundleRefiner(silhouette=...) end to end.

The bound is tests/test_gpu_bundle.py's: 4 n eps sum|terms| with n the pixel count of the frame and eps = 2^-52; the terms
themselves are the same bits on both sides."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import helpers
import silhouette_ref as sref
from test_gpu_bundle import DESCENT_STEP, TRUE_POSE_OFFSET

pytestmark = pytest.mark.gpu

E_ARG = -1
EPS = 2.0 ** -52
GARBAGE = float(np.frombuffer(b'\x5a' * 8, np.float64)[0])
GARBAGE_I32 = 0x5a5a5a5a
COMBOS = ((0, 6), (6, 0), (0, 1), (1, 0), (3, 6), (6, 6))          # (n_joints, n_cols)
INTR = (150.0, 140.0, 12.25, 9.5)


# ---------------------------------------------------------------------------------------------- the distance field
def _distance(mask, radius, null=None, odd=False, n=None, hw=None):
    """The C entry point on an output filled with garbage -> (rc, sd2 (N, H, W) int32)."""
    lib = eng.load_library()
    N, H, W = mask.shape
    m = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    out = torch.full((N * H * W + 2,), GARBAGE_I32, dtype=torch.int32, device='cuda')
    ptrs = [m.data_ptr(), out.data_ptr() + (2 if odd else 0)]
    ptrs = [None if null == k else C.c_void_p(p) for k, p in enumerate(ptrs)]
    H2, W2 = hw if hw is not None else (H, W)
    rc = lib.rope_mask_distance(ptrs[0], N if n is None else n, H2, W2, radius, ptrs[1], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[N * H * W:] == GARBAGE_I32).all()                                        # nothing written past the planes
    return rc, got[:N * H * W].reshape(N, H, W)


def _masks_37x53():
    H, W = 37, 53
    yy, xx = np.mgrid[0:H, 0:W]
    corners = np.zeros((H, W), bool)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    middle = np.zeros((H, W), bool)
    middle[18, 26] = True
    planes = [np.zeros((H, W), bool), np.ones((H, W), bool), corners, middle, (yy + xx) % 2 == 0,
              np.random.default_rng(11).random((H, W)) < 0.5, (yy - 18) ** 2 + (xx - 26) ** 2 <= 20 * 20,
              ~corners, (yy // 3 + xx // 5) % 2 == 0]
    return np.stack(planes).astype(np.uint8) * 3


@pytest.fixture(scope='module')
def masks_and_fields():
    masks = _masks_37x53()
    return masks, {R: sref.mask_distance(masks, R) for R in (1, 5, 16)}


@pytest.mark.parametrize('radius', [1, 5, 16])
def test_distance_field_is_the_reference_bit_for_bit(masks_and_fields, radius):
    """Nine planes of 37 x 53 in three calls of N = 3: two tiles by two, the last of each row and column partial."""
    masks, want = masks_and_fields
    for lo in (0, 3, 6):
        rc, got = _distance(masks[lo:lo + 3], radius)
        assert rc == 0
        bad = np.argwhere(got != want[radius][lo:lo + 3])
        assert len(bad) == 0, (radius, lo, bad[:5])
    far = radius * radius + 1
    assert (want[radius][0] == far).all() and (want[radius][1] == -far).all()
    if radius < 16:
        assert want[radius][6][18, 26] == -far                                          # the disc's interior


def test_distance_field_on_single_rows_and_columns_and_many_planes():
    rng = np.random.default_rng(4)
    for shape in ((2, 1, 71), (2, 67, 1), (1, 1, 1), (3, 33, 32), (2, 32, 65)):
        m = (rng.random(shape) < 0.4).astype(np.uint8)
        for R in (1, 7, 16):
            rc, got = _distance(m, R)
            assert rc == 0 and np.array_equal(got, sref.mask_distance(m, R)), (shape, R)
    rc, got = _distance(np.zeros((0, 4, 4), np.uint8), 3)
    assert rc == 0
    e = eng.Engine(0)
    try:
        m = torch.from_numpy(rng.random((5, 20, 40)) < 0.3).cuda()
        sd = e.mask_distance(m, 6)
        assert sd.dtype == torch.int32 and np.array_equal(sd.cpu().numpy(), sref.mask_distance(m.cpu().numpy(), 6))
        assert np.array_equal(e.mask_distance(m.to(torch.uint8) * 200, 6).cpu().numpy(), sd.cpu().numpy())
        assert tuple(e.mask_distance(m[:0], 6).shape) == (0, 20, 40)
        for bad in (lambda: e.mask_distance(m, 0), lambda: e.mask_distance(m, 17), lambda: e.mask_distance(m.cpu(), 4),
                    lambda: e.mask_distance(m.float(), 4), lambda: e.mask_distance(m[0], 4)):
            with pytest.raises(ValueError):
                bad()
    finally:
        e.close()


def test_distance_field_walks_the_planes_beyond_the_grids_height():
    """32 768 + 5 planes of 3 x 5 at radius 2: the grid is 32 768 workgroups high and the workgroups 0 .. 4 walk on to a second
    plane each.  Seven distinct masks, tiled: plane i is mask i % 7, so no two planes 32 768 apart are the same."""
    planes = 32768 + 5
    rng = np.random.default_rng(12)
    seven = (rng.random((7, 3, 5)) < 0.45).astype(np.uint8)
    seven[5], seven[6] = 0, 1                                                           # FAR everywhere, both signs
    want7 = sref.mask_distance(seven, 2)
    assert len({w.tobytes() for w in want7}) == 7 and 32768 % 7 != 0
    which = np.arange(planes) % 7
    rc, got = _distance(seven[which], 2)
    assert rc == 0
    for i in (0, 4, 5, 32767, 32768, 32769, planes - 1):
        assert np.array_equal(got[i], want7[i % 7]), i
    bad = np.flatnonzero((got != want7[which]).any(axis=(1, 2)))
    assert len(bad) == 0, bad[:8]


def test_distance_field_refuses_bad_arguments_and_writes_nothing():
    m = np.ones((2, 5, 6), np.uint8)
    for case in (dict(n=-1), dict(hw=(0, 6)), dict(hw=(5, 0)), dict(hw=(1 << 16, 1 << 15)), dict(radius=0), dict(radius=17), dict(radius=-3),
                 dict(null=0), dict(null=1), dict(odd=True)):
        kw = dict(radius=4)
        kw.update(case)
        rc, got = _distance(m, **kw)
        assert rc == E_ARG and (got == GARBAGE_I32).all(), case


# ---------------------------------------------------------------------------------------------- the normal equations
def _call(R, ids, sd2, joints, twists, n_links, intr, radius, null=None, odd=None, n_frames=None, hw=None, n_joints=None, n_cols=None):
    """The C entry point on an out buffer filled with garbage -> (rc, out (N, 96) float64).  Pointers by position: 0 render, 1 ids,
    2 field, 3 joints, 4 twists, 5 out, 6 work."""
    N, H, W = R.shape
    lib = eng.load_library()
    joints = np.zeros((N, 0, 6)) if joints is None else np.asarray(joints, np.float64)
    twists = np.zeros((N, 0, 6)) if twists is None else np.asarray(twists, np.float64)
    pad = lambda a: a if a.size else np.zeros((N, 1, 6))
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (R, ids, sd2, pad(joints), pad(twists))]
    out = torch.full((N, 96), GARBAGE, dtype=torch.float64, device='cuda')
    work = torch.full((max(1, lib.rope_silhouette_normal_workspace(N, H, W) // 8) + 1,), GARBAGE, dtype=torch.float64, device='cuda')
    ptrs = [x.data_ptr() for x in t] + [out.data_ptr(), work.data_ptr()]
    if odd is not None:
        ptrs[odd] += 2
    ptrs = [C.c_void_p(p) for p in ptrs]
    nj = joints.shape[1] if n_joints is None else n_joints
    nc = twists.shape[1] if n_cols is None else n_cols
    if joints.shape[1] == 0 and n_joints is None:
        ptrs[3] = None
    if twists.shape[1] == 0 and n_cols is None:
        ptrs[4] = None
    if null is not None:
        ptrs[null] = None
    H, W = hw if hw is not None else (H, W)
    rc = lib.rope_silhouette_normal_equations(ptrs[0], ptrs[1], ptrs[2], N if n_frames is None else n_frames, H, W, n_links,
                                              *[float(v) for v in intr], ptrs[3], nj, ptrs[4], nc, radius, ptrs[5], ptrs[6],
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert work[-1].item() == GARBAGE
    return rc, out.cpu().numpy()


def _hold(got, R, ids, sd2, joints, twists, n_links, intr, radius):
    want, mag = sref.normal_equations(R, ids, sd2, n_links, intr, joints, twists, radius)
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
    for f in range(len(got)):
        A, g = sref.unpack(got[f])
        assert not g[dead].any() and not A[dead].any() and not A[:, dead].any()
    return want


def _columns(rng, N, nj, nc):
    joints = np.concatenate([rng.uniform(-1, 1, (N, nj, 3)), rng.uniform(-.5, .5, (N, nj, 2)), rng.uniform(1.5, 2.5, (N, nj, 1))], axis=2) if nj else None
    return joints, (rng.uniform(-1, 1, (N, nc, 6)) if nc else None)


def _hand_planes():
    """Two frames of 20 x 30.  Frame 0: a cross on links 0 .. 4 that touches all four edges of the frame (no contour there), ids 4
    and 200 in it, against the mask of the cross moved by (2, -1).  Frame 1: a single rendered pixel inside its mask's reach."""
    H, W = 20, 30
    rng = np.random.default_rng(8)
    cross = np.zeros((H, W), bool)
    cross[7:13, :] = True
    cross[:, 11:19] = True
    ids = np.full((2, H, W), 255, np.uint8)
    ids[0][cross] = (np.arange(W)[None, :] * 5 // W + np.zeros((H, 1), int))[cross]
    ids[0, 9, 14], ids[0, 3, 15] = 4, 200
    ids[1, 10, 17] = 2
    R = rng.uniform(1.5, 2.5, ids.shape).astype(np.float32)
    mask = np.zeros((2, H, W), np.uint8)
    mask[0] = np.roll(cross, (2, -1), axis=(0, 1))
    mask[1, 8:14, 12:17] = 1
    return R, ids, mask


def test_kernel_agrees_with_the_reference_on_hand_built_planes_and_thin_frames():
    rng = np.random.default_rng(6)
    R, ids, mask = _hand_planes()
    for radius in (5, 2):
        sd2 = sref.mask_distance(mask, radius)
        for n_links in (6, 4):                                      # 4: the pixels of id 4 are background, and holes in the blob
            for nj, nc in COMBOS:
                joints, tw = _columns(rng, 2, nj, nc)
                rc, got = _call(R, ids, sd2, joints, tw, n_links, INTR, radius)
                assert rc == 0
                want = _hold(got, R, ids, sd2, joints, tw, n_links, INTR, radius)
            assert want[1, 0] == 1 and want[1, 2] == 1 and want[0, 0] > 40 and want[0, 2] > 0
    # no contour at the frame's edges: the cross without its holes has one only along the sides of its arms, 11 + 11 pixels above
    # and below the bar and 7 + 7 left and right of the post; the arms' ends, on the frame's edge, have none
    plain = np.where(ids[:1] == 200, 0, ids[:1]).astype(np.uint8)
    plain[0, 9, 14] = 0
    want, _ = sref.normal_equations(R[:1], plain, sref.mask_distance(mask[:1], 5), 6, INTR, None, np.zeros((1, 1, 6)), 5)
    assert want[0, 0] == 2 * (11 + 11) + 2 * (7 + 7) == 72
    # W = 1 and H = 1: the gradient across the frame is 0, along it one-sided at the ends
    for shape in ((2, 1, 23), (2, 19, 1), (1, 1, 1)):
        ids1 = np.where(rng.random(shape) < 0.5, 1, 255).astype(np.uint8)
        ids1[0, 0, 0] = 1
        R1 = rng.uniform(1.5, 2.5, shape).astype(np.float32)
        sd1 = sref.mask_distance(rng.random(shape) < 0.5, 3)
        joints, tw = _columns(rng, shape[0], 2, 6)
        rc, got = _call(R1, ids1, sd1, joints, tw, 6, INTR, 3)
        assert rc == 0
        want = _hold(got, R1, ids1, sd1, joints, tw, 6, INTR, 3)
        assert (want[:, 0] > 0).all() or shape == (1, 1, 1)
    # below, at and above a workgroup's 2048 pixels
    for Hh, Ww in ((23, 89), (32, 64), (47, 45)):
        blob = np.hypot(*(np.mgrid[0:Hh, 0:Ww] - np.array([Hh / 2, Ww / 2])[:, None, None])) < Hh / 2 - 2
        ids3 = np.where(np.stack([blob, np.roll(blob, 3, 1)]), 3, 255).astype(np.uint8)
        R3 = rng.uniform(1.5, 2.5, ids3.shape).astype(np.float32)
        sd3 = sref.mask_distance(np.stack([np.roll(blob, 2, 0), blob]), 6)
        joints, tw = _columns(rng, 2, 6, 6)
        rc, got = _call(R3, ids3, sd3, joints, tw, 6, INTR, 6)
        assert rc == 0
        _hold(got, R3, ids3, sd3, joints, tw, 6, INTR, 6)
        parts = [_call(R3[a:b], ids3[a:b], sd3[a:b], joints[a:b], tw[a:b], 6, INTR, 6)[1] for a, b in ((0, 1), (1, 2))]
        assert np.concatenate(parts).tobytes() == got.tobytes()


def test_argument_errors_return_their_code_and_leave_the_output_alone():
    R, ids, mask = _hand_planes()
    sd2 = sref.mask_distance(mask, 5)
    joints, tw = _columns(np.random.default_rng(2), 2, 2, 2)
    cases = [dict(n_frames=0), dict(n_frames=-1), dict(hw=(0, 23)), dict(hw=(20, 0)), dict(hw=(4097, 4096)), dict(n_links=0), dict(n_links=7),
             dict(n_joints=-1), dict(n_joints=7), dict(n_cols=-1), dict(n_cols=7), dict(n_joints=0, n_cols=0), dict(radius=0), dict(radius=17),
             dict(radius=-5)]
    cases += [dict(null=k) for k in range(7)] + [dict(odd=k) for k in (0, 2, 3, 4, 5, 6)]
    for case in cases:
        kw = dict(n_links=6, radius=5)
        kw.update(case)
        n_links, radius = kw.pop('n_links'), kw.pop('radius')
        rc, got = _call(R, ids, sd2, joints, tw, n_links, INTR, radius, **kw)
        assert rc == E_ARG and (got.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case
    for bad_intr in ((0.0, 140.0, 1.0, 1.0), (150.0, float('nan'), 1.0, 1.0), (150.0, 140.0, float('inf'), 1.0)):
        rc, got = _call(R, ids, sd2, joints, tw, 6, bad_intr, 5)
        assert rc == E_ARG and (got.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), bad_intr
    rc, got = _call(R, ids, sd2, None, tw, 6, INTR, 5)                     # a null pointer with a count of 0 is no error
    assert rc == 0 and not np.isnan(got).any()


@pytest.fixture(scope='module')
def renderer():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.simulation.render import Renderer
    r = Renderer('seg', DEFAULT_CAMERA_POSE, '1280_720_color', intrinsic_ds_factor=8)
    yield r
    r.engine.close()


def _scene(renderer, n=10, seed=1):
    """n random S / L / U poses under the true camera; the start: the camera one lattice step of the camera search away (5 mm,
    4 mrad at most) and every angle within one Descent step."""
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    rng = np.random.default_rng(seed)
    lim = renderer.robot.joint_limits
    slu = np.array([1, 1, 1, 0, 0, 0])
    truth = rng.uniform(lim[:, 0] * .5, lim[:, 1] * .5, (n, 6)) * slu
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + TRUE_POSE_OFFSET
    start_pose = true_pose + rng.uniform(-1, 1, 6) * np.array([.005, .005, .005, .004, .004, .004])
    start = truth + rng.uniform(-DESCENT_STEP, DESCENT_STEP, (n, 6)) * slu
    return truth, true_pose, start, start_pose


def test_kernel_on_renders_of_the_robot_against_the_reference(renderer):
    """4 frames at 160 x 90 = 14 400 pixels, eight workgroups a frame: the render one Descent step from the pose of the mask."""
    from rope_s3d_amd.prediction.refinement import BundleRefiner, camera_twists
    from rope_s3d_amd.projection import camera_matrix
    e, intr = renderer.engine, renderer.intrinsics
    assert (intr.width, intr.height) == (160, 90)
    truth, true_pose, _, _ = _scene(renderer, 4, 3)
    PV = np.tile(camera_matrix(true_pose, intr)[None], (4, 1, 1))
    _, ti = e.render_batch_device(truth, 6, PV)
    mask_t = ti < 6
    radius = 8
    sd2_t = e.mask_distance(mask_t, radius)
    sd2 = sd2_t.cpu().numpy()
    assert np.array_equal(sd2, sref.mask_distance(mask_t.cpu().numpy(), radius))
    q = truth + DESCENT_STEP * np.array([1, -1, 1, 0, 0, 0])
    rd, ri = e.render_batch_device(q, 6, PV)
    twists = np.tile(camera_twists(true_pose)[None], (4, 1, 1))
    joints = BundleRefiner(e, intr).joint_axes(true_pose, q)
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
    Rn, In = rd.cpu().numpy(), ri.cpu().numpy()
    got = e.silhouette_normal_equations(rd, ri, sd2_t, joints, twists, 6, radius, intr4)
    want = _hold(got, Rn, In, sd2, joints, twists, 6, intr4, radius)
    A, _ = sref.unpack(got[0])
    live = [0, 1, 2, 3, 4] + list(range(6, 12))
    assert (want[:, 0] > 100).all() and (want[:, 2] > 100).all() and (np.diag(A)[live] > 0).all() and A[5, 5] == 0
    assert (got[:, 1] / got[:, 0] < 9).all()                                # within three pixels of the mask, in the mean
    for nj, nc in ((3, 6), (6, 0), (0, 6)):
        part = e.silhouette_normal_equations(rd, ri, sd2_t, joints[:, :nj] if nj else None, twists[:, :nc] if nc else None, 6, radius, intr4)
        _hold(part, Rn, In, sd2, joints[:, :nj] if nj else None, twists[:, :nc] if nc else None, 6, intr4, radius)
    # a render on its own mask: no residual at all
    same = e.silhouette_normal_equations(*e.render_batch_device(truth, 6, PV), sd2_t, joints, twists, 6, radius, intr4)
    assert not same[:, 1].any() and not same[:, 3:16].any() and np.array_equal(same[:, 0], same[:, 2])
    # determinism: twice the same bytes; one call of 4 frames is two calls of 2, byte for byte
    again = e.silhouette_normal_equations(rd, ri, sd2_t, joints, twists, 6, radius, intr4)
    assert again.tobytes() == got.tobytes()
    parts = [e.silhouette_normal_equations(rd[a:b].contiguous(), ri[a:b].contiguous(), sd2_t[a:b].contiguous(), joints[a:b], twists[a:b], 6, radius,
                                           intr4) for a, b in ((0, 2), (2, 4))]
    assert np.concatenate(parts).tobytes() == got.tobytes()
    assert e.silhouette_normal_equations(rd[:0], ri[:0], sd2_t[:0], joints[:0], twists[:0], 6, radius, intr4).shape == (0, 96)
    for bad in ((rd.double(), ri, sd2_t), (rd, ri.int(), sd2_t), (rd, ri, sd2_t[:2]), (rd, ri, sd2_t.float()), (rd.cpu(), ri, sd2_t)):
        with pytest.raises(ValueError):
            e.silhouette_normal_equations(*bad, joints, twists, 6, radius, intr4)
    with pytest.raises(ValueError):
        e.silhouette_normal_equations(rd, ri, sd2_t, None, None, 6, radius, intr4)
    with pytest.raises(ValueError):
        e.silhouette_normal_equations(rd, ri, sd2_t, joints, twists, 6, 17, intr4)


# ---------------------------------------------------------------------------------------------- the refiner
@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_bundle_refiner_with_the_outline_term(renderer, mode):
    """Ten frames at 160 x 90, masks and depth from renders at the truth."""
    from rope_s3d_amd.prediction.refinement import BundleRefiner
    from rope_s3d_amd.projection import camera_matrix
    e, intr = renderer.engine, renderer.intrinsics
    truth, true_pose, start, start_pose = _scene(renderer)
    T_t, ti = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (10, 1, 1)))
    mask = (ti < 6).cpu().numpy()
    # the outline alone
    alone = BundleRefiner(renderer, intr, joints=mode, silhouette=1.0).refine(start_pose, start, None, mask)
    print(mode, 'outline alone: steps', alone.steps_taken, 'cost', alone.cost_silhouette_before, '->', alone.cost_silhouette_after,
          'pose error', np.abs(start_pose - true_pose), '->', np.abs(alone.pose - true_pose), 'sigma_pose', alone.sigma_pose)
    assert alone.cost_silhouette_after < alone.cost_silhouette_before and alone.steps_taken >= 1 and alone.inliers_silhouette > 500
    assert np.isnan(alone.cost_before) and np.isnan(alone.cost_after) and alone.inliers == 0 and np.isnan(alone.frame_cost).all()
    assert np.array_equal(alone.angles[:, 3:], start[:, 3:])
    # with depth: the cost a step is judged by never grows
    both = BundleRefiner(renderer, intr, joints=mode, silhouette=1.0).refine(start_pose, start, T_t, torch.from_numpy(mask).cuda())
    far2 = (np.sqrt(8 * 8 + 1.0) - 0.5) ** 2
    combined = lambda cd, cs: cd / (2.0 ** -5) ** 2 + cs / far2
    print(mode, 'both: steps', both.steps_taken, 'depth cost', both.cost_before, '->', both.cost_after, 'outline cost', both.cost_silhouette_before, '->',
          both.cost_silhouette_after, 'pose error', np.abs(both.pose - true_pose), 'sigma_pose', both.sigma_pose)
    assert combined(both.cost_after, both.cost_silhouette_after) <= combined(both.cost_before, both.cost_silhouette_before)
    assert both.cost_silhouette_before == alone.cost_silhouette_before and both.frame_cost.shape == (10,) and both.inliers > 0
    # without the term: what the call without the new arguments returns, byte for byte
    old = BundleRefiner(renderer, intr, joints=mode).refine(start_pose, start, T_t)
    off = BundleRefiner(renderer, intr, joints=mode, silhouette=0.0, radius=3).refine(start_pose, start, T_t, mask)
    assert old.pose.tobytes() == off.pose.tobytes() and old.angles.tobytes() == off.angles.tobytes() and old.sigma_pose.tobytes() == off.sigma_pose.tobytes()
    assert (old.cost_before, old.cost_after, old.steps_taken, old.inliers) == (off.cost_before, off.cost_after, off.steps_taken, off.inliers)
    assert old.frame_cost.tobytes() == off.frame_cost.tobytes() and np.isnan(off.cost_silhouette_after) and off.inliers_silhouette == 0


# ---------------------------------------------------------------------------------------------- the public interface
@pytest.mark.parametrize('mode', ['modelless', 'segmented'])
def test_predictor_switch_bundle_and_silhouette(mode):
    from rope_s3d_amd import CameraPredictor, ModellessCameraPredictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import BundleRefineResult
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
    kw = dict(base_intrinsics='640_480_color', refine='bundle+silhouette')
    p = ModellessCameraPredictor(start, 4, **kw) if mode == 'modelless' else CameraPredictor(start, 4, segmenter=ColorSegmenter(names), **kw)
    p.stages = [('descent', 6, 0.5, .001, [True] * 6, [0.002] * 6)]
    try:
        pose = p.run(np.stack(colors), np.stack(depths), qs.copy())
        res = p.last_refinement
        assert p.refine == 'bundle+silhouette' and isinstance(res, BundleRefineResult) and np.array_equal(pose, res.pose)
        assert p._robot_masks.shape == (4, 120, 160) and p._robot_masks.dtype == bool and p._robot_masks.any(axis=(1, 2)).all()
        assert res.inliers_silhouette > 0 and np.isfinite(res.cost_silhouette_before) and np.isfinite(res.cost_before)
        far2 = (np.sqrt(65.0) - 0.5) ** 2
        assert res.cost_after / 2.0 ** -10 + res.cost_silhouette_after / far2 <= res.cost_before / 2.0 ** -10 + res.cost_silhouette_before / far2
        print(mode, 'steps', res.steps_taken, 'depth cost', res.cost_before, '->', res.cost_after, 'outline cost', res.cost_silhouette_before, '->',
              res.cost_silhouette_after)
    finally:
        p.engine.close()


def test_calibrate_takes_the_switch_on_a_colour_coded_set(tmp_path):
    import json
    import os
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
    out = tmp_path / 'sil.json'
    r = subprocess.run([sys.executable, os.path.join(root, 'calibrate.py'), 'synthetic:8', '-frames', '8', '-joints', 'frame', '-ds_factor', '8',
                        '-iterations', '2', '-silhouette', '1', '-radius', '6', '-json', str(out)], cwd=root, capture_output=True, text=True)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(out.read_text())
    assert rep['silhouette'] == 1.0 and rep['radius'] == 6 and rep['inliers_silhouette'] > 0 and rep['inliers'] > 0
    far2 = (np.sqrt(37.0) - 0.5) ** 2                                     # the cost a step is judged by never grows
    assert rep['cost_after'] / 2.0 ** -10 + rep['cost_silhouette_after'] / far2 <= rep['cost_before'] / 2.0 ** -10 + rep['cost_silhouette_before'] / far2
    assert len(rep['sigma_angles']) == 8
    r = subprocess.run([sys.executable, os.path.join(root, 'calibrate.py'), 'synthetic:8', '-frames', '8', '-joints', 'fixed', '-silhouette', '1'],
                       cwd=root, capture_output=True, text=True)
    assert r.returncode != 0 and '-silhouette' in r.stderr
