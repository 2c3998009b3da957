"""CPU: camera_twists (prediction/refinement.py) held to central differences of the camera transform; the reference of
rope_camera_normal_equations (tests/camera_refine_ref.py) held to world planes whose depth under a camera pose is known in closed
form, and to a flat frame whose words are worked out by hand; the pooled loop on renderer-free scenes of planes."""
import os

import numpy as np

import camera_refine_ref as cref
import refine_ref
from refine_ref import CLIP

EPS = 2.0 ** -52
INTR = (150.0, 150.0, 11.5, 9.25)
H, W = 20, 24
POSE = np.array([0.1, -1.5, 0.55, 0.04, -0.07, 0.06])          # looks along +y of the world, a little off every axis
PLANES = np.array([[0.3, 1.0, -0.2], [-0.5, 1.0, 0.1], [0.1, 1.0, 0.6]])
POINTS = np.array([[0.0, 0.5, 0.5], [0.0, 0.42, 0.5], [0.0, 0.46, 0.5]])


def _world_planes(rows):
    n = PLANES[rows] / np.linalg.norm(PLANES[rows], axis=1)[:, None]
    return np.concatenate([n, (n * POINTS[rows]).sum(axis=1)[:, None]], axis=1)


def test_twists_are_the_derivative_of_the_camera_transform():
    """X_c(p) = Rwc(p) (X_w - t(p)); column k of camera_twists gives dX_c / dp_k = w x X_c + v.  Central difference with h = 1e-6
    on points within 3 m: truncation about h^2 |X| ~ 1e-12, rounding about eps |X| / h ~ 1e-9; 1e-8 covers both."""
    from rope_s3d_amd.prediction.refinement import camera_twists
    from rope_s3d_amd.projection import camera_pose_matrix
    rng = np.random.default_rng(1)
    h = 1e-6
    worst = 0.0
    for _ in range(20):
        p = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-np.pi, np.pi, 3)])
        X = rng.uniform(-3, 3, (16, 3)) / np.sqrt(3)
        tw = camera_twists(p)
        assert tw.shape == (6, 6) and not tw[:3, :3].any() and not tw[3:, 3:].any()
        Rwc, t = cref.Rwc_t(p, camera_pose_matrix)
        Xc = (X - t) @ Rwc.T
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            (Rp, tp), (Rm, tm) = cref.Rwc_t(p + d, camera_pose_matrix), cref.Rwc_t(p - d, camera_pose_matrix)
            central = ((X - tp) @ Rp.T - (X - tm) @ Rm.T) / (2 * h)
            mine = np.cross(tw[k, :3], Xc) + tw[k, 3:]
            worst = max(worst, np.abs(mine - central).max())
            assert np.abs(mine - central).max() <= 1e-8, (k, p)
    print(f"largest |twist velocity - central difference| {worst:.3e}")


def test_jacobian_of_a_world_plane_is_the_derivative_of_its_closed_form():
    """A world plane n_w . X_w = c_w on link 0, seen from the pose p, has the depth z(p) = d_c / (n_c . k) with n_c = Rwc(p) n_w and
    d_c = c_w - n_w . t(p) along the ray k = (kx, ky, 1).  The reference's J_k at p against (z(p + h e_k) - z(p - h e_k)) / 2h.

    The bound is tests/test_refine_refs.py's plane bound, read for this plane.  Along a translation z is linear in the parameter
    (n_c fixed, d_c linear): no truncation.  Along an angle n_c(theta) is a rotation of n_w between fixed rotations, every
    derivative of length at most 1, and d_c does not change: that test's c(theta) with the point on the axis o = 0, so
    |z'''| <= |d_c| |u'''| with its u''' bound, and the central difference is off by h^2 B3 / 6.  Rounding of the quotient:
    16 eps max|z| / h, as there.  The reference's normal: delta = 20 eps fx |k| + 4 eps relative, and J = z n.u / n.P with the
    velocity u = w x P + v in place of a x (P - o) moves by at most 10 delta (|u| + |J|)."""
    from rope_s3d_amd.prediction.refinement import camera_twists
    from rope_s3d_amd.projection import camera_pose_matrix
    h = 1e-6
    fx, fy, cx, cy = INTR
    pl = _world_planes([0])[0]
    kx = (np.arange(W) - cx) / fx
    ky = (np.arange(H) - cy) / fy
    K = np.stack([kx[None, :] + np.zeros((H, 1)), ky[:, None] + np.zeros((1, W)), np.ones((H, W))])
    knorm = np.sqrt((K * K).sum(axis=0))

    def z_of(p):
        Rwc, t = cref.Rwc_t(p, camera_pose_matrix)
        return (pl[3] - pl[:3] @ t) / np.einsum('i,ihw->hw', Rwc @ pl[:3], K)

    def inv_nk(p):
        Rwc, _ = cref.Rwc_t(p, camera_pose_matrix)
        return 1.0 / np.abs(np.einsum('i,ihw->hw', Rwc @ pl[:3], K))

    z = z_of(POSE)
    assert (z > 1.5).all() and (z < 3).all()
    ids = np.zeros((H, W), np.uint8)                                                     # link 0: the base carries the system
    tw = camera_twists(POSE)
    t = cref.pixel_terms(z, ids, z.astype(np.float32), 1, INTR, tw, CLIP)
    assert t['inlier'].all() and t['normal'].all()
    P = K * z
    d_c = abs(pl[3] - pl[:3] @ POSE[:3])
    delta = 20 * EPS * fx * knorm + 4 * EPS
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        central = (z_of(POSE + e) - z_of(POSE - e)) / (2 * h)
        u = np.maximum(inv_nk(POSE), np.maximum(inv_nk(POSE + e), inv_nk(POSE - e)))
        u3 = knorm * u ** 2 + 6 * knorm ** 2 * u ** 3 + 6 * knorm ** 3 * u ** 4
        B3 = d_c * u3 if k >= 3 else 0.0
        vel = np.cross(tw[k, :3], P, axisa=0, axisb=0, axisc=0) + tw[k, 3:, None, None]
        bound = h * h * B3 / 6 + 16 * EPS * np.abs(z).max() / h + 10 * delta * (np.sqrt((vel ** 2).sum(axis=0)) + np.abs(t['J'][k]))
        err = np.abs(t['J'][k] - central)
        print(f"parameter {k}: max |J - central| {err.max():.3e}, bound there {bound.flat[err.argmax()]:.3e}, max |J| {np.abs(t['J'][k]).max():.3f}")
        assert (err <= bound).all() and bound.max() < 1e-7 and np.abs(t['J'][k]).max() > 0.05, k
    # fewer columns: the ones given are the same, the others zero
    three = cref.pixel_terms(z, ids, z.astype(np.float32), 1, INTR, tw[:3], CLIP)
    assert np.array_equal(three['J'][:3], t['J'][:3]) and not three['J'][3:].any()


def test_hand_checked_words_of_a_flat_frame():
    R, ids, T, twists, words = cref.flat_frame()
    t = cref.pixel_terms(R[0], ids[0], T[0], 2, refine_ref.HAND_INTR, twists[0], CLIP)
    assert t['inlier'][:6].sum() == 6 * 23 - 1 and t['inlier'][0].all() and t['inlier'][5].all()       # link 0 carries the system
    assert not t['both'][6:10].any() and not t['inlier'][6:10].any()                                 # the background does not
    assert t['both'][15, 1] and not t['inlier'][15, 1] and not t['both'][3, 7]
    assert (t['J'][0][t['inlier']] == 1.0).all() and (t['J'][1][t['inlier']] == -0.5).all() and not t['J'][2:].any()
    sums, mag = cref.normal_equations(R, ids, T, 2, refine_ref.HAND_INTR, twists, CLIP)
    assert np.array_equal(sums[0], words), (sums[0], words)
    assert (np.abs(sums) <= mag).all() and mag[0, 4] == 2.0 ** -6 + 2.0 ** -7
    # one column: the second one's words are zero too
    one, _ = cref.normal_equations(R, ids, T, 2, refine_ref.HAND_INTR, twists[:, :1], CLIP)
    assert one[0, 5] == 0 and one[0, 11] == 0 and one[0, 16] == 0 and np.array_equal(one[0, [0, 1, 2, 3, 4, 10]], words[[0, 1, 2, 3, 4, 10]])
    # with one link drawn (n_links = 1) link 1 is not rendered: the system is link 0's alone
    base, _ = cref.normal_equations(R, ids, T, 1, refine_ref.HAND_INTR, twists, CLIP)
    assert base[0, 0] == 6 * 23 - 1 and base[0, 2] == 6 * 23 - 1 and base[0, 4] == 2.0 ** -6


def _plane_scene():
    """Two frames of planes (a corner of three, and two of them) seen at 40 x 48; the frames are what the true pose sees."""
    from rope_s3d_amd.prediction.refinement import camera_twists
    from rope_s3d_amd.projection import camera_pose_matrix
    Hs, Ws, intr = 40, 48, (150.0, 150.0, 23.5, 19.25)
    sets = [_world_planes([0, 1, 2]), _world_planes([2, 0])]

    def render(p):
        out = [cref.plane_depth(Hs, Ws, intr, *cref.Rwc_t(p, camera_pose_matrix), s) for s in sets]
        return np.stack([d.astype(np.float32) for d, _ in out]), np.stack([i for _, i in out])

    T = render(POSE)[0]

    def equations(p):
        R, ids = render(p)
        return cref.normal_equations(R, ids, T, 3, intr, np.tile(camera_twists(p)[None], (2, 1, 1)), CLIP)[0]
    return equations


def test_pooled_loop_never_raises_the_cost_and_marks_what_it_does_not_refine():
    from rope_s3d_amd.prediction import refinement as rf
    equations = _plane_scene()
    start = POSE + np.array([.004, -.003, .005, .003, -.002, .004])
    res = cref.refine(start, equations, range(6), iterations=4)
    print('cost', res['costs'], 'steps', res['steps_taken'], 'error', np.abs(start - POSE), '->', np.abs(res['pose'] - POSE), 'sigma', res['sigma'])
    assert res['costs'].shape == (5,) and (np.diff(res['costs']) <= 0).all() and res['cost_after'] <= res['cost_before']
    assert res['steps_taken'] >= 1 and res['cost_after'] < 0.25 * res['cost_before']
    assert np.linalg.norm(res['pose'] - POSE) < np.linalg.norm(start - POSE)             # the twists' signs are right
    assert np.isfinite(res['sigma']).all() and (res['sigma'] > 0).all() and res['frame_cost'].shape == (2,)
    xyz = cref.refine(start, equations, (0, 1, 2), iterations=3)
    assert np.array_equal(xyz['pose'][3:], start[3:]) and np.isnan(xyz['sigma'][3:]).all() and np.isfinite(xyz['sigma'][:3]).all()
    assert xyz['cost_after'] <= xyz['cost_before']
    # the host half of CameraPoseRefiner is the reference's
    words = equations(res['pose'])
    assert np.array_equal(rf.pool_frames(words), cref.pool(words))
    pooled = cref.pool(words)
    for active in (list(range(6)), [0, 1, 2]):
        assert np.array_equal(rf.formal_sigma(pooled, active), refine_ref.sigma(pooled, active), equal_nan=True)
        assert np.array_equal(rf.levenberg_step(pooled, active, 1e-3), refine_ref.step(pooled, active, 1e-3))
    assert rf.mean_cost(pooled[None])[0] == refine_ref.mean_cost(pooled)


def test_a_parameter_the_views_do_not_show_has_an_infinite_sigma():
    """One fronto-parallel plane z = 2 and the six unit twists: sliding the plane in itself (v = x, v = y) and turning it about the
    optical axis (w = z) move no pixel's depth — n . u is exactly 0 — so their diagonal entries are 0 and their sigma inf; v = z,
    w = x and w = y are seen (J = 1, ky z, -kx z: independent)."""
    Hh, Ww = 20, 23
    R = np.full((1, Hh, Ww), 2.0, np.float32)
    ids = np.zeros((1, Hh, Ww), np.uint8)
    T = (R + np.float32(2.0 ** -9) * ((np.arange(Hh)[:, None] + np.arange(Ww)[None, :]) % 3 - 1)).astype(np.float32)
    twists = np.zeros((1, 6, 6))
    twists[0, :3, 3:], twists[0, 3:, :3] = np.eye(3), np.eye(3)
    equations = lambda p: cref.normal_equations(R, ids, T, 1, refine_ref.HAND_INTR, twists, CLIP)[0]
    res = cref.refine(np.zeros(6), equations, range(6), iterations=1)
    assert np.isinf(res['sigma'][[0, 1, 5]]).all() and np.isfinite(res['sigma'][[2, 3, 4]]).all() and (res['sigma'][[2, 3, 4]] > 0).all()
    assert not res['pose'][[0, 1, 5]].any() and res['cost_after'] <= res['cost_before']
    part = cref.refine(np.zeros(6), equations, (0, 2), iterations=0)
    assert part['sigma'][0] == np.inf and np.isfinite(part['sigma'][2]) and np.isnan(part['sigma'][[1, 3, 4, 5]]).all()


def test_abi_is_declared_and_refuses_bad_arguments_before_a_device_is_touched():
    import ctypes as C
    import re
    from rope_s3d_amd import engine as eng
    lib = eng.load_library()
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, 'include', 'rope_s3d.h')).read()
    assert re.search(r'\bint rope_camera_normal_equations\(', hdr)
    assert 'rope_camera_normal_equations' in eng.ABI_SYMBOLS and len(lib.rope_camera_normal_equations.argtypes) == 17
    assert hasattr(eng.Engine, 'camera_normal_equations')
    buf = np.zeros(4096, np.float64)                 # host memory: a refused call reads and launches nothing
    p = C.c_void_p(buf.ctypes.data)
    odd = C.c_void_p(buf.ctypes.data + 2)
    good = dict(n=1, H=4, W=4, links=6, fx=100.0, fy=100.0, cols=6, clip=CLIP, ptrs=[p] * 6)
    cases = [dict(n=0), dict(H=0), dict(W=-1), dict(H=4097, W=4096), dict(links=0), dict(links=7), dict(cols=0), dict(cols=7),
             dict(clip=0.0), dict(clip=-1.0), dict(clip=float('nan')), dict(clip=float('inf')), dict(fx=0.0), dict(fy=float('nan'))]
    cases += [dict(ptrs=[None if i == k else p for i in range(6)]) for k in range(6)]
    cases += [dict(ptrs=[odd if i == k else p for i in range(6)]) for k in (0, 2, 3, 4, 5)]
    for case in cases:
        a = dict(good, **case)
        q = a['ptrs']
        rc = lib.rope_camera_normal_equations(q[0], q[1], q[2], a['n'], a['H'], a['W'], a['links'], a['fx'], a['fy'], 2.0, 2.0, q[3], a['cols'],
                                              a['clip'], q[4], q[5], None)
        assert rc == -1, case
    assert not buf.any()
