"""CPU: the plain-loop restatement of the native bundle polish (tests/bundle_polish_ref.py) against the host loop's own functions
(prediction/refinement.py: pool_bundle, schur_step, schur_sigma, bundle_columns_step, bundle_columns_sigma, camera_twists) on
fabricated words: per frame a random J (m x 12) and r, A = J^T J, g = J^T r, and frames built for the edges — a joint column of
zeros, two equal joint columns, all camera columns zero, a frame of all-zero words, pooled inliers below p + 1.

The bounds.  Pooling is the same additions in the same order: bit-equal.  The restatement eliminates with partial pivoting in one
order, LAPACK in another, and numpy's matrix products add in BLAS's order: two backward-stable solves of a p x p system agree to
a small multiple of p eps cond(M) (Higham, Accuracy and Stability, section 9.3: the forward error of GEPP is bounded by about
3 p^3 growth eps cond in theory and behaves like p eps cond in practice).  FACTOR = 64 is that multiple for both sides together at
p <= 12, with the growth factor of these diagonally heavy Gram blocks taken as 1: 2 sides x 12 x 2 (the products P_f = B^T X, a
sum of p terms on each side) = 48, rounded up to the next power of two.  It is a stated factor, not a measurement.
The arrow step goes through two solves in a row — X_f = D_f^-1 [B_f | g_f], then S d = -rhs with S built from the X_f — so the error
of X_f, relative eps cond(D_f), enters S and is amplified by cond(S): the bound for the step and the variances is
FACTOR eps cond(S) (1 + max_f cond(D_f)), relative to the largest entry of the host's answer.  The twelve-column solve is one
system: FACTOR eps cond(M)."""
import numpy as np
import pytest

from rope_s3d_amd.prediction import refinement as rf

import bundle_polish_ref as br

EPS = 2.0 ** -52
FACTOR = 64.0
# rope_camera_twists against refinement.camera_twists, absolute, every entry at most 1 in magnitude: numpy's vectorised sine and
# cosine may differ from libm's by 1 ulp each; an entry of R is a sum of two products of up to three of them (3 ulp + 3 roundings
# each, so 12 eps), and a twist entry is a three-term product sum of such entries with the axis (3 x 12 eps + 1 ulp of the axis'
# own terms + 3 roundings, and BLAS may fuse or reorder the sum): 64 eps covers it
TWIST_ULPS = 64


def _bits(mask, n=6):
    return [k for k in range(n) if (mask >> k) & 1]


def _cond_inf(M):
    M = np.asarray(M, np.float64)
    return 1.0 if M.size == 0 else np.linalg.norm(M, np.inf) * np.linalg.norm(np.linalg.inv(M), np.inf)


def _arrow_bound(words, jm, cm, lam):
    """FACTOR eps cond(S) (1 + max cond(D_f)) over the frames that stay in the sums, from the host's own blocks"""
    frames, kc, C, _ = rf._arrow_blocks(words, _bits(jm), _bits(cm))
    S = C + lam * np.diag(np.diag(C))
    worst = 0.0
    for idx, A, B, g in frames:
        if not idx:
            continue
        D = A + lam * np.diag(np.diag(A))
        X = rf._solve_finite(D, np.column_stack([B, g]))             # as schur_step decides whether the frame stays
        if X is None:
            continue
        worst = max(worst, _cond_inf(D))
        S = S - B.T @ X[:, :-1]
    return FACTOR * EPS * (_cond_inf(S) if kc else 1.0) * (1.0 + worst)


def _same_specials(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(a == 0, b == 0)


BATCHES = [(n, dead) for n in (1, 2, 5, 66) for dead in (False, True)]


@pytest.mark.parametrize('n, dead', BATCHES)
def test_pool_is_bit_equal(n, dead):
    words = br.fabricated_batch(n, camera_dead=dead)
    assert br.pool(words).tobytes() == rf.pool_bundle(words).tobytes()


@pytest.mark.parametrize('lam', [0.0, 1e-3])
@pytest.mark.parametrize('n, dead', BATCHES)
def test_schur_step_agrees_with_the_host_loop_up_to_the_conditioning(n, dead, lam):
    words = br.fabricated_batch(n, camera_dead=dead)
    pooled = rf.pool_bundle(words)
    rng = np.random.default_rng(n)
    q, pose = rng.uniform(-.5, .5, (n, 6)), rng.uniform(-1, 1, 6)
    wide = np.array([[-1e9, 1e9]] * 6)
    for jm, cm in br.MASKS:
        dq, dc = rf.schur_step(words, _bits(jm), _bits(cm), lam)
        t_q, t_pose = br.schur_step(words, pooled, q, pose, lam, jm, cm, wide)
        # the restatement's step: what it added, up to the rounding of the addition itself
        bound = _arrow_bound(words, jm, cm, lam)
        scale = max(np.abs(dq).max(), np.abs(dc).max(), 1e-300)
        err = max(np.abs((t_q - q) - dq).max(), np.abs((t_pose - pose) - dc).max())
        assert err <= bound * scale + 4 * EPS, (n, dead, lam, jm, cm, err, bound * scale)
        # zeros on both sides: joints and parameters that are not refined or not live, frames that leave the sums
        assert np.array_equal(dq == 0, t_q == q) and np.array_equal(dc == 0, t_pose == pose), (n, dead, lam, jm, cm)
        # and the clip is np.clip's
        c_q, c_pose = br.schur_step(words, pooled, q, pose, lam, jm, cm, br.LIMITS)
        assert np.array_equal(c_q, np.clip(t_q, br.LIMITS[:, 0], br.LIMITS[:, 1])) and np.array_equal(c_pose, t_pose)


@pytest.mark.parametrize('n, dead', BATCHES)
def test_schur_variance_agrees_with_schur_sigma_squared(n, dead):
    for inliers in (900.0, 1.0):                                    # 1 inlier a frame: pooled inliers below p + 1
        words = br.fabricated_batch(n, camera_dead=dead, inliers=inliers)
        pooled = rf.pool_bundle(words)
        for jm, cm in br.MASKS:
            sq, sc = rf.schur_sigma(words, _bits(jm), _bits(cm))
            vq, vc = br.schur_variance(words, pooled, jm, cm)
            assert _same_specials(np.isfinite(sq), np.isfinite(vq)) and _same_specials(np.isfinite(sc), np.isfinite(vc)), (n, dead, jm, cm)
            assert np.array_equal(np.isnan(sq), np.isnan(vq)) and np.array_equal(np.isnan(sc), np.isnan(vc))
            bound = _arrow_bound(words, jm, cm, 0.0)
            for host, ref in ((sq, vq), (sc, vc)):
                fin = np.isfinite(host)
                if fin.any():
                    assert np.abs(ref[fin] - host[fin] ** 2).max() <= bound * (host[fin] ** 2).max(), (n, dead, jm, cm)
            if inliers == 1.0 and (jm or cm) and n < 60:
                assert not np.isfinite(vq).any() and not np.isfinite(vc).any()


@pytest.mark.parametrize('lam', [0.0, 1e-3])
@pytest.mark.parametrize('n, dead', BATCHES)
def test_columns_step_and_variance_agree_with_the_host(n, dead, lam):
    words = br.fabricated_batch(n, camera_dead=dead)
    pooled = rf.pool_bundle(words)
    for slot_mask in (0, 0b111111111111, 0b111111000111, 0b000100000000, 0b000000000101, 0b010101101010):
        host = rf.bundle_columns_step(pooled, _bits(slot_mask, 12), lam)
        ref = np.array(br.columns_delta(pooled, slot_mask, lam))
        assert np.array_equal(host == 0, ref == 0), (n, dead, lam, slot_mask)
        if host.any():
            A, _ = rf.unpack_bundle(pooled)
            idx = [c for c in _bits(slot_mask, 12) if A[c, c] > 0]
            M = A[np.ix_(idx, idx)]
            M = M + lam * np.diag(np.diag(M))
            assert np.abs(ref - host).max() <= FACTOR * EPS * _cond_inf(M) * np.abs(host).max(), (n, dead, lam, slot_mask)
        sig = rf.bundle_columns_sigma(pooled, _bits(slot_mask, 12))
        var = br.columns_variance(pooled, slot_mask)
        assert np.array_equal(np.isnan(sig), np.isnan(var)) and np.array_equal(np.isinf(sig), np.isinf(var)), (n, dead, slot_mask)
        fin = np.isfinite(sig)
        if fin.any():
            A, _ = rf.unpack_bundle(pooled)
            idx = [c for c in _bits(slot_mask, 12) if A[c, c] > 0]
            assert np.abs(var[fin] - sig[fin] ** 2).max() <= FACTOR * EPS * _cond_inf(A[np.ix_(idx, idx)]) * (sig[fin] ** 2).max()
    # the rest of the step: pose + d[6:], off + d[:6], clip(q0 + off)
    rng = np.random.default_rng(n)
    q0, pose, off = rng.uniform(-1.5, 1.5, (n, 6)), rng.uniform(-1, 1, 6), rng.uniform(-.01, .01, 6)
    d = np.array(br.columns_delta(pooled, 4095, lam))
    t_pose, t_off, t_q = br.columns_step(pooled, lam, 4095, pose, off, q0, br.LIMITS)
    assert np.array_equal(t_pose, pose + d[6:]) and np.array_equal(t_off, off + d[:6])
    assert np.array_equal(t_q, np.clip(q0 + t_off, br.LIMITS[:, 0], br.LIMITS[:, 1])) and (t_q != q0 + t_off).any()


def test_edge_frames_do_what_their_names_say():
    rng = np.random.default_rng(8)
    edges = br.edge_frames(rng)
    full = br.fabricated_frame(rng)
    wide = np.array([[-1e9, 1e9]] * 6)
    q, pose = np.zeros((2, 6)), np.zeros(6)

    def both(words, jm, cm, lam):
        pooled = rf.pool_bundle(words)
        dq, dc = rf.schur_step(words, _bits(jm), _bits(cm), lam)
        t_q, t_pose = br.schur_step(words, pooled, q[:len(words)], pose, lam, jm, cm, wide)
        assert np.array_equal(dq == 0, t_q == 0) and np.array_equal(dc == 0, t_pose == 0)
        return t_q, t_pose

    # a joint column of zeros: joint 1 is not live, the others move
    w = np.stack([edges['joint column of zeros'], full])
    t_q, t_pose = both(w, 63, 63, 1e-3)
    assert t_q[0, 1] == 0 and t_q[0, [0, 2, 3, 4, 5]].all() and t_q[1].all() and t_pose.all()
    vq, vc = br.schur_variance(w, rf.pool_bundle(w), 63, 63)
    assert np.isposinf(vq[0, 1]) and np.isfinite(vq[0, [0, 2, 3, 4, 5]]).all() and np.isfinite(vc).all()
    # two equal joint columns: D_f is singular at lam = 0 on both sides (LAPACK raises), the frame leaves the sums — the camera
    # step is then the other frame's alone — and damping rescues it
    w = np.stack([edges['two equal joint columns'], full])
    A, _ = rf.unpack_bundle(w[0])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.solve(A[:6, :6], np.ones(6))
    t_q, t_pose = both(w, 63, 63, 0.0)
    assert not t_q[0].any() and t_q[1].all() and t_pose.all()
    alone_q, alone_pose = br.schur_step(w[1:], rf.pool_bundle(w), q[:1], pose, 0.0, 63, 63, wide)
    assert alone_q.tobytes() == t_q[1:].tobytes() and alone_pose.tobytes() == t_pose.tobytes()
    t_q, _ = both(w, 63, 63, 1e-3)
    assert t_q[0].all()
    t_q, _ = both(w, 0b101010, 63, 0.0)                              # without one of the twins the block is regular
    assert t_q[0, [1, 3, 5]].all()
    vq, _ = br.schur_variance(w, rf.pool_bundle(w), 63, 63)
    assert np.isposinf(vq[0]).all() and np.isfinite(vq[1]).all()
    # all camera columns zero in every frame: kc is empty, the pose stays, the joints move as six-column frames
    w = np.stack([edges['camera columns zero'], edges['camera columns zero']])
    t_q, t_pose = both(w, 63, 63, 1e-3)
    assert not t_pose.any() and t_q.all()
    vq, vc = br.schur_variance(w, rf.pool_bundle(w), 63, 63)
    assert np.isposinf(vc).all() and np.isfinite(vq).all()
    # a frame of all-zero words: no step, no variance, and the other frame is not disturbed
    w = np.stack([edges['all zero'], full])
    t_q, t_pose = both(w, 63, 63, 1e-3)
    assert not t_q[0].any() and t_q[1].all() and t_pose.all()
    vq, _ = br.schur_variance(w, rf.pool_bundle(w), 63, 63)
    assert np.isposinf(vq[0]).all() and np.isfinite(vq[1]).all()
    # pooled inliers below p + 1: p = 6 + 6 + 6 = 18 unknowns, 18 inliers are too few and 19 enough
    for inl, ok in ((18.0, False), (19.0, True)):
        w = np.stack([br.fabricated_frame(np.random.default_rng(1), inliers=inl - 9.0), br.fabricated_frame(np.random.default_rng(2), inliers=9.0)])
        sq, sc = rf.schur_sigma(w, list(range(6)), list(range(6)))
        vq, vc = br.schur_variance(w, rf.pool_bundle(w), 63, 63)
        assert np.isfinite(vq).all() == ok and np.isfinite(vc).all() == ok and np.isfinite(sq).all() == ok and np.isfinite(sc).all() == ok


def test_camera_twists_restate_the_host_function():
    for pose in ([.1, -1.4, .6, 0.1, 0.2, 1.5], [0, 0, 0, 0, 0, 0], [1.2, .3, -.4, -1.1, 2.9, -3.0], [.5, .5, .5, np.pi / 2, -np.pi / 2, np.pi]):
        Rwc, tc, tw = br.camera_twists(pose)
        host = rf.camera_twists(pose)
        M = rf.camera_pose_matrix(pose)
        assert np.abs(tw - host).max() <= TWIST_ULPS * EPS, np.abs(tw - host).max() / EPS
        assert np.abs(Rwc - np.diag([1.0, -1.0, -1.0]) @ M[:3, :3].T).max() <= TWIST_ULPS * EPS and np.array_equal(tc, M[:3, 3])
        assert not tw[:3, :3].any() and not tw[3:, 3:].any()


def test_library_twists_are_the_restatement_bit_for_bit():
    """rope_camera_twists is host code: the shipped library runs it here, without a GPU."""
    from rope_s3d_amd import engine as eng
    for pose in ([.1, -1.4, .6, 0.1, 0.2, 1.5], [0, 0, 0, 0, 0, 0], [1.2, .3, -.4, -1.1, 2.9, -3.0]):
        got, want = eng.camera_twists(pose), br.camera_twists(pose)
        for g, w in zip(got, want):
            assert np.array_equal(g, w) and np.array_equal(np.signbit(g), np.signbit(w))
    with pytest.raises(ValueError):
        eng.camera_twists([0, 0, 0, np.nan, 0, 0])


def test_refiner_switch_is_checked_on_the_host():
    from rope_s3d_amd.prediction.refinement import BundleRefiner
    with pytest.raises(ValueError, match='silhouette'):
        BundleRefiner(object(), None, silhouette=1.0, native=True)
    from rope_s3d_amd.prediction import camera_pose_prediction as cpp
    with pytest.raises(ValueError, match="bundle\\+native"):
        cpp._CameraStageMachine(np.zeros(6), 4, False, None, np.zeros(6), 5, '640_480_color', 0, refine='both')
