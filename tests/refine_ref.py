"""rope_pose_normal_equations' contract (include/rope_s3d.h) restated in numpy float64 from the header's text, every pixel of a
frame at once, and the refinement loop of prediction/refinement.py restated over a `render(angles)` callback.  Beside every sum
the reference returns the sum of the absolute values of its terms: what a reordered float64 summation may differ by is bounded by
a multiple of it (tests/test_gpu_refine.py)."""
import numpy as np

NEQ_WORDS = 32
CLIP = 2.0 ** -5


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def pixel_terms(R, ids, T, n_links, intr, joints, clip):
    """One frame: R, T (H, W) float32, ids (H, W) uint8, intr (fx, fy, cx, cy) as the float32 the kernel is handed, joints
    (n_joints, 6) float64 -> dict of (H, W) planes: both, cost (min(r^2, clip^2) on both), inlier, r, J (6, H, W), normal."""
    R, T, ids = np.asarray(R), np.asarray(T, np.float32), np.asarray(ids, np.uint8)       # R: float32 as rendered (float64 is taken as it is)
    H, W = R.shape
    joints = np.asarray(joints, np.float64).reshape(-1, 6)
    n_joints = len(joints)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in intr)
    clip = np.float64(np.float32(clip))
    with np.errstate(all='ignore'):
        z = R.astype(np.float64)
        kx = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :] + np.zeros((H, 1))
        ky = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None] + np.zeros((1, W))
        P = np.stack([kx * z, ky * z, z])

        def diff(axis):
            """forward difference, backward where the forward neighbour has another id or lies off the image, zero where both do"""
            n = ids.shape[axis]
            sl = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(2))
            same = ids[sl(1, n)] == ids[sl(0, n - 1)]                    # pixel i and i + 1 along the axis
            fwd_ok = np.zeros(ids.shape, bool)
            bwd_ok = np.zeros(ids.shape, bool)
            fwd_ok[sl(0, n - 1)] = same
            bwd_ok[sl(1, n)] = same
            d = np.zeros_like(P)
            f = np.zeros_like(P)
            b = np.zeros_like(P)
            psl = lambda a, b_: (slice(None),) + sl(a, b_)
            f[psl(0, n - 1)] = P[psl(1, n)] - P[psl(0, n - 1)]
            b[psl(1, n)] = P[psl(1, n)] - P[psl(0, n - 1)]
            d = np.where(fwd_ok[None], f, np.where(bwd_ok[None], b, 0.0))
            return d

        dX, dY = diff(1), diff(0)
        n = np.stack(_cross(dX, dY))
        normal = np.isfinite(n).all(axis=0) & ~((n == 0).all(axis=0))
        rendered = ids < n_links
        valid = np.isfinite(T) & (T > np.float32(0)) & (T < np.float32(128))
        both = rendered & valid
        r = z - T.astype(np.float64)
        r2 = r * r
        cost = np.where(both, np.where(r2 <= clip * clip, r2, clip * clip), 0.0)
        moving = (ids >= 1) & (ids <= n_joints)
        nn, nP, PP = _dot(n, n), _dot(n, P), _dot(P, P)
        facing = (nP * nP >= 0.01 * (nn * PP)) & (nP != 0)
        inlier = both & moving & normal & (np.abs(r) <= clip) & facing
        J = np.zeros((6, H, W))
        for j in range(n_joints):
            a, o = joints[j, :3], joints[j, 3:]
            d = (P[0] - o[0], P[1] - o[1], P[2] - o[2])
            c = _cross((a[0], a[1], a[2]), d)
            Jj = (z * _dot(n, c)) / nP
            J[j] = np.where(inlier & (ids > j), Jj, 0.0)
    return dict(both=both, cost=cost, inlier=inlier, r=np.where(inlier, r, 0.0), J=J, normal=normal)


def normal_equations(R, ids, T, n_links, intr, joints, clip=CLIP):
    """N frames -> (sums (N, 32), abs_sums (N, 32)): the words of the header, and for every word the sum of the absolute values of
    its terms (for the counts: the counts)."""
    R, ids, T = np.asarray(R), np.asarray(ids), np.asarray(T)
    N = len(R)
    joints = np.asarray(joints, np.float64).reshape(N, -1, 6)
    out, mag = np.zeros((N, NEQ_WORDS)), np.zeros((N, NEQ_WORDS))
    for f in range(N):
        t = pixel_terms(R[f], ids[f], T[f], n_links, intr, joints[f], clip)
        r, J = t['r'], t['J']
        terms = [t['both'].astype(np.float64), t['cost'], t['inlier'].astype(np.float64), r * r]
        terms += [J[j] * r for j in range(6)]
        terms += [J[j] * J[i] for j in range(6) for i in range(j, 6)]
        for w, x in enumerate(terms):
            out[f, w] = x.sum()
            mag[f, w] = np.abs(x).sum()
    return out, mag


# ---------------------------------------------------------------------------------------------- the loop
def unpack(words):
    """(32,) -> (A (6, 6) symmetric, g (6,))"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = words[10:31]
    A = A + np.triu(A, 1).T
    return A, words[4:10].copy()


def mean_cost(words):
    return words[1] / words[0] if words[0] > 0 else np.inf


def step(words, active, lam):
    """The Levenberg step (A + lam diag A) d = -g on the active joints whose diagonal entry is positive -> (6,), zero elsewhere and
    zero when the system cannot be solved."""
    A, g = unpack(words)
    idx = [j for j in active if A[j, j] > 0]
    d = np.zeros(6)
    if idx:
        S = A[np.ix_(idx, idx)]
        try:
            sol = np.linalg.solve(S + lam * np.diag(np.diag(S)), -g[idx])
        except np.linalg.LinAlgError:
            return d
        if np.isfinite(sol).all():
            d[idx] = sol
    return d


def sigma(words, active):
    """sqrt(s^2 diag(A^-1)), s^2 = [3] / ([2] - p) over the p active joints with a positive diagonal; inf for an active joint with a
    zero diagonal, for fewer inliers than p + 1 and for a singular A; nan for the joints that are not active."""
    A, _ = unpack(words)
    out = np.full(6, np.nan)
    out[list(active)] = np.inf
    idx = [j for j in active if A[j, j] > 0]
    p = len(idx)
    if p == 0 or words[2] < p + 1:
        return out
    try:
        cov = np.linalg.inv(A[np.ix_(idx, idx)])
    except np.linalg.LinAlgError:
        return out
    var = (words[3] / (words[2] - p)) * np.diag(cov)
    if np.isfinite(var).all() and (var >= 0).all():
        out[idx] = np.sqrt(var)
    return out


def refine(angles, equations, limits, active=(0, 1, 2), iterations=5, damping=1e-3):
    """The loop.  equations(angles (N, 6)) -> (N, 32): render at the angles, joint axes there, the normal equations against the
    frames.  -> dict(angles, sigma, cost_before, cost_after, steps_taken, inliers, costs, margins): costs (iterations + 1, N) is the
    mean truncated cost of the pose every frame holds after each round, margins (iterations, N) |trial cost - held cost| of every
    decision (inf where the trial was the held pose itself)."""
    q = np.array(angles, np.float64).reshape(-1, 6)
    N = len(q)
    limits = np.asarray(limits, np.float64)
    lam = np.full(N, float(damping))
    words = np.asarray(equations(q), np.float64)
    cost = np.array([mean_cost(w) for w in words])
    costs, steps, margins = [cost.copy()], np.zeros(N, np.int64), []
    for _ in range(iterations):
        trial = np.stack([np.clip(q[f] + step(words[f], active, lam[f]), limits[:, 0], limits[:, 1]) for f in range(N)])
        w_t = np.asarray(equations(trial), np.float64)
        c_t = np.array([mean_cost(w) for w in w_t])
        ok = c_t < cost
        with np.errstate(invalid='ignore'):
            margins.append(np.where((trial != q).any(axis=1), np.abs(c_t - cost), np.inf))      # how far the decision was from a tie
        q[ok], words[ok], cost[ok] = trial[ok], w_t[ok], c_t[ok]
        steps += ok
        lam[~ok] *= 10.0
        costs.append(cost.copy())
    return dict(angles=q, sigma=np.stack([sigma(w, active) for w in words]), cost_before=costs[0], cost_after=cost, steps_taken=steps,
                inliers=words[:, 2].copy(), costs=np.stack(costs), margins=np.stack(margins) if margins else np.zeros((0, N)))


def joint_axes_camera(link_poses, axes, camera_to_world):
    """Joint axes and points in the camera axes of the kernel (x right, y down, z forward): link_poses (7, 4, 4) world poses of the
    links (ForwardKinematics.calc), axes (6, 3) unit axes in their links' frames, camera_to_world the 4 x 4 pose of the GL camera
    (looks along -z, y up).  -> (6, 6): axis, point."""
    M = np.asarray(camera_to_world, np.float64)
    Rc, tc = M[:3, :3], M[:3, 3]
    flip = np.diag([1.0, -1.0, -1.0])
    out = np.zeros((6, 6))
    for j in range(6):
        Tl = link_poses[j + 1]
        out[j, :3] = flip @ (Rc.T @ (Tl[:3, :3] @ axes[j]))
        out[j, 3:] = flip @ (Rc.T @ (Tl[:3, 3] - tc))
    return out


# ---------------------------------------------------------------------------------------------- hand-built planes
HAND_INTR = (150.0, 150.0, 11.25, 9.75)        # float32 holds all four
HAND_LINKS, HAND_JOINTS = 4, 2                 # ids 0 .. 3 are links, joints 0 and 1 move links 1 and 2; link 3 is rendered and moves with none
HAND_H, HAND_W = 20, 23                        # the width is no multiple of anything
BAD_T = (0.0, np.nan, np.inf, 128.0, -1.0)
HAND_FLAT_WORDS = {0: 409.0, 1: 2.0 ** -8, 2: 361.0, 3: 2.0 ** -9}       # frame 1, worked by hand (hand_planes)


def tilted_depth(H, W, intr, n, c):
    """Depth of the plane n . X = c along the rays of the pixels, float64."""
    fx, fy, cx, cy = intr
    kx = (np.arange(W, dtype=np.float64) - cx) / fx
    ky = (np.arange(H, dtype=np.float64) - cy) / fy
    return c / (n[0] * kx[None, :] + n[1] * ky[:, None] + n[2])


def hand_planes():
    """-> (R, ids, T (3, 20, 23), joints (3, 2, 6)).
    Frame 0: a tilted plane, link 1 on the left and link 2 on the right, T = R + 2^-8 on the even columns; an ISLAND pixel (5, 5) of
      link 2 inside link 1 (no neighbour of its id: no normal).
    Frame 1: the plane z = 2 (exact in float32).  Row 0 link 0, row 1 link 3 (rendered, moved by no joint), row 2 id 4 (no link),
      row 3 background, rows 4 .. 19 link 1.  T = R but for row 10, columns 0 .. 4: BAD_T, and row 12: column 0 T = 2 - 2^-5 and
      column 4 T = 2 + 2^-5 (|r| = clip: inside), column 2 T = 2 - 2^-5 - 2^-22 and column 6 T = 2 + 2^-5 + 2^-22 (outside).  By hand:
      rendered 18 rows x 23 = 414, both 409; moving and both 16 x 23 - 5 = 363, inliers 361; [1] = 4 clip^2 = 2^-8, [3] = 2 clip^2.
    Frame 2: z = 2 on link 1 with a step to z = 3 at (8, 9): (8, 8) looks along the step's face (GRAZING); rows 16 .. 19
      background; T = 0 in rows 0 .. 2."""
    H, W = HAND_H, HAND_W
    R = np.full((3, H, W), 2.0, np.float32)
    ids = np.full((3, H, W), 1, np.uint8)
    n = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    R[0] = tilted_depth(H, W, HAND_INTR, n, 1.9).astype(np.float32)
    ids[0, :, W // 2:] = 2
    ids[0, 5, 5] = 2
    T = R.copy()
    T[0, :, ::2] += np.float32(2.0 ** -8)
    ids[1, 0], ids[1, 1], ids[1, 2], ids[1, 3] = 0, 3, 4, 255
    T[1, 10, :5] = np.array(BAD_T, np.float32)
    T[1, 12, [0, 2, 4, 6]] = np.array([2 - 2.0 ** -5, 2 - 2.0 ** -5 - 2.0 ** -22, 2 + 2.0 ** -5, 2 + 2.0 ** -5 + 2.0 ** -22], np.float32)
    R[2, 8, 9] = T[2, 8, 9] = 3.0
    ids[2, 16:] = 255
    T[2, :3] = 0.0
    joints = np.zeros((3, 2, 6))
    joints[:, 0] = [0.0, 1.0, 0.0, 0.1, 0.3, 2.5]              # a vertical axis behind the planes
    a1 = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    joints[:, 1] = [a1[0], a1[1], a1[2], -0.2, 0.1, 2.2]
    return R, ids, T, joints


def equations_of(render, T, n_links, intr, axes_of, clip=CLIP):
    """The loop's `equations` from a render(angles (N, 6)) -> (depth (N, H, W) float32, ids (N, H, W) uint8) callback, the frames T
    and axes_of(angles) -> (N, n_joints, 6)."""
    def equations(q):
        R, ids = render(q)
        return normal_equations(np.asarray(R), np.asarray(ids), T, n_links, intr, axes_of(q), clip)[0]
    return equations
