"""rope_camera_normal_equations' contract (include/rope_s3d.h) restated in numpy float64 from the header's text, every pixel of a
frame at once, and the pooled refinement loop of prediction/refinement.py (CameraPoseRefiner) restated over an
`equations(pose) -> (N, 32)` callback.  As tests/refine_ref.py does, every sum comes with the sum of the absolute values of its
terms: what a reordered float64 summation may differ by is a multiple of it (tests/test_gpu_camera_refine.py).

The geometry (points, differences, normal, the gates) is the header's steps 1 .. 4 written out again here and not imported, so that
this file can be read against the header alone; the hand planes, the constants and the loop's step, sigma and cost are
refine_ref's."""
import numpy as np

import refine_ref
from refine_ref import CLIP, NEQ_WORDS, _cross, _dot


def pixel_terms(R, ids, T, n_links, intr, twists, clip):
    """One frame: R, T (H, W) float32, ids (H, W) uint8, intr (fx, fy, cx, cy) as the float32 the kernel is handed, twists
    (n_cols, 6) float64 (w, v) -> dict of (H, W) planes: both, cost, inlier, r, J (6, H, W), normal."""
    R, T, ids = np.asarray(R), np.asarray(T, np.float32), np.asarray(ids, np.uint8)
    H, W = R.shape
    twists = np.asarray(twists, np.float64).reshape(-1, 6)
    n_cols = len(twists)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in intr)
    clip = np.float64(np.float32(clip))
    with np.errstate(all='ignore'):
        z = R.astype(np.float64)
        kx = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :] + np.zeros((H, 1))
        ky = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None] + np.zeros((1, W))
        P = np.stack([kx * z, ky * z, z])

        def diff(axis):
            """forward difference where the next pixel along the axis has the same id, else backward where the previous one has,
            else zero"""
            n = ids.shape[axis]
            at = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(2))
            same = ids[at(1, n)] == ids[at(0, n - 1)]                    # pixel i and i + 1 along the axis
            step = P[(slice(None),) + at(1, n)] - P[(slice(None),) + at(0, n - 1)]
            fwd_ok, bwd_ok = np.zeros(ids.shape, bool), np.zeros(ids.shape, bool)
            fwd_ok[at(0, n - 1)] = same
            bwd_ok[at(1, n)] = same
            f, b = np.zeros_like(P), np.zeros_like(P)
            f[(slice(None),) + at(0, n - 1)] = step
            b[(slice(None),) + at(1, n)] = step
            return np.where(fwd_ok[None], f, np.where(bwd_ok[None], b, 0.0))

        dX, dY = diff(1), diff(0)
        n = np.stack(_cross(dX, dY))
        normal = np.isfinite(n).all(axis=0) & ~((n == 0).all(axis=0))
        both = (ids < n_links) & np.isfinite(T) & (T > np.float32(0)) & (T < np.float32(128))
        r = z - T.astype(np.float64)
        r2 = r * r
        cost = np.where(both, np.where(r2 <= clip * clip, r2, clip * clip), 0.0)
        nn, nP, PP = _dot(n, n), _dot(n, P), _dot(P, P)
        facing = (nP * nP >= 0.01 * (nn * PP)) & (nP != 0)
        inlier = both & normal & (np.abs(r) <= clip) & facing              # MOVING is RENDERED here: every drawn link, link 0 too
        J = np.zeros((6, H, W))
        for k in range(n_cols):
            w, v = twists[k, :3], twists[k, 3:]
            c = _cross((w[0], w[1], w[2]), P)
            u = (c[0] + v[0], c[1] + v[1], c[2] + v[2])
            J[k] = np.where(inlier, (z * _dot(n, u)) / nP, 0.0)
    return dict(both=both, cost=cost, inlier=inlier, r=np.where(inlier, r, 0.0), J=J, normal=normal)


def normal_equations(R, ids, T, n_links, intr, twists, clip=CLIP):
    """N frames -> (sums (N, 32), abs_sums (N, 32)): the words of the header and, for every word, the sum of the absolute values
    of its terms (for the counts: the counts)."""
    R, ids, T = np.asarray(R), np.asarray(ids), np.asarray(T)
    N = len(R)
    twists = np.asarray(twists, np.float64).reshape(N, -1, 6)
    out, mag = np.zeros((N, NEQ_WORDS)), np.zeros((N, NEQ_WORDS))
    for f in range(N):
        t = pixel_terms(R[f], ids[f], T[f], n_links, intr, twists[f], clip)
        r, J = t['r'], t['J']
        terms = [t['both'].astype(np.float64), t['cost'], t['inlier'].astype(np.float64), r * r]
        terms += [J[j] * r for j in range(6)]
        terms += [J[j] * J[i] for j in range(6) for i in range(j, 6)]
        for w, x in enumerate(terms):
            out[f, w] = x.sum()
            mag[f, w] = np.abs(x).sum()
    return out, mag


# ---------------------------------------------------------------------------------------------- twists and the loop
def Rwc_t(pose, camera_pose_matrix):
    """X_c = Rwc (X_w - t) in the kernel's axes (x right, y down, z forward) for the GL camera pose matrix of `pose`."""
    M = camera_pose_matrix(pose)
    return np.diag([1.0, -1.0, -1.0]) @ M[:3, :3].T, M[:3, 3].copy()


def pool(words):
    """(N, 32) -> (32,), added in frame order"""
    s = np.zeros(NEQ_WORDS)
    for w in np.asarray(words, np.float64):
        s = s + w
    return s


def refine(pose, equations, active=tuple(range(6)), iterations=5, damping=1e-3):
    """The pooled loop.  equations(pose (6,)) -> (N, 32): render every frame under the pose, the twists there, the normal equations
    against the frames.  -> dict(pose, sigma, cost_before, cost_after, steps_taken, inliers, frame_cost, costs, margins): costs
    (iterations + 1,) the pooled mean truncated cost held after each round, margins (iterations,) |trial cost - held cost| of every
    decision (inf where the trial was the held pose itself)."""
    p = np.array(pose, np.float64).reshape(6)
    active = list(active)
    lam = float(damping)
    words = np.asarray(equations(p), np.float64)
    pooled = pool(words)
    cost = refine_ref.mean_cost(pooled)
    costs, steps, margins = [cost], 0, []
    for _ in range(iterations):
        trial = p + refine_ref.step(pooled, active, lam)
        w_t = np.asarray(equations(trial), np.float64)
        p_t = pool(w_t)
        c_t = refine_ref.mean_cost(p_t)
        with np.errstate(invalid='ignore'):
            margins.append(abs(c_t - cost) if (trial != p).any() else np.inf)
        if c_t < cost:
            p, words, pooled, cost = trial, w_t, p_t, c_t
            steps += 1
        else:
            lam *= 10.0
        costs.append(cost)
    return dict(pose=p, sigma=refine_ref.sigma(pooled, active), cost_before=costs[0], cost_after=cost, steps_taken=steps,
                inliers=pooled[2], frame_cost=np.array([refine_ref.mean_cost(w) for w in words]), costs=np.array(costs),
                margins=np.array(margins))


# ---------------------------------------------------------------------------------------------- renderer-free scenes
def plane_depth(H, W, intr, Rwc, t, planes):
    """World planes n_w . X_w = c_w (rows of `planes`: n_w (3), c_w) seen from the camera (Rwc, t): per pixel the nearest positive
    depth along its ray, in closed form — n_c = Rwc n_w, d_c = c_w - n_w . t, z = d_c / (n_c . k), k = (kx, ky, 1) — and the index
    of the plane that gives it (255 where none does).  float64."""
    fx, fy, cx, cy = intr
    kx = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :] + np.zeros((H, 1))
    ky = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None] + np.zeros((1, W))
    best, which = np.full((H, W), np.inf), np.full((H, W), 255, np.uint8)
    for i, pl in enumerate(np.asarray(planes, np.float64).reshape(-1, 4)):
        nc = Rwc @ pl[:3]
        with np.errstate(all='ignore'):
            z = (pl[3] - pl[:3] @ t) / (nc[0] * kx + nc[1] * ky + nc[2])
        take = np.isfinite(z) & (z > 0) & (z < best)
        best[take], which[take] = z[take], i
    return np.where(which < 255, best, 0.0), which


def flat_frame():
    """z = 2 (exact in float32) on 20 x 23: rows 0 .. 5 link 0, rows 6 .. 9 background, rows 10 .. 19 link 1.  T = R but for
    (2, 3): 2 - 2^-6 (r = 2^-6, link 0), (12, 5): 2 + 2^-7 (r = -2^-7), (15, 1): 2 + 2^-4 (beyond the clip) and (3, 7): 0 (no
    measurement).  Columns: two pure translations along the optical axis, v = (0, 0, 1) and v = (0, 0, -1/2).  On z = 2 the normal
    is (0, 0, n.z) exactly, n.P = 2 n.z and z (n . v) = 2 n.z v.z, both exact: J_0 = 1 and J_1 = -1/2 on every inlier.  By hand:
    rendered 16 x 23 = 368, both 367, inliers 366; [1] = 2^-12 + 2^-14 + 2^-10; [3] = 2^-12 + 2^-14; [4] = 2^-6 - 2^-7 = 2^-7;
    [5] = -2^-8; [10] = 366; [11] = -183; [16] = 91.5; every other word 0."""
    Hh, Ww = refine_ref.HAND_H, refine_ref.HAND_W
    R = np.full((1, Hh, Ww), 2.0, np.float32)
    ids = np.full((1, Hh, Ww), 1, np.uint8)
    ids[0, :6], ids[0, 6:10] = 0, 255
    T = R.copy()
    T[0, 2, 3], T[0, 12, 5], T[0, 15, 1], T[0, 3, 7] = 2 - 2.0 ** -6, 2 + 2.0 ** -7, 2 + 2.0 ** -4, 0.0
    twists = np.zeros((1, 2, 6))
    twists[0, 0, 5], twists[0, 1, 5] = 1.0, -0.5
    words = np.zeros(32)
    words[[0, 1, 2, 3, 4, 5, 10, 11, 16]] = [367, 2.0 ** -12 + 2.0 ** -14 + 2.0 ** -10, 366, 2.0 ** -12 + 2.0 ** -14, 2.0 ** -7, -2.0 ** -8,
                                            366, -183, 91.5]
    return R, ids, T, twists, words
