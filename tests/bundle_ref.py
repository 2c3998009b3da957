"""rope_bundle_normal_equations' contract (include/rope_s3d.h) restated in numpy float64 from the header's text, every pixel of a
frame at once, and the two loops of prediction/refinement.py's BundleRefiner ('frame': a block-arrow system solved by its Schur
complement; 'offset': one pooled 12-column system) restated over an `equations(pose, angles) -> (N, 96)` callback.  As
tests/refine_ref.py does, every sum comes with the sum of the absolute values of its terms: what a reordered float64 summation
may differ by is a multiple of it (tests/test_gpu_bundle.py).

The geometry is the header's steps 1 .. 4' written out again and not imported, so that this file can be read against the header
alone.  `variant` builds the reference WRONG on purpose in one of three ways; tests/test_bundle_refs.py shows that its checks tell
each of them from the right one."""
import numpy as np

from refine_ref import CLIP, _cross, _dot

BNEQ_WORDS = 96
SLOTS = 12
TRIU = np.triu_indices(SLOTS)


def pixel_terms(R, ids, T, n_links, intr, joints, twists, clip, variant=None):
    """One frame: R, T (H, W) float32, ids (H, W) uint8, intr (fx, fy, cx, cy) as the float32 the kernel is handed, joints
    (n_joints, 6) and twists (n_cols, 6) float64, either may be None or empty -> dict of (H, W) planes: both, cost, inlier, r,
    J (12, H, W)."""
    R, T, ids = np.asarray(R), np.asarray(T, np.float32), np.asarray(ids, np.uint8)
    H, W = R.shape
    joints = np.zeros((0, 6)) if joints is None else np.asarray(joints, np.float64).reshape(-1, 6)
    twists = np.zeros((0, 6)) if twists is None else np.asarray(twists, np.float64).reshape(-1, 6)
    n_joints, n_cols = len(joints), len(twists)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in intr)
    clip = np.float64(np.float32(clip))
    with np.errstate(all='ignore'):
        z = R.astype(np.float64)
        kx = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :] + np.zeros((H, 1))
        ky = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None] + np.zeros((1, W))
        P = np.stack([kx * z, ky * z, z])

        def diff(axis):
            """forward where the next pixel along the axis has the same id, else backward where the previous one has, else zero"""
            n = ids.shape[axis]
            at = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(2))
            same = ids[at(1, n)] == ids[at(0, n - 1)]
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
        inlier = both & normal & (np.abs(r) <= clip) & facing              # rule 4': every drawn link, the base too
        if variant == 'no_base':
            inlier = inlier & (ids >= 1)
        J = np.zeros((SLOTS, H, W))
        for j in range(n_joints):                                          # slot j: step 5
            a, o = joints[j, :3], joints[j, 3:]
            d = (P[0] - o[0], P[1] - o[1], P[2] - o[2])
            c = _cross((a[0], a[1], a[2]), d)
            J[j] = np.where(inlier & (ids > j), (z * _dot(n, c)) / nP, 0.0)
        for k in range(n_cols):                                            # slot 6 + k: step 5'
            w, v = twists[k, :3], twists[k, 3:]
            c = _cross((w[0], w[1], w[2]), P)
            u = (c[0] + v[0], c[1] + v[1], c[2] + v[2])
            J[6 + k] = np.where(inlier, (z * _dot(n, u)) / nP, 0.0)
        if variant == 'swapped':                                           # the camera in slots 0 .. 5, the joints behind it
            J = np.concatenate([J[6:], J[:6]])
    return dict(both=both, cost=cost, inlier=inlier, r=np.where(inlier, r, 0.0), J=J)


def normal_equations(R, ids, T, n_links, intr, joints, twists, clip=CLIP, variant=None):
    """N frames -> (sums (N, 96), abs_sums (N, 96)).  joints (N, n_joints, 6) or None, twists (N, n_cols, 6) or None."""
    R, ids, T = np.asarray(R), np.asarray(ids), np.asarray(T)
    N = len(R)
    joints = None if joints is None else np.asarray(joints, np.float64).reshape(N, -1, 6)
    twists = None if twists is None else np.asarray(twists, np.float64).reshape(N, -1, 6)
    out, mag = np.zeros((N, BNEQ_WORDS)), np.zeros((N, BNEQ_WORDS))
    for f in range(N):
        t = pixel_terms(R[f], ids[f], T[f], n_links, intr, None if joints is None else joints[f], None if twists is None else twists[f], clip,
                        variant)
        r, J = t['r'], t['J']
        terms = [t['both'].astype(np.float64), t['cost'], t['inlier'].astype(np.float64), r * r]
        terms += [J[c] * r for c in range(SLOTS)]
        if variant == 'transposed':                                        # the cross block written column by column
            order = [(a, b) if not (a < 6 <= b) else (b - 6, a + 6) for a in range(SLOTS) for b in range(a, SLOTS)]
        else:
            order = [(a, b) for a in range(SLOTS) for b in range(a, SLOTS)]
        terms += [J[a] * J[b] for a, b in order]
        for w, x in enumerate(terms):
            out[f, w] = x.sum()
            mag[f, w] = np.abs(x).sum()
    return out, mag


# ---------------------------------------------------------------------------------------------- the systems
def unpack(words):
    """(96,) -> (A (12, 12) symmetric, g (12,))"""
    A = np.zeros((SLOTS, SLOTS))
    A[TRIU] = words[16:94]
    return A + np.triu(A, 1).T, np.array(words[4:16], np.float64)


def pool(words):
    """(N, 96) -> (96,), added in frame order"""
    s = np.zeros(BNEQ_WORDS)
    for w in np.asarray(words, np.float64).reshape(-1, BNEQ_WORDS):
        s = s + w
    return s


def mean_cost(words):
    return words[1] / words[0] if words[0] > 0 else np.inf


def _solve(M, rhs):
    """np.linalg.solve, or None for a matrix that is singular or a solution that is not finite"""
    try:
        x = np.linalg.solve(M, rhs)
    except np.linalg.LinAlgError:
        return None
    return x if np.isfinite(x).all() else None


def arrow_blocks(words, active_j, active_c):
    """The frames' words -> (frames [(idx_f, A_f, B_f, g_f)], kc, C, gc): idx_f the active joints of frame f with a positive
    diagonal, A_f their block, B_f their rows of the joint x camera block, g_f their gradient; kc the active camera parameters
    with a positive diagonal in C = sum of the frames' camera blocks, added in frame order, and gc likewise."""
    pooled = pool(words)
    Ap, gp = unpack(pooled)
    kc = [k for k in active_c if Ap[6 + k, 6 + k] > 0]
    cc = [6 + k for k in kc]
    frames = []
    for w in words:
        A, g = unpack(w)
        idx = [j for j in active_j if A[j, j] > 0]
        frames.append((idx, A[np.ix_(idx, idx)], A[np.ix_(idx, cc)], g[idx]))
    return frames, kc, Ap[np.ix_(cc, cc)], gp[cc]


def schur_step(words, active_j, active_c, lam):
    """The Levenberg step of the block-arrow system by its Schur complement -> (dq (N, 6), dc (6,)).
    D_f = A_f + lam diag A_f;  S = C + lam diag C - sum B_f^T D_f^-1 B_f;  dc = -S^-1 (gc - sum B_f^T D_f^-1 g_f);
    dq_f = -D_f^-1 (g_f + B_f dc).  A singular D_f: a zero step for that frame's joints, and the frame leaves the sums; a singular
    S: a zero step for the camera."""
    words = np.asarray(words, np.float64).reshape(-1, BNEQ_WORDS)
    frames, kc, C, gc = arrow_blocks(words, active_j, active_c)
    N = len(words)
    dq, dc = np.zeros((N, 6)), np.zeros(6)
    S = C + lam * np.diag(np.diag(C))
    rhs = gc.copy()
    solved = []
    for idx, A, B, g in frames:
        X = _solve(A + lam * np.diag(np.diag(A)), np.column_stack([B, g])) if idx else None      # D_f^-1 [B_f, g_f]
        solved.append(X)
        if X is not None:
            S = S - B.T @ X[:, :-1]
            rhs = rhs - B.T @ X[:, -1]
    d = _solve(S, -rhs) if kc else None
    if d is None:
        d = np.zeros(len(kc))
    dc[kc] = d
    for f, ((idx, A, B, g), X) in enumerate(zip(frames, solved)):
        if X is not None:
            dq[f, idx] = -(X[:, -1] + X[:, :-1] @ d)
    return dq, dc


def schur_sigma(words, active_j, active_c):
    """Formal sigmas of the lam = 0 arrow system -> (sigma_angles (N, 6), sigma_pose (6,)): s^2 = sum [3] / (sum [2] - p), p all
    live unknowns; cov_c = S0^-1, cov_qf = A_f^-1 + A_f^-1 B_f S0^-1 B_f^T A_f^-1.  inf for an active unknown with a zero diagonal,
    for fewer inliers than p + 1 and for a singular block; nan for what is not active."""
    words = np.asarray(words, np.float64).reshape(-1, BNEQ_WORDS)
    N = len(words)
    sq, sc = np.full((N, 6), np.nan), np.full(6, np.nan)
    sq[:, list(active_j)] = np.inf
    sc[list(active_c)] = np.inf
    frames, kc, C, _ = arrow_blocks(words, active_j, active_c)
    pooled = pool(words)
    p = len(kc) + sum(len(fr[0]) for fr in frames)
    if p == 0 or pooled[2] < p + 1:
        return sq, sc
    s2 = pooled[3] / (pooled[2] - p)
    S0 = C.copy()
    solved = []
    for idx, A, B, g in frames:
        X = _solve(A, np.column_stack([B, np.eye(len(idx))])) if idx else None                   # A_f^-1 [B_f, I]
        solved.append(X)
        if X is not None:
            S0 = S0 - B.T @ X[:, :len(kc)]
    covc = _solve(S0, np.eye(len(kc))) if kc else np.zeros((0, 0))
    if covc is None:
        return sq, sc
    var = s2 * np.diag(covc)
    if np.isfinite(var).all() and (var >= 0).all():
        sc[kc] = np.sqrt(var)
    for f, ((idx, A, B, g), X) in enumerate(zip(frames, solved)):
        if X is None:
            continue
        Y, Ainv = X[:, :len(kc)], X[:, len(kc):]                                                 # A_f^-1 B_f, A_f^-1
        var = s2 * np.diag(Ainv + Y @ covc @ Y.T)
        if np.isfinite(var).all() and (var >= 0).all():
            sq[f, idx] = np.sqrt(var)
    return sq, sc


def columns_step(pooled, active, lam):
    """refine_ref.step over the twelve slots: (A + lam diag A) d = -g on the active slots with a positive diagonal -> (12,)"""
    A, g = unpack(pooled)
    idx = [c for c in active if A[c, c] > 0]
    d = np.zeros(SLOTS)
    if idx:
        S = A[np.ix_(idx, idx)]
        sol = _solve(S + lam * np.diag(np.diag(S)), -g[idx])
        if sol is not None:
            d[idx] = sol
    return d


def columns_sigma(pooled, active):
    """refine_ref.sigma over the twelve slots -> (12,)"""
    A, _ = unpack(pooled)
    out = np.full(SLOTS, np.nan)
    out[list(active)] = np.inf
    idx = [c for c in active if A[c, c] > 0]
    p = len(idx)
    if p == 0 or pooled[2] < p + 1:
        return out
    cov = _solve(A[np.ix_(idx, idx)], np.eye(p))
    if cov is None:
        return out
    var = (pooled[3] / (pooled[2] - p)) * np.diag(cov)
    if np.isfinite(var).all() and (var >= 0).all():
        out[idx] = np.sqrt(var)
    return out


# ---------------------------------------------------------------------------------------------- the loops
def refine(pose, angles, equations, limits, mode='frame', active_j=(0, 1, 2), active_c=tuple(range(6)), iterations=5, damping=1e-3):
    """equations(pose (6,), angles (N, 6)) -> (N, 96).  -> dict(pose, angles, offsets, sigma_pose, sigma_angles | sigma_offsets,
    cost_before, cost_after, steps_taken, inliers, frame_cost, costs, margins): costs (iterations + 1,) the pooled mean truncated
    cost held after each round, margins (iterations,) |trial cost - held cost| (inf where the trial was what is held)."""
    p = np.array(pose, np.float64).reshape(6)
    q0 = np.array(angles, np.float64).reshape(-1, 6)
    limits = np.asarray(limits, np.float64)
    active_j, active_c = list(active_j), list(active_c)
    q, off = q0.copy(), np.zeros(6)
    lam = float(damping)
    words = np.asarray(equations(p, q), np.float64)
    pooled = pool(words)
    cost = mean_cost(pooled)
    costs, steps, margins = [cost], 0, []
    for _ in range(iterations):
        if mode == 'frame':
            dq, dc = schur_step(words, active_j, active_c, lam)
            t_p, t_off, t_q = p + dc, off, np.clip(q + dq, limits[:, 0], limits[:, 1])
        else:
            d = columns_step(pooled, active_j + [6 + k for k in active_c], lam)
            t_p, t_off = p + d[6:], off + d[:6]
            t_q = np.clip(q0 + t_off, limits[:, 0], limits[:, 1])
        w_t = np.asarray(equations(t_p, t_q), np.float64)
        p_t = pool(w_t)
        c_t = mean_cost(p_t)
        with np.errstate(invalid='ignore'):
            margins.append(abs(c_t - cost) if (t_p != p).any() or (t_q != q).any() else np.inf)
        if c_t < cost:
            p, off, q, words, pooled, cost = t_p, t_off, t_q, w_t, p_t, c_t
            steps += 1
        else:
            lam *= 10.0
        costs.append(cost)
    out = dict(pose=p, angles=q, cost_before=costs[0], cost_after=cost, steps_taken=steps, inliers=pooled[2],
               frame_cost=np.array([mean_cost(w) for w in words]), costs=np.array(costs), margins=np.array(margins))
    if mode == 'frame':
        sq, sc = schur_sigma(words, active_j, active_c)
        out.update(offsets=np.full(6, np.nan), sigma_pose=sc, sigma_angles=sq)
    else:
        s = columns_sigma(pooled, active_j + [6 + k for k in active_c])
        out.update(offsets=np.where(np.isin(np.arange(6), active_j), off, 0.0), sigma_pose=s[6:], sigma_offsets=s[:6])
    return out
