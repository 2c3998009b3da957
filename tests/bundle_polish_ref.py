"""The contracts of csrc/rope_bundle_polish.hip (include/rope_s3d.h: rope_camera_twists, rope_bundle_pool, rope_bundle_schur_step,
rope_bundle_schur_variance, rope_bundle_columns_step, rope_bundle_columns_variance, rope_refine_bundle) restated with plain loops
over Python floats — every float64 operation ONE IEEE operation in the order the header writes it, no numpy arithmetic and no
np.linalg — so that the kernels can be held to it bit for bit.  numpy only carries the arrays."""
import math

import numpy as np

INF, NAN = float('inf'), float('nan')
WORDS = 96


def tri12(i: int, j: int) -> int:
    """word of A[i][j], i <= j, among the 96"""
    return 16 + 12 * i - (i * (i - 1)) // 2 + (j - i)


def entry(w, i: int, j: int) -> float:
    return float(w[tri12(i, j) if i <= j else tri12(j, i)])


def live(w, mask: int, first: int, count: int) -> list:
    """the slots first + k, bit k of mask set, with a positive diagonal in w"""
    return [first + k for k in range(count) if (mask >> k) & 1 and float(w[tri12(first + k, first + k)]) > 0.0]


def eliminate(M, B):
    """THE ELIMINATION with several right-hand sides: M p x p, B p x m (lists of lists), in place -> X (p x m) or None when
    singular.  The pivot row is the FIRST row r >= k with the largest |M[r][k]|; every row operation goes over all right-hand sides."""
    p = len(M)
    m = len(B[0]) if p else 0
    for k in range(p):
        piv, best = k, abs(M[k][k])
        for r in range(k + 1, p):
            if abs(M[r][k]) > best:
                piv, best = r, abs(M[r][k])
        pv = M[piv][k]
        if pv == 0.0 or not math.isfinite(pv):
            return None
        if piv != k:
            M[k], M[piv] = M[piv], M[k]
            B[k], B[piv] = B[piv], B[k]
        for i in range(k + 1, p):
            f = M[i][k] / pv
            for c in range(k + 1, p):
                M[i][c] = M[i][c] - f * M[k][c]
            for c in range(m):
                B[i][c] = B[i][c] - f * B[k][c]
    X = [[0.0] * m for _ in range(p)]
    for c in range(m):
        for i in range(p - 1, -1, -1):
            s = B[i][c]
            for j in range(i + 1, p):
                s = s - M[i][j] * X[j][c]
            X[i][c] = s / M[i][i]
    return X


def finite(X) -> bool:
    return all(math.isfinite(v) for row in X for v in row)


def first_sum(terms) -> float:
    """a sum from the first product: t_0, then + t_1 ...; 0.0 when empty"""
    s = 0.0
    for k, t in enumerate(terms):
        s = t if k == 0 else s + t
    return s


def clip(v: float, lo: float, hi: float) -> float:
    v = lo if v < lo else v
    return hi if v > hi else v


def block(w, idx, lam):
    M = [[entry(w, a, b) for b in idx] for a in idx]
    if lam is not None:
        for k in range(len(idx)):
            M[k][k] = M[k][k] + float(lam) * M[k][k]
    return M


# ---------------------------------------------------------------------------------------------- the twists
def camera_twists(pose6):
    """rope_camera_twists -> (Rwc (3, 3), tc (3,), twists (6, 6))"""
    x, y, z, a3, a4, a5 = (float(v) for v in pose6)
    yaw, pitch, roll = a5, a3, a4 + 3.141592653589793 / 2
    c0, c1, c2 = math.cos(yaw), math.cos(pitch), math.cos(roll)
    s0, s1, s2 = math.sin(yaw), math.sin(pitch), math.sin(roll)
    R = [[c0 * c1, c0 * s1 * s2 - c2 * s0, s0 * s2 + c0 * c2 * s1],
         [c1 * s0, c0 * c2 + (s0 * s1) * s2, c2 * s0 * s1 - c0 * s2],
         [-1 * s1, c1 * s2, c1 * c2]]
    Rwc = [[R[j][i] if i == 0 else -R[j][i] for j in range(3)] for i in range(3)]
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    axis = [[-sy, cy, 0.0], [cy * cp, sy * cp, -sp], [0.0, 0.0, 1.0]]
    tw = [[0.0] * 6 for _ in range(6)]
    for k in range(3):
        for r in range(3):
            tw[k][3 + r] = -Rwc[r][k]
    for k in range(3):
        for r in range(3):
            tw[3 + k][r] = -((Rwc[r][0] * axis[k][0] + Rwc[r][1] * axis[k][1]) + Rwc[r][2] * axis[k][2])
    return np.array(Rwc), np.array([x, y, z]), np.array(tw)


# ---------------------------------------------------------------------------------------------- the pool
def pool(words) -> np.ndarray:
    words = np.asarray(words, np.float64).reshape(-1, WORDS)
    out = np.empty(WORDS)
    for k in range(WORDS):
        s = 0.0
        for w in words:
            s = s + float(w[k])
        out[k] = s
    return out


# ---------------------------------------------------------------------------------------------- the arrow system
def _frame_share(w, idx, kc, lam, identity: bool):
    """-> (X or None, P): X = D^-1 [B | g] (step) or A^-1 [B | I] (variance); P[a][b] = sum_r B[r][a] X[r][b]"""
    if not idx:
        return None, None
    p, nk = len(idx), len(kc)
    rhs = [[entry(w, j, c) for c in kc] + ([1.0 if r == k else 0.0 for k in range(p)] if identity else [float(w[4 + j])])
           for r, j in enumerate(idx)]
    X = eliminate(block(w, idx, None if identity else lam), rhs)
    if X is None or not finite(X):
        return None, None
    cols = nk if identity else nk + 1
    P = [[first_sum(entry(w, idx[r], kc[a]) * X[r][b] for r in range(p)) for b in range(cols)] for a in range(nk)]
    return X, P


def schur_step(words, pooled, q, pose, lam, joint_mask: int, camera_mask: int, limits):
    """rope_bundle_schur_step -> (trial_q (N, 6), trial_pose (6,))"""
    words, q = np.asarray(words, np.float64).reshape(-1, WORDS), np.asarray(q, np.float64).reshape(-1, 6)
    lam = float(lam)
    kc = live(pooled, camera_mask, 6, 6)
    nk = len(kc)
    S = [[entry(pooled, a, b) for b in kc] for a in kc]
    for a in range(nk):
        S[a][a] = S[a][a] + lam * S[a][a]
    rhs = [float(pooled[4 + c]) for c in kc]
    shares = []
    for w in words:
        idx = live(w, joint_mask, 0, 6)
        X, P = _frame_share(w, idx, kc, lam, False)
        shares.append((idx, X))
        if X is not None:
            for a in range(nk):
                for b in range(nk):
                    S[a][b] = S[a][b] - P[a][b]
                rhs[a] = rhs[a] - P[a][nk]
    d = [0.0] * nk
    if nk:
        x = eliminate(S, [[-v] for v in rhs])
        if x is not None and finite(x):
            d = [row[0] for row in x]
    dc = [0.0] * 6
    for a, c in enumerate(kc):
        dc[c - 6] = d[a]
    trial = np.empty((len(words), 6))
    for f, (idx, X) in enumerate(shares):
        dq = [0.0] * 6
        if X is not None:
            for r, j in enumerate(idx):
                dq[j] = -(X[r][nk] + first_sum(X[r][a] * d[a] for a in range(nk)))
        for j in range(6):
            trial[f, j] = clip(float(q[f, j]) + dq[j], float(limits[j][0]), float(limits[j][1]))
    return trial, np.array([float(pose[k]) + dc[k] for k in range(6)])


def schur_variance(words, pooled, joint_mask: int, camera_mask: int):
    """rope_bundle_schur_variance -> (var_q (N, 6), var_pose (6,))"""
    words = np.asarray(words, np.float64).reshape(-1, WORDS)
    var_q = np.array([[INF if (joint_mask >> j) & 1 else NAN for j in range(6)] for _ in words]).reshape(-1, 6)
    var_c = np.array([INF if (camera_mask >> k) & 1 else NAN for k in range(6)])
    kc = live(pooled, camera_mask, 6, 6)
    nk = len(kc)
    idxs = [live(w, joint_mask, 0, 6) for w in words]
    p = nk + sum(len(i) for i in idxs)
    if p == 0 or float(pooled[2]) < float(p + 1):
        return var_q, var_c
    s2 = float(pooled[3]) / (float(pooled[2]) - float(p))
    S0 = [[entry(pooled, a, b) for b in kc] for a in kc]
    shares = []
    for w, idx in zip(words, idxs):
        X, P = _frame_share(w, idx, kc, None, True)
        shares.append(X)
        if X is not None:
            for a in range(nk):
                for b in range(nk):
                    S0[a][b] = S0[a][b] - P[a][b]
    cov = []
    if nk:
        cov = eliminate(S0, [[1.0 if a == b else 0.0 for b in range(nk)] for a in range(nk)])
        if cov is None or not finite(cov):
            return var_q, var_c
    vc = [s2 * cov[a][a] for a in range(nk)]
    if all(math.isfinite(v) and v >= 0.0 for v in vc):
        for a, c in enumerate(kc):
            var_c[c - 6] = vc[a]
    for f, (idx, X) in enumerate(zip(idxs, shares)):
        if X is None:
            continue
        vq = []
        for r in range(len(idx)):
            t = [first_sum(cov[a][b] * X[r][b] for b in range(nk)) for a in range(nk)]
            u = first_sum(X[r][a] * t[a] for a in range(nk))
            vq.append(s2 * (X[r][nk + r] + u))
        if all(math.isfinite(v) and v >= 0.0 for v in vq):
            for r, j in enumerate(idx):
                var_q[f, j] = vq[r]
    return var_q, var_c


# ---------------------------------------------------------------------------------------------- the pooled twelve columns
def columns_delta(pooled, slot_mask: int, lam) -> list:
    idx = live(pooled, slot_mask, 0, 12)
    d = [0.0] * 12
    if idx:
        x = eliminate(block(pooled, idx, lam), [[-float(pooled[4 + c])] for c in idx])
        if x is not None and finite(x):
            for k, c in enumerate(idx):
                d[c] = x[k][0]
    return d


def columns_step(pooled, lam, slot_mask: int, pose, off, q0, limits):
    """rope_bundle_columns_step -> (trial_pose (6,), trial_off (6,), trial_q (N, 6))"""
    q0 = np.asarray(q0, np.float64).reshape(-1, 6)
    d = columns_delta(pooled, slot_mask, lam)
    t_pose = np.array([float(pose[k]) + d[6 + k] for k in range(6)])
    t_off = np.array([float(off[j]) + d[j] for j in range(6)])
    trial = np.empty((len(q0), 6))
    for f in range(len(q0)):
        for j in range(6):
            trial[f, j] = clip(float(q0[f, j]) + float(t_off[j]), float(limits[j][0]), float(limits[j][1]))
    return t_pose, t_off, trial


def columns_variance(pooled, slot_mask: int) -> np.ndarray:
    out = np.array([INF if (slot_mask >> c) & 1 else NAN for c in range(12)])
    idx = live(pooled, slot_mask, 0, 12)
    p = len(idx)
    if p == 0 or float(pooled[2]) < float(p + 1):
        return out
    s2 = float(pooled[3]) / (float(pooled[2]) - float(p))
    X = eliminate(block(pooled, idx, None), [[1.0 if a == b else 0.0 for b in range(p)] for a in range(p)])
    if X is None or not finite(X):
        return out
    var = [s2 * X[k][k] for k in range(p)]
    if all(math.isfinite(v) and v >= 0.0 for v in var):
        for k, c in enumerate(idx):
            out[c] = var[k]
    return out


# ---------------------------------------------------------------------------------------------- the loop
def pooled_cost(p) -> float:
    return float(p[1]) / float(p[0]) if float(p[0]) > 0.0 else INF


def refine(mode: str, pose, q, equations, step, variance, iterations: int, damping: float) -> dict:
    """rope_refine_bundle's loop.  equations(pose (6,), angles (N, 6)) -> (words (N, 96), pooled (96,)); step(words, pooled, q, q0,
    pose, off, lam) -> (trial_pose, trial_off, trial_q); variance(words, pooled) -> (var_pose (6,), var_joints): the caller's (a
    test hands in the engine's own exports, or the restatements above)."""
    pose, q = np.array(pose, np.float64).reshape(6), np.array(q, np.float64).reshape(-1, 6)
    q0, off, lam = q.copy(), np.zeros(6), float(damping)
    words, pooled = equations(pose, q)
    cost = pooled_cost(pooled)
    cost_before, steps, costs, ties = cost, 0, [cost], []
    for it in range(iterations):
        t_pose, t_off, t_q = step(words, pooled, q, q0, pose, off, lam)
        w_t, p_t = equations(t_pose, t_q)
        c_t = pooled_cost(p_t)
        costs.append(c_t)
        if c_t < cost:
            pose, off, q, words, pooled, cost = t_pose, t_off, t_q, w_t, p_t, c_t
            steps += 1
        else:
            if c_t == cost:
                ties.append((it, cost))
            lam = lam * 10.0
    var_pose, var_joints = variance(words, pooled)
    return dict(pose=pose, angles=q, offsets=off if mode == 'offset' else np.full(6, NAN), var_pose=var_pose, var_joints=var_joints,
                costs=np.array([cost_before, cost, float(pooled[2])]), steps=steps, words=words, trial_costs=costs, ties=ties,
                frame_cost=np.array([pooled_cost(w) for w in words]))


# ---------------------------------------------------------------------------------------------- fabricated words
def words_of(A, g, n_both=4000.0, cost_sum=2.0, inliers=900.0, rss=0.5) -> np.ndarray:
    """A (12, 12) symmetric, g (12,) -> one frame's 96 words"""
    w = np.zeros(WORDS)
    w[0], w[1], w[2], w[3] = n_both, cost_sum, inliers, rss
    w[4:16] = g
    w[16:94] = np.asarray(A, np.float64)[np.triu_indices(12)]
    return w


def fabricated_frame(rng, m: int = 40, zero_cols=(), equal_cols=None, **kw) -> np.ndarray:
    """A = J^T J, g = J^T r from a random J (m x 12) and r; zero_cols: columns of J set to 0 (a slot that is not live); equal_cols
    (a, b): column b a copy of column a (an exactly singular block)."""
    J = rng.normal(size=(m, 12))
    for c in zero_cols:
        J[:, c] = 0.0
    if equal_cols is not None:
        J[:, equal_cols[1]] = J[:, equal_cols[0]]
    r = rng.normal(size=m) * 0.01
    A = J.T @ J
    if equal_cols is not None:                          # the products of equal columns, made equal bit for bit
        a, b = equal_cols
        A[b, :], A[:, b] = A[a, :], A[:, a]
        A[b, b] = A[a, a]
    g = J.T @ r
    if equal_cols is not None:
        g[equal_cols[1]] = g[equal_cols[0]]
    return words_of((A + A.T) / 2.0 if equal_cols is None else A, g, **kw)


def edge_frames(rng) -> dict:
    """The frames built for the edges -> {name: words (96,)}"""
    return {
        'joint column of zeros': fabricated_frame(rng, zero_cols=(1,)),
        'two equal joint columns': fabricated_frame(rng, equal_cols=(0, 2)),
        'camera columns zero': fabricated_frame(rng, zero_cols=tuple(range(6, 12))),
        'all zero': np.zeros(WORDS),
    }


def fabricated_batch(n: int, seed: int = 3, camera_dead: bool = False, inliers: float = 900.0) -> np.ndarray:
    """n frames; the edge frames stand at 0, 63, 64 and n - 1 where the batch reaches them.  camera_dead: every frame's camera
    columns are zero, so kc is empty."""
    rng = np.random.default_rng(seed)
    zero = tuple(range(6, 12)) if camera_dead else ()
    words = np.stack([fabricated_frame(rng, zero_cols=zero, inliers=inliers) for _ in range(n)])
    edges = edge_frames(rng)
    for at, name in ((0, 'joint column of zeros'), (63, 'two equal joint columns'), (64, 'all zero'), (n - 1, 'camera columns zero')):
        if 0 <= at < n and (n > 1 or name == 'joint column of zeros'):
            w = edges[name].copy()
            if camera_dead:
                w[[4 + c for c in range(6, 12)]] = 0.0
                A = np.zeros((12, 12))
                A[np.triu_indices(12)] = w[16:94]
                A[:, 6:] = 0.0
                w[16:94] = A[np.triu_indices(12)]
            w[2] = 0.0 if name == 'all zero' else inliers
            words[at] = w
    return words


LIMITS = np.array([[-1.0, 1.0], [-0.9, 1.1], [-1.2, 0.8], [-2.0, 2.0], [-1.5, 1.5], [-3.0, 3.0]])
MASKS = ((0b111111, 0b111111), (0b000111, 0b111111), (0, 0b111111), (0b000111, 0b000100), (0b111111, 0), (0b101010, 0b010101))
