"""The contracts of csrc/rope_polish.hip (include/rope_s3d.h: rope_joint_axes, rope_levenberg_step, rope_formal_variance,
rope_refine_poses) restated with plain loops over Python floats — every float64 operation ONE IEEE operation in the order the
header writes it, no numpy arithmetic and no np.linalg — so that the kernels can be held to it bit for bit.  numpy only carries
the arrays.  The joint axes take oracle.sincos (the device's det_sincos, bit for bit) and aff_mul's operation order."""
import math

import numpy as np

from oracle import oracle as orc

INF, NAN = float('inf'), float('nan')


def tri_word(i: int, j: int) -> int:
    """word of A[i][j], i <= j, among a frame's 32"""
    return 10 + 6 * i - (i * (i - 1)) // 2 + (j - i)


def entry(w, i: int, j: int) -> float:
    return float(w[tri_word(i, j) if i <= j else tri_word(j, i)])


def live_joints(w, active_mask: int) -> list:
    return [j for j in range(6) if (active_mask >> j) & 1 and float(w[tri_word(j, j)]) > 0.0]


def eliminate(M, b):
    """Gaussian elimination with partial pivoting and back substitution, in place on the lists M (p x p) and b (p) -> x, or None for
    a pivot that is 0 or not finite.  The pivot row is the FIRST row r >= k with the largest |M[r][k]|."""
    p = len(b)
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
            b[k], b[piv] = b[piv], b[k]
        for i in range(k + 1, p):
            f = M[i][k] / pv
            for c in range(k + 1, p):
                M[i][c] = M[i][c] - f * M[k][c]
            b[i] = b[i] - f * b[k]
    x = [0.0] * p
    for i in range(p - 1, -1, -1):
        s = b[i]
        for c in range(i + 1, p):
            s = s - M[i][c] * x[c]
        x[i] = s / M[i][i]
    return x


def damped_block(w, idx, lam):
    """M = A[idx][idx], the diagonal A_kk + lam A_kk (lam None: undamped)"""
    M = [[entry(w, a, b) for b in idx] for a in idx]
    if lam is not None:
        for k in range(len(idx)):
            M[k][k] = M[k][k] + float(lam) * M[k][k]
    return M


def step_delta(w, active_mask: int, lam: float) -> list:
    """rope_levenberg_step's d before the clip: six floats"""
    idx = live_joints(w, active_mask)
    d = [0.0] * 6
    if not idx:
        return d
    x = eliminate(damped_block(w, idx, lam), [-float(w[4 + j]) for j in idx])
    if x is None or not all(math.isfinite(v) for v in x):
        return d
    for k, j in enumerate(idx):
        d[j] = x[k]
    return d


def clip(v: float, lo: float, hi: float) -> float:
    v = lo if v < lo else v
    return hi if v > hi else v


def levenberg_step(words, q, lam, active_mask: int, limits) -> np.ndarray:
    """(N, 32), (N, 6), (N,), limits (6, 2) -> trial (N, 6)"""
    words, q = np.asarray(words, np.float64).reshape(-1, 32), np.asarray(q, np.float64).reshape(-1, 6)
    out = np.empty((len(words), 6))
    for f, w in enumerate(words):
        d = step_delta(w, active_mask, float(lam[f]))
        for j in range(6):
            out[f, j] = clip(float(q[f, j]) + d[j], float(limits[j][0]), float(limits[j][1]))
    return out


def formal_variance(words, active_mask: int) -> np.ndarray:
    """(N, 32) -> (N, 6): rope_formal_variance"""
    words = np.asarray(words, np.float64).reshape(-1, 32)
    out = np.empty((len(words), 6))
    for f, w in enumerate(words):
        row = [INF if (active_mask >> j) & 1 else NAN for j in range(6)]
        idx = live_joints(w, active_mask)
        p = len(idx)
        var = []
        if p > 0 and not float(w[2]) < float(p + 1):
            s2 = float(w[3]) / (float(w[2]) - float(p))
            for k in range(p):
                x = eliminate(damped_block(w, idx, None), [1.0 if r == k else 0.0 for r in range(p)])
                if x is None:
                    break
                v = s2 * x[k]
                if not (math.isfinite(v) and v >= 0.0):
                    break
                var.append(v)
            if len(var) == p:
                for k, j in enumerate(idx):
                    row[j] = var[k]
        out[f] = row
    return out


# ---------------------------------------------------------------------------------------------- the axes
def dot3(u, v) -> float:
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def aff_mul(A, B) -> list:
    O = [0.0] * 12
    for r in range(3):
        for c in range(3):
            O[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]
        O[4 * r + 3] = ((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3]
    return O


def joint_matrix(q: float, j: int, joint_fixed, joint_axes, sincos) -> list:
    s, co = sincos(q)
    t = 1.0 - co
    ax, ay, az = (float(v) for v in joint_axes[j])
    R = [(t * ax) * ax + co, (t * ax) * ay - s * az, (t * ax) * az + s * ay, 0.0,
         (t * ax) * ay + s * az, (t * ay) * ay + co, (t * ay) * az - s * ax, 0.0,
         (t * ax) * az - s * ay, (t * ay) * az + s * ax, (t * az) * az + co, 0.0]
    return aff_mul([float(v) for v in np.asarray(joint_fixed[j]).reshape(12)], R)


def libm_sincos(x: float):
    return math.sin(x), math.cos(x)


def joint_axes(q, joint_fixed, joint_axes_, Rwc, tc, sincos=orc.sincos) -> np.ndarray:
    """rope_joint_axes: (N, 6) angles -> (N, 6, 6).  joint_fixed (6, 3, 4) or (6, 12), joint_axes_ (6, 3): the robot's, as
    rope_set_robot takes them; Rwc (3, 3), tc (3,).  sincos: oracle.sincos is the device's; libm_sincos the host mirror's."""
    q = np.asarray(q, np.float64).reshape(-1, 6)
    Rwc = [[float(v) for v in row] for row in np.asarray(Rwc, np.float64).reshape(3, 3)]
    tc = [float(v) for v in np.asarray(tc, np.float64).reshape(3)]
    out = np.empty((len(q), 6, 6))
    for f in range(len(q)):
        T = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        for j in range(6):
            T = aff_mul(T, joint_matrix(float(q[f, j]), j, joint_fixed, joint_axes_, sincos))
            a = [float(v) for v in joint_axes_[j]]
            a_w = [dot3(T[4 * r:4 * r + 3], a) for r in range(3)]
            o = [T[3] - tc[0], T[7] - tc[1], T[11] - tc[2]]
            for r in range(3):
                out[f, j, r] = dot3(Rwc[r], a_w)
                out[f, j, 3 + r] = dot3(Rwc[r], o)
    return out


def camera_axes(pose6):
    """rope_refine_poses' camera: [x, y, z, a3, a4, a5] -> (Rwc (3, 3), tc (3,)): rope_camera_matrix's camera-to-world rotation R
    (libm's sin and cos, one operation per step), Rwc = diag(1, -1, -1) R^T taken as row 0 of R^T and the NEGATED rows 1 and 2."""
    x, y, z, a3, a4, a5 = (float(v) for v in pose6)
    yaw, pitch, roll = a5, a3, a4 + 3.141592653589793 / 2
    c0, c1, c2 = math.cos(yaw), math.cos(pitch), math.cos(roll)
    s0, s1, s2 = math.sin(yaw), math.sin(pitch), math.sin(roll)
    R = [[c0 * c1, c0 * s1 * s2 - c2 * s0, s0 * s2 + c0 * c2 * s1],
         [c1 * s0, c0 * c2 + (s0 * s1) * s2, c2 * s0 * s1 - c0 * s2],
         [-1 * s1, c1 * s2, c1 * c2]]
    Rwc = np.array([[R[j][i] if i == 0 else -R[j][i] for j in range(3)] for i in range(3)])
    return Rwc, np.array([x, y, z])


# ---------------------------------------------------------------------------------------------- the loop
def mean_cost(w) -> float:
    return float(w[1]) / float(w[0]) if float(w[0]) > 0.0 else INF


def refine(q, equations, active_mask: int, limits, iterations: int, damping: float) -> dict:
    """rope_refine_poses' loop.  equations(angles (N, 6)) -> (N, 32): render and normal equations at those angles, the caller's
    (a test hands in the engine's own render and kernel with the axes of joint_axes above)."""
    q = np.array(q, np.float64).reshape(-1, 6)
    N = len(q)
    lam = [float(damping)] * N
    words = np.array(equations(q), np.float64)
    cost = [mean_cost(w) for w in words]
    cost_before, steps = list(cost), [0] * N
    ties = []                                       # (round, frame, cost held, trial's cost) where the two were equal
    for it in range(iterations):
        trial = levenberg_step(words, q, lam, active_mask, limits)
        w_t = np.array(equations(trial), np.float64)
        for f in range(N):
            c_t = mean_cost(w_t[f])
            if c_t < cost[f]:
                q[f], words[f], cost[f] = trial[f], w_t[f], c_t
                steps[f] += 1
            else:
                if c_t == cost[f]:
                    ties.append((it, f, cost[f], c_t))
                lam[f] = lam[f] * 10.0
    return dict(angles=q, var=formal_variance(words, active_mask), cost_before=np.array(cost_before), cost_after=np.array(cost),
                steps=np.array(steps, np.int32), inliers=words[:, 2].copy(), words=words, ties=ties)


# ---------------------------------------------------------------------------------------------- a table of systems
def words_of(A, g, n_both=1000.0, cost_sum=1.0, inliers=500.0, rss=0.25) -> np.ndarray:
    """A (6, 6) symmetric, g (6,) -> one frame's 32 words"""
    A = np.asarray(A, np.float64)
    w = np.zeros(32)
    w[0], w[1], w[2], w[3] = n_both, cost_sum, inliers, rss
    w[4:10] = g
    w[10:31] = A[np.triu_indices(6)]
    return w


def embed(block, joints, g_block) -> tuple:
    A, g = np.zeros((6, 6)), np.zeros(6)
    A[np.ix_(joints, joints)] = block
    g[list(joints)] = g_block
    return A, g


def system_table() -> list:
    """-> [(name, words (32,), lam, q (6,))]: the systems tests/test_polish_refs.py and tests/test_gpu_polish.py share.  cond <= 1e8
    for every block that is not singular on purpose."""
    rng = np.random.default_rng(5)
    table = []
    q0 = np.array([0.1, -0.2, 0.3, 0.05, -0.1, 0.2])
    for p in range(7):                                                          # p live joints: a random SPD block on the first p
        B = rng.normal(size=(max(p, 1) + 3, max(p, 1)))
        blk = (B.T @ B)[:p, :p] * 1e4
        A, g = embed(blk, range(p), rng.normal(size=p) * 10.0)
        table.append((f'spd p={p}', words_of(A, g), 1e-3, q0))
    # an active joint with a zero diagonal: joint 1 carries nothing, 0 and 2 do
    A, g = embed([[4e4, 1e3], [1e3, 9e4]], (0, 2), [30.0, -20.0])
    table.append(('zero diagonal', words_of(A, g), 1e-3, q0))
    # row swaps: at k = 0 ([[1,2],[2,5]]: |2| > |1|), and at k > 0 (the 3 x 3 below keeps row 0 and swaps rows 1, 2)
    A, g = embed([[1.0, 2.0], [2.0, 5.0]], (0, 1), [1.0, -1.0])
    table.append(('swap at k=0', words_of(A, g), 0.0, q0))
    A, g = embed([[4.0, 2.0, 1.0], [2.0, 1.5, 2.0], [1.0, 2.0, 9.0]], (0, 1, 2), [1.0, 2.0, -1.0])
    table.append(('swap at k=1', words_of(A, g), 0.0, q0))
    # exactly singular: two equal columns (and rows); lam = 0 and lam = 1e-3
    A, g = embed([[2.0, 2.0, 1.0], [2.0, 2.0, 1.0], [1.0, 1.0, 3.0]], (0, 1, 2), [1.0, 1.0, 0.5])
    table.append(('singular lam=0', words_of(A, g), 0.0, q0))
    table.append(('singular lam=1e-3', words_of(A, g), 1e-3, q0))
    # a step that leaves the limits at each end (the limits of LIMITS below are about +-1 rad: d is +-50)
    A, g = embed([[1.0, 0.0], [0.0, 1.0]], (0, 1), [-50.0, 50.0])
    table.append(('beyond the limits', words_of(A, g), 0.0, q0))
    # [2] = p and [2] = p + 1
    A, g = embed([[4e4, 1e3], [1e3, 9e4]], (0, 1), [3.0, -2.0])
    table.append(('inliers = p', words_of(A, g, inliers=2.0), 1e-3, q0))
    table.append(('inliers = p + 1', words_of(A, g, inliers=3.0), 1e-3, q0))
    # nothing to compare at all
    table.append(('empty', np.zeros(32), 1e-3, q0))
    return table


LIMITS = np.array([[-1.0, 1.0], [-0.9, 1.1], [-1.2, 0.8], [-2.0, 2.0], [-1.5, 1.5], [-3.0, 3.0]])
MASKS = (0, 1, 0b000111, 0b111111)
