"""Plain restatements for the dataset verification (rope_frame_agreement, data/verification.py), in numpy with int64 and float64:
the 28 sums per frame, cv2.addWeighted on bytes, and the IQR outlier rule of the reference (robotpose/utils.py:68-80)."""
import numpy as np

WORDS = 28
LAST_BELOW_128 = np.float32(128.0) - np.float32(2.0 ** -17)


def q(x) -> np.ndarray:
    """floor(x 2^32) as int64: exact in float64 for a float32 below 128 (at most 24 significant bits below 2^39)."""
    return np.floor(np.asarray(x, np.float32).astype(np.float64) * 4294967296.0).astype(np.int64)


def frame_sums(render_depth, render_ids, frame_depth, n_links: int, tol) -> np.ndarray:
    """(N, H, W) float32, uint8, float32 -> (N, 28) uint64.  A render depth outside [0, 128) counts as the nearer end, NaN as 0
    (include/rope_s3d.h); the renderer writes none."""
    R, I, T = np.asarray(render_depth, np.float32), np.asarray(render_ids, np.uint8), np.asarray(frame_depth, np.float32)
    assert R.shape == I.shape == T.shape and R.ndim == 3
    tq = int(np.floor(float(np.float32(tol)) * 4294967296.0))
    out = np.zeros((len(R), WORDS), np.uint64)
    for i in range(len(R)):
        with np.errstate(invalid='ignore'):
            valid = np.isfinite(T[i]) & (T[i] > 0) & (T[i] < 128)
            r = np.clip(np.where(np.isnan(R[i]), np.float32(0), R[i]), np.float32(0), LAST_BELOW_128)
        rendered = I[i] < n_links
        both = rendered & valid
        d = q(r) - q(np.where(valid, T[i], np.float32(0)))            # q(R) - q(T); only read where T is valid
        close = both & (np.abs(d) <= tq)
        front = both & (d > tq)                                       # q(T) < q(R) - q(tol)
        words = [valid.sum(), rendered.sum(), np.abs(d)[both].sum(), ((I[i] >= n_links) & (I[i] < 255)).sum()]
        for l in range(n_links):
            m = I[i] == l
            words += [m.sum(), (m & both).sum(), (m & close).sum(), (m & front).sum()]
        out[i, :len(words)] = np.array([int(w) for w in words], np.uint64)
    return out


def add_weighted(a, alpha, b, beta, gamma=0.0) -> np.ndarray:
    """cv2.addWeighted for uint8: float32 arithmetic, round half to even, saturate."""
    x = np.asarray(a, np.uint8).astype(np.float32) * np.float32(alpha) + np.asarray(b, np.uint8).astype(np.float32) * np.float32(beta) \
        + np.float32(gamma)
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def iqr_upper_fence(data, iqr_mult=1.5) -> float:
    """The upper bound of reject_outliers_iqr (utils.py:72-75)."""
    percentiles = np.percentile(data, [75, 25])
    iqr = np.subtract(*percentiles)
    return float(percentiles[0] + iqr_mult * iqr)


def flagged(sums, n_links: int):
    """Frames with nothing both rendered and valid under a render, or with [2] / both / 2^32 above the fence of the scored
    frames.  -> (indices, the per-frame mean in metres with NaN where both == 0)."""
    s = np.asarray(sums, np.uint64).astype(np.int64)
    both = s[:, 5:4 + 4 * n_links:4].sum(axis=1)
    rendered = s[:, 1]
    m = np.array([s[i, 2] / both[i] / 4294967296.0 if both[i] else np.nan for i in range(len(s))])
    scored = both > 0
    fence = iqr_upper_fence(m[scored]) if scored.any() else np.inf
    return np.array([i for i in range(len(s)) if (rendered[i] > 0 and not scored[i]) or (scored[i] and m[i] > fence)], np.int64), m


# The end-to-end case of tests/test_gpu_verify.py, checked on CPU renders first (tests/test_verify_refs.py): a synthetic set whose
# frames SHIFTED have their recorded L angle moved by SHIFT_RAD after rendering.
E2E_FRAMES, E2E_SEED, E2E_SHIFTED, E2E_SHIFT_RAD = 24, 5300, (3, 11, 20), 0.3


def e2e_angles(limits) -> tuple:
    """(true, recorded) joint angles of the set: make_synthetic_dataset's poses ('SLU' drawn uniformly in the limits from
    default_rng(seed + f)), and the same with the shift."""
    mask = np.array([1, 1, 1, 0, 0, 0.0])
    true = np.stack([np.random.default_rng(E2E_SEED + f).uniform(limits[:, 0], limits[:, 1]) * mask for f in range(E2E_FRAMES)])
    recorded = true.copy()
    recorded[list(E2E_SHIFTED), 1] += E2E_SHIFT_RAD
    return true, recorded


# ---- the hand-made case: every kind of pixel at once, the expected words written out by hand
U = 2.0 ** -32                                   # one unit of q
TOL = 2.0 ** -5                                  # q(TOL) = 2^27
A = np.float32(2.0 ** -5 + 2.0 ** -28)           # q(A) = 2^27 + 16
NAN, INF = np.nan, np.inf


def hand_planes():
    """3 x 4 planes, n_links = 2, every case at once.  Pixel by pixel (R, id, T):
       0  background, T valid                          -> valid
       1  id 5: no link, not the background            -> valid, word 3
       2  link 0, T = 0          3  link 0, T < 0      -> rendered only
       4  link 1, T NaN          5  link 1, T inf      6  link 1, T = 128   -> rendered only
       7  link 0, q(R) - q(T) = 2^27      = q(tol)     -> both, close
       8  link 0, q(R) - q(T) = 2^27 + 1  (T = 15.5 units: floor, not round)   -> both, front
       9  link 1, q(R) - q(T) = -2^27                  -> both, close
      10  link 1, q(R) - q(T) = -(2^27 + 1)            -> both, behind (neither close nor front)
      11  link 0, q(R) - q(T) = 2^27 - 1               -> both, close"""
    R = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, A, A, 16 * U, 15 * U, A], np.float32).reshape(1, 3, 4)
    ids = np.array([255, 5, 0, 0, 1, 1, 1, 0, 0, 1, 1, 0], np.uint8).reshape(1, 3, 4)
    T = np.array([1.0, 1.0, 0.0, -1.0, NAN, INF, 128.0, 16 * U, 15.5 * U, A, A, 17 * U], np.float32).reshape(1, 3, 4)
    return R, ids, T


HAND_WORDS = [7, 10, 5 * 2 ** 27 + 1, 1,
              5, 3, 2, 1,                        # link 0: rendered 2 3 7 8 11, both 7 8 11, close 7 11, front 8
              5, 2, 1, 0] + [0] * 16             # link 1: rendered 4 5 6 9 10, both 9 10, close 9
