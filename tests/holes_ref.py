"""The depth holes' integer contract (rope_depth_holes, csrc/rope_synth.hip) restated in numpy.

Philox4x32-10 in uint64 arithmetic, the thresholds from math.erfc, one seed bit per (pixel, frame, dilation), and the morphology
through imgproc.dilate / imgproc.erode — the functions NoiseMaker.holes itself calls — on uint8 planes."""
import math

import numpy as np

from rope_s3d_amd.imgproc import dilate, erode

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Counter words (arrays or scalars) and a key -> the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                  # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def thresholds(std=.22, thresh_factor=1, max_size=25):
    """-> (dilation sizes, T = floor(P(|N(0, std)| >= 1 - thresh_factor / d) * 2^32) per size, as Python ints)."""
    sizes = [int(d) for d in np.arange(3, max_size, 3)]
    T = []
    for d in sizes:
        thresh = 1 - thresh_factor / d
        T.append(min(math.floor(math.erfc(thresh / (std * math.sqrt(2))) * 2.0 ** 32), 0xFFFFFFFF))
    return sizes, T


def seeds(H: int, W: int, frame: int, seed: int, T) -> np.ndarray:
    """-> (len(T), H, W) bool: dilation j's seed bit of pixel i = y W + x is word (j & 3) of the generator with key (seed low, seed
    high) and counter (i, frame, j >> 2, 0), compared as word < T[j]."""
    i = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    out = np.zeros((len(T), H, W), bool)
    for call in range((len(T) + 3) // 4):
        words = philox4x32_10(i, frame, call, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        for w in range(4):
            j = 4 * call + w
            if j < len(T):
                out[j] = words[w] < np.uint64(T[j])
    return out


def hole_mask(H: int, W: int, frame: int, seed: int, std=.22, thresh_factor=1, max_size=25, connection_factor=20) -> np.ndarray:
    """-> (H, W) bool: close_connection(OR_j dilate_dj(seed_j)), the windows, anchors and borders of imgproc."""
    sizes, T = thresholds(std, thresh_factor, max_size)
    s = seeds(H, W, frame, seed, T)
    union = np.zeros((H, W), np.uint8)
    for j, d in enumerate(sizes):
        union |= dilate(s[j].astype(np.uint8), d)
    return erode(dilate(union, connection_factor), connection_factor) != 0


def holes(depth: np.ndarray, frame: int, seed: int, **kw) -> np.ndarray:
    """A copy of the (H, W) depth plane with 0 where the frame's hole mask is set; every other value as it was."""
    out = np.array(depth, copy=True)
    out[hole_mask(depth.shape[0], depth.shape[1], frame, seed, **kw)] = 0
    return out
