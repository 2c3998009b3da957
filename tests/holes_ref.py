"""The depth holes' integer contract (rope_depth_holes, csrc/rope_synth.hip) restated in numpy.

Philox4x32-10 in uint64 arithmetic, the thresholds from math.erfc, one seed bit per (pixel, frame, dilation), and the morphology
through imgproc.dilate / imgproc.erode — the functions NoiseMaker.holes itself calls — on uint8 planes.

hole_mask takes NoiseMaker.holes' settings, hole_mask_raw the sizes, thresholds and window themselves (what rope_depth_holes takes);
hole_mask_loops is a second restatement from the written contract alone, in loops over seeds and pixels, for small images.  The
keyword switches of hole_mask_raw and hole_mask_loops each state the contract wrongly in one way: tests/test_holes_host.py shows for
every one a case of HOLE_EDGE_CASES that tells it from the contract, so a kernel wrong in that way fails tests/test_gpu_hole_edges.py."""
import math

import numpy as np

from rope_s3d_amd.imgproc import dilate, erode

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments
MASK = np.uint64(0xFFFFFFFF)
TILE = 64                                  # the kernel's output tile, both axes


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


def words(H: int, W: int, frame: int, seed: int, call: int):
    """The four words of generator call `call` for every pixel of frame `frame` (taken modulo 2^32) -> four (H, W) uint64 arrays."""
    i = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    return philox4x32_10(i, frame, call, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def seeds(H: int, W: int, frame: int, seed: int, T, le=False, first_call_only=False, drop_partial_call=False, carry_frame=False) -> np.ndarray:
    """-> (len(T), H, W) bool: dilation j's seed bit of pixel i = y W + x is word (j & 3) of the generator with key (seed low, seed
    high) and counter (i, frame mod 2^32, j >> 2, 0), compared as word < T[j].

    Wrong on purpose — le: word <= T[j]; first_call_only: word j & 3 of call 0 for every j; drop_partial_call: no seeds from a last
    call of fewer than four dilations; carry_frame: bit 32 of the frame index carried into the counter's third word."""
    out = np.zeros((len(T), H, W), bool)
    for call in range((len(T) + 3) // 4):
        if drop_partial_call and 4 * call + 4 > len(T):
            break
        w4 = words(H, W, frame, seed, (0 if first_call_only else call) + ((frame >> 32) if carry_frame else 0))
        for w in range(4):
            j = 4 * call + w
            if j < len(T):
                out[j] = (w4[w] <= np.uint64(T[j])) if le else (w4[w] < np.uint64(T[j]))
    return out


def _flipped(fn, img, k):
    """fn with its window mirrored: x - (k - 1 - k//2) .. x + k//2 where fn looks at x - k//2 .. x - k//2 + k - 1."""
    return fn(img[::-1, ::-1], k)[::-1, ::-1]


def _padded(fn, img, k, value):
    """fn on the image surrounded by k pixels of `value`: the outside counts as that value instead of being ignored."""
    H, W = img.shape
    p = np.full((H + 2 * k, W + 2 * k), value, img.dtype)
    p[k:k + H, k:k + W] = img
    return fn(p, k)[k:k + H, k:k + W]


def mask_of_seeds(s: np.ndarray, sizes, connection: int, mirror_d=False, mirror_k=False, erode_outside_clear=False,
                  dilate_outside_set=False) -> np.ndarray:
    """(n_d, H, W) seed bits -> (H, W) bool: close_connection(OR_j dilate_dj(seed_j)), the windows, anchors and borders of imgproc.

    Wrong on purpose — mirror_d / mirror_k: the anchor of the blocks / of the close's two windows at k - 1 - k//2 (differs for an
    even size); erode_outside_clear: the erosion counts the outside of the image as clear; dilate_outside_set: the close's dilation
    counts it as set."""
    union = np.zeros(s.shape[1:], np.uint8)
    for j, d in enumerate(sizes):
        b = s[j].astype(np.uint8)
        union |= _flipped(dilate, b, d) if mirror_d else dilate(b, d)
    k = connection
    dil = (lambda i, w: _flipped(dilate, i, w)) if mirror_k else dilate
    ero = (lambda i, w: _flipped(erode, i, w)) if mirror_k else erode
    dilated = _padded(dil, union, k, 1) if dilate_outside_set else dil(union, k)
    return (_padded(ero, dilated, k, 0) if erode_outside_clear else ero(dilated, k)) != 0


def exact_halo(sizes, connection: int):
    """-> (before, after): how far before and after a pixel, per axis, a seed can lie that decides it — 2 k//2 + max d//2 and
    2 (k - 1 - k//2) + max (d - 1 - d//2)."""
    a = connection // 2
    return (2 * a + max((d // 2 for d in sizes), default=0), 2 * (connection - 1 - a) + max((d - 1 - d // 2 for d in sizes), default=0))


def hole_mask_raw(H: int, W: int, frame: int, seed: int, sizes, T, connection: int, tile_halo=None, **wrong) -> np.ndarray:
    """-> (H, W) bool: the hole mask of frame `frame` for explicit dilation sizes, thresholds and close window.

    tile_halo = (before, after): every 64 x 64 tile is closed from the seeds of the tile and that many pixels around it alone.  The
    exact halo gives the mask itself; (0, 0) is a kernel whose tiles do not see each other.  The other switches: seeds(),
    mask_of_seeds()."""
    assert len(sizes) == len(T)
    seed_kw = {n: wrong.pop(n) for n in ('le', 'first_call_only', 'drop_partial_call', 'carry_frame') if n in wrong}
    s = seeds(H, W, frame, seed, T, **seed_kw)
    if tile_halo is None:
        return mask_of_seeds(s, sizes, connection, **wrong)
    before, after = tile_halo
    out = np.zeros((H, W), bool)
    for y0 in range(0, H, TILE):
        for x0 in range(0, W, TILE):
            near = np.zeros_like(s)
            win = np.s_[:, max(y0 - before, 0):y0 + TILE + after, max(x0 - before, 0):x0 + TILE + after]
            near[win] = s[win]
            out[y0:y0 + TILE, x0:x0 + TILE] = mask_of_seeds(near, sizes, connection, **wrong)[y0:y0 + TILE, x0:x0 + TILE]
    return out


def hole_mask(H: int, W: int, frame: int, seed: int, std=.22, thresh_factor=1, max_size=25, connection_factor=20) -> np.ndarray:
    """-> (H, W) bool: close_connection(OR_j dilate_dj(seed_j)), the windows, anchors and borders of imgproc."""
    sizes, T = thresholds(std, thresh_factor, max_size)
    return hole_mask_raw(H, W, frame, seed, sizes, T, connection_factor)


def holes_raw(depth: np.ndarray, frame: int, seed: int, sizes, T, connection: int) -> np.ndarray:
    """A copy of the (H, W) depth plane with 0 where hole_mask_raw is set; every other value as it was, bit for bit."""
    out = np.array(depth, copy=True)
    out[hole_mask_raw(depth.shape[0], depth.shape[1], frame, seed, sizes, T, connection)] = 0
    return out


def holes(depth: np.ndarray, frame: int, seed: int, **kw) -> np.ndarray:
    """A copy of the (H, W) depth plane with 0 where the frame's hole mask is set; every other value as it was."""
    out = np.array(depth, copy=True)
    out[hole_mask(depth.shape[0], depth.shape[1], frame, seed, **kw)] = 0
    return out


def hole_mask_loops(H: int, W: int, frame: int, seed: int, sizes, T, connection: int, mirror_d=False, mirror_k=False,
                    erode_outside_clear=False, dilate_outside_set=False) -> np.ndarray:
    """The same mask from the written contract alone (the header of rope_synth.hip), without imgproc: a loop over the
    seeds, each covering s - (d - 1 - d/2) .. s + d/2 per axis, then a loop over the pixels for each half of the close, the window of
    x being x - k/2 .. x - k/2 + k - 1; what lies outside the image is clear for the dilation and set for the erosion.  For images
    of some forty pixels a side.  The switches are those of mask_of_seeds."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    union = [[False] * W for _ in range(H)]
    for j in range(len(sizes)):
        d, t = sizes[j], T[j]
        lo, hi = (d // 2, d - 1 - d // 2) if mirror_d else (d - 1 - d // 2, d // 2)
        for sy in range(H):
            word = philox4x32_10(np.arange(sy * W, sy * W + W), frame % 2 ** 32, j >> 2, 0, k0, k1)[j & 3]
            for sx in range(W):
                if int(word[sx]) < t:
                    for y in range(max(sy - lo, 0), min(sy + hi, H - 1) + 1):
                        for x in range(max(sx - lo, 0), min(sx + hi, W - 1) + 1):
                            union[y][x] = True
    k = connection
    first = k - 1 - k // 2 if mirror_k else k // 2                  # the window of x is x - first .. x - first + k - 1

    def window(img, y, x, outside):
        ys, xs = range(y - first, y - first + k), range(x - first, x - first + k)
        inside = img[max(ys[0], 0):ys[-1] + 1, max(xs[0], 0):xs[-1] + 1]
        cut = inside.size < k * k                                   # part of the window lies outside the image
        return inside, cut and outside

    u = np.array(union, bool).reshape(H, W)
    dilated, out = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            inside, outside_set = window(u, y, x, dilate_outside_set)
            dilated[y, x] = bool(inside.any()) or outside_set
    for y in range(H):
        for x in range(W):
            inside, outside_clear = window(dilated, y, x, erode_outside_clear)
            out[y, x] = bool(inside.all()) and not outside_clear
    return out


# ---- the cases tests/test_gpu_hole_edges.py runs on the GPU; tests/test_holes_host.py shows on the reference alone what each is for

SEED = 0x9E3779B97F4A7C15


def T_of(*p):
    """Seed probabilities -> thresholds floor(p 2^32)."""
    return [min(math.floor(q * 2.0 ** 32), 0xFFFFFFFF) for q in p]


def T_count(H: int, W: int, *c):
    """Expected seed counts in an H x W image -> thresholds."""
    return T_of(*[x / (H * W) for x in c])


def _cases():
    """name -> (n, H, W, frame0, seed, sizes, T, connection).  Every frame index was searched upward from 0 on the reference alone
    until the case met what tests/test_holes_host.py asserts of it; it is a constant here."""
    c = {}
    p36 = T_of(2e-3, 1e-3)
    # the close window at its ends: at 32 every plane in LDS is used to its last row and column
    for k in (1, 2, 3, 31, 32):
        c[f'130x70, close window {k}'] = (1, 70, 130, 0, SEED, [3, 6], p36, k)
    c['70x130, close window 32'] = (1, 130, 70, 0, SEED, [3, 6], p36, 32)
    # one dilation at the ends of its range
    for d, p, frame in ((1, 5e-3, 42), (2, 5e-3, 2), (31, 3e-4, 0), (32, 3e-4, 0)):
        c[f'130x70, one dilation of {d}'] = (1, 70, 130, frame, SEED, [d], T_of(p), 5)
    c['70x130, one dilation of 32'] = (1, 130, 70, 1, SEED, [32], T_of(3e-4), 5)
    # the number of dilations: none, whole generator calls (4, 12, 16) and calls cut short (5, 9, 13)
    c['no dilations'] = (1, 70, 130, 0, SEED, [], [], 20)
    order = [7, 2, 12, 1, 5, 32, 3, 9, 4, 16, 6, 31, 8, 10, 14, 11]
    for n_d, k, frame in ((4, 4, 1), (5, 3, 1), (9, 20, 0), (12, 5, 1), (13, 32, 20), (16, 2, 1)):
        sizes = order[:n_d]
        c[f'200x120, {n_d} dilations'] = (1, 120, 200, frame, SEED, sizes, T_count(120, 200, *[5 if d <= 4 else 4 if d <= 12 else 2 for d in sizes]), k)
    # thresholds at their ends, and one that is a pixel's own word: 2600538 is the seventh smallest word 0 of frame 0 at 130 x 70
    c['threshold 0'] = (1, 70, 130, 0, SEED, [3, 6], [0, 0], 20)
    c['threshold 0xFFFFFFFF'] = (1, 70, 130, 0, SEED, [1], [0xFFFFFFFF], 1)
    c['threshold 0 beside a live one'] = (1, 70, 130, 0, SEED, [6, 3], [0] + T_of(2e-3), 3)
    c['threshold equal to a word'] = (1, 70, 130, 0, SEED, [1], [2600538], 1)
    # where the image ends relative to a tile, with all windows at 32 and with small ones
    for (H, W), f32, f3 in (((63, 63), 0, 0), ((64, 64), 0, 0), ((65, 65), 0, 3), ((70, 129), 0, 0), ((129, 70), 0, 0), ((64, 128), 0, 0),
                            ((127, 65), 0, 0), ((1, 200), 7, 0), ((200, 1), 7, 0), ((31, 33), 71, 0)):
        c[f'{W}x{H}, windows of 32'] = (1, H, W, f32, SEED, [32, 5], T_count(H, W, 1.2, 5), 32)
        c[f'{W}x{H}, small windows'] = (1, H, W, f3, SEED, [2, 9], T_count(H, W, 6, 2), 3)
    c['7x5, small windows'] = (1, 5, 7, 57, SEED, [2, 9], T_count(5, 7, 2, 1), 3)
    c['1x1'] = (3, 1, 1, 0, SEED, [1], [2 ** 31], 1)
    c['1x1, windows of 32'] = (3, 1, 1, 0, SEED, [32], [2 ** 31], 32)
    # the frame counter through 2^32 inside one launch
    c['three frames from 0xFFFFFFFE'] = (3, 70, 130, 0xFFFFFFFE, SEED, [3, 6], p36, 7)
    # seeds in the halo's outermost column or row decide pixels of the tile: one pixel less before / after changes these masks
    c['70x130, halo before'] = (1, 130, 70, 2, SEED, [3], T_of(2e-3), 2)
    c['130x70, halo before and after'] = (1, 70, 130, 1, SEED, [3], T_of(2e-2), 2)
    return c


HOLE_EDGE_CASES = _cases()
# what a case is for beyond its name, asserted on the reference by tests/test_holes_host.py: holes on all four borders; a hole across
# column 64 / row 64; the three kinds whose masks are not both set and clear; thresholds no single dilation can be taken out of
HOLE_CASE_NEEDS = {
    '130x70, close window 31': ('borders', 'cross_x', 'cross_y'), '130x70, close window 32': ('borders', 'cross_x', 'cross_y'),
    '70x130, close window 32': ('borders', 'cross_x', 'cross_y'),
    '130x70, one dilation of 31': ('cross_x',), '130x70, one dilation of 32': ('cross_x',), '70x130, one dilation of 32': ('cross_y',),
    **{f'200x120, {n_d} dilations': ('cross_x', 'cross_y') for n_d in (4, 5, 9, 12, 13, 16)},
    'no dilations': ('nothing',), 'threshold 0': ('nothing',), 'threshold 0xFFFFFFFF': ('everything',),
    'threshold 0 beside a live one': ('extreme',),
}
