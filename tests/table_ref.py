"""The stored lookup table (rope_table.hip: crop_total / table_count / table_fill / table_score / table_score_frames;
rope_kernels.hip: argmin_sets / finalize for ROPE_LOSS_LOOKUP) restated plainly, and the inputs the GPU tests feed those kernels.

The reference is dense and exact: no compaction, no "total minus what the groups change" — every sample of the unpadded crop is
converted and summed as Python integers, and the float64 epilogue is mean_std_parts' written order in Python floats (IEEE
doubles, one rounding per written step).  tests/test_table_refs.py holds it to the oracle's bits on rendered rows and asserts
that every builder below reaches the edge it is named for; tests/test_gpu_table_kernels.py holds the kernels to it."""
import functools
import math

import numpy as np

MASK64 = (1 << 64) - 1
Q32 = 4294967296.0


# ------------------------------------------------------------------------------------------------ reference
def q32(x):
    """floor(x * 2^32) of finite float32 x >= 0 -> list of Python integers (the scaling is by a power of two: exact in float64)."""
    x = np.asarray(x, np.float32).ravel()
    assert np.isfinite(x).all() and not (x < 0).any(), "the contract covers finite values >= 0"
    return [int(math.floor(float(v) * Q32)) for v in x]


def sums(T, D):
    """(S1, AA, AB, BB) of |T - D| over the whole crop, modulo 2^64; T, D float32 of one shape."""
    T, D = np.asarray(T, np.float32), np.asarray(D, np.float32)
    assert T.shape == D.shape
    S1 = AA = AB = BB = 0
    for dq in q32(np.abs(T - D)):                       # float32 - float32: one IEEE single subtraction
        a, b = dq >> 20, dq & 0xFFFFF
        S1 += dq
        AA += a * a
        AB += a * b
        BB += b * b
    return S1 & MASK64, AA & MASK64, AB & MASK64, BB & MASK64


def score_of(s, n_pix):
    """mean_std_parts' order on the four sums -> m1 * sqrt(var).  float(int) rounds to nearest (even)."""
    S1, AA, AB, BB = (float(v) for v in s)
    N = float(n_pix)
    m1 = (S1 * 2.0 ** -32) / N
    S2 = (AA * 2.0 ** 40 + AB * 2.0 ** 21) + BB
    m2 = (S2 * 2.0 ** -64) / N
    var = m2 - m1 * m1
    if var < 0.0:
        var = 0.0
    return m1 * math.sqrt(var)


def score(T, D):
    return score_of(sums(T, D), T.size)


def delta_s1(T, D):
    """What the groups of a row add to S1 before the frame's total is added back: sum of |T - D| - |T|, signed."""
    T, D = np.asarray(T, np.float32), np.asarray(D, np.float32)
    return sum(q32(np.abs(T - D))) - sum(q32(np.abs(T - np.float32(0.0))))


def groups(D):
    """The ordered groups of a dense row D (ch, cw): (goff uint32 (n,), gval float32 (n, 4)) of every group of four consecutive
    samples of a crop row (columns 4k .. 4k+3, columns past cw read as 0.0) that holds a sample != 0; goff = 4 x its number."""
    D = np.asarray(D, np.float32)
    ch, cw = D.shape
    gw = (cw + 3) // 4
    pad = np.zeros((ch, 4 * gw), np.float32)
    pad[:, :cw] = D
    v = pad.reshape(ch * gw, 4)
    keep = np.nonzero((v != 0).any(axis=1))[0]
    return (4 * keep).astype(np.uint32), v[keep].copy()


def argmin(vals):
    """First index of the minimum; a NaN never beats a number; all NaN: index 0."""
    best, bi = None, 0
    for i, v in enumerate(np.asarray(vals, np.float64).tolist()):
        if v != v:
            continue
        if best is None or v < best:
            best, bi = v, i
    return bi


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ input values
B_ONES = [np.float32((2 ** 20 - 1) * 2.0 ** -32),           # dq = 0xFFFFF: a = 0, b all ones
          np.float32((2 ** 24 - 1) * 2.0 ** -32),           # dq = 0xFFFFFF: a = 15, b all ones
          np.float32((2 ** 23 + 2 ** 20 - 1) * 2.0 ** -32)]  # a = 8, b all ones
SUBNORMALS = [np.float32(1e-45), np.float32(2.0 ** -130)]
BELOW_Q32 = [np.float32(2.0 ** -33), np.float32(1.5 * 2.0 ** -40)]       # normal numbers with dq == 0
SPECIALS = np.array(B_ONES + SUBNORMALS + BELOW_Q32 + [np.float32(0.0), np.nextafter(np.float32(128.0), np.float32(0.0)), np.float32(1.0)],
                    np.float32)
SCALES = np.array([127.0, 4.0, 1.0, 2.0 ** -10, 2.0 ** -31, 2.0 ** -34])


def values(rng, n, positive=False):
    """n finite float32 values in [0, 128): every magnitude down to below one unit of 2^-32, every third one of SPECIALS (in turn,
    from a random start).  positive: none of them zero."""
    v = (rng.random(n) * rng.choice(SCALES, n)).astype(np.float32)
    k = int(rng.integers(len(SPECIALS)))
    v[::3] = SPECIALS[(k + np.arange(len(v[::3]))) % len(SPECIALS)]
    if positive:
        v[v == 0] = np.float32(0.75)
    assert np.isfinite(v).all() and (v >= 0).all() and (v < 128).all()
    return v


def target_plane(rng, W, H, r0, r1, c0, c1):
    """An H x W float32 plane: NaN outside the crop (a read past the crop poisons a sum), values() inside."""
    plane = np.full((H, W), np.nan, np.float32)
    ch, cw = r1 - r0 + 1, c1 - c0 + 1
    plane[r0:r1 + 1, c0:c1 + 1] = values(rng, ch * cw).reshape(ch, cw)
    return plane


ROW_NAMES = ('empty', 'dense', 'first', 'last', 'alternating', 'negzero', 'duplicate')


def table_rows(rng, T):
    """The seven dense rows (7, ch, cw) for a cropped target T, in ROW_NAMES' order:
    empty        nothing: zero groups
    dense        every sample != 0, three in four of them equal to T where T != 0 (pairs T == D: the row's delta goes negative)
    first        only the first group of the crop
    last         only the last group of the last crop row (the padded tail column when cw % 4 != 0)
    alternating  every other group; inside a kept group 0, -0.0 and values mixed; the groups between hold only -0.0
    negzero      only -0.0: zero groups, though no sample has the bits of 0.0
    duplicate    the dense row again: scores tie exactly"""
    T = np.asarray(T, np.float32)
    ch, cw = T.shape
    gw = (cw + 3) // 4
    rows = np.zeros((len(ROW_NAMES), ch, cw), np.float32)
    dense = values(rng, ch * cw, positive=True).reshape(ch, cw)
    same = (T != 0) & (rng.random((ch, cw)) < 0.75)
    dense[same] = T[same]
    rows[1] = dense
    rows[2][0, :min(4, cw)] = dense[0, :min(4, cw)]
    rows[3][ch - 1, 4 * (gw - 1):] = dense[ch - 1, 4 * (gw - 1):]
    g = np.arange(ch)[:, None] * gw + np.arange(cw)[None, :] // 4            # group number of every sample
    col = np.arange(cw)[None, :] % 4 + np.zeros((ch, 1), int)
    alt = values(rng, ch * cw).reshape(ch, cw)
    alt[col == 0] = dense[col == 0]                                        # a kept group holds at least its first sample
    alt[col == 1] = np.float32(-0.0)
    alt[col == 2] = np.where(g[col == 2] % 4 == 0, np.float32(0.0), alt[col == 2])
    rows[4] = np.where(g % 2 == 0, alt, np.float32(-0.0))
    rows[5] = np.float32(-0.0)
    rows[6] = rows[1]
    return rows


# ------------------------------------------------------------------------------------------------ crops
CROP_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65)
CROP_HEIGHTS = (1, 2, 17)
CROP_LONG = ((1020, 1), (1021, 1), (1025, 1), (36, 57))         # 255, 256, 257 and 513 groups
CROP_SHAPES = tuple((cw, ch) for cw in CROP_WIDTHS for ch in CROP_HEIGHTS) + CROP_LONG


def crop_frames(cw, ch):
    """The three images a (cw, ch) crop is cut from -> [(name, W, H, r0, r1, c0, c1)]:
    whole   W = cw: the crop is the whole image
    right   W = cw + 3: c0 = 3 (c0 % 4 != 0), c1 = W - 1, a row above and below
    left / inner   W = cw + 9: c0 = 0 and r0 = 0 with rows below, or (odd cw + ch) c0 = 5 with rows and columns on every side"""
    out = [('whole', cw, ch, 0, ch - 1, 0, cw - 1), ('right', cw + 3, ch + 2, 1, ch, 3, cw + 2)]
    if (cw + ch) % 2:
        out.append(('inner', cw + 9, ch + 3, 2, ch + 1, 5, cw + 4))
    else:
        out.append(('left', cw + 9, ch + 1, 0, ch - 1, 0, cw - 1))
    return out


def _case(rng, frame, rows=None):
    name, W, H, r0, r1, c0, c1 = frame
    plane = target_plane(rng, W, H, r0, r1, c0, c1)
    T = plane[r0:r1 + 1, c0:c1 + 1]
    rows = table_rows(rng, T) if rows is None else rows
    s = [sums(T, D) for D in rows]
    sc = np.array([score_of(v, T.size) for v in s], np.float64)
    return dict(name=name, W=W, H=H, r0=r0, r1=r1, c0=c0, c1=c1, cw=c1 - c0 + 1, ch=r1 - r0 + 1, plane=plane, T=T, rows=rows,
                groups=[groups(D) for D in rows], sums=np.array(s, np.uint64), scores=sc, best=argmin(sc))


@functools.lru_cache(maxsize=None)
def crop_cases(cw, ch):
    """The (cw, ch) crop in each of crop_frames' images with its seven rows and the reference's answers."""
    rng = np.random.default_rng(1000 * cw + ch)
    return [_case(rng, f) for f in crop_frames(cw, ch)]


@functools.lru_cache(maxsize=None)
def empty_table_case():
    """Seven rows that hold nothing (three of them only -0.0): used == 0."""
    rng = np.random.default_rng(77)
    rows = np.zeros((7, 2, 5), np.float32)
    rows[1::2] = np.float32(-0.0)
    return _case(rng, ('inner', 14, 5, 2, 3, 5, 9), rows)


# ------------------------------------------------------------------------------------------------ many frames
FRAME_COUNTS = (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 129, 130)
CHILD_FRAME_COUNTS = (1, 9, 33, 65, 129, 130)
N_FRAMES = 130
FRAMES_GEOM = (33, 11, 2, 9, 5, 28)                             # W, H, r0, r1, c0, c1: a 24 x 8 crop, c0 % 4 == 1
TABLE_VARIANTS = ((2, 16), (4, 16), (8, 16), (2, 8), (4, 8), (2, 64), (4, 64), (8, 64), (8, 8))      # (8, 8) runs <4, 8>


@functools.lru_cache(maxsize=None)
def frames_case():
    """130 mutually different frames around one 24 x 8 crop, the seven rows (built on frame 0), and scores[f, row] / best[f]."""
    rng = np.random.default_rng(2024)
    W, H, r0, r1, c0, c1 = FRAMES_GEOM
    planes = np.stack([target_plane(rng, W, H, r0, r1, c0, c1) for _ in range(N_FRAMES)])
    crops = planes[:, r0:r1 + 1, c0:c1 + 1]
    rows = table_rows(rng, crops[0])
    sc = np.array([[score(T, D) for D in rows] for T in crops], np.float64)
    return dict(planes=planes, crops=crops, rows=rows, scores=sc, best=np.array([argmin(s) for s in sc]))


def frames_of_batch(n):
    """Which of the 130 frames a batch of n holds, in order: a frame sits at another index in every batch size."""
    return (n + 7 * np.arange(n)) % N_FRAMES


# ------------------------------------------------------------------------------------------------ argmin
ARGMIN_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def block_of(C):
    """Threads of the argmin workgroup for C values (launch_argmin_sets, launch_finalize)."""
    return 64 if C <= 64 else (256 if C <= 256 else 1024)


def tie_places(C):
    """Where the minimum is put among C values -> [(name, indices)]; the first of the indices is the answer.
    wave    63 and 64: two waves of one workgroup
    stride  7 and B + 3: a later element of a LOWER lane must not win over an earlier one of a higher lane
    thread  5, 5 + B (and 5 + 2B): elements of one thread, B its stride
    ends    0 and C - 1"""
    B = block_of(C)
    out = [('first', (0,)), ('last', (C - 1,))]
    if C > 1:
        out.append(('ends', (0, C - 1)))
    if C > 64:
        out.append(('wave', (63, 64)))
    if C > B + 3:
        out.append(('stride', (7, B + 3)))
    if C > B + 5:
        out.append(('thread', (5, 5 + B) + ((5 + 2 * B,) if C > 5 + 2 * B else ())))
    return out


def argmin_sets_cases(C):
    """-> [(name, C doubles, expected index)]: tie_places with 0.25 among distinct values above 1, and the NaN / inf rules."""
    rng = np.random.default_rng(C)
    base = 1.0 + rng.permutation(C) / C + rng.random(C) / (4 * C)          # distinct
    out = []
    for name, idx in tie_places(C):
        v = base.copy()
        v[list(idx)] = 0.25
        out.append((name, v, idx[0]))
    p = C // 2
    if C > 1:
        v = base.copy()
        v[:p] = np.nan
        v[p] = 0.25
        out.append(('nan_before_min', v, p))
        v = base.copy()
        v[0] = np.nan
        v[C - 1] = 0.25
        out.append(('nan_first_min_last', v, C - 1))
    out.append(('all_nan', np.full(C, np.nan), 0))
    v = np.full(C, np.inf)
    v[p] = 3.0
    out.append(('inf_but_one', v, p))
    out.append(('all_inf', np.full(C, np.inf), 0))
    if C > 1:
        v = np.full(C, np.nan)
        v[C - 1] = np.inf
        out.append(('nan_then_inf', v, C - 1))                 # +inf is a number: it beats every NaN
    return out


TIE_GEOM = (7, 4, 1, 2, 3, 6)                                   # W, H, r0, r1, c0, c1: a 4 x 2 crop


@functools.lru_cache(maxsize=None)
def tie_pool():
    """A 4 x 2 crop, 4097 dense rows that all score worse than the row `best`, and their scores.  Tables for finalize's argmin are
    the first C rows of the pool with `best` copied to the places of a tie: duplicated rows, so the scores tie exactly."""
    rng = np.random.default_rng(4097)
    W, H, r0, r1, c0, c1 = TIE_GEOM
    plane = np.full((H, W), np.nan, np.float32)
    T = (1.0 + rng.random((2, 4))).astype(np.float32)
    plane[r0:r1 + 1, c0:c1 + 1] = T
    best = T.copy()
    best[1, 2] = np.float32(T[1, 2] * 0.5)                      # one sample off: a small score above zero
    rows = (T[None] + 8.0 + 100.0 * rng.random((max(ARGMIN_SIZES), 2, 4))).astype(np.float32)
    return dict(plane=plane, T=T, best=best, best_score=score(T, best), rows=rows,
                scores=np.array([score(T, D) for D in rows], np.float64))


def tie_table(C, idx):
    """-> (rows (C, 2, 4), reference scores (C,)) with the best row at every index of idx."""
    p = tie_pool()
    rows, sc = p['rows'][:C].copy(), p['scores'][:C].copy()
    rows[list(idx)] = p['best']
    sc[list(idx)] = p['best_score']
    return rows, sc
