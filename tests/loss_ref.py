"""The loss pass restated, and targets built for its edges.  numpy and Python integers only: no GPU, no oracle.

sums_ref is written from the contract alone — DESIGN.md §3 steps 6-7, its "Camera-pose path" section for the ROPE_LOSS_CAMFULL
words, and the comments on rope_set_target / rope_set_frames in include/rope_s3d.h: one loop over the pixels of the image, no
tiles, no delta form, "nothing rendered" is z = 0 and nothing else.  The builders below make the targets whose VALUES take the
branches of score_pixel / score_tile (rope_lossmath.h) that a render of the robot a few degrees away never takes.

Domain.  Bits 39 and 48-63 of a tq word are outside the header's contract, and the builders never set them.  Non-finite or
negative float targets are outside it too — there the oracle's q32_of_f32 is a C conversion with no defined result — and the
builders never produce them.
"""
import functools
import math

import numpy as np

SUM_WORDS, SUM_CNT, SUM_S1, SUM_AA, SUM_AB, SUM_BB, SUM_LINK0 = 23, 0, 1, 2, 3, 4, 5
LOSS_DEPTH, LOSS_FULL, LOSS_LOOKUP, LOSS_TSWEEP, LOSS_CAMFULL = 0, 1, 2, 3, 4
M64, T_MASK, T_MAX = (1 << 64) - 1, (1 << 39) - 1, (1 << 39) - 1
TILE_W, TILE_H = 128, 96
F32 = np.float32

WRONG = ('ab term dropped', 'depth masked to 38 bits', '9-bit link fields', 'T = 0 mask pixels skipped', 'link 0 as the other links',
         "crop's last column ignored")


# ------------------------------------------------------------------------------------------------ pixel maths
def q32_of_bits(b: int) -> int:
    """floor(x * 2^32) of the finite float32 x >= 0 with bit pattern b, from the bits: x = m * 2^(e - 150)"""
    e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
    assert b >> 31 == 0 and e != 0xFF, "negative or non-finite: outside the contract"
    if e == 0:
        e = 1                                   # denormal: no hidden bit, exponent of the smallest normal
    else:
        m |= 0x800000
    sh = e - 150 + 32
    return m << sh if sh >= 0 else m >> -sh


def q32(x) -> int:
    return q32_of_bits(int(np.asarray(x, F32).view(np.uint32)))


def sqrt_q32_exact(dq: int) -> int:
    """floor(sqrt(dq * 2^-32) * 2^32) = floor(sqrt(dq * 2^32)), every digit of it"""
    return math.isqrt(dq << 32)


def round_sqrt_f64(n: int):
    """The correctly rounded float64 square root of the integer n > 0, from integers alone -> (significand, exponent) with
    sqrt(n) ~ significand * 2^exponent, 2^52 <= significand < 2^53.  A square root is never half-way between two floats (its
    square would need 2 x 54 - 1 bits below the leading one and n * 4^k has none left), so the next digit decides."""
    k = max(0, 54 - (n.bit_length() + 1) // 2)              # isqrt(n << 2k) has 54 or 55 bits
    r = math.isqrt(n << (2 * k))
    exact = r * r == n << (2 * k)
    drop = r.bit_length() - 53
    sig, rest = r >> drop, r & ((1 << drop) - 1)
    half = 1 << (drop - 1)
    assert not (exact and rest == half)
    if rest > half or rest == half:                         # the digits isqrt dropped lie above `rest` when r is not exact
        sig += 1
    if sig == 1 << 53:
        sig, drop = sig >> 1, drop + 1
    return sig, drop - k


@functools.lru_cache(maxsize=1 << 16)
def sqrt_q32(dq: int) -> int:
    """The CAMFULL root as the contract's arithmetic has it (camera_pose_prediction.py:958,964: np.abs(diff) ** .5 in float64):
    the correctly rounded float64 root of dq — dq < 2^39 converts exactly — times 2^16, truncated.  Equal to sqrt_q32_exact
    except where the rounding lifts the root onto a multiple of 2^-16 it lies just below (dq = 2^30 + 1 is the smallest such dq
    above 2^30: tests/test_loss_refs.py shows both)."""
    if dq == 0:
        return 0
    sig, ex = round_sqrt_f64(dq)
    sh = ex + 16
    return sig << sh if sh >= 0 else sig >> -sh


def _acc_sq(s, dq, wrong):
    a, b = dq >> 20, dq & 0xFFFFF
    s[SUM_S1] += dq
    s[SUM_AA] += a * a
    if 'ab term dropped' not in wrong:
        s[SUM_AB] += a * b
    s[SUM_BB] += b * b


# ------------------------------------------------------------------------------------------------ the reference
def sums_ref(depth_f32, ids, loss, n_render, tq=None, t32=None, link_planes=None, crop=None, wrong=()):
    """The 23 sum words (Python ints modulo 2^64) of the image (depth, ids) — what rope_render and the oracle's render return —
    against a target.  tq (H, W) uint64, t32 (H, W) float32, link_planes (6, H, W) uint64, crop (r0, r1, c0, c1) inclusive
    (ROPE_LOSS_LOOKUP).  `wrong`: deliberate mistakes (WRONG), for the tests that must tell them from the right sums."""
    H, W = ids.shape
    zb = np.ascontiguousarray(depth_f32, F32).view(np.uint32).ravel().tolist()
    idl = np.ascontiguousarray(ids).ravel().tolist()
    s = [0] * SUM_WORDS
    r0, r1, c0, c1 = (0, H - 1, 0, W - 1) if loss != LOSS_LOOKUP else [int(v) for v in crop]
    if "crop's last column ignored" in wrong and loss == LOSS_LOOKUP:
        c1 -= 1
    t_mask = (1 << 38) - 1 if 'depth masked to 38 bits' in wrong else T_MASK
    if loss in (LOSS_LOOKUP, LOSS_TSWEEP):
        t = np.ascontiguousarray(t32, F32)
        a = np.sqrt(t) if loss == LOSS_TSWEEP else t                      # float32 sqrtf: correctly rounded
        diff = np.abs(a - np.sqrt(np.ascontiguousarray(depth_f32, F32)))   # float32 subtraction
        assert diff.dtype == F32
        db = diff.view(np.uint32).ravel().tolist()
        for r in range(r0, r1 + 1):
            for c in range(c0, c1 + 1):
                _acc_sq(s, q32_of_bits(db[r * W + c]), wrong)
        return [w & M64 for w in s]
    tql = np.ascontiguousarray(tq, np.uint64).ravel().tolist()
    tll = [np.ascontiguousarray(p, np.uint64).ravel().tolist() for p in link_planes] if loss == LOSS_CAMFULL else None
    fields = {}                                                            # '9-bit link fields': counts per (tile, link, word)
    for i in range(H * W):
        t, zq, idv = tql[i], q32_of_bits(zb[i]), idl[i]
        T = t & t_mask
        dq = abs(T - zq)
        if loss == LOSS_CAMFULL:
            if dq:
                s[SUM_CNT] += 1
                s[SUM_S1] += dq
                s[SUM_AA] += sqrt_q32(dq)
            for l in range(n_render):
                w = tll[l][i]
                M = (w >> 40) & 1
                # base_link's blue value 0 is the black background's too: its render mask holds every empty pixel
                R = int(idv == l or (l == 0 and idv == 255 and 'link 0 as the other links' not in wrong))
                dl = abs((w & t_mask) - (zq if R else 0))
                s[SUM_LINK0 + 3 * l] += int(M != R)
                if dl:
                    s[SUM_LINK0 + 3 * l + 1] += 1
                    s[SUM_LINK0 + 3 * l + 2] += sqrt_q32(dl)
            continue
        if dq:
            s[SUM_CNT] += 1
            _acc_sq(s, dq, wrong)
        if loss == LOSS_FULL:
            mask = (t >> 40) & 0xFF
            if 'T = 0 mask pixels skipped' in wrong and T == 0:
                mask = 0
            first = 0 if 'link 0 as the other links' in wrong else 1
            for l in range(first, n_render):
                M, R = (mask >> l) & 1, int(idv == l)
                dl = abs((T if M else 0) - (zq if R else 0))
                if '9-bit link fields' in wrong:
                    key = ((i // W) // TILE_H, (i % W) // TILE_W, l)
                    f = fields.setdefault(key, [0, 0])
                    f[0] += int(M != R)
                    f[1] += int(dl != 0)
                else:
                    s[SUM_LINK0 + 3 * l] += int(M != R)
                    s[SUM_LINK0 + 3 * l + 1] += int(dl != 0)
                s[SUM_LINK0 + 3 * l + 2] += dl
    for (_, _, l), f in fields.items():                                    # a field that runs over loses its carry when it is unpacked
        s[SUM_LINK0 + 3 * l] += f[0] & 0x1FF
        s[SUM_LINK0 + 3 * l + 1] += f[1] & 0x1FF
    return [w & M64 for w in s]


def n_pix_of(loss, W, H, crop):
    return (crop[1] - crop[0] + 1) * (crop[3] - crop[2] + 1) if loss == LOSS_LOOKUP else W * H


# ------------------------------------------------------------------------------------------------ the kernels' block mapping
def samples_per_thread(n_threads, r_lo, r_hi, block_g, live):
    """score_tile's delta form (rope_lossmath.h): item `it` of rows r_lo..r_hi of a tile is the four-sample group g of tile row
    `row`; thread t takes the items t, t + n_threads, ...  -> the most samples of live (TILE_H, TILE_W bool) one thread meets."""
    bg, brows, bpr_sh = block_g, 64 >> block_g, 5 - block_g
    n_items = (r_hi - r_lo + 1) * (TILE_W // 4)
    most = 0
    for t in range(n_threads):
        n = 0
        for it in range(t, n_items, n_threads):
            b, l = it >> 6, it & 63
            g = ((b & ((1 << bpr_sh) - 1)) << bg) | (l & ((1 << bg) - 1))
            i4 = (r_lo + (b >> bpr_sh) * brows + (l >> bg)) * (TILE_W // 4) + g
            row, col = (4 * i4) // TILE_W, (4 * i4) % TILE_W
            assert r_lo <= row <= r_hi, "the mapping leaves the band it was given"
            n += int(live[row, col:col + 4].sum())
        most = max(most, n)
    return most


def samples_per_thread_plain(n_threads, live):
    """score_tile's plain form (empty_tile_kernel): sample i of the tile goes to thread i % n_threads"""
    flat = live.ravel()
    return max(int(flat[t::n_threads].sum()) for t in range(n_threads))


def band_counts():
    """Row bands launch_score_gtile can be given (rope_abi.hip: 1 doubled while below 8)"""
    return (1, 2, 4, 8)


# ------------------------------------------------------------------------------------------------ edge targets
DEPTH_KINDS = ('0', '1', '2^20-1', '2^20', '2^39-1', 'b all ones', 'zq', 'zq+1', 'zq-1')
FLOAT_KINDS = ('0', 'denormal', '2^-33', '2^-32', 'below 1', '127.99999', '65535', 'below 2^32', 'sqrtf(z)', 'z')
LINK_KINDS = tuple((m, d) for d in ('0', 'zq', 'zq+1', '2^39-1', '1') for m in (0, 1))      # (bit 40, depth)
FLOAT_VALUES = {'0': F32(0), 'denormal': F32(1e-45), '2^-33': F32(2.0 ** -33), '2^-32': F32(2.0 ** -32),
                'below 1': np.nextafter(F32(1), F32(0)), '127.99999': F32(127.99999), '65535': F32(65535),
                'below 2^32': np.nextafter(F32(2.0 ** 32), F32(0))}


def tiles_of(W, H):
    return [(ty, tx) for ty in range((H + TILE_H - 1) // TILE_H) for tx in range((W + TILE_W - 1) // TILE_W)]


def seam_lines(W, H, crop=None):
    """name -> pixel indices (rows, cols) of the lines every kind is placed along: the image's last row and column, both sides
    of every tile seam, and — for the float plane — the four borders of every crop in `crop`"""
    lines = {'last row': (np.full(W, H - 1), np.arange(W)), 'last column': (np.arange(H), np.full(H, W - 1))}
    for y in range(TILE_H, H, TILE_H):
        lines[f'above seam {y}'], lines[f'below seam {y}'] = (np.full(W, y - 1), np.arange(W)), (np.full(W, y), np.arange(W))
    for x in range(TILE_W, W, TILE_W):
        lines[f'left of seam {x}'], lines[f'right of seam {x}'] = (np.arange(H), np.full(H, x - 1)), (np.arange(H), np.full(H, x))
    for k, (r0, r1, c0, c1) in enumerate(crop or ()):
        rr, cc = np.arange(r0, r1 + 1), np.arange(c0, c1 + 1)
        lines[f'crop {k} top'], lines[f'crop {k} bottom'] = (np.full(len(cc), r0), cc), (np.full(len(cc), r1), cc)
        lines[f'crop {k} left'], lines[f'crop {k} right'] = (rr, np.full(len(rr), c0)), (rr, np.full(len(rr), c1))
    return lines


def _kind_plane(drawn, n_kinds, seed, lines):
    """A kind index per pixel: inside every tile the drawn and the undrawn pixels each run through the kinds in turn (from a
    start that depends on the seed), then every line does"""
    H, W = drawn.shape
    kind = np.zeros((H, W), np.int64)
    free = np.ones((H, W), bool)                                          # the pixels off every line keep the tiles' turn whole
    for rr, cc in lines.values():
        free[rr, cc] = False
    for ty, tx in tiles_of(W, H):
        sl = (slice(ty * TILE_H, min(H, (ty + 1) * TILE_H)), slice(tx * TILE_W, min(W, (tx + 1) * TILE_W)))
        sub, d, f = kind[sl], drawn[sl], free[sl]
        for side in (True, False):
            n = int(((d == side) & f).sum())
            sub[(d == side) & f] = (np.arange(n) + seed + 3 * ty + 5 * tx) % n_kinds
    for k, (name, (rr, cc)) in enumerate(sorted(lines.items())):
        if len(rr) >= n_kinds:                                            # a crop of one column: its borders are too short, left as they are
            kind[rr, cc] = (np.arange(len(rr)) + seed + k) % n_kinds
    return kind


def _counts(kind, names, drawn, lines):
    """{'tiles': {(ty, tx): {name: [on drawn, on undrawn]}}, 'lines': {line: set of names}}"""
    H, W = drawn.shape
    tiles = {}
    for ty, tx in tiles_of(W, H):
        sl = (slice(ty * TILE_H, min(H, (ty + 1) * TILE_H)), slice(tx * TILE_W, min(W, (tx + 1) * TILE_W)))
        tiles[(ty, tx)] = {n: [int(((kind[sl] == k) & drawn[sl]).sum()), int(((kind[sl] == k) & ~drawn[sl]).sum())] for k, n in enumerate(names)}
    return {'tiles': tiles, 'lines': {name: {names[k] for k in set(kind[rr, cc].tolist())} for name, (rr, cc) in lines.items()}}


def _zq_of_rows(renders):
    """Per pixel the Q32 depth and link id of the first sampled row that draws it (0 / 255 where none does)"""
    H, W = renders[0][1].shape
    zq, who = np.zeros((H, W), np.uint64), np.full((H, W), 255, np.uint8)
    z32 = np.zeros((H, W), F32)
    for depth, ids in reversed(renders):
        on = ids != 255
        bits = np.ascontiguousarray(depth, F32).view(np.uint32)
        q = np.array([q32_of_bits(b) for b in bits[on].tolist()], np.uint64)
        zq[on], who[on], z32[on] = q, ids[on], depth[on]
    return zq, who, z32


def _depth_values(kind, zq, names=DEPTH_KINDS):
    zi = zq.astype(object)
    table = {'0': 0 * zi, '1': 0 * zi + 1, '2^20-1': 0 * zi + (1 << 20) - 1, '2^20': 0 * zi + (1 << 20), '2^39-1': 0 * zi + T_MAX,
             'b all ones': zi + ((3 << 20) | 0xFFFFF), 'zq': zi, 'zq+1': zi + 1, 'zq-1': np.maximum(zi - 1, 0)}
    out = np.zeros(kind.shape, np.uint64)
    for k, n in enumerate(names):
        out[kind == k] = table[n][kind == k].astype(np.uint64)
    assert int(out.max()) <= T_MAX
    return out


def build_tq(renders, seed=0, all_masks_tile=None):
    """renders: [(depth, ids)] of the sampled rows -> (tq plane, counts).  Depth kinds and the 64 values of mask bits 0-5 run
    through the pixels independently (9 and 64 have no common factor: every pair of them turns up).  counts['depth'] and
    counts['mask'] as _counts gives them, plus counts['named']: per tile, samples with a mask and T = 0, with a mask of a link
    other than the one drawn there, with a mask where nothing is drawn.  all_masks_tile (ty, tx): that whole tile carries
    masks 1-5 and T = 2^39 - 1 instead."""
    zq, who, _ = _zq_of_rows(renders)
    drawn = who != 255
    H, W = drawn.shape
    lines = seam_lines(W, H)
    dk, mk = _kind_plane(drawn, len(DEPTH_KINDS), seed, lines), _kind_plane(drawn, 64, seed, lines)
    T = _depth_values(dk, zq)
    tq = T | (mk.astype(np.uint64) << np.uint64(40))
    counts = {'depth': _counts(dk, DEPTH_KINDS, drawn, lines), 'mask': _counts(mk, list(range(64)), drawn, lines), 'named': {}}
    if all_masks_tile is not None:
        ty, tx = all_masks_tile
        tq[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W] = np.uint64(T_MAX | (0x3E << 40))
    other = np.zeros((H, W), bool)
    for l in range(1, 6):
        other |= (((tq >> np.uint64(40 + l)) & np.uint64(1)) != 0) & drawn & (who != l)
    any_mask = ((tq >> np.uint64(41)) & np.uint64(0x1F)) != 0
    for ty, tx in tiles_of(W, H):
        sl = (slice(ty * TILE_H, (ty + 1) * TILE_H), slice(tx * TILE_W, (tx + 1) * TILE_W))
        counts['named'][(ty, tx)] = {'mask, T = 0': [int((any_mask & ((tq & np.uint64(T_MASK)) == 0) & d)[sl].sum()) for d in (drawn, ~drawn)],
                                     'mask of another link': int(other[sl].sum()), 'mask, nothing drawn': int((any_mask & ~drawn)[sl].sum()),
                                     'drawn': int(drawn[sl].sum()), 'undrawn': int((~drawn)[sl].sum())}
    return tq, counts


def build_t32(renders, seed=0, crop=None):
    """-> (float32 plane, counts): FLOAT_KINDS through the pixels, along the seams and along the crop's borders; finite and >= 0"""
    zq, who, z32 = _zq_of_rows(renders)
    drawn = who != 255
    H, W = drawn.shape
    lines = seam_lines(W, H, crop)
    fk = _kind_plane(drawn, len(FLOAT_KINDS), seed, lines)
    out = np.zeros((H, W), F32)
    for k, n in enumerate(FLOAT_KINDS):
        out[fk == k] = FLOAT_VALUES[n] if n in FLOAT_VALUES else (np.sqrt(z32) if n == 'sqrtf(z)' else z32)[fk == k]
    assert np.isfinite(out).all() and (out >= 0).all()
    return out, {'float': _counts(fk, FLOAT_KINDS, drawn, lines)}


def build_link_planes(renders, seed=0):
    """-> (planes (6, H, W) uint64, counts): per link LINK_KINDS — bit 40 with and without depth, depth without bit 40 —
    through the pixels, from another start for every link.  counts['link'][l]: per kind [where link l is drawn (link 0: or
    nothing is), where it is not] over the image, beside the per-tile counts of _counts."""
    zq, who, _ = _zq_of_rows(renders)
    drawn = who != 255
    H, W = drawn.shape
    lines = seam_lines(W, H)
    planes, counts = np.zeros((6, H, W), np.uint64), {'link': {}, 'tiles': {}}
    zi = zq.astype(object)
    depth_of = {'0': 0 * zi, 'zq': zi, 'zq+1': zi + 1, '2^39-1': 0 * zi + T_MAX, '1': 0 * zi + 1}
    for l in range(6):
        lk = _kind_plane(drawn, len(LINK_KINDS), seed + 7 * l, lines)
        for k, (m, d) in enumerate(LINK_KINDS):
            planes[l][lk == k] = depth_of[d][lk == k].astype(np.uint64) | np.uint64(m << 40)
        here = (who == l) | (~drawn if l == 0 else False)
        counts['link'][l] = {kd: [int(((lk == k) & here).sum()), int(((lk == k) & ~here).sum())] for k, kd in enumerate(LINK_KINDS)}
        counts['tiles'][l] = _counts(lk, LINK_KINDS, drawn, lines)
    return planes, counts
