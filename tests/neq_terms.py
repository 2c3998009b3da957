"""Frames that pin the PER-PIXEL TERMS of the four normal-equation reductions bit for bit (rope_pose_normal_equations,
rope_camera_normal_equations, rope_bundle_normal_equations, rope_silhouette_normal_equations; include/rope_s3d.h) without a word
about the order of their sums, which the header leaves free.

A frame with ONE inlier pixel has sums that ARE that pixel's terms (0.0 + x is exact); a frame with TWO has sums a + b, which IEEE
addition gives the same in either order.  So the kernel's words on such frames must equal the reference's as values, exactly,
whatever the order of either side's summation — and they are generic values: a curved surface, camera terms, axes and twists that
are no dyadic numbers, on which a fused multiply-add, a reassociated dot product or a reciprocal in place of a divide changes the
last bits (`fused_share` below shows it on the reference alone; on the hand-built planes of refine_ref it cannot show).

The surfaces are generated here from fixed seeds and coefficients; tests/test_neq_terms_refs.py holds, by the references alone,
that they bite (enough inliers, the special pixels out, the two-inlier frames two inliers), tests/test_gpu_neq_terms.py holds the
kernels to them."""
import functools
import math
from fractions import Fraction

import numpy as np

from refine_ref import BAD_T, CLIP

COEF = (2.3, -1.7, 0.9)                          # z = 1.9 + a kx^2 + b ky^2 + c kx ky: curved, so neighbour differences are irregular
Z0 = 1.9
NOISE = 0.03                                     # |T - R| <= 0.03 < CLIP = 2^-5: no residual near the truncation by accident
H1, W1 = 24, 32                                  # the single-inlier surface: 768 pixels, one workgroup a frame
INTR1 = tuple(float(np.float32(v)) for v in (151.3, 148.7, 15.4, 11.6))
H2, W2 = 47, 45                                  # the two-inlier surface: 2115 pixels, two workgroups a frame
INTR2 = tuple(float(np.float32(v)) for v in (151.3, 148.7, 21.7, 23.2))
SIL_H, SIL_W = 12, 16                            # the silhouette's window of the first surface: 192 frames
SIL_RADIUS = 6
SIL2_DISC, SIL2_RADIUS = 15, 16                  # the second surface's mask and field
CHUNK, THREADS, WAVE = 2048, 256, 64             # a workgroup's pixels, a pass's, a wave's (csrc/rope_refine.hip)
assert NOISE < CLIP


def columns(rng, N, nj, nc):
    """test_gpu_bundle's `_columns`: (joints (N, nj, 6) or None, twists (N, nc, 6) or None), unit-free generic values; the points
    of the axes lie about the surface's depth."""
    joints = np.concatenate([rng.uniform(-1, 1, (N, nj, 3)), rng.uniform(-.5, .5, (N, nj, 2)), rng.uniform(1.5, 2.5, (N, nj, 1))], axis=2) if nj else None
    return joints, (rng.uniform(-1, 1, (N, nc, 6)) if nc else None)


def _surface(H, W, intr, stripes, seed, island, nolink, hole, bad):
    """-> dict(R, T (H, W) float32, ids (H, W) uint8, special: names -> lists of (y, x)).  Vertical stripes of links 0 ..
    stripes - 1; `island`: one pixel of the next stripe's id (no neighbour of its id: no normal); `nolink`: one pixel of id
    `stripes` (no link when n_links = stripes); `hole`: the corner of a 2 x 2 block of background; `bad`: the first of
    len(BAD_T) pixels of a row that carry BAD_T."""
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in intr)
    kx = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :]
    ky = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None]
    a, b, c = COEF
    R = (Z0 + a * kx * kx + b * ky * ky + c * kx * ky).astype(np.float32)
    ids = (np.arange(W)[None, :] * stripes // W + np.zeros((H, 1), int)).astype(np.uint8)
    rng = np.random.default_rng(seed)
    T = (R.astype(np.float64) + rng.uniform(-NOISE, NOISE, R.shape)).astype(np.float32)
    special = {}
    ids[island] = ids[island] + 1
    special['island'] = [island]
    ids[nolink] = stripes
    special['nolink'] = [nolink]
    y, x = hole
    ids[y:y + 2, x:x + 2] = 255
    R[y:y + 2, x:x + 2] = 0.0
    special['hole'] = [(y + i, x + j) for i in range(2) for j in range(2)]
    y, x = bad
    T[y, x:x + len(BAD_T)] = np.array(BAD_T, np.float32)
    special['bad'] = [(y, x + i) for i in range(len(BAD_T))]
    return dict(R=R, T=T, ids=ids, special=special)


@functools.lru_cache(maxsize=None)
def surface1(stripes=4):
    """24 x 32.  stripes = 4: links 0 .. 3 eight columns each (n_links 4; the pixel of id 4 is no link).  stripes = 6: links 0 .. 5
    (n_links 6; the pixel of id 6 is no link) for the pose kernel's column counts.  The special pixels sit on moving links."""
    return _surface(H1, W1, INTR1, stripes, 101, island=(5, 12), nolink=(9, 20), hole=(14, 26), bad=(10, 9))


@functools.lru_cache(maxsize=None)
def surface2():
    """47 x 45, links 0 .. 3 in stripes (columns 0 .. 11, 12 .. 22, 23 .. 33, 34 .. 44)."""
    return _surface(H2, W2, INTR2, 4, 202, island=(7, 17), nolink=(30, 28), hole=(20, 38), bad=(12, 14))


def single_frames(s):
    """Frame f = the surface with T zero everywhere but at pixel f -> (R, ids, T), each (H W, H, W)."""
    H, W = s['R'].shape
    n = H * W
    T = np.zeros((n, n), np.float32)
    T[np.arange(n), np.arange(n)] = s['T'].reshape(n)
    return (np.ascontiguousarray(np.broadcast_to(s['R'], (n, H, W))), np.ascontiguousarray(np.broadcast_to(s['ids'], (n, H, W))),
            T.reshape(n, H, W))


def frames_with(s, positions):
    """One frame per entry of `positions` (each a tuple of flat pixel indices): T zero but at those pixels -> (R, ids, T)."""
    H, W = s['R'].shape
    n = len(positions)
    T = np.zeros((n, H * W), np.float32)
    for f, ps in enumerate(positions):
        T[f, list(ps)] = s['T'].reshape(-1)[list(ps)]
    return (np.ascontiguousarray(np.broadcast_to(s['R'], (n, H, W))), np.ascontiguousarray(np.broadcast_to(s['ids'], (n, H, W))),
            T.reshape(n, H, W))


# ---------------------------------------------------------------------------------------------- the pairs of the two-inlier frames
LEVELS = ('wave', 'pass', 'thread', 'threads', 'workgroup')


def level_of(p, q):
    """Where the terms of pixels p < q of one frame first meet in the kernels' reduction: 'wave' the same wave of one pass, 'pass'
    two waves of one pass, 'thread' two passes of one thread (q = p + 256), 'threads' two passes of two threads, 'workgroup' two
    workgroups of the frame."""
    if p // CHUNK != q // CHUNK:
        return 'workgroup'
    if p // THREADS != q // THREADS:
        return 'thread' if (q - p) % THREADS == 0 else 'threads'
    return 'wave' if p // WAVE == q // WAVE else 'pass'


def _plain(s, ok=None):
    """The flat indices of the pixels of links 1 .. 3 that are no special pixel and touch none, where `ok` (H, W) allows."""
    H, W = s['ids'].shape
    keep = (s['ids'] >= 1) & (s['ids'] <= 3)
    for ps in s['special'].values():
        for y, x in ps:
            keep[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = False
    if ok is not None:
        keep &= ok
    return np.flatnonzero(keep.reshape(-1))


def _pairs(plain):
    """Eight pairs a level from the plain pixels, walked in a fixed order: -> list of (p, q)."""
    plain = [int(p) for p in plain]
    have = set(plain)
    out = []
    for level in LEVELS:
        found = []
        step = 97                                              # a stride coprime to 64, 256 and the row length: spreads the pairs
        for i in range(len(plain)):
            p = plain[(i * step) % len(plain)]
            if level == 'thread':
                cand = [p + THREADS, p + 3 * THREADS]
            elif level == 'workgroup':
                cand = [q for q in plain if q >= CHUNK][len(found)::8] if p < CHUNK else []
            else:
                cand = [p + d for d in (1, 5, 37, 45, 46, 70, 131, 190, 300, 777, 1100)]
            for q in cand:
                if q in have and q > p and level_of(p, q) == level and all(p not in pr and q not in pr for pr in found):
                    found.append((p, q))
                    break
            if len(found) == 8:
                break
        out += found
    return out


@functools.lru_cache(maxsize=None)
def depth_pairs():
    return _pairs(_plain(surface2()))


# ---------------------------------------------------------------------------------------------- the silhouette's frames
def disc_mask(H, W, radius, shift=(2, -1)):
    """A disc about the window's centre moved by `shift` (rows, columns) -> (H, W) uint8"""
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy - (H // 2 + shift[0])) ** 2 + (xx - (W // 2 + shift[1])) ** 2 <= radius * radius).astype(np.uint8)


def sil_ids(H, W):
    """The id a lone rendered pixel carries: every link 0 .. 5 occurs, so every count of joints before the link does."""
    yy, xx = np.mgrid[0:H, 0:W]
    return ((3 * yy + xx) % 6).astype(np.uint8)


def sil_single_frames():
    """192 frames of 12 x 16: frame f has pixel f alone rendered, on link sil_ids; depth the first surface's; the mask a disc of
    radius 6 moved by (2, -1) -> (R, ids, mask), each (192, 12, 16)."""
    n = SIL_H * SIL_W
    R = np.ascontiguousarray(np.broadcast_to(surface1()['R'][:SIL_H, :SIL_W], (n, SIL_H, SIL_W)))
    R = np.where(R > 0, R, np.float32(Z0)).astype(np.float32)
    ids = np.full((n, n), 255, np.uint8)
    ids[np.arange(n), np.arange(n)] = sil_ids(SIL_H, SIL_W).reshape(n)
    mask = np.ascontiguousarray(np.broadcast_to(disc_mask(SIL_H, SIL_W, 6), (n, SIL_H, SIL_W)))
    return R, ids.reshape(n, SIL_H, SIL_W), mask


@functools.lru_cache(maxsize=None)
def sil_pairs():
    """Pairs of the second surface within the field's reach of the disc's boundary, and not next to each other's neighbours."""
    yy, xx = np.mgrid[0:H2, 0:W2]
    near = np.hypot(yy - (H2 // 2 + 2), xx - (W2 // 2 - 1)) <= SIL2_DISC + SIL2_RADIUS - 3
    return _pairs(_plain(surface2(), near))


def sil_frames_with(positions):
    """One frame of 47 x 45 per entry of `positions`: those pixels alone rendered -> (R, ids, mask)."""
    n = len(positions)
    s = surface2()
    R = np.ascontiguousarray(np.broadcast_to(np.where(s['R'] > 0, s['R'], np.float32(Z0)).astype(np.float32), (n, H2, W2)))
    ids = np.full((n, H2 * W2), 255, np.uint8)
    link = sil_ids(H2, W2).reshape(-1)
    for f, ps in enumerate(positions):
        ids[f, list(ps)] = link[list(ps)]
    mask = np.ascontiguousarray(np.broadcast_to(disc_mask(H2, W2, SIL2_DISC), (n, H2, W2)))
    return R, ids.reshape(n, H2, W2), mask


# ---------------------------------------------------------------------------------------------- what a contraction would change
def fma(a, b, c):
    """a b + c rounded ONCE, exactly: math.fma where the interpreter has it, else through rationals (an int / int division of
    Python is correctly rounded)."""
    if hasattr(math, 'fma'):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def pose_term(s, y, x, intr, joint, fused):
    """(J_0 r, J_0 J_0) of pixel (y, x) of the surface for one joint (6,), step by step from the header in Python floats (IEEE doubles).
    fused = False: one rounding per written operation, the contract.  fused = True: what a compiler that contracts would make of
    the cross and dot products, a b - c d -> fma(a, b, -(c d)) and (a b + c d) + e f -> fma(e, f, fma(c, d, a b))."""
    R, ids, T = s['R'], s['ids'], s['T']
    H, W = R.shape
    fx, fy, cx, cy = (float(np.float32(v)) for v in intr)

    def K(yy, xx):
        return (float(xx) - cx) / fx, (float(yy) - cy) / fy

    def P(yy, xx):
        z = float(R[yy, xx])
        kx, ky = K(yy, xx)
        return (kx * z, ky * z, z)

    def sub(u, v):
        return (u[0] - v[0], u[1] - v[1], u[2] - v[2])

    def step(yy, xx, forward):
        """P(yy, xx) - p, or p - P(yy, xx); fused, the neighbour's products go into the subtraction"""
        if not fused:
            return sub(P(yy, xx), p) if forward else sub(p, P(yy, xx))
        (kx, ky), z = K(yy, xx), float(R[yy, xx])
        if forward:
            return (fma(kx, z, -p[0]), fma(ky, z, -p[1]), z - p[2])
        return (fma(-kx, z, p[0]), fma(-ky, z, p[1]), p[2] - z)

    def cross(u, v):
        if fused:
            return (fma(u[1], v[2], -(u[2] * v[1])), fma(u[2], v[0], -(u[0] * v[2])), fma(u[0], v[1], -(u[1] * v[0])))
        return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])

    def dot(u, v):
        if fused:
            return fma(u[2], v[2], fma(u[1], v[1], u[0] * v[0]))
        return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    p, me = P(y, x), ids[y, x]
    dX = dY = (0.0, 0.0, 0.0)
    if x + 1 < W and ids[y, x + 1] == me:
        dX = step(y, x + 1, True)
    elif x > 0 and ids[y, x - 1] == me:
        dX = step(y, x - 1, False)
    if y + 1 < H and ids[y + 1, x] == me:
        dY = step(y + 1, x, True)
    elif y > 0 and ids[y - 1, x] == me:
        dY = step(y - 1, x, False)
    n = cross(dX, dY)
    nP = dot(n, p)
    a, o = [float(v) for v in joint[:3]], [float(v) for v in joint[3:]]
    J = (p[2] * dot(n, cross(a, sub(p, o)))) / nP
    return J * (p[2] - float(T[y, x])), J * J


def fused_share(s, intr, joints, inlier):
    """Over the inlier pixels f (flat indices; joints[f] is frame f's joint 0) -> (share of them whose J_0 r or J_0 J_0 changes
    when the products are fused, the unfused terms (n, 2)): the data sees a contraction where the share is large."""
    W = s['R'].shape[1]
    plain = np.array([pose_term(s, f // W, f % W, intr, joints[f], False) for f in inlier])
    fused = np.array([pose_term(s, f // W, f % W, intr, joints[f], True) for f in inlier])
    return float((plain != fused).any(axis=1).mean()), plain
