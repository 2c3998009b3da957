"""rope_shade_frames' contract (include/rope_s3d.h) restated in numpy float32, from the header's text: every intermediate is a
float32 array, so every written operation is one correctly rounded IEEE operation, in the header's order.  Philox is the one the
hole tests restate (holes_ref.philox4x32_10)."""
import numpy as np

from holes_ref import philox4x32_10

F = np.float32


def noise(H: int, W: int, frame: int, seed: int, noise_q: int) -> np.ndarray:
    """Step 7 -> (H, W, 3) int64: ((b0 + b1 + b2 + b3 - 510) * noise_q) >> 10 of word c of the generator with key (seed low, seed
    high) and counter (y W + x, frame, 0, 1); zeros, and nothing drawn, when noise_q is 0."""
    out = np.zeros((H, W, 3), np.int64)
    if noise_q == 0:
        return out
    i = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    words = philox4x32_10(i, frame & 0xFFFFFFFF, 0, 1, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for c in range(3):
        w = words[c].astype(np.int64)
        s = (w & 255) + ((w >> 8) & 255) + ((w >> 16) & 255) + ((w >> 24) & 255) - 510
        out[..., c] = (s * int(noise_q)) >> 10                    # numpy's >> on signed integers is arithmetic
    return out


def _diff(P, ids, axis):
    """Step 2 along an axis (1: x, 0: y) -> (H, W, 3) float32."""
    n = ids.shape[axis]
    fwd_ok, bwd_ok = np.zeros(ids.shape, bool), np.zeros(ids.shape, bool)
    nxt, prv = np.roll(ids, -1, axis), np.roll(ids, 1, axis)
    idx = np.arange(n).reshape((-1, 1) if axis == 0 else (1, -1))
    fwd_ok[...] = (idx + 1 < n) & (nxt == ids)
    bwd_ok[...] = (idx > 0) & (prv == ids)
    with np.errstate(invalid='ignore', over='ignore'):
        fwd = (np.roll(P, -1, axis) - P).astype(F)
        bwd = (P - np.roll(P, 1, axis)).astype(F)
    return np.where(fwd_ok[..., None], fwd, np.where(bwd_ok[..., None], bwd, F(0))).astype(F)


def lambert(depth, ids, intr, light):
    """Steps 1-3 -> lam (H, W) float32 for every pixel (robot or not)."""
    fx, fy, cx, cy = (F(v) for v in intr)
    H, W = depth.shape
    z = np.asarray(depth, F)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        kx = ((np.arange(W, dtype=F) - cx) / fx).astype(F)[None, :]
        ky = ((np.arange(H, dtype=F) - cy) / fy).astype(F)[:, None]
        P = np.stack([(kx * z).astype(F), (ky * z).astype(F), z], -1)
        dX, dY = _diff(P, ids, 1), _diff(P, ids, 0)
        m = lambda a, b: (a * b).astype(F)                                                   # noqa: E731
        nx = (m(dX[..., 1], dY[..., 2]) - m(dX[..., 2], dY[..., 1])).astype(F)
        ny = (m(dX[..., 2], dY[..., 0]) - m(dX[..., 0], dY[..., 2])).astype(F)
        nz = (m(dX[..., 0], dY[..., 1]) - m(dX[..., 1], dY[..., 0])).astype(F)
        L = np.asarray(light, F)
        nn = ((m(nx, nx) + m(ny, ny)).astype(F) + m(nz, nz)).astype(F)
        dot = ((m(nx, L[0]) + m(ny, L[1])).astype(F) + m(nz, L[2])).astype(F)
        pos = np.where(dot > 0, dot, F(0)).astype(F)                                         # a NaN dot gives 0 ...
        lam = np.where(nn == 0, F(1), (pos / np.sqrt(nn).astype(F)).astype(F)).astype(F)      # ... and 0 / sqrt(NaN) is NaN
    return lam


def to_byte(v, n):
    """Step 8: float32 values and integer noise -> uint8."""
    with np.errstate(invalid='ignore', over='ignore'):
        t = (np.asarray(v, F) + n.astype(F)).astype(F)
        out = np.where(t > 0, np.where(t < 255, t, F(255)), F(0))
    return out.astype(np.uint8)


def shade_frame(depth, ids, intr, rec, n_links: int, backgrounds=None, frame: int = 0, seed: int = 0):
    """One frame -> (bgr (H, W, 3) uint8, depth_out (H, W) float32).  rec: one record of engine.SHADE_DTYPE."""
    depth, ids = np.asarray(depth, F), np.asarray(ids, np.uint8)
    H, W = depth.shape
    robot = ids < n_links
    lam = lambert(depth, ids, intr, rec['light'])
    amb = F(rec['ambient'])
    with np.errstate(invalid='ignore', over='ignore'):
        s = (amb + ((F(1) - amb) * lam).astype(F)).astype(F)
        shade = np.where(s > 1, F(1), s).astype(F)
        albedo = np.asarray(rec['albedo'], np.uint8)[np.where(robot, ids, 0)].astype(F)       # (H, W, 3)
        gain = np.asarray(rec['gain'], F)
        v = np.rint(((albedo * shade[..., None]).astype(F) * gain).astype(F)).astype(F)
    if int(rec['bg_index']) >= 0:
        back = np.asarray(backgrounds[int(rec['bg_index'])], np.uint8).astype(F)
    else:
        back = np.broadcast_to(np.asarray(rec['bg_colour'], np.uint8).astype(F), (H, W, 3))
    v = np.where(robot[..., None], v, back)
    bgr = to_byte(v, noise(H, W, frame, seed, int(rec['noise_q'])))
    return bgr, np.where(robot, depth, F(rec['bg_depth'])).astype(F)


def shade_frames(depth, ids, intr, params, n_links: int, backgrounds=None, frame0: int = 0, seed: int = 0):
    """N frames -> (bgr (N, H, W, 3) uint8, depth_out (N, H, W) float32)."""
    out = [shade_frame(depth[m], ids[m], intr, params[m], n_links, backgrounds, frame0 + m, seed) for m in range(len(depth))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def blob_scene(rng, H: int, W: int, n_links: int = 6):
    """A seeded scene with the edges the kernel can trip over: patches of one id with their own depth ramps, background between
    them, a one-pixel island, an id that is no link, and a link touching every image edge.  -> (depth float32, ids uint8)."""
    ids = np.full((H, W), 255, np.uint8)
    depth = np.zeros((H, W), F)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for _ in range(6):
        h, w = int(rng.integers(1, max(H // 2, 2))), int(rng.integers(1, max(W // 2, 2)))
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        sel = (yy >= y) & (yy < y + h) & (xx >= x) & (xx < x + w)
        ids[sel] = rng.integers(0, n_links)
        depth[sel] = (rng.uniform(.8, 2.5) + rng.uniform(-.004, .004) * xx + rng.uniform(-.004, .004) * yy)[sel]
    edge = (yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)
    ids[edge] = 1                                                  # a link along every edge
    depth[edge] = (1.5 + .002 * xx + .001 * yy)[edge]
    if H > 4 and W > 4:
        ids[2, 2], depth[2, 2] = 3, 1.25                           # an island ...
        ids[1:4, 1:4][np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], bool)] = 255
        ids[H - 2, W - 3] = n_links                                # ... and an id that counts as background
    return depth, ids
