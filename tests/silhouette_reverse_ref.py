"""rope_render_nearest's and rope_silhouette_normal_equations_reverse's contracts (include/rope_s3d.h) restated in plain numpy and
Python loops from the header's text, as tests/silhouette_ref.py does for the forward direction: phi, far and the cross product are
that file's, every sum comes with the sum of the absolute values of its terms, and every line is one IEEE operation per written
operation, so the terms are the kernel's bits and the sums differ from its in their order alone."""
import numpy as np

from silhouette_ref import BNEQ_WORDS, SLOTS, _cross, far, phi

CODE_SIDE = 33
CODE_MAX = CODE_SIDE * CODE_SIDE - 1
FAR_CODE = -1


def encode(dy, dx):
    return (dy + 16) * CODE_SIDE + (dx + 16)


def decode(code):
    """a code that is not FAR -> (dy, dx)"""
    code = int(code)
    return code // CODE_SIDE - 16, code % CODE_SIDE - 16


def render_nearest(ids, n_links, radius):
    """ids (N, H, W) uint8 -> (N, H, W) int16.  The offsets are visited in raster order, dy upward and dx upward within it, and an
    offset replaces what a pixel holds only when it is STRICTLY nearer: of several pixels at the least distance the first in raster
    order stays."""
    rendered = np.asarray(ids) < n_links
    N, H, W = rendered.shape
    R = int(radius)
    best = np.full((N, H, W), far(R), np.int64)
    code = np.full((N, H, W), FAR_CODE, np.int16)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = dx * dx + dy * dy
            if d2 == 0 or d2 > R * R:
                continue
            py, px = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))      # p whose partner p + (dx, dy) is in the image
            if py.start >= py.stop or px.start >= px.stop:
                continue
            qy, qx = slice(py.start + dy, py.stop + dy), slice(px.start + dx, px.stop + dx)
            better = (rendered[:, py, px] != rendered[:, qy, qx]) & (d2 < best[:, py, px])
            best[:, py, px] = np.where(better, d2, best[:, py, px])
            code[:, py, px] = np.where(better, encode(dy, dx), code[:, py, px])
    return code


def derived_sd(near, ids, n_links, radius):
    """What follows from the codes: (N, H, W) int32, -(dx^2 + dy^2) where rendered, + where not, +-(R^2 + 1) for FAR."""
    near = np.asarray(near).astype(np.int64)
    dy, dx = near // CODE_SIDE - 16, near % CODE_SIDE - 16
    m = np.where(near < 0, far(radius), dx * dx + dy * dy)
    return np.where(np.asarray(ids) < n_links, -m, m).astype(np.int32)


def anchor(code, rendered, y, x):
    """The rendered pixel that carries the boundary p = (y, x) sees -> (cy, cx); code: near[p], not FAR."""
    dy, dx = decode(code)
    cy, cx = y + dy, x + dx
    if rendered:
        if abs(dx) >= abs(dy):
            cx -= 1 if dx > 0 else -1
        else:
            cy -= 1 if dy > 0 else -1
    return cy, cx


def frame_terms(mask, near, R, ids, n_links, intr, joints, twists, radius):
    """One frame -> a list with, per contour pixel OF THE MASK in pixel order, (e, inlier, J (12,), (y, x), anchor or None)."""
    mask, near, R, ids = np.asarray(mask) != 0, np.asarray(near), np.asarray(R), np.asarray(ids)
    H, W = ids.shape
    joints = np.zeros((0, 6)) if joints is None else np.asarray(joints, np.float64).reshape(-1, 6)
    twists = np.zeros((0, 6)) if twists is None else np.asarray(twists, np.float64).reshape(-1, 6)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in intr)
    rad = int(radius)
    rendered = ids < n_links
    sd = derived_sd(near[None], ids[None], n_links, rad)[0]
    out = []
    with np.errstate(all='ignore'):
        for y in range(H):
            for x in range(W):
                if not mask[y, x]:
                    continue
                nb = [(yy, xx) for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)) if 0 <= yy < H and 0 <= xx < W]
                if all(mask[q] for q in nb):
                    continue                                                # no contour: the frame's edge is no outline
                f = phi(sd[y, x], rad)
                e = f + 0.5
                J = np.zeros(SLOTS)
                inlier = abs(int(sd[y, x])) <= rad * rad
                c = None
                if inlier:
                    if x - 1 >= 0 and x + 1 < W:
                        gx = (phi(sd[y, x + 1], rad) - phi(sd[y, x - 1], rad)) / 2.0
                    elif x + 1 < W:
                        gx = phi(sd[y, x + 1], rad) - f
                    elif x - 1 >= 0:
                        gx = f - phi(sd[y, x - 1], rad)
                    else:
                        gx = np.float64(0.0)
                    if y - 1 >= 0 and y + 1 < H:
                        gy = (phi(sd[y + 1, x], rad) - phi(sd[y - 1, x], rad)) / 2.0
                    elif y + 1 < H:
                        gy = phi(sd[y + 1, x], rad) - f
                    elif y - 1 >= 0:
                        gy = f - phi(sd[y - 1, x], rad)
                    else:
                        gy = np.float64(0.0)
                    c = anchor(near[y, x], rendered[y, x], y, x)
                    z = np.float64(R[c])
                    kx, ky = (np.float64(c[1]) - cx) / fx, (np.float64(c[0]) - cy) / fy
                    P = (kx * z, ky * z, z)
                    us = {}
                    for j in range(min(int(ids[c]), len(joints))):          # the joints before the anchor's link
                        a, o = joints[j, :3], joints[j, 3:]
                        us[j] = _cross(a, (P[0] - o[0], P[1] - o[1], P[2] - o[2]))
                    for k in range(len(twists)):
                        w, v = twists[k, :3], twists[k, 3:]
                        cr = _cross(w, P)
                        us[6 + k] = (cr[0] + v[0], cr[1] + v[1], cr[2] + v[2])
                    for s, u in us.items():
                        vx = (fx * (u[0] - kx * u[2])) / z
                        vy = (fy * (u[1] - ky * u[2])) / z
                        J[s] = -(gx * vx + gy * vy)
                out.append((e, inlier, J, (y, x), c))
    return out


def normal_equations(mask, near, R, ids, n_links, intr, joints, twists, radius):
    """N frames -> (sums (N, 96), abs_sums (N, 96)).  joints (N, n_joints, 6) or None, twists (N, n_cols, 6) or None."""
    mask, near, R, ids = np.asarray(mask), np.asarray(near), np.asarray(R), np.asarray(ids)
    N = len(R)
    joints = None if joints is None else np.asarray(joints, np.float64).reshape(N, -1, 6)
    twists = None if twists is None else np.asarray(twists, np.float64).reshape(N, -1, 6)
    out, mag = np.zeros((N, BNEQ_WORDS)), np.zeros((N, BNEQ_WORDS))
    pairs = [(a, b) for a in range(SLOTS) for b in range(a, SLOTS)]
    for f in range(N):
        terms = frame_terms(mask[f], near[f], R[f], ids[f], n_links, intr, None if joints is None else joints[f],
                            None if twists is None else twists[f], radius)
        cols = [[] for _ in range(BNEQ_WORDS)]
        for e, inlier, J, _, _ in terms:
            cols[0].append(1.0)
            cols[1].append(e * e)
            if not inlier:
                continue
            cols[2].append(1.0)
            cols[3].append(e * e)
            for c in range(SLOTS):
                cols[4 + c].append(J[c] * e)
            for w, (a, b) in enumerate(pairs):
                cols[16 + w].append(J[a] * J[b])
        with np.errstate(all='ignore'):
            for w, col in enumerate(cols):
                x = np.array(col, np.float64)
                out[f, w] = x.sum()
                mag[f, w] = np.abs(x).sum()
    return out, mag
