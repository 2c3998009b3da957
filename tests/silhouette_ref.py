"""rope_mask_distance's and rope_silhouette_normal_equations' contracts (include/rope_s3d.h) restated in plain numpy and Python
loops from the header's text, one pixel at a time where that is the plainest way to say it.  As tests/bundle_ref.py does, every
sum of normal_equations comes with the sum of the absolute values of its terms: what a reordered float64 summation may differ by
is a multiple of it (tests/test_gpu_silhouette.py).  Python's floats are IEEE doubles and every line below is one operation per
written operation, so the terms are the kernel's bits and the sums differ from its in their order alone."""
import numpy as np

BNEQ_WORDS = 96
SLOTS = 12
MAX_RADIUS = 16


def far(radius):
    return radius * radius + 1


def mask_distance(mask, radius):
    """mask (N, H, W), non-zero = robot -> (N, H, W) int32: -m inside, +m outside, m the least dx^2 + dy^2 over the pixels of the
    other state inside the image with |dx|, |dy| <= radius; radius^2 + 1 where there is none or the least is larger."""
    inn = np.asarray(mask) != 0
    N, H, W = inn.shape
    R = int(radius)
    m = np.full((N, H, W), far(R), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = dx * dx + dy * dy
            if d2 == 0 or d2 > R * R:
                continue
            # p over the pixels whose partner q = p + (dx, dy) is inside the image
            py = slice(max(0, -dy), min(H, H - dy))
            px = slice(max(0, -dx), min(W, W - dx))
            qy = slice(max(0, -dy) + dy, min(H, H - dy) + dy)
            qx = slice(max(0, -dx) + dx, min(W, W - dx) + dx)
            if py.start >= py.stop or px.start >= px.stop:
                continue
            other = inn[:, py, px] != inn[:, qy, qx]
            m[:, py, px] = np.where(other, np.minimum(m[:, py, px], d2), m[:, py, px])
    return np.where(inn, -m, m).astype(np.int32)


def phi(sd, radius):
    """step 1: the signed distance to the boundary in pixels"""
    m = min(abs(int(sd)), far(radius))
    d = np.sqrt(np.float64(m)) - 0.5
    return -d if sd < 0 else d


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def frame_terms(R, ids, sd2, n_links, intr, joints, twists, radius):
    """One frame -> a list with, per CONTOUR pixel in pixel order, (e, inlier, J (12,)); J is zero for what is no inlier."""
    R, ids, sd2 = np.asarray(R), np.asarray(ids), np.asarray(sd2)
    H, W = ids.shape
    joints = np.zeros((0, 6)) if joints is None else np.asarray(joints, np.float64).reshape(-1, 6)
    twists = np.zeros((0, 6)) if twists is None else np.asarray(twists, np.float64).reshape(-1, 6)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in intr)
    rad = int(radius)
    rendered = ids < n_links
    out = []
    with np.errstate(all='ignore'):
        for y in range(H):
            for x in range(W):
                if not rendered[y, x]:
                    continue
                nb = [(yy, xx) for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)) if 0 <= yy < H and 0 <= xx < W]
                if all(rendered[q] for q in nb):
                    continue                                                # no contour: the frame's edge is no outline
                f = phi(sd2[y, x], rad)
                e = f + 0.5
                J = np.zeros(SLOTS)
                inlier = abs(int(sd2[y, x])) <= rad * rad
                if inlier:
                    if x - 1 >= 0 and x + 1 < W:
                        gx = (phi(sd2[y, x + 1], rad) - phi(sd2[y, x - 1], rad)) / 2.0
                    elif x + 1 < W:
                        gx = phi(sd2[y, x + 1], rad) - f
                    elif x - 1 >= 0:
                        gx = f - phi(sd2[y, x - 1], rad)
                    else:
                        gx = np.float64(0.0)
                    if y - 1 >= 0 and y + 1 < H:
                        gy = (phi(sd2[y + 1, x], rad) - phi(sd2[y - 1, x], rad)) / 2.0
                    elif y + 1 < H:
                        gy = phi(sd2[y + 1, x], rad) - f
                    elif y - 1 >= 0:
                        gy = f - phi(sd2[y - 1, x], rad)
                    else:
                        gy = np.float64(0.0)
                    z = np.float64(R[y, x])
                    kx, ky = (np.float64(x) - cx) / fx, (np.float64(y) - cy) / fy
                    P = (kx * z, ky * z, z)
                    us = {}
                    for j in range(min(int(ids[y, x]), len(joints))):       # the joints before the link
                        a, o = joints[j, :3], joints[j, 3:]
                        us[j] = _cross(a, (P[0] - o[0], P[1] - o[1], P[2] - o[2]))
                    for k in range(len(twists)):
                        w, v = twists[k, :3], twists[k, 3:]
                        c = _cross(w, P)
                        us[6 + k] = (c[0] + v[0], c[1] + v[1], c[2] + v[2])
                    for c, u in us.items():
                        vx = (fx * (u[0] - kx * u[2])) / z
                        vy = (fy * (u[1] - ky * u[2])) / z
                        J[c] = gx * vx + gy * vy
                out.append((e, inlier, J))
    return out


def normal_equations(R, ids, sd2, n_links, intr, joints, twists, radius):
    """N frames -> (sums (N, 96), abs_sums (N, 96)).  joints (N, n_joints, 6) or None, twists (N, n_cols, 6) or None."""
    R, ids, sd2 = np.asarray(R), np.asarray(ids), np.asarray(sd2)
    N = len(R)
    joints = None if joints is None else np.asarray(joints, np.float64).reshape(N, -1, 6)
    twists = None if twists is None else np.asarray(twists, np.float64).reshape(N, -1, 6)
    out, mag = np.zeros((N, BNEQ_WORDS)), np.zeros((N, BNEQ_WORDS))
    pairs = [(a, b) for a in range(SLOTS) for b in range(a, SLOTS)]
    for f in range(N):
        terms = frame_terms(R[f], ids[f], sd2[f], n_links, intr, None if joints is None else joints[f], None if twists is None else twists[f],
                            radius)
        cols = [[] for _ in range(BNEQ_WORDS)]
        for e, inlier, J in terms:
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


def unpack(words):
    """(96,) -> (A (12, 12) symmetric, g (12,))"""
    A = np.zeros((SLOTS, SLOTS))
    A[np.triu_indices(SLOTS)] = words[16:94]
    return A + np.triu(A, 1).T, np.array(words[4:16], np.float64)
