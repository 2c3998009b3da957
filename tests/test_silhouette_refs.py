"""CPU: tests/silhouette_ref.py on its own — the restatement that tests/test_gpu_silhouette.py holds the kernels of
csrc/rope_silhouette.hip to must itself say what include/rope_s3d.h says.  The distance field against an all-pairs search, the
image edge, and the normal equations on a fronto-parallel plate whose answer is known in closed form."""
import numpy as np
import pytest

import silhouette_ref as sref

PLATE_INTR = (60.0, 60.0, 23.5, 15.5)
PLATE_Z = 1.5
PLATE_HW = (32, 48)
PLATE_BOX = (8, 22, 14, 30)             # y0, y1, x0, x1: rows 8 .. 21, columns 14 .. 29
X_TRANSLATION = np.array([[[0, 0, 0, 1.0, 0, 0]]])


def brute_force(mask, R):
    """All pairs: for every p, every q of the plane."""
    inn = np.asarray(mask) != 0
    H, W = inn.shape
    out = np.zeros((H, W), np.int32)
    for py in range(H):
        for px in range(W):
            m = None
            for qy in range(H):
                for qx in range(W):
                    dy, dx = qy - py, qx - px
                    if abs(dy) <= R and abs(dx) <= R and inn[qy, qx] != inn[py, px]:
                        d2 = dx * dx + dy * dy
                        m = d2 if m is None or d2 < m else m
            if m is None or m > R * R:
                m = R * R + 1
            out[py, px] = -m if inn[py, px] else m
    return out


@pytest.mark.parametrize('shape', [(12, 12), (1, 12), (11, 1), (7, 10), (1, 1)])
def test_distance_field_against_an_all_pairs_search(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    H, W = shape
    masks = [rng.random(shape) < 0.5, rng.random(shape) < 0.08, rng.random(shape) > 0.08, np.zeros(shape, bool)]
    masks[3][H // 2, W // 2] = True
    for R in (1, 2, 5, 16):
        got = sref.mask_distance(np.stack(masks).astype(np.uint8) * 7, R)
        assert got.dtype == np.int32 and got.shape == (4, H, W)
        for m, g in zip(masks, got):
            assert np.array_equal(g, brute_force(m, R)), (shape, R)
        assert (got != 0).all() and (np.abs(got) <= R * R + 1).all() and np.array_equal(got < 0, np.stack(masks))


def test_the_image_edge_is_no_boundary():
    for R in (1, 8, 16):
        for value in (0, 1):
            got = sref.mask_distance(np.full((2, 9, 13), value, np.uint8), R)
            assert (got == (-(R * R + 1) if value else R * R + 1)).all()
    # and a pixel next to the edge measures to the mask alone
    m = np.zeros((1, 5, 5), np.uint8)
    m[0, 0, 0] = 1
    got = sref.mask_distance(m, 2)
    assert got[0, 0, 0] == -1 and got[0, 0, 1] == 1 and got[0, 1, 1] == 2 and got[0, 2, 2] == 5 and got[0, 0, 3] == 5 and got[0, 4, 4] == 5


def plate(shift=0):
    """(R, ids, mask) of one frame: a plate at PLATE_Z on link 0, and the mask of the same plate `shift` pixels further in x."""
    H, W = PLATE_HW
    y0, y1, x0, x1 = PLATE_BOX
    ids = np.full((1, H, W), 255, np.uint8)
    ids[0, y0:y1, x0:x1] = 0
    R = np.where(ids == 0, np.float32(PLATE_Z), np.float32(0)).astype(np.float32)
    mask = np.zeros((1, H, W), np.uint8)
    mask[0, y0:y1, x0 + shift:x1 + shift] = 1
    return R, ids, mask


@pytest.mark.parametrize('k', [1, 2, 3, -1, -2, -3])
def test_a_shifted_plate_asks_for_the_shift(k):
    """The mask is the plate k pixels further in x; the one column is the camera's pure x translation, under which a point at depth
    z moves fx / z pixels per metre.  The left and right edges carry e = +-k and J = -+fx / z exactly; the corners, where the
    field is sampled at pixel centres off the axis, bend the answer by less than half a pixel's worth."""
    R, ids, mask = plate(k)
    sd2 = sref.mask_distance(mask, 8)
    words, _ = sref.normal_equations(R, ids, sd2, 1, PLATE_INTR, None, X_TRANSLATION, 8)
    A, g = sref.unpack(words[0])
    y0, y1, x0, x1 = PLATE_BOX
    assert words[0, 0] == 2 * (y1 - y0) + 2 * (x1 - x0) - 4 == words[0, 2]
    step = -g[6] / A[6, 6]
    want = k * PLATE_Z / PLATE_INTR[0]
    print(f"shift {k}: step {step:.6f} m, k z / fx {want:.6f} m, half a pixel {0.5 * PLATE_Z / PLATE_INTR[0]:.6f} m")
    assert abs(step - want) <= 0.5 * PLATE_Z / PLATE_INTR[0] and np.sign(step) == np.sign(k)
    # the middle of the left edge, by hand
    t = sref.frame_terms(R[0], ids[0], sd2[0], 1, PLATE_INTR, None, X_TRANSLATION[0], 8)
    left = [(e, J[6]) for (e, inl, J), (y, x) in zip(t, [(y, x) for y in range(y0, y1) for x in range(x0, x1) if y in (y0, y1 - 1) or x in (x0, x1 - 1)])
            if x == x0 and y0 + 4 <= y < y1 - 4]
    assert left and all(e == k and J == -PLATE_INTR[0] / PLATE_Z for e, J in left)


def test_an_aligned_plate_has_no_residual_and_no_gradient():
    R, ids, mask = plate(0)
    sd2 = sref.mask_distance(mask, 8)
    rng = np.random.default_rng(1)
    joints = np.concatenate([rng.uniform(-1, 1, (1, 6, 3)), rng.uniform(-.5, .5, (1, 6, 3))], axis=2)
    twists = rng.uniform(-1, 1, (1, 6, 6))
    ids2 = np.where(ids == 0, 3, ids).astype(np.uint8)                     # link 3: joints 0 .. 2 move it
    words, _ = sref.normal_equations(R, ids2, sd2, 6, PLATE_INTR, joints, twists, 8)
    assert words[0, 0] > 0 and words[0, 0] == words[0, 2]
    assert words[0, 1] == 0 and words[0, 3] == 0 and not words[0, 4:16].any()
    A, _ = sref.unpack(words[0])
    live = [0, 1, 2] + list(range(6, 12))
    assert (np.diag(A)[live] > 0).all() and not A[3:6].any() and not A[:, 3:6].any()


@pytest.mark.parametrize('nj,nc', [(0, 6), (6, 0), (2, 3), (1, 1)])
def test_slots_that_are_not_given_are_exactly_zero(nj, nc):
    R, ids, mask = plate(2)
    ids = np.where(ids == 0, 5, ids).astype(np.uint8)
    sd2 = sref.mask_distance(mask, 8)
    rng = np.random.default_rng(nj * 7 + nc)
    joints = np.concatenate([rng.uniform(-1, 1, (1, nj, 3)), rng.uniform(-.5, .5, (1, nj, 3))], axis=2) if nj else None
    twists = rng.uniform(-1, 1, (1, nc, 6)) if nc else None
    words, mag = sref.normal_equations(R, ids, sd2, 6, PLATE_INTR, joints, twists, 8)
    A, g = sref.unpack(words[0])
    dead = [c for c in range(12) if (c < 6 and c >= nj) or (c >= 6 and c - 6 >= nc)]
    live = [c for c in range(12) if c not in dead and c != 5]              # link 5 moves with the joints 0 .. 4
    assert not g[dead].any() and not A[dead].any() and not A[:, dead].any() and not mag[0, 94:].any() and not words[0, 94:].any()
    assert (np.diag(A)[live] > 0).all() and g[live].all()


def test_far_pixels_count_in_the_cost_and_not_in_the_system():
    """A mask far from the render: every contour pixel is FAR, [1] is their count times (sqrt(R R + 1))^2 and [2] .. [93] are 0."""
    R, ids, _ = plate(0)
    mask = np.zeros_like(ids)
    mask[0, 0:2, 0:2] = 1
    sd2 = sref.mask_distance(mask, 4)
    words, _ = sref.normal_equations(R, ids, sd2, 1, PLATE_INTR, None, X_TRANSLATION, 4)
    e = (np.sqrt(np.float64(17)) - 0.5) + 0.5
    assert words[0, 0] > 0 and not words[0, 2:].any() and abs(words[0, 1] - words[0, 0] * e * e) <= 1e-9
    # a field made with a larger radius than the call's is truncated by the call
    sd16 = sref.mask_distance(mask, 16)
    again, _ = sref.normal_equations(R, ids, sd16, 1, PLATE_INTR, None, X_TRANSLATION, 4)
    assert np.array_equal(again, words)


def test_the_library_exports_the_two_calls():
    from rope_s3d_amd import build, engine as eng
    lib = eng.load_library()
    assert {'rope_mask_distance', 'rope_silhouette_normal_equations', 'rope_silhouette_normal_workspace'} <= set(eng.ABI_SYMBOLS)
    assert len(lib.rope_mask_distance.argtypes) == 7 and len(lib.rope_silhouette_normal_equations.argtypes) == 19
    assert 'rope_silhouette.hip' in build._SOURCES and 'rope_silhouette.hip' in build._DEPS
    assert lib.rope_silhouette_normal_workspace(3, 90, 160) == 3 * 8 * 96 * 8 and lib.rope_silhouette_normal_workspace(0, 90, 160) == 0
    assert lib.rope_silhouette_normal_workspace(1, 4097, 4096) == 0
