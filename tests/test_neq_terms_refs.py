"""CPU: the frames of tests/neq_terms.py bite, by the references alone.  tests/test_gpu_neq_terms.py compares the kernels with
the references on frames of one and of two inlier pixels, exactly; that says something only if the frames have the inliers they
are meant to have, the special pixels are out, and the values are such that a contracted multiply-add would change them."""
import numpy as np
import pytest

import bundle_ref as bref
import camera_refine_ref as cref
import neq_terms as nt
import refine_ref
import silhouette_ref as sref
from refine_ref import CLIP

MIN_INLIER_SHARE = 0.6


@pytest.fixture(scope='module')
def singles():
    """The 768 single-T frames under the three depth references: name -> (words (768, 32 or 96), share of inlier frames)."""
    s = nt.surface1()
    R, ids, T = nt.single_frames(s)
    rng = np.random.default_rng(31)
    joints, twists = nt.columns(rng, len(R), 3, 6)
    out = {'joints': joints,
           'pose': refine_ref.normal_equations(R, ids, T, 4, nt.INTR1, joints, CLIP)[0],
           'camera': cref.normal_equations(R, ids, T, 4, nt.INTR1, twists, CLIP)[0],
           'bundle': bref.normal_equations(R, ids, T, 4, nt.INTR1, joints, twists, CLIP)[0]}
    return out


@pytest.mark.parametrize('kernel', ['pose', 'camera', 'bundle'])
def test_single_frames_have_one_inlier_or_none_and_the_special_pixels_none(singles, kernel):
    s = nt.surface1()
    words = singles[kernel]
    assert np.isfinite(words).all()
    assert set(np.unique(words[:, 2])) <= {0.0, 1.0} and set(np.unique(words[:, 0])) <= {0.0, 1.0}
    share = float((words[:, 2] == 1).mean())
    print(f"{kernel}: {int((words[:, 2] == 1).sum())} of {len(words)} single-T frames are inliers ({share:.3f})")
    assert share >= MIN_INLIER_SHARE
    for name, ps in s['special'].items():
        for y, x in ps:
            f = y * nt.W1 + x
            assert words[f, 2] == 0 and not words[f, 3:].any(), (name, y, x)
            assert words[f, 0] == (1 if name == 'island' else 0), (name, y, x)        # the island is rendered and measured: BOTH
    if kernel == 'pose':                                                               # the base moves with no joint
        base = np.flatnonzero((s['ids'] == 0).reshape(-1))
        assert not words[base, 2].any() and words[base, 0].all()
    # an inlier frame carries its term in every live word: nothing the comparison looks at is trivially zero
    live = words[words[:, 2] == 1]
    assert (live[:, 3] > 0).all() and (live[:, 1] == live[:, 3]).all()
    A = live[:, 10:31] if kernel != 'bundle' else live[:, 16:94]
    assert (np.count_nonzero(A, axis=1) > 0).all()


def test_pose_column_counts_have_inliers_on_every_link_they_move():
    s = nt.surface1(6)
    R, ids, T = nt.single_frames(s)
    for nj in range(1, 7):
        joints, _ = nt.columns(np.random.default_rng(40 + nj), len(R), nj, 0)
        words = refine_ref.normal_equations(R, ids, T, 6, nt.INTR1, joints, CLIP)[0]
        link = s['ids'].reshape(-1)
        inl = words[:, 2] == 1
        assert set(np.unique(link[inl])) == set(range(1, min(nj, 5) + 1)), nj           # MOVING: 1 <= id <= n_joints
        for j in range(6):                                                             # J_j lives on the links behind joint j alone
            on = words[:, 4 + j] != 0
            assert (link[on] > j).all() and (on.any() == (j < min(nj, 5))), (nj, j)


def test_two_inlier_frames_have_two_inliers_at_every_level_of_the_reduction():
    s = nt.surface2()
    pairs = nt.depth_pairs()
    levels = [nt.level_of(p, q) for p, q in pairs]
    assert all(levels.count(lv) >= 4 for lv in nt.LEVELS), levels
    assert any(q - p == nt.THREADS for p, q in pairs) and all(p < q < nt.H2 * nt.W2 for p, q in pairs)
    R, ids, T = nt.frames_with(s, pairs)
    Ra, ia, Ta = nt.frames_with(s, [(p,) for p, _ in pairs])
    Rb, ib, Tb = nt.frames_with(s, [(q,) for _, q in pairs])
    joints, twists = nt.columns(np.random.default_rng(32), len(pairs), 3, 6)
    for name, run in (('pose', lambda *a: refine_ref.normal_equations(*a, 4, nt.INTR2, joints, CLIP)[0]),
                      ('camera', lambda *a: cref.normal_equations(*a, 4, nt.INTR2, twists, CLIP)[0]),
                      ('bundle', lambda *a: bref.normal_equations(*a, 4, nt.INTR2, joints, twists, CLIP)[0])):
        both, a, b = run(R, ids, T), run(Ra, ia, Ta), run(Rb, ib, Tb)
        assert (both[:, 2] == 2).all() and (a[:, 2] == 1).all() and (b[:, 2] == 1).all(), name
        assert np.isfinite(both).all() and np.array_equal(both, a + b), name           # the reference's own sum is a + b


def test_a_contraction_would_show_on_the_surface_and_not_on_the_hand_planes(singles):
    """(iii): J_0 r and J_0 J_0 with their cross and dot products fused (each a b + c rounded once, exactly) against the contract's one rounding
    per operation.  More than half of the inlier pixels change; on the flat hand plane (z = 2, steps of 2^-5) none can."""
    s = nt.surface1()
    words = singles['pose']
    inlier = np.flatnonzero(words[:, 2] == 1)
    share, plain = nt.fused_share(s, nt.INTR1, singles['joints'][:, 0], inlier)
    assert np.array_equal(plain, words[inlier][:, [4, 10]])                            # the scalar restatement is the reference's terms
    print(f"J_0 r or J_0 J_0 differs from its fused evaluation on {share:.3f} of {len(inlier)} inlier pixels")
    assert share > 0.5
    R, ids, T, joints = refine_ref.hand_planes()
    flat = dict(R=R[1], ids=ids[1], T=T[1])
    t = refine_ref.pixel_terms(R[1], ids[1], T[1], refine_ref.HAND_LINKS, refine_ref.HAND_INTR, joints[1], CLIP)
    inl = np.flatnonzero(t['inlier'].reshape(-1))
    axis = np.tile(joints[1, 0], (R[1].size, 1))            # n = (0, 0, n.z), a = (0, 1, 0): every fused product has a zero partner
    share_flat, _ = nt.fused_share(flat, refine_ref.HAND_INTR, axis, inl)
    assert len(inl) == refine_ref.HAND_FLAT_WORDS[2] and share_flat == 0.0


@pytest.fixture(scope='module')
def sil_singles():
    R, ids, mask = nt.sil_single_frames()
    sd2 = sref.mask_distance(mask[:1], nt.SIL_RADIUS)
    sd2 = np.ascontiguousarray(np.broadcast_to(sd2[0], mask.shape))
    joints, twists = nt.columns(np.random.default_rng(33), len(R), 6, 6)
    return sd2, sref.normal_equations(R, ids, sd2, 6, nt.INTR1, joints, twists, nt.SIL_RADIUS)[0]


def test_silhouette_single_frames_are_one_contour_pixel_each(sil_singles):
    """(iv): a lone rendered pixel is a contour pixel wherever it has a neighbour inside the frame: everywhere on 12 x 16."""
    sd2, words = sil_singles
    assert np.isfinite(words).all() and (words[:, 0] == 1).all()
    near = (np.abs(sd2[0]) <= nt.SIL_RADIUS ** 2).reshape(-1)
    assert np.array_equal(words[:, 2] == 1, near) and set(np.unique(words[:, 2])) <= {0.0, 1.0}
    share = float(near.mean())
    print(f"silhouette: {int(near.sum())} of {len(near)} single-pixel frames are inliers ({share:.3f})")
    assert share >= MIN_INLIER_SHARE
    link = nt.sil_ids(nt.SIL_H, nt.SIL_W).reshape(-1)
    for j in range(6):                                                                 # joint slot j lives on the links behind it alone
        on = words[:, 4 + j] != 0
        assert (link[on] > j).all() and on.any() == (j < 5)
    # the camera block (6.6 .. 11.11) is live wherever the field has a gradient (it has none at the disc's middle)
    assert (np.count_nonzero(words[:, 73:94], axis=1) == 21).sum() >= MIN_INLIER_SHARE * len(words)
    # 1 x 1: the one pixel has no neighbour inside the frame: no contour
    one = sref.normal_equations(np.full((1, 1, 1), 1.9, np.float32), np.zeros((1, 1, 1), np.uint8), np.full((1, 1, 1), 1, np.int32), 6, nt.INTR1,
                                None, np.ones((1, 1, 6)), nt.SIL_RADIUS)[0]
    assert not one.any()


def test_silhouette_two_pixel_frames_have_two_inliers():
    pairs = nt.sil_pairs()
    levels = [nt.level_of(p, q) for p, q in pairs]
    assert all(levels.count(lv) >= 4 for lv in nt.LEVELS), levels
    R, ids, mask = nt.sil_frames_with(pairs)
    sd2 = np.ascontiguousarray(np.broadcast_to(sref.mask_distance(mask[:1], nt.SIL2_RADIUS)[0], mask.shape))
    joints, twists = nt.columns(np.random.default_rng(34), len(pairs), 6, 6)
    run = lambda frames: sref.normal_equations(frames[0], frames[1], sd2, 6, nt.INTR2, joints, twists, nt.SIL2_RADIUS)[0]
    both = run((R, ids))
    a, b = run(nt.sil_frames_with([(p,) for p, _ in pairs])), run(nt.sil_frames_with([(q,) for _, q in pairs]))
    assert (both[:, 0] == 2).all() and (both[:, 2] == 2).all() and (a[:, 2] == 1).all() and (b[:, 2] == 1).all()
    # side by side the two pixels are each other's neighbours, which changes nothing a term is made of: the sum is still a + b
    assert np.isfinite(both).all() and np.array_equal(both, a + b)
