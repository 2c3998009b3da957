"""GPU: the per-pixel TERMS of rope_pose_normal_equations, rope_camera_normal_equations (csrc/rope_refine.hip),
rope_bundle_normal_equations (csrc/rope_bundle.hip) and rope_silhouette_normal_equations (csrc/rope_silhouette.hip) against their
numpy restatements, EXACTLY — the header's "one correctly rounded IEEE operation per written operation, in the order written".

The other tests of these kernels allow 4 n eps sum|terms| for the order of the summation, which the header leaves free; a term that
is an ulp off on every pixel hides in that.  Here every frame has one inlier pixel, so its sums are that pixel's terms, or two, so
its sums are a + b in either order (tests/neq_terms.py): no bound, no eps, and nothing assumed about the order.  The values are
generic (a curved surface, camera terms, axes and twists that are no dyadic numbers); tests/test_neq_terms_refs.py shows by the
references alone that the frames have the inliers they should and that a contracted multiply-add would change the terms.

Values are compared, not bits: a term of -0.0 sums to +0.0 on both sides.  A NaN anywhere fails."""
import numpy as np
import pytest

import bundle_ref as bref
import camera_refine_ref as cref
import neq_terms as nt
import refine_ref
import silhouette_ref as sref
from refine_ref import CLIP
from test_gpu_bundle import COMBOS as BUNDLE_COMBOS, _call as bundle_call
from test_gpu_camera_refine import _call as camera_call
from test_gpu_refine import _call as pose_call
from test_gpu_silhouette import COMBOS as SIL_COMBOS, _call as sil_call

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    """Every word of every frame the same value; the reference finite first."""
    assert np.isfinite(want).all(), what
    assert got.shape == want.shape, what
    bad = np.argwhere(~(got == want))                                  # a NaN of the kernel is unequal to everything
    print(f"{what}: {len(got)} frames, {int((want[:, 2] >= 1).sum())} with inliers, {got.shape[1]} words each; {len(bad)} words differ")
    assert len(bad) == 0, (what, bad[:8], [(got[f, w].hex(), want[f, w].hex()) for f, w in bad[:8]])
    assert np.array_equal(got, want)


@pytest.fixture(scope='module')
def frames1():
    return {stripes: nt.single_frames(nt.surface1(stripes)) for stripes in (4, 6)}


# ---------------------------------------------------------------------------------------------- one inlier a frame
@pytest.mark.parametrize('n_links,n_joints', [(4, 3)] + [(6, nj) for nj in range(1, 7)])
def test_pose_kernel_single_inlier_frames_are_the_references_terms(frames1, n_links, n_joints):
    """768 frames of 24 x 32, frame f with T at pixel f alone.  n_links 4: links 0 .. 3 and joints 0 .. 2; n_links 6: links 0 .. 5
    under every count of joints, so `j < n_joints && j < id` and `id <= n_joints` see both sides of every edge."""
    R, ids, T = frames1[n_links]
    joints, _ = nt.columns(np.random.default_rng(100 + 10 * n_links + n_joints), len(R), n_joints, 0)
    want = refine_ref.normal_equations(R, ids, T, n_links, nt.INTR1, joints, CLIP)[0]
    rc, got = pose_call(R, ids, T, joints, n_links, nt.INTR1)
    assert rc == 0
    assert set(np.unique(want[:, 2])) == {0.0, 1.0}
    _same(got, want, f"pose, {n_links} links, {n_joints} joints")


@pytest.mark.parametrize('n_cols', [1, 3, 6])
def test_camera_kernel_single_inlier_frames_are_the_references_terms(frames1, n_cols):
    R, ids, T = frames1[4]
    _, twists = nt.columns(np.random.default_rng(200 + n_cols), len(R), 0, n_cols)
    want = cref.normal_equations(R, ids, T, 4, nt.INTR1, twists, CLIP)[0]
    rc, got = camera_call(R, ids, T, twists, 4, nt.INTR1)
    assert rc == 0
    assert set(np.unique(want[:, 2])) == {0.0, 1.0}
    _same(got, want, f"camera, {n_cols} columns")


@pytest.mark.parametrize('n_links,nj,nc', [(4,) + c for c in BUNDLE_COMBOS] + [(6, 6, 6)])
def test_bundle_kernel_single_inlier_frames_are_the_references_terms(frames1, n_links, nj, nc):
    R, ids, T = frames1[n_links]
    joints, twists = nt.columns(np.random.default_rng(300 + 100 * n_links + 10 * nj + nc), len(R), nj, nc)
    want = bref.normal_equations(R, ids, T, n_links, nt.INTR1, joints, twists, CLIP)[0]
    rc, got = bundle_call(R, ids, T, joints, twists, n_links, nt.INTR1)
    assert rc == 0
    assert set(np.unique(want[:, 2])) == {0.0, 1.0}
    _same(got, want, f"bundle, {n_links} links, {nj} joints, {nc} columns")


@pytest.fixture(scope='module')
def sil1():
    R, ids, mask = nt.sil_single_frames()
    sd2 = np.ascontiguousarray(np.broadcast_to(sref.mask_distance(mask[:1], nt.SIL_RADIUS)[0], mask.shape))
    return R, ids, sd2


@pytest.mark.parametrize('nj,nc', SIL_COMBOS)
def test_silhouette_kernel_single_pixel_frames_are_the_references_terms(sil1, nj, nc):
    """192 frames of 12 x 16, frame f with pixel f alone rendered: one contour pixel, its gradient the field's alone."""
    R, ids, sd2 = sil1
    joints, twists = nt.columns(np.random.default_rng(400 + 10 * nj + nc), len(R), nj, nc)
    want = sref.normal_equations(R, ids, sd2, 6, nt.INTR1, joints, twists, nt.SIL_RADIUS)[0]
    rc, got = sil_call(R, ids, sd2, joints, twists, 6, nt.INTR1, nt.SIL_RADIUS)
    assert rc == 0
    assert (want[:, 0] == 1).all() and set(np.unique(want[:, 2])) == {0.0, 1.0}
    _same(got, want, f"silhouette, {nj} joints, {nc} columns")


# ---------------------------------------------------------------------------------------------- two inliers a frame
def _two(run, frames_of, pairs, what):
    """The kernel and the reference on the frames of the pairs, and the reference on each pixel alone: all three a + b."""
    both = frames_of(pairs)
    want = run('ref', both)
    a, b = run('ref', frames_of([(p,) for p, _ in pairs])), run('ref', frames_of([(q,) for _, q in pairs]))
    assert (want[:, 2] == 2).all() and (a[:, 2] == 1).all() and (b[:, 2] == 1).all(), what
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.array_equal(want, a + b), what
    got = run('gpu', both)
    _same(got, a + b, what)
    _same(got, want, what)
    levels = [nt.level_of(p, q) for p, q in pairs]
    for lv in nt.LEVELS:
        assert levels.count(lv) >= 4, (what, lv)


@pytest.mark.parametrize('kernel,nj,nc', [('pose', 3, 0), ('pose', 6, 0), ('camera', 0, 6), ('bundle', 3, 6), ('bundle', 6, 6)])
def test_depth_kernels_two_inlier_frames_are_a_plus_b(kernel, nj, nc):
    """47 x 45 = 2115 pixels, two workgroups a frame; the two pixels meet in one wave, in two waves of a pass, in two passes of one
    thread and of two, and in two workgroups."""
    s = nt.surface2()
    pairs = nt.depth_pairs()
    joints, twists = nt.columns(np.random.default_rng(500 + 10 * nj + nc), len(pairs), nj, nc)

    def run(side, fr):
        R, ids, T = fr
        if kernel == 'pose':
            out = refine_ref.normal_equations(R, ids, T, 4, nt.INTR2, joints, CLIP)[0] if side == 'ref' else pose_call(R, ids, T, joints, 4, nt.INTR2)
        elif kernel == 'camera':
            out = cref.normal_equations(R, ids, T, 4, nt.INTR2, twists, CLIP)[0] if side == 'ref' else camera_call(R, ids, T, twists, 4, nt.INTR2)
        else:
            out = (bref.normal_equations(R, ids, T, 4, nt.INTR2, joints, twists, CLIP)[0] if side == 'ref' else
                   bundle_call(R, ids, T, joints, twists, 4, nt.INTR2))
        if side == 'gpu':
            assert out[0] == 0
            return out[1]
        return out

    _two(run, lambda ps: nt.frames_with(s, ps), pairs, f"{kernel}, {nj} joints, {nc} columns, two inliers")


@pytest.mark.parametrize('nj,nc', [(3, 6), (6, 6), (6, 0)])
def test_silhouette_kernel_two_pixel_frames_are_a_plus_b(nj, nc):
    pairs = nt.sil_pairs()
    joints, twists = nt.columns(np.random.default_rng(600 + 10 * nj + nc), len(pairs), nj, nc)
    sd2_one = sref.mask_distance(nt.disc_mask(nt.H2, nt.W2, nt.SIL2_DISC)[None], nt.SIL2_RADIUS)[0]

    def run(side, fr):
        R, ids, _ = fr
        sd2 = np.ascontiguousarray(np.broadcast_to(sd2_one, R.shape))
        if side == 'ref':
            return sref.normal_equations(R, ids, sd2, 6, nt.INTR2, joints, twists, nt.SIL2_RADIUS)[0]
        rc, out = sil_call(R, ids, sd2, joints, twists, 6, nt.INTR2, nt.SIL2_RADIUS)
        assert rc == 0
        return out

    _two(run, nt.sil_frames_with, pairs, f"silhouette, {nj} joints, {nc} columns, two inliers")


# ---------------------------------------------------------------------------------------------- the shared gather and pack bodies
@pytest.mark.parametrize('kernel', ['bundle', 'silhouette'])
def test_twelve_slot_kernels_on_three_frames_of_two_workgroups(kernel):
    """Three frames of 47 x 45: two workgroups a frame, and the gather kernel's last workgroup holds one frame of its two (the pose
    and camera kernels meet both in tests/test_gpu_refine.py and tests/test_gpu_camera_refine.py).  The two-inlier frames of the
    tests above, the first, the middle and the last pair; bit for bit against the reference."""
    pairs = nt.depth_pairs() if kernel == 'bundle' else nt.sil_pairs()
    pairs = [pairs[0], pairs[len(pairs) // 2], pairs[-1]]
    joints, twists = nt.columns(np.random.default_rng(700), 3, 6, 6)
    if kernel == 'bundle':
        R, ids, T = nt.frames_with(nt.surface2(), pairs)
        want = bref.normal_equations(R, ids, T, 4, nt.INTR2, joints, twists, CLIP)[0]
        rc, got = bundle_call(R, ids, T, joints, twists, 4, nt.INTR2)
    else:
        R, ids, _ = nt.sil_frames_with(pairs)
        sd2 = np.ascontiguousarray(np.broadcast_to(sref.mask_distance(nt.disc_mask(nt.H2, nt.W2, nt.SIL2_DISC)[None], nt.SIL2_RADIUS)[0], R.shape))
        want = sref.normal_equations(R, ids, sd2, 6, nt.INTR2, joints, twists, nt.SIL2_RADIUS)[0]
        rc, got = sil_call(R, ids, sd2, joints, twists, 6, nt.INTR2, nt.SIL2_RADIUS)
    assert rc == 0 and len(R) == 3 and R.shape[1] * R.shape[2] > 2048
    assert (want[:, 2] == 2).all()
    _same(got, want, f"{kernel}, three frames of two workgroups")
