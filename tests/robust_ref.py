"""rope_residual_histogram's and rope_bundle_normal_equations_robust's contracts (include/rope_s3d.h) restated in numpy float64
from the header's text: the histogram pixel by pixel, and the robust words on bundle_ref.pixel_terms — the classification, the
surface and the columns are that file's, the table of weights and cost shares is written out here.  As bundle_ref does, every sum
comes with the sum of the absolute values of its terms, and here with the number of its terms too: what the kernel's sum may differ
by is (n + 8) 2^-52 times the former (tests/test_gpu_robust.py says why).

`occluder_scene` is the behaviour scene of tests/test_robust_refs.py and tests/test_gpu_robust.py: renderer-free planes
(camera_refine_ref.plane_depth) with a patch of the frames a constant 2 cm in front of the surface."""
import numpy as np

import bundle_ref
import camera_refine_ref as cref
from refine_ref import CLIP

RESID_WORDS = 258
BINS = 256
HUBER, TUKEY = 1, 2
KINDS = {'huber': HUBER, 'tukey': TUKEY}
BNEQ_WORDS, SLOTS = bundle_ref.BNEQ_WORDS, bundle_ref.SLOTS


def histogram(R, ids, T, n_links, clip=CLIP):
    """N frames -> (N, 258) uint32."""
    R, ids, T = np.asarray(R), np.asarray(ids, np.uint8), np.asarray(T, np.float32)
    clip = np.float64(np.float32(clip))
    inv = 256.0 / clip
    out = np.zeros((len(R), RESID_WORDS), np.uint32)
    with np.errstate(all='ignore'):
        for f in range(len(R)):
            both = (ids[f] < n_links) & np.isfinite(T[f]) & (T[f] > np.float32(0)) & (T[f] < np.float32(128))
            a = np.abs(R[f].astype(np.float64) - T[f].astype(np.float64))
            within = both & (a <= clip)
            b = np.minimum(255, (a[within] * inv).astype(np.int64))
            out[f, :BINS] = np.bincount(b, minlength=BINS)
            out[f, BINS] = (both & ~within).sum()
            out[f, BINS + 1] = (~both).sum()
    return out


def weights(r, both, clip, kind, scale):
    """The header's table on planes: r (H, W) float64 residuals, both (H, W) bool -> (within, w, cost share), each (H, W)."""
    clip, k = np.float64(np.float32(clip)), np.float64(np.float32(scale))
    with np.errstate(all='ignore'):
        a, r2 = np.abs(r), r * r
        if kind == HUBER:
            within = a <= clip
            w = np.where(a <= k, 1.0, k / a)
            cost = np.where(a <= k, r2, np.where(within, (2.0 * k) * a - k * k, (2.0 * k) * clip - k * k))
        elif kind == TUKEY:
            within = a <= k
            u = r2 / (k * k)
            q = 1.0 - u
            w = q * q
            cost = np.where(within, ((k * k) / 3.0) * (1.0 - (q * q) * q), (k * k) / 3.0)
        else:
            raise ValueError(kind)
    return within & both, np.where(within & both, w, 0.0), np.where(both, cost, 0.0)


def normal_equations(R, ids, T, n_links, intr, joints, twists, clip, kind, scale):
    """N frames -> (sums (N, 96), abs_sums (N, 96), counts (N, 96)): counts[f, w] is the number of terms of word w — the BOTH
    pixels for words 0 and 1, the inliers for every other word."""
    R, ids, T = np.asarray(R), np.asarray(ids), np.asarray(T)
    N = len(R)
    joints = None if joints is None else np.asarray(joints, np.float64).reshape(N, -1, 6)
    twists = None if twists is None else np.asarray(twists, np.float64).reshape(N, -1, 6)
    out, mag, cnt = np.zeros((N, BNEQ_WORDS)), np.zeros((N, BNEQ_WORDS)), np.zeros((N, BNEQ_WORDS))
    clip64 = np.float64(np.float32(clip))
    for f in range(N):
        # the surface, the gates and the columns at the truncation the robust rule keeps (Tukey's inliers are a subset of them)
        t = bundle_ref.pixel_terms(R[f], ids[f], T[f], n_links, intr, None if joints is None else joints[f], None if twists is None else twists[f], clip)
        with np.errstate(all='ignore'):
            r_all = R[f].astype(np.float64) - np.asarray(T[f], np.float32).astype(np.float64)
        within, w, cost = weights(r_all, t['both'], clip64, kind, scale)
        inlier = t['inlier'] & within                                      # both, within, a normal, facing
        with np.errstate(all='ignore'):
            s = np.where(inlier, np.sqrt(w), 0.0)
            v = [np.where(inlier, s * t['J'][c], 0.0) for c in range(SLOTS)] + [np.where(inlier, s * t['r'], 0.0)]
        terms = [t['both'].astype(np.float64), cost, inlier.astype(np.float64), v[SLOTS] * v[SLOTS]]
        terms += [v[c] * v[SLOTS] for c in range(SLOTS)]
        terms += [v[a] * v[b] for a in range(SLOTS) for b in range(a, SLOTS)]
        n_both, n_in = float(t['both'].sum()), float(inlier.sum())
        for k, x in enumerate(terms):
            out[f, k], mag[f, k], cnt[f, k] = x.sum(), np.abs(x).sum(), n_both if k < 2 else n_in
    return out, mag, cnt


def scale_from_histogram(hist, clip, kind):
    """prediction/refinement.py's robust_scale_from_histogram with a plain loop."""
    bins = np.asarray(hist, np.int64).reshape(-1, RESID_WORDS)[:, :BINS].sum(axis=0)
    n = int(bins.sum())
    if n == 0:
        return float(clip)
    run, need = 0, -(-n // 2)
    for b in range(BINS):
        run += int(bins[b])
        if run >= need:
            break
    m = (b + 1) * float(clip) / 256
    s = (1.345 if kind == 'huber' else 4.685) * (1.4826 * m)
    return min(max(s, float(clip) / 128), float(clip))


# ---------------------------------------------------------------------------------------------- the behaviour scene
SCENE_H, SCENE_W = 20, 24
SCENE_INTR = (150.0, 150.0, 11.5, 9.25)
SCENE_POSE = np.array([0.1, -1.5, 0.55, 0.04, -0.07, 0.06])          # the true camera: looks along +y of the world (test_camera_refine_refs.py's)
SCENE_START = SCENE_POSE + np.array([.004, -.003, .005, .003, -.002, .004])      # one lattice step of the camera search off
_NORMALS = np.array([[0.3, 1.0, -0.2], [-0.5, 1.0, 0.1], [0.1, 1.0, 0.6]])
_POINTS = np.array([[0.0, 0.5, 0.5], [0.0, 0.42, 0.5], [0.0, 0.46, 0.5]])
SCENE_SETS = ((0, 1, 2), (2, 0, 1), (1, 2, 0))                        # the planes of a frame; a plane's place in its set is its link id
SCENE_LINKS = 3
SCENE_OCCLUDER = 0.02                                                  # metres in front of the surface: inside CLIP = 2^-5
SCENE_PATCH = (slice(2, 10), slice(3, 12))                            # rows, columns: 72 of 480 pixels, all drawn — a seventh
SCENE_ACTIVE_C = tuple(range(6))


def _world_planes(rows):
    n = _NORMALS[list(rows)] / np.linalg.norm(_NORMALS[list(rows)], axis=1)[:, None]
    return np.concatenate([n, (n * _POINTS[list(rows)]).sum(axis=1)[:, None]], axis=1)


def scene_render(pose):
    """The frames' planes seen from the camera `pose` -> (R (N, H, W) float32, ids (N, H, W) uint8)."""
    from rope_s3d_amd.projection import camera_pose_matrix
    out = [cref.plane_depth(SCENE_H, SCENE_W, SCENE_INTR, *cref.Rwc_t(pose, camera_pose_matrix), _world_planes(s)) for s in SCENE_SETS]
    return np.stack([d.astype(np.float32) for d, _ in out]), np.stack([i for _, i in out])


def scene_twists(pose):
    from rope_s3d_amd.prediction.refinement import camera_twists
    return np.tile(camera_twists(pose)[None], (len(SCENE_SETS), 1, 1))


def occluder_scene():
    """-> (T (N, H, W) float32: what the true camera sees, with T = R - 0.02 on SCENE_PATCH of every frame, the patch (N, H, W) bool)."""
    R, ids = scene_render(SCENE_POSE)
    patch = np.zeros(R.shape, bool)
    patch[(slice(None),) + SCENE_PATCH] = True
    patch &= ids < SCENE_LINKS
    T = R.copy()
    T[patch] = (R[patch].astype(np.float64) - SCENE_OCCLUDER).astype(np.float32)
    return T, patch


def scene_equations(T, kind=None, scale=None, clip=CLIP):
    """bundle_ref.refine's `equations(pose, angles)` on the scene: the plain words (kind None), or the robust ones."""
    def equations(pose, angles):
        R, ids = scene_render(pose)
        if kind is None:
            return bundle_ref.normal_equations(R, ids, T, SCENE_LINKS, SCENE_INTR, None, scene_twists(pose), clip)[0]
        return normal_equations(R, ids, T, SCENE_LINKS, SCENE_INTR, None, scene_twists(pose), clip, KINDS[kind], scale)[0]
    return equations


def scene_refine(T, kind=None, scale=None, iterations=5):
    """bundle_ref.refine from SCENE_START in 'frame' mode with no joint refined: the camera's six parameters on the pooled frames."""
    limits = np.tile([-3.0, 3.0], (6, 1))
    return bundle_ref.refine(SCENE_START, np.zeros((len(SCENE_SETS), 6)), scene_equations(T, kind, scale), limits, 'frame', (), SCENE_ACTIVE_C,
                             iterations, 1e-3)


def scene_auto_scale(T, kind):
    """The scale BundleRefiner(robust_scale='auto') fixes at SCENE_START, as the float32 the kernel is handed."""
    R, ids = scene_render(SCENE_START)
    return float(np.float32(scale_from_histogram(histogram(R, ids, T, SCENE_LINKS, CLIP), CLIP, kind)))


def pose_error(pose):
    """How far a camera pose is from the scene's true one: the norm over the six parameters (metres and radians alike)."""
    return float(np.linalg.norm(np.asarray(pose, np.float64) - SCENE_POSE))
