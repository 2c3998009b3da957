"""CPU: the robust weights of the bundle polish held by the references alone — robust_scale_from_histogram worked by hand, the
numpy restatement of rope_bundle_normal_equations_robust (tests/robust_ref.py) against bundle_ref at the scale where the two must
agree exactly, what BundleRefiner refuses, the three exports, and what the weights are for: a scene with an occluder inside the
truncation, polished on the plain and on the robust words."""
import os
import re

import numpy as np
import pytest

import bundle_ref as bref
import robust_ref as rref
from refine_ref import CLIP, HAND_INTR, HAND_LINKS, hand_planes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
SYMBOLS = ('rope_residual_histogram', 'rope_bundle_normal_equations_robust', 'rope_bundle_normal_workspace_robust')


def _hist(**bins):
    h = np.zeros(258, np.uint32)
    for b, c in bins.items():
        h[int(b[1:])] = c
    return h


def test_scale_from_histogram_worked_by_hand():
    """clip = 2^-5, so a bin is 2^-13 m wide.  Counts 5 in bin 3 and 4 in bin 10: n = 9, ceil(n / 2) = 5 is reached in bin 3, the
    median 4 x 2^-13, sigma = 1.4826 x that.  Words 256 and 257 do not count."""
    from rope_s3d_amd.prediction.refinement import robust_scale_from_histogram as scale
    w = 2.0 ** -13
    h = _hist(b3=5, b10=4, b256=1000, b257=5000)
    assert scale(h, CLIP, 'huber') == 1.345 * (1.4826 * (4 * w)) and scale(h, CLIP, 'tukey') == 4.685 * (1.4826 * (4 * w))
    # 4 and 4: ceil(8 / 2) = 4 is reached in bin 3 still; 4 and 5: ceil(9 / 2) = 5 only in bin 10
    assert scale(_hist(b3=4, b10=4), CLIP, 'huber') == 1.345 * (1.4826 * (4 * w))
    assert scale(_hist(b3=4, b10=5), CLIP, 'huber') == 1.345 * (1.4826 * (11 * w))
    # frames are pooled before the median is taken: (N, 258)
    assert scale(np.stack([_hist(b3=2, b10=4), _hist(b3=3)]), CLIP, 'tukey') == 4.685 * (1.4826 * (4 * w))
    # nothing within clip: the scale is clip
    assert scale(_hist(b256=7, b257=9), CLIP, 'huber') == CLIP and scale(np.zeros((0, 258), np.uint32), CLIP, 'tukey') == CLIP
    # the floor, two bin widths: a perfect fit, everything in bin 0, gives 1.345 x 1.4826 x 1 bin = 1.99 bins
    assert scale(_hist(b0=100), CLIP, 'huber') == CLIP / 128 == 2 * w
    assert scale(_hist(b0=100), CLIP, 'tukey') == 4.685 * (1.4826 * w) > CLIP / 128
    # the ceiling: a median in bin 200 gives 1.99 x 201 bins for Huber, above the 256 of clip
    assert scale(_hist(b200=3), CLIP, 'huber') == CLIP and scale(_hist(b40=3), CLIP, 'tukey') == CLIP
    assert scale(_hist(b100=3), CLIP, 'huber') == 1.345 * (1.4826 * (101 * w)) < CLIP
    for kind in ('huber', 'tukey'):                                        # and the plain loop of robust_ref says the same
        for h in (_hist(b3=5, b10=4), _hist(b0=100), _hist(b200=3), _hist(b256=7), _hist(b17=1, b18=1, b90=1)):
            assert scale(h, CLIP, kind) == rref.scale_from_histogram(h, CLIP, kind)
    with pytest.raises(ValueError):
        scale(h, CLIP, 'cauchy')
    with pytest.raises(ValueError):
        scale(np.zeros(256), CLIP, 'huber')
    with pytest.raises(ValueError):
        scale(h, 0.0, 'huber')


def test_reference_histogram_on_the_hand_planes():
    """Frame 1 of hand_planes: 23 x 20 = 460 pixels, 409 BOTH (refine_ref.HAND_FLAT_WORDS); of them 405 have r = 0 (bin 0), two
    |r| = clip exactly (bin min(255, 256) = 255) and two lie 2^-22 beyond clip (word 256)."""
    R, ids, T, _ = hand_planes()
    h = rref.histogram(R, ids, T, HAND_LINKS, CLIP)
    assert h.shape == (3, 258) and h.dtype == np.uint32 and (h.sum(axis=1) == 20 * 23).all()
    assert h[1, 0] == 405 and h[1, 255] == 2 and h[1, 256] == 2 and h[1, 257] == 460 - 409 and h[1, 1:255].sum() == 0
    # frame 0: T = R + 2^-8 on the even columns: |r| = 2^-8 = 32 bins exactly, up to the rounding of R + 2^-8 in float32
    assert h[0, 0] >= 20 * 11 - 1 and h[0, 31:33].sum() >= 20 * 12 - 1


def test_huber_at_scale_clip_is_the_plain_reference_exactly_and_smaller_scales_are_not():
    R, ids, T, joints = hand_planes()
    tw = np.random.default_rng(4).uniform(-1, 1, (3, 6, 6))
    plain, pmag = bref.normal_equations(R, ids, T, HAND_LINKS, HAND_INTR, joints, tw, CLIP)
    got, mag, cnt = rref.normal_equations(R, ids, T, HAND_LINKS, HAND_INTR, joints, tw, CLIP, rref.HUBER, CLIP)
    assert got.tobytes() == plain.tobytes() and mag.tobytes() == pmag.tobytes()
    assert np.array_equal(cnt[:, 0], plain[:, 0]) and np.array_equal(cnt[:, 5], plain[:, 2])
    for kind in (rref.HUBER, rref.TUKEY):
        w4, _, _ = rref.normal_equations(R, ids, T, HAND_LINKS, HAND_INTR, joints, tw, CLIP, kind, CLIP / 4)
        assert np.array_equal(w4[:, [0, 94, 95]], plain[:, [0, 94, 95]])
        assert (w4[:, 1] <= plain[:, 1]).all() and (w4[1, 1] < plain[1, 1]) and (w4[:, 3] <= plain[:, 3]).all()
        # Tukey's inliers end at the scale: the two pixels of frame 1 at |r| = clip leave; Huber keeps them at weight 1 / 4
        assert w4[1, 2] == plain[1, 2] - (2 if kind == rref.TUKEY else 0)
    h4, _, _ = rref.normal_equations(R, ids, T, HAND_LINKS, HAND_INTR, joints, tw, CLIP, rref.HUBER, CLIP / 4)
    # frame 1 by hand: r = 0 but two pixels at |r| = clip = 4 k (w = 1 / 4: w r^2 = clip^2 / 4 each, cost 2 k clip - k^2 = 7 clip^2 / 16) and two
    # beyond (cost the same 7 clip^2 / 16)
    assert h4[1, 3] == 2 * CLIP * CLIP / 4 and h4[1, 1] == 4 * 7 * CLIP * CLIP / 16


def test_the_refiner_refuses_what_is_not_built():
    from types import SimpleNamespace
    from rope_s3d_amd.prediction.refinement import BundleRefineResult, BundleRefiner
    intr = SimpleNamespace(fx=150.0, fy=150.0, cx=11.5, cy=9.25)
    engine = SimpleNamespace(n_links=6, device=0)
    ok = BundleRefiner(engine, intr, robust='huber')
    assert ok.robust == 'huber' and ok.robust_scale == 'auto'
    assert BundleRefiner(engine, intr, robust='tukey', robust_scale=0.01).robust_scale == 0.01
    assert BundleRefiner(engine, intr).robust is None
    for bad in (dict(robust='huber', native=True), dict(robust='tukey', silhouette=1.0), dict(robust='cauchy'), dict(robust='huber', robust_scale=0.0),
                dict(robust='huber', robust_scale=2 * CLIP), dict(robust='huber', robust_scale=float('nan')), dict(robust='huber', robust_scale='median')):
        with pytest.raises(ValueError):
            BundleRefiner(engine, intr, **bad)
    assert np.isnan(BundleRefineResult.__dataclass_fields__['robust_scale'].default)


def test_symbols_are_declared_listed_and_exported_and_the_file_is_built():
    from rope_s3d_amd import build, engine as eng
    hdr = open(os.path.join(ROOT, 'include', 'rope_s3d.h')).read()
    lib = eng.load_library()
    for name, n_args in zip(SYMBOLS, (10, 21, 3)):
        assert re.search(r'\b(?:int|size_t) ' + name + r'\(', hdr), name
        assert name in eng.ABI_SYMBOLS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args, name
    assert '#define ROPE_RESID_WORDS 258' in hdr and '#define ROPE_ROBUST_HUBER 1' in hdr and '#define ROPE_ROBUST_TUKEY 2' in hdr
    assert eng.RESID_WORDS == 258 and eng.ROBUST_KINDS == {'huber': 1, 'tukey': 2}
    assert 'rope_robust.hip' in build._SOURCES and 'rope_robust.hip' in build._DEPS
    with open(os.path.join(build._CSRC, 'rope_robust.hip')) as f:
        text = f.read()
    assert '#include "rope_neq.h"' in text and 'bneq_pack_and_own_words' in text and 'neq_gather<ROPE_BNEQ_WORDS>' in text
    assert not re.search(r'atomicAdd\s*\(\s*\(?\s*(?:float|double)', text) and 'unsafeAtomicAdd' not in text


def test_an_occluder_inside_the_truncation_pulls_the_plain_polish_and_the_robust_one_less():
    """robust_ref's scene: three frames of 20 x 24 with three tilted planes each (1 440 drawn pixels), seen by the true camera, and
    on 216 of them — 3 x 72, a seventh of the drawn pixels — the frame lies 2 cm in front of the surface, inside clip = 31 mm.  All
    six camera parameters are polished from one lattice step off (|error| 8.888e-3 over the six parameters), five rounds.

    By the references alone (bundle_ref.refine on bundle_ref's and on robust_ref's words):
        plain                               ends at |error| 7.504e-2 — the patch drags the camera further off than it started
        Huber, auto scale 4.138 mm          ends at |error| 2.368e-2: 3.2 times closer than plain
        Tukey, auto scale 14.41 mm          ends at |error| 6.414e-6: the patch, at 20 mm, is beyond the scale and carries nothing
    """
    T, patch = rref.occluder_scene()
    drawn = (rref.scene_render(rref.SCENE_POSE)[1] < rref.SCENE_LINKS).sum()
    assert patch.sum() == 216 and 6 * patch.sum() <= drawn <= 8 * patch.sum()
    start = rref.pose_error(rref.SCENE_START)
    plain = rref.scene_refine(T)
    e_plain = rref.pose_error(plain['pose'])
    print(f"start {start:.6e}; plain: {plain['steps_taken']} steps, |error| {e_plain:.6e}")
    assert plain['steps_taken'] >= 1
    for kind in ('huber', 'tukey'):
        k = rref.scene_auto_scale(T, kind)
        res = rref.scene_refine(T, kind, k)
        e = rref.pose_error(res['pose'])
        print(f"{kind}: scale {k:.6e} m, {res['steps_taken']} steps, cost {res['costs'][0]:.6e} -> {res['costs'][-1]:.6e}, |error| {e:.6e}, "
              f"least relative margin {(res['margins'] / res['costs'][:-1]).min():.3e}")
        assert CLIP / 128 <= k < CLIP and res['steps_taken'] >= 1 and (np.diff(res['costs']) <= 0).all()
        assert e < e_plain and 2 * e <= e_plain                            # strictly closer, and by the factor the scene was chosen for
    # without the occluder the three agree: the weights cost nothing on clean frames
    clean = rref.scene_render(rref.SCENE_POSE)[0]
    e_clean = [rref.pose_error(rref.scene_refine(clean, kind, None if kind is None else rref.scene_auto_scale(clean, kind))['pose'])
               for kind in (None, 'huber', 'tukey')]
    print('clean frames: |error| plain, huber, tukey', e_clean)
    assert max(e_clean) < 0.05 * start


class _ReferenceEngine:
    """What BundleRefiner asks of an Engine, answered by the references on numpy planes."""
    n_links, device = rref.SCENE_LINKS, 0

    def bundle_normal_equations(self, rd, ri, T, axes, twists, n_links, clip, intr):
        return bref.normal_equations(rd, ri, T, n_links, intr, axes, twists, clip)[0]

    def bundle_normal_equations_robust(self, rd, ri, T, axes, twists, n_links, clip, intr, kind, scale):
        return rref.normal_equations(rd, ri, T, n_links, intr, axes, twists, clip, rref.KINDS[kind], scale)[0]

    def residual_histogram(self, rd, ri, T, n_links, clip):
        return rref.histogram(rd, ri, T, n_links, clip)


@pytest.mark.parametrize('kind', [None, 'huber', 'tukey'])
def test_the_refiners_host_loop_on_the_weighted_words_is_the_reference_loop(monkeypatch, kind):
    """BundleRefiner's own loop, scale and result on the scene, with the references in the engine's place: the host half adds
    nothing of its own, so every field equals bundle_ref.refine's byte for byte; the scale is fixed once, at the start pose."""
    from types import SimpleNamespace
    from rope_s3d_amd.prediction import refinement as rf
    renders = []
    monkeypatch.setattr(rf, '_render_under', lambda e, intr, pose, angles, n_links: renders.append(np.array(pose)) or rref.scene_render(pose))
    monkeypatch.setattr(rf, '_stage_depth', lambda e, depth, N: depth)
    fx, fy, cx, cy = rref.SCENE_INTR
    T, _ = rref.occluder_scene()
    got = rf.BundleRefiner(_ReferenceEngine(), SimpleNamespace(fx=fx, fy=fy, cx=cx, cy=cy), do_angles='', robust=kind).refine(
        rref.SCENE_START, np.zeros((len(rref.SCENE_SETS), 6)), T)
    k = None if kind is None else rref.scene_auto_scale(T, kind)
    want = rref.scene_refine(T, kind, k)
    assert (np.isnan(got.robust_scale) if kind is None else got.robust_scale == k)
    assert len(renders) == (6 if kind is None else 7) and np.array_equal(renders[0], rref.SCENE_START)
    for name in ('pose', 'sigma_pose', 'cost_before', 'cost_after', 'steps_taken', 'inliers', 'frame_cost'):
        g, w = np.asarray(getattr(got, name), np.float64), np.asarray(want[name], np.float64)
        assert g.tobytes() == w.tobytes(), (name, g, w)
