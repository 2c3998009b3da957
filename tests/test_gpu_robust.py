"""GPU: rope_residual_histogram and rope_bundle_normal_equations_robust (csrc/rope_robust.hip; Engine.residual_histogram,
Engine.bundle_normal_equations_robust) against the numpy restatement of their contracts (tests/robust_ref.py) and against
rope_bundle_normal_equations on the same planes, what they refuse, and BundleRefiner(robust=...) on the occluder scene of
tests/test_robust_refs.py.

The shapes: 47 x 45 (2 115 pixels: a full chunk of 2 048 and one of 67, rows that split across waves), three frames (the gather
takes two a workgroup), 1 x 1, and refine_ref's hand planes.  On top of the 47 x 45 frames lie, by hand, residuals exactly at a bin
edge of the histogram, exactly at the scale k = clip / 4, exactly at clip and one float32 step beyond it; the surface brings every
refine_ref.BAD_T and an id that is no link.

The bound.  The kernel's words and the reference's are sums of the SAME products (s x)(s y), s = sqrt(w), when the device's square
root is correctly rounded; where it were one unit off, s x carries one more rounding error and a product two, 2 x 2^-52 of its
size to first order.  A sum of n terms added in any order is within (n - 1) 2^-53 sum|terms| of the exact sum, two orders within
(n - 1) 2^-52.  (n + 8) 2^-52 sum|terms| covers both with the second-order terms; n is the word's own count of terms.  Derived, not
measured.  The counts, words 0, 2, 94 and 95, are exact."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import bundle_ref as bref
import neq_terms
import robust_ref as rref
from refine_ref import BAD_T, CLIP, HAND_INTR, HAND_LINKS, hand_planes

pytestmark = pytest.mark.gpu

E_ARG = -1
EPS = 2.0 ** -52
GARBAGE = float(np.frombuffer(b'\x5a' * 8, np.float64)[0])
K4 = CLIP / 4                                        # the scale of the weighted cases
BIN_EDGE = 8 * CLIP / 256                            # |r| = 2^-10: the lower edge of bin 8
BEYOND = CLIP + 2.0 ** -22                           # one float32 step of a depth in [1, 2) above clip: 2^-23 would do, 2^-22 as hand_planes
OVERLAY = (BIN_EDGE, K4, CLIP, BEYOND)


@pytest.fixture(scope='module')
def engine():
    e = eng.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def frames():
    """Three frames of neq_terms.surface2 (47 x 45, links 0 .. 3 in stripes, an island, a pixel of id 4, a hole, every BAD_T), each
    with its own noise within 0.03 m, and on plain pixels of every frame T = R - d for d in OVERLAY (r = +d) and, eight rows below,
    T = R + d (r = -d) -> dict(R, ids, T, joints, twists, where: the overlay's pixels)."""
    s = neq_terms.surface2()
    H, W = s['R'].shape
    R = np.ascontiguousarray(np.broadcast_to(s['R'], (3, H, W)))
    ids = np.ascontiguousarray(np.broadcast_to(s['ids'], (3, H, W)))
    rng = np.random.default_rng(77)
    T = (R.astype(np.float64) + rng.uniform(-neq_terms.NOISE, neq_terms.NOISE, R.shape)).astype(np.float32)
    y, x = s['special']['bad'][0]
    T[:, y, x:x + len(BAD_T)] = np.array(BAD_T, np.float32)
    where = []
    for f in range(3):
        for i, d in enumerate(OVERLAY):
            for sign, row in ((-1, 25 + f), (+1, 33 + f)):
                px = (row, 3 + 9 * i + f)                                  # a plain pixel of another stripe each, away from the special ones
                T[f, px[0], px[1]] = np.float32(np.float64(R[f, px[0], px[1]]) + sign * d)
                where.append((f,) + px + (-sign * d,))
    joints, twists = neq_terms.columns(np.random.default_rng(78), 3, 3, 6)
    return dict(R=R, ids=ids, T=T, joints=joints, twists=twists, where=where, intr=neq_terms.INTR2, n_links=4)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def test_the_overlay_is_what_it_says(frames):
    """By the references alone: the residuals laid on top are exact, and land in the bin, at the scale, at clip and beyond it."""
    R, T, ids = frames['R'], frames['T'], frames['ids']
    for f, y, x, r in frames['where']:
        assert np.float64(R[f, y, x]) - np.float64(T[f, y, x]) == r and ids[f, y, x] < 4, (f, y, x, r)
    h = rref.histogram(R, ids, T, 4, CLIP)
    quiet = rref.histogram(R, ids, np.where(np.isin(np.abs(R.astype(np.float64) - T), OVERLAY), R, T), 4, CLIP)
    for f in range(3):
        d = h[f].astype(np.int64) - quiet[f].astype(np.int64)              # against the same frame with the overlay at r = 0
        assert d[8] == 2 and d[64] == 2 and d[255] == 2 and d[256] == 2 and d[0] == -8 and d[257] == 0, np.flatnonzero(d)
        assert h[f, 257] >= 4 + len(BAD_T) + 1                             # the hole, every BAD_T, the pixel of id 4


def _hist_call(R, ids, T, n_links, clip=CLIP, odd=False, null=None, n_frames=None, hw=None):
    """The C entry point on an output filled with garbage -> (rc, hist (N, 258) uint32)."""
    lib = eng.load_library()
    N, H, W = R.shape
    t = _dev(R, ids, T)
    out = torch.full((N * 258 + 2,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    ptrs = [x.data_ptr() for x in t] + [out.data_ptr() + (2 if odd else 0)]
    ptrs = [None if k == null else C.c_void_p(p) for k, p in enumerate(ptrs)]
    H, W = hw if hw is not None else (H, W)
    rc = lib.rope_residual_histogram(ptrs[0], ptrs[1], ptrs[2], N if n_frames is None else n_frames, H, W, n_links, clip, ptrs[3],
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[N * 258:] == 0x5a5a5a5a).all()                             # nothing written past the words
    return rc, got[:N * 258].reshape(N, 258)


def test_histogram_is_the_reference_and_does_not_depend_on_the_batch(engine, frames):
    R, ids, T = frames['R'], frames['ids'], frames['T']
    want = rref.histogram(R, ids, T, 4, CLIP)
    rc, got = _hist_call(R, ids, T, 4)
    assert rc == 0 and got.dtype == np.uint32 and np.array_equal(got, want), np.argwhere(got != want)
    assert (got.sum(axis=1) == 47 * 45).all()
    t = _dev(R, ids, T)
    whole = engine.residual_histogram(*t, 4, CLIP)
    assert whole.shape == (3, 258) and whole.dtype == np.uint32 and whole.tobytes() == want.tobytes()
    parts = [engine.residual_histogram(*(x[a:b].contiguous() for x in t), 4, CLIP) for a, b in ((0, 1), (1, 3))]
    assert np.concatenate(parts).tobytes() == whole.tobytes() == engine.residual_histogram(*t, 4, CLIP).tobytes()
    assert engine.residual_histogram(*(x[:0] for x in t), 4, CLIP).shape == (0, 258)
    # another truncation moves the bins: clip / 2 puts |r| = clip / 4 at the edge of bin 128 and the pixels at clip beyond it
    half = engine.residual_histogram(*t, 4, CLIP / 2)
    assert np.array_equal(half, rref.histogram(R, ids, T, 4, CLIP / 2)) and (half.sum(axis=1) == 47 * 45).all()
    # the hand planes (NaN, inf, 0, 128, negative depths, ids 4 and 255) and 1 x 1: a pixel both, one not, one beyond
    Rh, Ih, Th, _ = hand_planes()
    th = _dev(Rh, Ih, Th)
    got = engine.residual_histogram(*th, HAND_LINKS, CLIP)
    assert np.array_equal(got, rref.histogram(Rh, Ih, Th, HAND_LINKS, CLIP)) and (got.sum(axis=1) == 20 * 23).all() and got[1, 255] == 2
    R1 = np.array([2.0, 2.0, 2.0, np.nan], np.float32).reshape(4, 1, 1)
    T1 = np.array([2.0, 0.0, 2.5, 2.0], np.float32).reshape(4, 1, 1)
    got = engine.residual_histogram(*_dev(R1, np.zeros((4, 1, 1), np.uint8), T1), 1, CLIP)
    assert np.array_equal(np.argwhere(got)[:, 1], [0, 257, 256, 256]) and (got.sum(axis=1) == 1).all()       # a NaN residual: word 256


def _call(p, kind, scale, clip=CLIP, frames=slice(None), odd=None, null=None, plain=False, **over):
    """rope_bundle_normal_equations_robust (or, plain=True, rope_bundle_normal_equations) on an out buffer filled with garbage ->
    (rc, out (N, 96)).  Pointers by position: 0 render, 1 ids, 2 frames, 3 joints, 4 twists, 5 out, 6 work."""
    lib = eng.load_library()
    R, ids, T, joints, twists = (p[k][frames] for k in ('R', 'ids', 'T', 'joints', 'twists'))
    N, H, W = R.shape
    t = _dev(R, ids, T, joints, twists)
    out = torch.full((N, 96), GARBAGE, dtype=torch.float64, device='cuda')
    work = torch.full((max(1, lib.rope_bundle_normal_workspace_robust(N, H, W) // 8) + 1,), GARBAGE, dtype=torch.float64, device='cuda')
    ptrs = [x.data_ptr() for x in t] + [out.data_ptr(), work.data_ptr()]
    if odd is not None:
        ptrs[odd] += 2
    ptrs = [None if k == null else C.c_void_p(v) for k, v in enumerate(ptrs)]
    head = (ptrs[0], ptrs[1], ptrs[2], over.get('n_frames', N), H, W, over.get('n_links', p['n_links']), *[float(v) for v in p['intr']],
            ptrs[3], joints.shape[1], ptrs[4], twists.shape[1], clip)
    tail = (ptrs[5], ptrs[6], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = lib.rope_bundle_normal_equations(*head, *tail) if plain else lib.rope_bundle_normal_equations_robust(*head, kind, scale, *tail)
    torch.cuda.synchronize()
    assert work[-1].item() == GARBAGE                                      # nothing written past the workspace
    return rc, out.cpu().numpy()


def _hand():
    R, ids, T, joints = hand_planes()
    return dict(R=R, ids=ids, T=T, joints=joints, twists=np.random.default_rng(6).uniform(-1, 1, (3, 6, 6)), intr=HAND_INTR, n_links=HAND_LINKS)


def _tiny():
    """1 x 1: no pixel has a normal, the BOTH sums stay; the second frame's pixel lies beyond the scale."""
    R = np.array([2.0, 2.0], np.float32).reshape(2, 1, 1)
    T = np.array([2.0 + K4 / 2, 2.0 + 2 * K4], np.float32).reshape(2, 1, 1)
    joints, twists = neq_terms.columns(np.random.default_rng(8), 2, 2, 2)
    return dict(R=R, ids=np.zeros((2, 1, 1), np.uint8), T=T, joints=joints, twists=twists, intr=HAND_INTR, n_links=1)


def test_huber_at_the_scale_of_the_truncation_gives_the_plain_kernels_bytes(engine, frames):
    for p in (frames, _hand(), _tiny()):
        rc, got = _call(p, rref.HUBER, CLIP)
        rc0, plain = _call(p, 0, 0.0, plain=True)
        assert rc == 0 and rc0 == 0 and got.tobytes() == plain.tobytes(), np.argwhere(got != plain)
    t = _dev(frames['R'], frames['ids'], frames['T'])
    a = engine.bundle_normal_equations_robust(*t, frames['joints'], frames['twists'], 4, CLIP, frames['intr'], 'huber', CLIP)
    b = engine.bundle_normal_equations(*t, frames['joints'], frames['twists'], 4, CLIP, frames['intr'])
    assert a.tobytes() == b.tobytes() and a.shape == (3, 96) and (b[:, 2] > 1000).all()
    # either group of columns alone, and another truncation
    for joints, twists in ((frames['joints'], None), (None, frames['twists'])):
        a = engine.bundle_normal_equations_robust(*t, joints, twists, 4, CLIP / 2, frames['intr'], 'huber', CLIP / 2)
        assert a.tobytes() == engine.bundle_normal_equations(*t, joints, twists, 4, CLIP / 2, frames['intr']).tobytes()


@pytest.mark.parametrize('kind', ['huber', 'tukey'])
def test_weighted_words_against_the_reference_and_their_determinism(engine, frames, kind):
    code = rref.KINDS[kind]
    for name, p in (('47 x 45', frames), ('hand planes', _hand()), ('1 x 1', _tiny())):
        want, mag, cnt = rref.normal_equations(p['R'], p['ids'], p['T'], p['n_links'], p['intr'], p['joints'], p['twists'], CLIP, code, K4)
        rc, got = _call(p, code, K4)
        assert rc == 0 and got.shape == want.shape
        assert np.array_equal(got[:, [0, 2, 94, 95]], want[:, [0, 2, 94, 95]]), (got[:, [0, 2]], want[:, [0, 2]])
        err, bound = np.abs(got - want), (cnt + 8) * EPS * mag
        share = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = np.unravel_index(np.argmax(share), err.shape)
        print(f"{kind}, {name}: inliers {want[:, 2]}, words that differ from the reference at all: {(got != want).sum()} of {got.size}; largest "
              f"|kernel - reference| {err.max():.3e}; nearest to its bound at word {worst}: {err[worst]:.3e} of {bound[worst]:.3e}")
        assert (err <= bound).all(), (worst, err[worst], bound[worst])
        rc, again = _call(p, code, K4)
        assert rc == 0 and again.tobytes() == got.tobytes()
        N = len(p['R'])
        parts = [_call(p, code, K4, frames=slice(a, b))[1] for a, b in ((0, 1), (1, N))]
        assert np.concatenate(parts).tobytes() == got.tobytes()
    # the weights bite on the big frames: fewer inliers for Tukey (|r| up to 0.03 against k = 2^-7), a smaller cost for both
    plain, _ = bref.normal_equations(frames['R'], frames['ids'], frames['T'], 4, frames['intr'], frames['joints'], frames['twists'], CLIP)
    want, _, _ = rref.normal_equations(frames['R'], frames['ids'], frames['T'], 4, frames['intr'], frames['joints'], frames['twists'], CLIP, code, K4)
    assert (want[:, 1] < plain[:, 1]).all() and (want[:, 3] < plain[:, 3]).all() and (want[:, 2] > 300).all()
    assert (want[:, 2] < plain[:, 2]).all() if kind == 'tukey' else np.array_equal(want[:, 2], plain[:, 2])
    t = _dev(frames['R'], frames['ids'], frames['T'])
    via = engine.bundle_normal_equations_robust(*t, frames['joints'], frames['twists'], 4, CLIP, frames['intr'], kind, K4)
    assert via.tobytes() == _call(frames, code, K4)[1].tobytes()
    assert engine.bundle_normal_equations_robust(*(x[:0] for x in t), frames['joints'][:0], frames['twists'][:0], 4, CLIP, frames['intr'], kind,
                                                 K4).shape == (0, 96)


def test_argument_errors_return_their_code_and_leave_the_output_alone(engine):
    p = _hand()
    garbage = np.float64(GARBAGE).view(np.uint64)
    cases = [dict(kind=0), dict(kind=3), dict(kind=-1), dict(scale=0.0), dict(scale=float('nan')), dict(scale=float('inf')), dict(scale=-K4),
             dict(scale=float(np.nextafter(np.float32(CLIP), np.float32(1.0)))), dict(scale=2 * CLIP), dict(clip=0.0), dict(clip=float('nan')),
             dict(n_frames=0), dict(n_links=0), dict(n_links=7)]
    cases += [dict(null=k) for k in range(7)] + [dict(odd=k) for k in (0, 2, 3, 4, 5, 6)]
    for case in cases:
        kw = dict(kind=rref.HUBER, scale=K4)
        kw.update(case)
        rc, got = _call(p, kw.pop('kind'), kw.pop('scale'), **kw)
        assert rc == E_ARG and (got.view(np.uint64) == garbage).all(), case
    assert _call(p, rref.TUKEY, CLIP)[0] == 0                              # the scale may be the truncation itself
    Rh, Ih, Th = p['R'], p['ids'], p['T']
    for case in (dict(odd=True), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(clip=0.0), dict(clip=float('inf')), dict(clip=-CLIP),
                 dict(n_frames=0), dict(hw=(0, 23)), dict(hw=(4097, 4096)), dict(n_links=0), dict(n_links=7)):
        kw = dict(n_links=HAND_LINKS)
        kw.update(case)
        n_links = kw.pop('n_links')
        rc, got = _hist_call(Rh, Ih, Th, n_links, **kw)
        assert rc == E_ARG and (got == 0x5a5a5a5a).all(), case
    t = _dev(Rh, Ih, Th)
    for call in (lambda: engine.bundle_normal_equations_robust(*t, p['joints'], p['twists'], HAND_LINKS, CLIP, HAND_INTR, 'cauchy', K4),
                 lambda: engine.bundle_normal_equations_robust(*t, p['joints'], p['twists'], HAND_LINKS, CLIP, HAND_INTR, 'huber', 2 * CLIP),
                 lambda: engine.bundle_normal_equations_robust(*t, None, None, HAND_LINKS, CLIP, HAND_INTR, 'huber', K4),
                 lambda: engine.residual_histogram(t[0], t[1], t[2][:2], HAND_LINKS, CLIP),
                 lambda: engine.residual_histogram(*t, HAND_LINKS, -1.0)):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------------------------- the refiner
class _PlaneEngine:
    """An Engine whose drawn links are the scene's three planes: everything else is the real engine's."""

    def __init__(self, e):
        self._e, self.n_links, self.device = e, rref.SCENE_LINKS, e.device

    def __getattr__(self, name):
        return getattr(self._e, name)


def test_bundle_refiner_with_weights_walks_the_reference_loop_and_ends_closer_than_without(engine, monkeypatch):
    """The occluder scene of tests/test_robust_refs.py through BundleRefiner on the device: the renders are the scene's planes
    (refinement._render_under is replaced by robust_ref.scene_render; no robot is drawn), the histogram, the scale, the weighted
    words and the loop are the product's.  The reference loop sees the same planes, so the two differ by the order of the kernel's
    sums alone; its decisions are no near ties (tests/test_robust_refs.py prints the margins: 1.5e-7 of the cost at the least)."""
    from rope_s3d_amd.prediction import refinement as rf
    calls = []

    def render_under(e, intr, pose, angles, n_links):
        assert n_links == rref.SCENE_LINKS and len(angles) == len(rref.SCENE_SETS)
        calls.append(np.array(pose))
        return tuple(_dev(*rref.scene_render(pose)))

    monkeypatch.setattr(rf, '_render_under', render_under)
    fx, fy, cx, cy = rref.SCENE_INTR
    intr = SimpleNamespace(fx=fx, fy=fy, cx=cx, cy=cy)
    T, _ = rref.occluder_scene()
    angles = np.zeros((len(rref.SCENE_SETS), 6))
    plain = rf.BundleRefiner(_PlaneEngine(engine), intr, do_angles='').refine(rref.SCENE_START, angles, T)
    want_plain = rref.scene_refine(T)
    assert np.isnan(plain.robust_scale) and plain.steps_taken == want_plain['steps_taken'] and len(calls) == 6       # not a launch more
    e_plain = rref.pose_error(plain.pose)
    for kind in ('huber', 'tukey'):
        del calls[:]
        got = rf.BundleRefiner(_PlaneEngine(engine), intr, do_angles='', robust=kind).refine(rref.SCENE_START, angles, T)
        k = rref.scene_auto_scale(T, kind)
        want = rref.scene_refine(T, kind, k)
        e = rref.pose_error(got.pose)
        print(f"{kind}: scale {got.robust_scale:.6e} m, steps {got.steps_taken}, cost {got.cost_before:.6e} -> {got.cost_after:.6e}, |error| start "
              f"{rref.pose_error(rref.SCENE_START):.6e}, plain {e_plain:.6e}, {kind} {e:.6e}; pose against the reference loop "
              f"{np.abs(got.pose - want['pose']).max():.3e}")
        assert got.robust_scale == k and len(calls) == 7                   # the histogram's render at the start, then the loop's six
        assert got.steps_taken == want['steps_taken'] and got.cost_after <= got.cost_before
        assert got.frame_cost.shape == (3,) and np.isfinite(got.sigma_pose).all()
        assert e < e_plain
    fixed = rf.BundleRefiner(_PlaneEngine(engine), intr, do_angles='', robust='huber', robust_scale=0.005).refine(rref.SCENE_START, angles, T)
    assert fixed.robust_scale == float(np.float32(0.005)) and rref.pose_error(fixed.pose) < e_plain


def test_calibrate_with_robust_weights_records_kind_and_scale(tmp_path):
    """calibrate.py -robust on a synthetic set: the report names the kind and the scale the run fixed, and what does not go together
    is refused before anything is opened on the device."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
    out = tmp_path / 'robust.json'
    base = [sys.executable, os.path.join(root, 'calibrate.py'), 'synthetic:8', '-frames', '8', '-ds_factor', '8', '-iterations', '2']
    r = subprocess.run(base + ['-joints', 'offset', '-robust', 'tukey', '-json', str(out)], cwd=root, capture_output=True, text=True)
    print(r.stdout[-800:])
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(out.read_text())
    assert rep['robust'] == 'tukey' and CLIP / 128 <= rep['robust_scale'] <= CLIP and rep['cost_after'] <= rep['cost_before']
    assert 0 <= rep['steps_taken'] <= 2 and rep['inliers'] > 0 and len(rep['offsets']) == 6
    r = subprocess.run(base + ['-joints', 'offset', '-robust', 'huber', '-native'], cwd=root, capture_output=True, text=True)
    assert r.returncode != 0 and '-robust' in r.stderr
    from rope_s3d_amd import CameraPredictor, ModellessCameraPredictor      # the switch is known to both predictors
    for cls in (ModellessCameraPredictor, CameraPredictor):
        with pytest.raises(ValueError, match='bundle\\+robust'):
            cls(refine='bundle+huber')
