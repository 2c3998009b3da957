"""CPU: the outline term's second direction, mask -> render.  The restatement of rope_render_nearest and
rope_silhouette_normal_equations_reverse (tests/silhouette_reverse_ref.py) against what their contracts imply — the derived field
is rope_mask_distance's of the coverage, the tie-break, the anchor pixel, a mask that is the coverage has no residual — then the host
side over a stub engine (BundleRefiner(both_ways=), calibrate.py's and the predictors' switches), the ABI, and the compiler's
resource report for the new kernels and for the two they stand beside."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from rope_s3d_amd import build
from rope_s3d_amd import engine as eng
from rope_s3d_amd.prediction import refinement as rf

import silhouette_ref as sref
import silhouette_reverse_ref as rref
from test_silhouette_host import ANGLES, DEPTH, MASK, POSE, StubEngine, _intr, on_the_host  # noqa: F401  (on_the_host: a fixture)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
INTR = (150.0, 140.0, 12.25, 9.5)


# ---------------------------------------------------------------------------------------------- the restatement
def _id_planes():
    """Planes of 23 x 31 with ids in 0 .. 5 and 255: random at three densities, a disc, a disc with a hole, stripes, all and none."""
    H, W = 23, 31
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (yy - 11) ** 2 + (xx - 15) ** 2 <= 81
    covers = [rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.05, rng.random((H, W)) < 0.95, disc, disc & ~((yy - 11) ** 2 + (xx - 13) ** 2 <= 9),
              (yy // 4 + xx // 6) % 2 == 0, np.ones((H, W), bool), np.zeros((H, W), bool)]
    ids = np.where(np.stack(covers), rng.integers(0, 6, (len(covers), H, W)), 255).astype(np.uint8)
    ids[0, 3, 4] = 7                                                    # an id that is neither a link's nor the background's: not rendered
    return ids


@pytest.mark.parametrize('radius', [1, 3, 8, 16])
def test_the_derived_field_is_the_distance_field_of_the_coverage(radius):
    ids = _id_planes()
    for n_links in (6, 4):
        near = rref.render_nearest(ids, n_links, radius)
        assert near.dtype == np.int16 and near.min() >= -1 and near.max() <= rref.CODE_MAX
        assert np.array_equal(rref.derived_sd(near, ids, n_links, radius), sref.mask_distance(ids < n_links, radius)), (radius, n_links)
        assert (near[7] == -1).all() and (n_links < 6 or (near[6] == -1).all())      # none rendered, or all (at 6 links): the image edge is no boundary
        # a code points at a pixel of the other state inside the image
        rendered = ids < n_links
        for f, y, x in np.argwhere(near >= 0):
            dy, dx = rref.decode(near[f, y, x])
            assert max(abs(dy), abs(dx)) <= radius and rendered[f, y + dy, x + dx] != rendered[f, y, x]


def test_the_tie_break_is_the_first_pixel_in_raster_order():
    for single_is_rendered in (False, True):
        for y, x, want in ((2, 2, (-1, 0)), (0, 0, (0, 1)), (4, 4, (-1, 0)), (0, 4, (0, -1)), (4, 0, (-1, 0)), (2, 0, (-1, 0)), (0, 2, (0, -1))):
            ids = np.full((1, 5, 5), 255 if single_is_rendered else 2, np.uint8)
            ids[0, y, x] = 2 if single_is_rendered else 255
            near = rref.render_nearest(ids, 6, 4)
            assert rref.decode(near[0, y, x]) == want, (single_is_rendered, y, x)
            for py in range(5):                                         # every other pixel: the single one, no tie
                for px in range(5):
                    if (py, px) != (y, x):
                        d2 = (y - py) ** 2 + (x - px) ** 2
                        assert (near[0, py, px] == -1 and d2 > 16) or rref.decode(near[0, py, px]) == (y - py, x - px)
    # two at the same distance in one row, and in one column: the left one, the upper one; and the upper before the left
    ids = np.full((1, 7, 7), 255, np.uint8)
    ids[0, 3, 1] = ids[0, 3, 5] = 0
    assert rref.decode(rref.render_nearest(ids, 6, 5)[0, 3, 3]) == (0, -2)
    assert rref.decode(rref.render_nearest(ids.transpose(0, 2, 1).copy(), 6, 5)[0, 3, 3]) == (-2, 0)
    ids[0, 1, 3] = 0
    assert rref.decode(rref.render_nearest(ids, 6, 5)[0, 3, 3]) == (-2, 0)
    assert rref.encode(-16, -16) == 0 and rref.encode(16, 16) == rref.CODE_MAX == 1088 and rref.encode(0, 0) == 16 * 33 + 16


def _columns(rng, N, nj, nc):
    joints = np.concatenate([rng.uniform(-1, 1, (N, nj, 3)), rng.uniform(-.5, .5, (N, nj, 2)), rng.uniform(1.5, 2.5, (N, nj, 1))], axis=2) if nj else None
    return joints, (rng.uniform(-1, 1, (N, nc, 6)) if nc else None)


@pytest.mark.parametrize('radius', [2, 6])
def test_the_anchor_is_a_rendered_pixel_between_the_mask_pixel_and_the_boundary(radius):
    ids = _id_planes()
    rng = np.random.default_rng(5)
    N, H, W = ids.shape
    masks = np.roll(ids < 6, (2, -3), axis=(1, 2)) | (rng.random(ids.shape) < 0.1)
    R = rng.uniform(1.5, 2.5, ids.shape).astype(np.float32)
    near = rref.render_nearest(ids, 6, radius)
    joints, tw = _columns(rng, N, 6, 6)
    inliers = 0
    for f in range(N):
        rendered = ids[f] < 6
        for e, inlier, J, (y, x), c in rref.frame_terms(masks[f], near[f], R[f], ids[f], 6, INTR, joints[f], tw[f], radius):
            assert (c is not None) == inlier
            if not inlier:
                assert abs(e) == np.sqrt(radius * radius + 1.0) - 0.5 + (0.5 if not rendered[y, x] else -0.5) and not J.any()
                continue
            inliers += 1
            dy, dx = rref.decode(near[f, y, x])
            u = (y + dy, x + dx)
            assert 0 <= c[0] < H and 0 <= c[1] < W and rendered[c]
            assert min(y, u[0]) <= c[0] <= max(y, u[0]) and min(x, u[1]) <= c[1] <= max(x, u[1])          # between p and u
            d2c = (c[0] - y) ** 2 + (c[1] - x) ** 2
            if rendered[y, x]:
                assert d2c < dy * dy + dx * dx                          # strictly nearer than the nearest unrendered pixel
                assert abs(c[0] - u[0]) + abs(c[1] - u[1]) == 1 and (c[0] == u[0]) == (abs(dx) >= abs(dy))
            else:
                assert c == u
            assert np.isfinite(J).all() and not J[int(ids[f][c]):6].any()                                 # joint j moves the links behind it
    assert inliers > 200


def test_a_mask_that_is_the_coverage_has_no_residual_and_the_forward_terms_contour():
    ids = _id_planes()
    rng = np.random.default_rng(6)
    N = len(ids)
    R = rng.uniform(1.5, 2.5, ids.shape).astype(np.float32)
    joints, tw = _columns(rng, N, 6, 6)
    cover = (ids < 6).astype(np.uint8)
    for radius in (1, 5):
        near = rref.render_nearest(ids, 6, radius)
        back, mag = rref.normal_equations(cover * 200, near, R, ids, 6, INTR, joints, tw, radius)
        fwd, _ = sref.normal_equations(R, ids, sref.mask_distance(cover, radius), 6, INTR, joints, tw, radius)
        assert not back[:, 1].any() and not back[:, 3].any() and not back[:, 4:16].any()
        assert np.array_equal(back[:, 0], back[:, 2]) and np.array_equal(back[:, 0], fwd[:, 0]) and back[:3, 0].min() > 20
        assert back[6, 0] == 0 and back[7, 0] == 0 and not back[:, 94:].any()
        assert (mag >= np.abs(back)).all()
    # one pixel of difference: a mask one pixel larger than a rendered square, the residual of every contour pixel is exactly 1
    ids1 = np.full((1, 12, 12), 255, np.uint8)
    ids1[0, 4:8, 4:8] = 3
    mask1 = np.zeros((1, 12, 12), np.uint8)
    mask1[0, 3:9, 3:9] = 1
    back, _ = rref.normal_equations(mask1, rref.render_nearest(ids1, 6, 4), np.full((1, 12, 12), 2.0, np.float32), ids1, 6, INTR, None,
                                    np.eye(6)[None], 4)
    assert back[0, 0] == back[0, 2] == 20 and abs(back[0, 1] - (16 * 1.0 + 4 * 2.0)) < 1e-12          # the corners are sqrt(2) away
    assert back[0, 16 + 12 * 6 - 15] > 0                                # the camera's x column moves that outline


# ---------------------------------------------------------------------------------------------- the refiner over a stub engine
class StubBoth(StubEngine):
    def render_nearest(self, ri, n_links, radius):
        self.calls.append(('render_nearest', ri.dtype, tuple(ri.shape), n_links, radius))
        return torch.zeros(ri.shape, dtype=torch.int16)

    def silhouette_normal_equations_reverse(self, mask, near, rd, ri, axes, twists, n_links, radius, intr):
        assert mask.dtype == torch.uint8 and near.dtype == torch.int16 and mask.shape == near.shape == rd.shape == ri.shape
        self.calls.append('silhouette_reverse')
        return self._words(len(rd), 6.0, 4.0 / (1 + self.calls.count('silhouette_reverse')))


def _names(calls):
    return [c if isinstance(c, str) else c[0] for c in calls]


@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_both_ways_calls_both_directions_on_every_render_and_sums_their_words(on_the_host, mode):
    e, intr = StubBoth(), _intr()
    res = rf.BundleRefiner(e, intr, joints=mode, iterations=2, silhouette=1.0, radius=5, both_ways=True).refine(POSE, ANGLES, None, MASK)
    assert e.calls[0] == ('mask_distance', torch.uint8, (3, 6, 8), 5)
    assert _names(e.calls[1:]) == ['render', 'silhouette', 'render_nearest', 'silhouette_reverse'] * 3
    assert e.calls[3] == ('render_nearest', torch.uint8, (3, 6, 8), 6, 5)
    # the cost is that of the summed words: 10 contour pixels a frame at 9 / (1 + k) and 6 at 4 / (1 + k)
    assert res.cost_silhouette_before == (10 * 9.0 / 2 + 6 * 4.0 / 2) / 16 and res.cost_silhouette_after == (10 * 9.0 / 4 + 6 * 4.0 / 4) / 16
    assert res.steps_taken == 2 and res.inliers_silhouette == 30 and res.inliers_silhouette_reverse == 18
    assert np.isfinite(res.sigma_pose).all() and np.isnan(res.cost_before) and res.inliers == 0
    # with depth: the bundle's call stands where it stood
    e = StubBoth()
    res = rf.BundleRefiner(e, intr, joints=mode, iterations=1, silhouette=2.0, both_ways=True).refine(POSE, ANGLES, DEPTH, MASK)
    assert _names(e.calls[1:]) == ['render', 'bundle', 'silhouette', 'render_nearest', 'silhouette_reverse'] * 2
    assert res.cost_before == 1e-4 / 2 and res.inliers == 120 and res.inliers_silhouette_reverse == 18


@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_the_step_of_both_ways_is_the_one_ways_step_on_the_summed_words(on_the_host, mode):
    """A stub whose forward call already returns forward + reverse, run one way, takes the steps both_ways takes on the two."""
    class Summed(StubEngine):
        def silhouette_normal_equations(self, rd, ri, sd2, axes, twists, n_links, radius, intr):
            self.calls.append('silhouette')
            k = self.calls.count('silhouette')
            return self._words(len(rd), 10.0, 9.0 / (1 + k)) + self._words(len(rd), 6.0, 4.0 / (1 + k))

    intr = _intr()
    a = rf.BundleRefiner(StubBoth(), intr, joints=mode, iterations=2, silhouette=1.5, both_ways=True).refine(POSE, ANGLES, DEPTH, MASK)
    b = rf.BundleRefiner(Summed(), intr, joints=mode, iterations=2, silhouette=1.5).refine(POSE, ANGLES, DEPTH, MASK)
    assert a.pose.tobytes() == b.pose.tobytes() and a.angles.tobytes() == b.angles.tobytes() and a.sigma_pose.tobytes() == b.sigma_pose.tobytes()
    assert (a.cost_silhouette_before, a.cost_silhouette_after, a.steps_taken) == (b.cost_silhouette_before, b.cost_silhouette_after, b.steps_taken)
    assert a.inliers_silhouette + a.inliers_silhouette_reverse == b.inliers_silhouette and b.inliers_silhouette_reverse == 0


@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_without_both_ways_exactly_todays_calls_and_bytes(on_the_host, mode):
    intr = _intr()
    e1, e2 = StubBoth(), StubEngine()
    a = rf.BundleRefiner(e1, intr, joints=mode, iterations=2, silhouette=2.0, radius=5, both_ways=False).refine(POSE, ANGLES, DEPTH, MASK)
    b = rf.BundleRefiner(e2, intr, joints=mode, iterations=2, silhouette=2.0, radius=5).refine(POSE, ANGLES, DEPTH, MASK)
    assert e1.calls == e2.calls and e1.calls[1:] == ['render', 'bundle', 'silhouette'] * 3
    for k in ('pose', 'angles', 'offsets', 'sigma_pose', 'frame_cost'):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert (a.cost_before, a.cost_after, a.cost_silhouette_before, a.cost_silhouette_after, a.steps_taken, a.inliers, a.inliers_silhouette) == \
           (b.cost_before, b.cost_after, b.cost_silhouette_before, b.cost_silhouette_after, b.steps_taken, b.inliers, b.inliers_silhouette)
    assert a.inliers_silhouette_reverse == 0 and b.inliers_silhouette_reverse == 0
    assert rf.BundleRefineResult.__dataclass_fields__['inliers_silhouette_reverse'].default == 0
    e3 = StubBoth()
    rf.BundleRefiner(e3, intr, joints=mode, iterations=2).refine(POSE, ANGLES, DEPTH)
    assert e3.calls == ['render', 'bundle'] * 3


def test_what_both_ways_refuses():
    e, intr = StubBoth(), _intr()
    for kw in (dict(), dict(silhouette=0.0), dict(native=True), dict(robust='huber')):
        with pytest.raises(ValueError):
            rf.BundleRefiner(e, intr, both_ways=True, **kw)
    for kw in (dict(native=True), dict(robust='tukey')):                # and with the term on, what silhouette > 0 refuses already
        with pytest.raises(ValueError):
            rf.BundleRefiner(e, intr, silhouette=1.0, both_ways=True, **kw)
    with pytest.raises(ValueError, match='mask'):
        rf.BundleRefiner(e, intr, silhouette=1.0, both_ways=True).refine(POSE, ANGLES, DEPTH)
    r = rf.BundleRefiner(e, intr, silhouette=1.0, both_ways=True)
    assert r.both_ways is True and rf.BundleRefiner(e, intr, silhouette=1.0).both_ways is False and e.calls == []


def test_the_predictors_and_calibrate_know_the_switch():
    from rope_s3d_amd.prediction import camera_pose_prediction as cpp
    assert 'bundle+silhouette+both' in cpp.OUTLINE_REFINES and 'bundle+silhouette' in cpp.OUTLINE_REFINES
    with pytest.raises(ValueError) as err:
        cpp.ModellessCameraPredictor(refine='bundle+both')
    for name in ('bundle', 'bundle+silhouette', 'bundle+native', 'bundle+robust', 'bundle+silhouette+both'):
        assert repr(name) in str(err.value)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'calibrate.py'), '-h'], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and '-both_ways' in r.stdout


# ---------------------------------------------------------------------------------------------- the ABI and the build
def test_the_two_calls_are_declared_bound_and_built_from_their_own_file():
    with open(os.path.join(ROOT, 'include', 'rope_s3d.h')) as f:
        pub = f.read()
    for name in ('rope_render_nearest', 'rope_silhouette_normal_equations_reverse'):
        assert name in eng.ABI_SYMBOLS and f'int {name}(' in pub
    assert '#define ROPE_SIL_NEAREST_MAX 1088' in pub
    assert hasattr(eng.Engine, 'render_nearest') and hasattr(eng.Engine, 'silhouette_normal_equations_reverse')
    assert 'rope_silhouette_reverse.hip' in build._SOURCES and 'rope_silhouette_reverse.hip' in build._DEPS
    with open(os.path.join(build._CSRC, 'rope_silhouette_reverse.hip')) as f:
        text = f.read()
    assert '#include "rope_neq.h"' in text and 'bneq_pack_and_own_words' in text and 'neq_gather<ROPE_BNEQ_WORDS>' in text
    assert 'atomic' not in text.lower()
    build.build()                                                       # a no-op when the library is of these sources
    lib = eng.load_library()
    assert len(lib.rope_render_nearest.argtypes) == 8 and len(lib.rope_silhouette_normal_equations_reverse.argtypes) == 20


@pytest.fixture(scope='module')
def hipcc():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip("no hipcc: the resource table needs the compiler")


def test_the_new_kernels_use_no_scratch_and_the_old_ones_keep_their_resources(hipcc):
    new = build.resource_usage(source='rope_silhouette_reverse.hip')
    names = [r['symbol'] for r in new]
    assert len(new) == 3 and all(any(k in n for n in names) for k in ('render_nearest_kernel', 'rneq_partial_kernel', 'rneq_gather_kernel')), names
    for r in new:
        print(r['symbol'], {k: r[k] for k in ('vgprs', 'agprs', 'sgprs', 'lds_bytes', 'occupancy', 'scratch_bytes', 'vgpr_spills', 'sgpr_spills')})
        assert r['scratch_bytes'] == 0 and r['vgpr_spills'] == 0, r
    nearest = next(r for r in new if 'render_nearest_kernel' in r['symbol'])
    partial = next(r for r in new if 'rneq_partial_kernel' in r['symbol'])
    assert nearest['lds_bytes'] == 1024 and nearest['occupancy'] == 8                # two 64-word arrays, as mask_distance_kernel
    assert partial['lds_bytes'] <= 27472 and partial['occupancy'] >= 5              # bneq_pack_and_own_words' LDS, sneq_partial_kernel's occupancy
    # the kernels of rope_silhouette.hip at the registers and LDS recorded when they were written
    with open(os.path.join(ROOT, 'tests', 'golden', 'silhouette_resources_gfx950.json')) as f:
        golden = json.load(f)['kernels']
    old = build.resource_usage(source='rope_silhouette.hip')
    assert len(old) == 3
    for k in ('mask_distance_kernel', 'sneq_partial_kernel'):
        r = next(r for r in old if k in r['symbol'])
        assert (r['vgprs'], r['lds_bytes'], r['occupancy'], r['scratch_bytes']) == \
               (golden[k]['vgprs'], golden[k]['lds_bytes'], golden[k]['occupancy'], golden[k]['scratch_bytes']), r
