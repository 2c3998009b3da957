"""GPU: rope_render_nearest and rope_silhouette_normal_equations_reverse (csrc/rope_silhouette_reverse.hip) against the restatement
of their contracts (tests/silhouette_reverse_ref.py) — the codes bit for bit, against rope_mask_distance on the same coverage, the
counts of the normal equations exactly and every float sum within the worst case of a reordered float64 summation — their
determinism, what they refuse, and BundleRefiner(both_ways=True), calibrate.py -both_ways and the predictors' switch end to end.

The bound is tests/test_gpu_silhouette.py's: 4 n eps sum|terms| with n the pixel count of the frame and eps = 2^-52; the terms
themselves are the same bits on both sides."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import silhouette_ref as sref
import silhouette_reverse_ref as rref
from test_gpu_bundle import TRUE_POSE_OFFSET
from test_gpu_silhouette import E_ARG, EPS, GARBAGE, INTR, _columns, _masks_37x53, _scene, renderer  # noqa: F401  (renderer: a fixture)

pytestmark = pytest.mark.gpu

GARBAGE_I16 = 0x5a5a
RADII = (1, 8, 16)


# ---------------------------------------------------------------------------------------------- the nearest pixel
def _nearest(ids, n_links, radius, null=None, odd=False, n=None, hw=None):
    """The C entry point on an output filled with garbage -> (rc, near (N, H, W) int16)."""
    lib = eng.load_library()
    N, H, W = ids.shape
    i = torch.from_numpy(np.ascontiguousarray(ids, np.uint8)).cuda()
    out = torch.full((N * H * W + 3,), GARBAGE_I16, dtype=torch.int16, device='cuda')
    ptrs = [i.data_ptr(), out.data_ptr() + (1 if odd else 0)]
    ptrs = [None if null == k else C.c_void_p(p) for k, p in enumerate(ptrs)]
    H2, W2 = hw if hw is not None else (H, W)
    rc = lib.rope_render_nearest(ptrs[0], N if n is None else n, H2, W2, n_links, radius, ptrs[1], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[N * H * W:] == GARBAGE_I16).all()                                        # nothing written past the planes
    return rc, got[:N * H * W].reshape(N, H, W)


def _ids_of(cover, rng):
    """coverage (N, H, W) bool -> ids: links 0 .. 5 where covered, 255 and a few 6 .. 254 (no link's) where not"""
    off = np.where(rng.random(cover.shape) < 0.1, rng.integers(6, 255, cover.shape), 255)
    return np.where(cover, rng.integers(0, 6, cover.shape), off).astype(np.uint8)


def _tile_corner_plane():
    cover = np.zeros((33, 33), bool)
    for y, x in ((0, 0), (0, 31), (0, 32), (31, 0), (32, 0), (31, 31), (32, 32), (31, 32), (32, 31), (16, 16)):
        cover[y, x] = True
    return cover


@pytest.fixture(scope='module')
def id_planes():
    rng = np.random.default_rng(31)
    sets = {'37x53': _masks_37x53() != 0, '1x70': rng.random((2, 1, 70)) < 0.4, '70x1': rng.random((2, 70, 1)) < 0.4,
            'corners': np.stack([_tile_corner_plane(), ~_tile_corner_plane()])}
    sets = {k: _ids_of(c, rng) for k, c in sets.items()}
    return sets, {(k, R): rref.render_nearest(i, 6, R) for k, i in sets.items() for R in RADII}


@pytest.mark.parametrize('radius', RADII)
def test_nearest_is_the_reference_bit_for_bit_and_the_distance_kernels_field(id_planes, radius):
    sets, want = id_planes
    e = eng.Engine(0)
    try:
        for name, ids in sets.items():
            rc, got = _nearest(ids, 6, radius)
            assert rc == 0
            bad = np.argwhere(got != want[name, radius])
            assert len(bad) == 0, (name, radius, bad[:5], got[tuple(bad[0])], want[name, radius][tuple(bad[0])])
            # GPU against GPU: what the codes imply is rope_mask_distance's field of the coverage
            ids_t = torch.from_numpy(ids).cuda()
            near_t = e.render_nearest(ids_t, 6, radius)
            assert near_t.dtype == torch.int16 and np.array_equal(near_t.cpu().numpy(), got)
            sd = e.mask_distance((ids_t < 6).contiguous(), radius).cpu().numpy()
            assert np.array_equal(rref.derived_sd(got, ids, 6, radius), sd), (name, radius)
        assert (want['37x53', radius][0] == -1).all() and (want['37x53', radius][1] == -1).all()      # none rendered; all rendered
        # fewer links: ids 4 and 5 are not rendered then
        rc, got = _nearest(sets['37x53'][2:5], 4, radius)
        assert rc == 0 and np.array_equal(got, rref.render_nearest(sets['37x53'][2:5], 4, radius))
        assert tuple(e.render_nearest(ids_t[:0], 6, radius).shape) == (0,) + tuple(ids_t.shape[1:])
    finally:
        e.close()


def test_nearest_walks_the_planes_beyond_the_grids_height():
    """32 768 + 7 planes of 1 x 3 at radius 2: the grid is 32 768 workgroups high and the workgroups 0 .. 6 walk on to a second plane
    each.  Seven planes, tiled: plane i is plane i % 7 and plane i + 32 768 is plane (i + 1) % 7.  Three pixels of two states have
    four code planes between them (a coverage and its complement share theirs), so the seven are ordered such that every plane's
    codes differ from the next one's, the last one's from the first's: a workgroup that wrote its second plane with its first plane's
    codes, or not at all, is seen."""
    planes = 32768 + 7
    seven = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [1, 255, 255], [255, 2, 255], [255, 255, 0]], np.uint8).reshape(7, 1, 3)
    want7 = rref.render_nearest(seven, 6, 2)
    assert 32768 % 7 == 1 and all(want7[i].tobytes() != want7[(i + 1) % 7].tobytes() for i in range(7)) and (want7[3] == -1).all()
    which = np.arange(planes) % 7
    rc, got = _nearest(seven[which], 6, 2)
    assert rc == 0
    bad = np.flatnonzero((got != want7[which]).any(axis=(1, 2)))
    assert len(bad) == 0, bad[:8]


def test_nearest_refuses_bad_arguments_and_writes_nothing():
    ids = np.zeros((2, 5, 6), np.uint8)
    ids[:, 2, 3] = 255
    for case in (dict(n=-1), dict(hw=(0, 6)), dict(hw=(5, 0)), dict(hw=(1 << 16, 1 << 15)), dict(radius=0), dict(radius=17), dict(radius=-3),
                 dict(n_links=0), dict(n_links=256), dict(n_links=-1), dict(null=0), dict(null=1), dict(odd=True)):
        kw = dict(radius=4, n_links=6)
        kw.update(case)
        rc, got = _nearest(ids, kw.pop('n_links'), kw.pop('radius'), **kw)
        assert rc == E_ARG and (got == GARBAGE_I16).all(), case
    rc, _ = _nearest(np.zeros((0, 4, 4), np.uint8), 6, 3)
    assert rc == 0
    rc, got = _nearest(ids, 255, 4)                                     # 255 links: only the id 255 is not rendered
    assert rc == 0 and np.array_equal(got, rref.render_nearest(ids, 255, 4)) and (got >= 0).any()
    e = eng.Engine(0)
    try:
        t = torch.from_numpy(ids).cuda()
        for bad in (lambda: e.render_nearest(t, 6, 0), lambda: e.render_nearest(t, 6, 17), lambda: e.render_nearest(t.cpu(), 6, 4),
                    lambda: e.render_nearest(t.float(), 6, 4), lambda: e.render_nearest(t[0], 6, 4), lambda: e.render_nearest(t, 0, 4),
                    lambda: e.render_nearest(t, 256, 4)):
            with pytest.raises(ValueError):
                bad()
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- the normal equations
def _call(mask, near, R, ids, joints, twists, n_links, intr, radius, null=None, odd=None, n_frames=None, hw=None, n_joints=None, n_cols=None):
    """The C entry point on an out buffer filled with garbage -> (rc, out (N, 96) float64).  Pointers by position: 0 mask, 1 near,
    2 render, 3 ids, 4 joints, 5 twists, 6 out, 7 work."""
    N, H, W = R.shape
    lib = eng.load_library()
    joints = np.zeros((N, 0, 6)) if joints is None else np.asarray(joints, np.float64)
    twists = np.zeros((N, 0, 6)) if twists is None else np.asarray(twists, np.float64)
    pad = lambda a: a if a.size else np.zeros((N, 1, 6))
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (np.asarray(mask, np.uint8), np.asarray(near, np.int16), R, ids, pad(joints), pad(twists))]
    out = torch.full((N, 96), GARBAGE, dtype=torch.float64, device='cuda')
    work = torch.full((max(1, lib.rope_silhouette_normal_workspace(N, H, W) // 8) + 1,), GARBAGE, dtype=torch.float64, device='cuda')
    ptrs = [x.data_ptr() for x in t] + [out.data_ptr(), work.data_ptr()]
    if odd is not None:
        ptrs[odd] += 1 if odd == 1 else 2
    ptrs = [C.c_void_p(p) for p in ptrs]
    nj = joints.shape[1] if n_joints is None else n_joints
    nc = twists.shape[1] if n_cols is None else n_cols
    if joints.shape[1] == 0 and n_joints is None:
        ptrs[4] = None
    if twists.shape[1] == 0 and n_cols is None:
        ptrs[5] = None
    if null is not None:
        ptrs[null] = None
    H, W = hw if hw is not None else (H, W)
    rc = lib.rope_silhouette_normal_equations_reverse(ptrs[0], ptrs[1], ptrs[2], ptrs[3], N if n_frames is None else n_frames, H, W, n_links,
                                                      *[float(v) for v in intr], ptrs[4], nj, ptrs[5], nc, radius, ptrs[6], ptrs[7],
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert work[-1].item() == GARBAGE
    return rc, out.cpu().numpy()


def _hold(got, mask, near, R, ids, joints, twists, n_links, intr, radius):
    """tests/test_gpu_silhouette.py's _hold with this direction's restatement returning the sums and their magnitudes."""
    want, mag = rref.normal_equations(mask, near, R, ids, n_links, intr, joints, twists, radius)
    n = R.shape[1] * R.shape[2]
    nj = 0 if joints is None else np.asarray(joints).shape[1]
    nc = 0 if twists is None else np.asarray(twists).shape[1]
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 2, 94, 95]], want[:, [0, 2, 94, 95]]), (got[:, [0, 2]], want[:, [0, 2]])
    err, bound = np.abs(got - want), 4 * n * EPS * mag
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{R.shape}, {nj} joints, {nc} columns: largest |kernel - reference| {err.max():.3e}; nearest to its bound at word {worst}: "
          f"{err[worst]:.3e} of {bound[worst]:.3e}")
    assert (err <= bound).all(), (worst, err[worst], bound[worst])
    dead = [c for c in range(12) if (c < 6 and c >= nj) or (c >= 6 and c - 6 >= nc)]
    for f in range(len(got)):
        A, g = sref.unpack(got[f])
        assert not g[dead].any() and not A[dead].any() and not A[:, dead].any()
    return want


def _hand_planes(H, W):
    """Three frames.  Frame 0: a render of two link bands whose right end stops at column 33, one past the 32-pixel tile edge, against a
    mask that ends at column 30 and reaches the frame's top and left edges — mask contour pixels at x = 30 see render pixels across
    the tile edge, and the mask's edge pixels have no contour there.  Frame 1: the mask is empty.  Frame 2: the render is empty."""
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:H, 0:W]
    ids = np.full((3, H, W), 255, np.uint8)
    body = (yy >= 4) & (yy < H - 3) & (xx >= 6) & (xx < 34)
    ids[0][body] = np.where(xx < 20, 1, 4)[body]
    ids[0, H // 2, 12] = 200                                            # a hole in the render
    ids[1][(yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= 36] = 2
    mask = np.zeros((3, H, W), np.uint8)
    mask[0][(yy < H - 6) & (xx <= 30)] = 1
    mask[0, 2, W - 1] = mask[0, H - 1, W - 2] = 7                       # single pixels on the frame's edge, far from the render
    mask[2][(yy >= 5) & (yy < 12) & (xx >= 3) & (xx < 15)] = 255
    R = rng.uniform(1.5, 2.5, ids.shape).astype(np.float32)
    return mask, R, ids


@pytest.mark.parametrize('shape', [(20, 40), (37, 53)])
def test_reverse_kernel_agrees_with_the_reference_on_hand_built_planes(shape):
    rng = np.random.default_rng(7)
    mask, R, ids = _hand_planes(*shape)
    for radius in (5, 2):
        rc, near = _nearest(ids, 6, radius)
        assert rc == 0 and np.array_equal(near, rref.render_nearest(ids, 6, radius))
        for nj in (0, 3, 6):
            for nc in (0, 6):
                if nj + nc == 0:
                    continue
                joints, tw = _columns(rng, 3, nj, nc)
                rc, got = _call(mask, near, R, ids, joints, tw, 6, INTR, radius)
                assert rc == 0
                want = _hold(got, mask, near, R, ids, joints, tw, 6, INTR, radius)
        assert want[0, 0] > 40 and 0 < want[0, 2] < want[0, 0]          # the far single pixels are contour and no inliers
        assert not want[1].any()                                        # no mask: nothing at all
        assert want[2, 0] > 20 and want[2, 2] == 0 and not want[2, 3:].any() and want[2, 1] > 0      # no render: all contour, all FAR
        # the pixels at x = 30 of frame 0 see the render's column 33 at radius 5: across the tile edge
        terms = rref.frame_terms(mask[0], near[0], R[0], ids[0], 6, INTR, None, np.zeros((1, 6)), radius)
        across = [c for _, inlier, _, (y, x), c in terms if inlier and x == 30 and c[1] >= 32]
        assert (len(across) > 0) == (radius == 5)
    radius = 5
    rc, near = _nearest(ids, 6, radius)
    joints, tw = _columns(rng, 3, 6, 6)
    rc, got = _call(mask, near, R, ids, joints, tw, 6, INTR, radius)
    again = _call(mask, near, R, ids, joints, tw, 6, INTR, radius)[1]
    assert rc == 0 and again.tobytes() == got.tobytes()
    parts = [_call(mask[a:b], near[a:b], R[a:b], ids[a:b], joints[a:b], tw[a:b], 6, INTR, radius)[1] for a, b in ((0, 1), (1, 3))]
    assert np.concatenate(parts).tobytes() == got.tobytes()
    # n_links 4: the band of link 4 is not rendered, in the codes and in the equations alike
    rc, near4 = _nearest(ids, 4, radius)
    rc, got = _call(mask, near4, R, ids, joints, tw, 4, INTR, radius)
    assert rc == 0
    _hold(got, mask, near4, R, ids, joints, tw, 4, INTR, radius)
    # a plane of codes the field kernel never writes is read as FAR: nothing is addressed through it
    rc, got = _call(mask, np.full(ids.shape, 0x7fff, np.int16), R, ids, joints, tw, 6, INTR, radius)
    assert rc == 0 and not got[:, 2:].any() and np.array_equal(got[:, 0], want[:, 0])
    # and so are codes of ANOTHER render, whose anchors are not rendered in this one: dropped, never a row of NaN
    rc, got = _call(mask, near, R, np.full_like(ids, 255), joints, tw, 6, INTR, radius)
    assert rc == 0 and np.isfinite(got).all() and not got[:, 2:].any() and np.array_equal(got[:, 0], want[:, 0])


def test_reverse_argument_errors_return_their_code_and_leave_the_output_alone():
    mask, R, ids = _hand_planes(20, 40)
    near = rref.render_nearest(ids, 6, 5)
    joints, tw = _columns(np.random.default_rng(2), 3, 2, 2)
    cases = [dict(n_frames=0), dict(n_frames=-1), dict(hw=(0, 23)), dict(hw=(20, 0)), dict(hw=(4097, 4096)), dict(n_links=0), dict(n_links=7),
             dict(n_joints=-1), dict(n_joints=7), dict(n_cols=-1), dict(n_cols=7), dict(n_joints=0, n_cols=0), dict(radius=0), dict(radius=17),
             dict(radius=-5)]
    cases += [dict(null=k) for k in range(8)] + [dict(odd=k) for k in (1, 2, 4, 5, 6, 7)]
    for case in cases:
        kw = dict(n_links=6, radius=5)
        kw.update(case)
        n_links, radius = kw.pop('n_links'), kw.pop('radius')
        rc, got = _call(mask, near, R, ids, joints, tw, n_links, INTR, radius, **kw)
        assert rc == E_ARG and (got.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), case
    for bad_intr in ((0.0, 140.0, 1.0, 1.0), (150.0, float('nan'), 1.0, 1.0), (150.0, 140.0, float('inf'), 1.0)):
        rc, got = _call(mask, near, R, ids, joints, tw, 6, bad_intr, 5)
        assert rc == E_ARG and (got.view(np.uint64) == np.float64(GARBAGE).view(np.uint64)).all(), bad_intr
    rc, got = _call(mask, near, R, ids, None, tw, 6, INTR, 5)             # a null pointer with a count of 0 is no error
    assert rc == 0 and not np.isnan(got).any()


def test_reverse_on_renders_of_the_robot(renderer):
    """Ten frames at 160 x 90 = 14 400 pixels, eight workgroups a frame.  A mask that is the render's own coverage: no residual at
    all and the forward call's contour count; against the masks of the truth, one Descent step off: the reference."""
    from rope_s3d_amd.prediction.refinement import BundleRefiner, camera_twists
    from rope_s3d_amd.projection import camera_matrix
    e, intr = renderer.engine, renderer.intrinsics
    assert (intr.width, intr.height) == (160, 90)
    truth, true_pose, start, _ = _scene(renderer)
    PV = np.tile(camera_matrix(true_pose, intr)[None], (10, 1, 1))
    radius = 8
    intr4 = (intr.fx, intr.fy, intr.cx, intr.cy)
    rd, ri = e.render_batch_device(start, 6, PV)
    twists = np.tile(camera_twists(true_pose)[None], (10, 1, 1))
    joints = BundleRefiner(e, intr).joint_axes(true_pose, start)
    near_t = e.render_nearest(ri, 6, radius)
    own = (ri < 6).to(torch.uint8).contiguous()
    same = e.silhouette_normal_equations_reverse(own, near_t, rd, ri, joints, twists, 6, radius, intr4)
    fwd = e.silhouette_normal_equations(rd, ri, e.mask_distance(own, radius), joints, twists, 6, radius, intr4)
    assert same.shape == (10, 96) and not same[:, 1].any() and not same[:, 3].any() and not same[:, 4:16].any()
    assert np.array_equal(same[:, 0], fwd[:, 0]) and np.array_equal(same[:, 0], same[:, 2]) and (same[:, 0] > 100).all()
    assert e.silhouette_normal_equations_reverse(own.bool(), near_t, rd, ri, joints, twists, 6, radius, intr4).tobytes() == same.tobytes()
    # the masks of the truth against renders at the start, four frames against the reference
    _, ti = e.render_batch_device(truth, 6, PV)
    mask_t = (ti < 6).to(torch.uint8).contiguous()
    got = e.silhouette_normal_equations_reverse(mask_t, near_t, rd, ri, joints, twists, 6, radius, intr4)
    s = slice(0, 4)
    _hold(got[s], mask_t[s].cpu().numpy(), near_t[s].cpu().numpy(), rd[s].cpu().numpy(), ri[s].cpu().numpy(), joints[s], twists[s], 6, intr4, radius)
    A, _ = sref.unpack(got[0])
    live = [0, 1, 2, 3, 4] + list(range(6, 12))
    assert (got[:, 2] > 100).all() and (np.diag(A)[live] > 0).all() and A[5, 5] == 0
    parts = [e.silhouette_normal_equations_reverse(mask_t[a:b].contiguous(), near_t[a:b].contiguous(), rd[a:b].contiguous(), ri[a:b].contiguous(),
                                                   joints[a:b], twists[a:b], 6, radius, intr4) for a, b in ((0, 3), (3, 10))]
    assert np.concatenate(parts).tobytes() == got.tobytes()
    assert e.silhouette_normal_equations_reverse(mask_t[:0], near_t[:0], rd[:0], ri[:0], joints[:0], twists[:0], 6, radius, intr4).shape == (0, 96)
    for bad in ((mask_t.float(), near_t, rd, ri), (mask_t, near_t.int(), rd, ri), (mask_t[:2], near_t, rd, ri), (mask_t, near_t[:, :50], rd, ri),
                (mask_t, near_t, rd.double(), ri), (mask_t.cpu(), near_t, rd, ri)):
        with pytest.raises(ValueError):
            e.silhouette_normal_equations_reverse(*bad, joints, twists, 6, radius, intr4)
    with pytest.raises(ValueError):
        e.silhouette_normal_equations_reverse(mask_t, near_t, rd, ri, None, None, 6, radius, intr4)
    with pytest.raises(ValueError):
        e.silhouette_normal_equations_reverse(mask_t, near_t, rd, ri, joints, twists, 6, 17, intr4)


# ---------------------------------------------------------------------------------------------- the refiner
@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_bundle_refiner_both_ways(renderer, mode):
    """Ten frames at 160 x 90, masks from renders at the truth, the start off the truth; the outline alone, both ways."""
    from rope_s3d_amd.prediction.refinement import BundleRefiner
    from rope_s3d_amd.projection import camera_matrix
    e, intr = renderer.engine, renderer.intrinsics
    truth, true_pose, start, start_pose = _scene(renderer)
    T_t, ti = e.render_batch_device(truth, 6, np.tile(camera_matrix(true_pose, intr)[None], (10, 1, 1)))
    mask = (ti < 6).cpu().numpy()
    res = BundleRefiner(renderer, intr, joints=mode, silhouette=1.0, both_ways=True).refine(start_pose, start, None, mask)
    print(mode, 'both ways: steps', res.steps_taken, 'cost', res.cost_silhouette_before, '->', res.cost_silhouette_after, 'inliers',
          res.inliers_silhouette, res.inliers_silhouette_reverse, 'pose error', np.abs(start_pose - true_pose), '->', np.abs(res.pose - true_pose))
    assert res.cost_silhouette_after < res.cost_silhouette_before and res.steps_taken >= 1
    assert res.inliers_silhouette_reverse > 0 and res.inliers_silhouette > 0
    with_depth = BundleRefiner(renderer, intr, joints=mode, silhouette=1.0, both_ways=True).refine(start_pose, start, T_t, torch.from_numpy(mask).cuda())
    assert with_depth.cost_silhouette_before == res.cost_silhouette_before and with_depth.inliers > 0 and with_depth.inliers_silhouette_reverse > 0
    # the switch off: every field has the bytes of a refiner built without the argument
    old = BundleRefiner(renderer, intr, joints=mode, silhouette=1.0).refine(start_pose, start, T_t, mask)
    off = BundleRefiner(renderer, intr, joints=mode, silhouette=1.0, both_ways=False).refine(start_pose, start, T_t, mask)
    for f in dataclasses.fields(old):
        a, b = getattr(old, f.name), getattr(off, f.name)
        assert (a is None and b is None) or np.asarray(a).tobytes() == np.asarray(b).tobytes(), f.name
    assert off.inliers_silhouette_reverse == 0


# ---------------------------------------------------------------------------------------------- the public interface
def test_calibrate_takes_both_ways_on_a_colour_coded_set(tmp_path):
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
    out = tmp_path / 'both.json'
    r = subprocess.run([sys.executable, os.path.join(root, 'calibrate.py'), 'synthetic:8', '-frames', '8', '-joints', 'frame', '-ds_factor', '8',
                        '-iterations', '2', '-silhouette', '1', '-both_ways', '-radius', '6', '-json', str(out)], cwd=root, capture_output=True, text=True)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'both ways' in r.stdout
    rep = json.loads(out.read_text())
    assert rep['silhouette'] == 1.0 and rep['both_ways'] is True and rep['radius'] == 6
    assert rep['inliers_silhouette'] > 0 and rep['inliers_silhouette_reverse'] > 0 and rep['inliers'] > 0
    far2 = (np.sqrt(37.0) - 0.5) ** 2                                     # the cost a step is judged by never grows
    assert rep['cost_after'] / 2.0 ** -10 + rep['cost_silhouette_after'] / far2 <= rep['cost_before'] / 2.0 ** -10 + rep['cost_silhouette_before'] / far2
    r = subprocess.run([sys.executable, os.path.join(root, 'calibrate.py'), 'synthetic:8', '-frames', '8', '-joints', 'frame', '-both_ways'],
                       cwd=root, capture_output=True, text=True)
    assert r.returncode != 0 and '-both_ways' in r.stderr


@pytest.mark.parametrize('mode', ['modelless', 'segmented'])
def test_predictor_switch_bundle_silhouette_both(mode):
    from rope_s3d_amd import CameraPredictor, ModellessCameraPredictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.prediction.refinement import BundleRefineResult
    from rope_s3d_amd.segmentation import ColorSegmenter
    from rope_s3d_amd.simulation.render import Renderer
    true_pose = np.array(DEFAULT_CAMERA_POSE, float) + TRUE_POSE_OFFSET
    r = Renderer('seg', true_pose, '640_480_color')
    lim = r.robot.joint_limits
    qs = np.random.default_rng(9).uniform(lim[:, 0] * .5, lim[:, 1] * .5, (4, 6)) * np.array([1, 1, 1, 0, 0, 0])
    colors, depths = [], []
    for q in qs:
        r.setJointAngles(q)
        c, d = r.render()
        colors.append(c); depths.append(np.asarray(d, np.float64))
    names = ['BG'] + list(r.robot.link_names[:6])
    r.engine.close()
    start = true_pose + np.array([.004, -.003, .003, .002, -.002, .002])
    kw = dict(base_intrinsics='640_480_color', refine='bundle+silhouette+both')
    p = ModellessCameraPredictor(start, 4, **kw) if mode == 'modelless' else CameraPredictor(start, 4, segmenter=ColorSegmenter(names), **kw)
    p.stages = [('descent', 6, 0.5, .001, [True] * 6, [0.002] * 6)]
    try:
        pose = p.run(np.stack(colors), np.stack(depths), qs.copy())
        res = p.last_refinement
        assert p.refine == 'bundle+silhouette+both' and isinstance(res, BundleRefineResult) and np.array_equal(pose, res.pose)
        assert p._robot_masks.shape == (4, 120, 160) and p._robot_masks.any(axis=(1, 2)).all()
        assert res.inliers_silhouette > 0 and res.inliers_silhouette_reverse > 0 and np.isfinite(res.cost_silhouette_before)
        far2 = (np.sqrt(65.0) - 0.5) ** 2
        assert res.cost_after / 2.0 ** -10 + res.cost_silhouette_after / far2 <= res.cost_before / 2.0 ** -10 + res.cost_silhouette_before / far2
    finally:
        p.engine.close()
