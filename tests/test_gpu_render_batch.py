"""Many poses to images in one launch: rope_render_batch (Engine.render_batch), Renderer.render_batch, DatasetRenderer,
RobotLookupCreator and the batched reads of SyntheticDataset — every image bit for bit what the one-pose render gives."""
import ctypes as C

import numpy as np
import pytest

from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR
from rope_s3d_amd.projection import camera_matrix

import helpers

pytestmark = pytest.mark.gpu

# a camera 0.12 m from the upper arm, tilted: triangles cross the near plane (tests/test_gpu_fullsize.py), so the clipping
# instantiation of the render launch runs
NEAR_POSE = [0.3, -0.12, 0.77, 0, 0.2, 0.3]
SIZES = [('1280_720_color', 8), ('640_480_color', 1), ('1280_720_color', 1)]


def make_engine(preset, ds, pose=DEFAULT_CAMERA_POSE):
    rb = helpers.robot()
    intr, PV = helpers.camera(preset, ds=ds, pose=pose)
    e = eng.Engine(0)
    e.set_robot(rb)
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    return e, intr, PV


def slu_poses(n, seed):
    lim = helpers.robot().joint_limits
    q = np.zeros((n, 6))
    q[:, :3] = np.random.default_rng(seed).uniform(lim[:3, 0], lim[:3, 1], (n, 3))
    return q


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('preset,ds', SIZES)
def test_batch_equals_single_renders(preset, ds):
    """64 poses, n_render 1 to 6: depth and ids equal Engine.render pose by pose; six of them equal the oracle too."""
    e, intr, PV = make_engine(preset, ds)
    q = slu_poses(66, 11)
    for n_render in range(1, 7):
        rows = q[n_render - 1::6]
        depth, ids = e.render_batch(rows, n_render)
        assert depth.shape == (len(rows), intr.height, intr.width) and ids.dtype == np.uint8
        for k, r in enumerate(rows):
            d1, i1 = e.render(r, n_render)
            assert same(depth[k], d1) and same(ids[k], i1), (n_render, k)
        if intr.width <= 640:
            o = helpers.make_oracle(helpers.robot(), intr, PV)
            d_ref, id_ref = o.render(rows[0], n_render)
            assert same(ids[0], id_ref) and same(depth[0].view(np.uint32), d_ref.view(np.uint32)), n_render
    assert (ids != 255).any()


def test_batch_past_the_fused_geometry_launch():
    """More than 256 rows: forward kinematics and boxes in their own launches; the images do not change."""
    e, intr, PV = make_engine('1280_720_color', 8)
    q = slu_poses(300, 12)
    depth, ids = e.render_batch(q, 6)
    for k in range(0, 300, 7):
        d1, i1 = e.render(q[k], 6)
        assert same(depth[k], d1) and same(ids[k], i1), k
    d_small, i_small = e.render_batch(q[:40], 6)
    assert same(d_small, depth[:40]) and same(i_small, ids[:40])


def test_per_pose_cameras_leave_the_context_camera_alone():
    e, intr, PV = make_engine('640_480_color', 2)
    rb = helpers.robot()
    q = slu_poses(12, 13)
    q[5] = 0
    poses = [DEFAULT_CAMERA_POSE, [0.2, -1.3, 0.9, 0.1, -0.2, 0.05], NEAR_POSE, [-0.4, -1.6, 0.6, 0, 0.1, -0.1]]
    cams = [poses[k % len(poses)] for k in range(12)]
    cams[5] = NEAR_POSE
    PVs = np.stack([camera_matrix(p, intr, ZNEAR, ZFAR) for p in cams])
    # what the context camera gives before the batch
    d0, i0 = e.render(q[0], 6)
    tq, t32, flags, *_ = helpers.synthetic_target(d0, i0)
    e.set_target(tq, t32, flags)
    cand = q[:8] + 0.05
    err0, sums0, _, _ = e.eval(cand, 6, eng.LOSS_FULL, want_sums=True)
    depth, ids = e.render_batch(q, 6, PV=PVs)
    assert (ids[5] != 255).mean() > 0.2                                # the near camera sees a good part of the robot
    ec = eng.Engine(0)
    ec.set_robot(rb)
    for k in range(12):
        ec.set_camera(PVs[k], intr.width, intr.height, ZNEAR, ZFAR)
        d1, i1 = ec.render(q[k], 6)
        assert same(depth[k], d1) and same(ids[k], i1), k
    # the batch's cameras did not replace the context's
    d2, i2 = e.render(q[0], 6)
    assert same(d2, d0) and same(i2, i0)
    err, sums, _, _ = e.eval(cand, 6, eng.LOSS_FULL, want_sums=True)
    assert same(sums, sums0) and same(err, err0)
    # only the default camera in the PV list: same images as no PV at all
    dd, ii = e.render_batch(q[:4], 6, PV=np.stack([PV] * 4))
    dn, inn = e.render_batch(q[:4], 6)
    assert same(dd, dn) and same(ii, inn)


def test_crop_and_chunks():
    e, intr, PV = make_engine('640_480_color', 1)
    q = slu_poses(20, 14)
    depth, ids = e.render_batch(q, 6)
    # a crop whose rows start on a multiple of four (wide stores) and one that does not
    for crop in ((40, 400, 64, 575), (3, 470, 5, 41), (0, 479, 0, 639), (100, 100, 7, 7)):
        r0, r1, c0, c1 = crop
        dc, ic = e.render_batch(q, 6, crop=crop)
        assert same(dc, np.ascontiguousarray(depth[:, r0:r1 + 1, c0:c1 + 1])), crop
        assert same(ic, np.ascontiguousarray(ids[:, r0:r1 + 1, c0:c1 + 1])), crop
    # one output only
    d_only, none = e.render_batch(q, 6, ids=False)
    none2, i_only = e.render_batch(q, 6, depth=False)
    assert none is None and none2 is None and same(d_only, depth) and same(i_only, ids)
    # N = 0: nothing is called
    d0, i0 = e.render_batch(np.zeros((0, 6)), 6)
    assert d0.shape == (0, 480, 640) and i0.shape == (0, 480, 640)
    # 1280x720: 128 poses are three chunks of the 256 MiB output budget (58 poses each)
    e2, intr2, PV2 = make_engine('1280_720_color', 1)
    q2 = slu_poses(128, 15)
    d2, i2 = e2.render_batch(q2, 6)
    for k in range(0, 128, 9):
        d1, i1 = e2.render(q2[k], 6)
        assert same(d2[k], d1) and same(i2[k], i1), k
    d3, i3 = e2.render_batch(q2[56:61], 6)                            # across the first chunk boundary, unchunked
    assert same(d3, d2[56:61]) and same(i3, i2[56:61])


def test_argument_errors_leave_the_context_usable():
    e, intr, PV = make_engine('1280_720_color', 8)
    q = slu_poses(3, 16)
    d0, i0 = e.render_batch(q, 6)
    lib, ctx = e._lib, e._ctx
    H, W = intr.height, intr.width
    depth = np.empty((3, H, W), np.float32)
    ids = np.empty((3, H, W), np.uint8)
    pq, pd, pi = eng._p(q), eng._p(depth), eng._p(ids)
    bad_pv = np.stack([PV] * 3)
    bad_pv[1, 2, 3] = np.nan
    bad_crop = np.array([0, H, 0, W - 1], np.int32)
    calls = [(None, None, 3, 6, None, pd, pi), (pq, None, 0, 6, None, pd, pi), (pq, None, -1, 6, None, pd, pi),
             (pq, None, 3, 6, None, None, None), (pq, None, 3, 0, None, pd, pi), (pq, None, 3, 7, None, pd, pi),
             (pq, None, 3, 6, eng._p(bad_crop), pd, pi), (pq, eng._p(bad_pv), 3, 6, None, pd, pi)]
    for args in calls:
        assert lib.rope_render_batch(ctx, *args) == -1, args
        assert lib.rope_last_error(ctx).decode().startswith('rope_render_batch:'), args
    fresh = eng.Engine(0)
    assert lib.rope_render_batch(fresh._ctx, pq, None, 3, 6, None, pd, pi) == -1
    assert b'robot and camera' in lib.rope_last_error(fresh._ctx)
    fresh.set_robot(helpers.robot())
    assert lib.rope_render_batch(fresh._ctx, pq, None, 3, 6, None, pd, pi) == -1
    d1, i1 = e.render_batch(q, 6)
    assert same(d1, d0) and same(i1, i0)
    with pytest.raises(eng.EngineError):
        e.render_batch(q, 6, crop=(0, H, 0, W - 1))
    with pytest.raises(ValueError):
        e.render_batch(q, 6, PV=np.stack([PV] * 2))


@pytest.mark.parametrize('mode,parts', [('seg', None), ('seg_full', None), ('real', None), ('seg', 3)])
def test_renderer_batch_equals_the_render_loop(mode, parts):
    from rope_s3d_amd.simulation.render import Renderer
    r = Renderer(mode, DEFAULT_CAMERA_POSE, '1280_720_color', intrinsic_ds_factor=8)
    if parts is not None:
        r.setMaxParts(parts)
    q = slu_poses(10, 17)
    cams = np.array([DEFAULT_CAMERA_POSE, [0.2, -1.3, 0.9, 0.1, -0.2, 0.05]] * 5, float)
    r.setJointAngles([0.1, 0.2, 0.3, 0, 0, 0])
    c_before, d_before = r.render()
    colors, depths = r.render_batch(q)
    colors_c, depths_c = r.render_batch(q, cams)
    assert colors.shape == (10, 90, 160, 3) and colors.dtype == np.uint8 and depths.dtype == np.float32
    # the renderer's own pose is as it was
    c_after, d_after = r.render()
    assert same(c_after, c_before) and same(d_after, d_before)
    for k in range(10):
        r.setJointAngles(q[k])
        c1, d1 = r.render()
        assert same(colors[k], c1) and same(depths[k], d1), k
        r.setCameraPose(cams[k])
        c1, d1 = r.render()
        assert same(colors_c[k], c1) and same(depths_c[k], d1), k
        r.setCameraPose(DEFAULT_CAMERA_POSE)
    d_ids, ids = r.render_ids_batch(q[:2])
    assert same(d_ids, depths[:2]) and ids.dtype == np.uint8


def test_dataset_renderer(tmp_path):
    from rope_s3d_amd.data.dataset import write_dataset
    from rope_s3d_amd.projection import Intrinsics
    from rope_s3d_amd.simulation import DatasetRenderer
    from rope_s3d_amd.simulation.render import Renderer
    intr = Intrinsics('1280_720_color')
    intr.downscale(8)
    n = 9
    q = slu_poses(n, 18)
    cams = np.array([DEFAULT_CAMERA_POSE, [0.2, -1.3, 0.9, 0.1, -0.2, 0.05], [-0.4, -1.6, 0.6, 0, 0.1, -0.1]] * 3, float)
    name = str(tmp_path / 'varying')
    write_dataset(name, np.zeros((n, intr.height, intr.width, 3), np.uint8), np.zeros((n, intr.height, intr.width)), q, cams, str(intr))
    dr = DatasetRenderer(name)
    ref = Renderer('seg', cams[0], str(intr))
    colors, depths = dr.render_range(2, 8)
    ci, di = dr.render_indices([8, 0])
    for i in range(n):
        ref.setJointAngles(q[i])
        ref.setCameraPose(cams[i])
        c1, d1 = ref.render()
        c, d = dr.render_at(i)
        assert same(c, c1) and same(d, d1), i
        if 2 <= i < 8:
            assert same(colors[i - 2], c1) and same(depths[i - 2], d1), i
    assert same(ci[0], dr.render_at(8)[0]) and same(di[1], dr.render_at(0)[1])
    dr.close()
    assert dr.ds is None
    # a synthetic name: frame i renders to what the set itself holds for it
    ds_name = 'synthetic:6:321:1280_720_color'
    sr = DatasetRenderer(ds_name)
    colors, depths = sr.render_range(0, 6)
    for i in (0, 3, 5):
        c, d = sr.render_at(i)
        assert same(c, sr.ds.og_img[i]) and same(d.astype(np.float64), sr.ds.depthmaps[i]), i
        assert same(colors[i], c) and same(depths[i], d), i
    sr.close()


def test_synthetic_dataset_slices_render_once():
    from rope_s3d_amd.data.dataset import SyntheticDataset
    ds = SyntheticDataset(12, '1280_720_color', seed=99)
    singles = [(ds.og_img[i], ds.depthmaps[i]) for i in range(12)]
    calls = []
    batch = ds._r.render_batch

    def counted(*a, **k):
        calls.append(1)
        return batch(*a, **k)
    ds._r.render_batch = counted
    og, dm = ds.og_img[2:9], ds.depthmaps[2:9]
    assert len(calls) == 1
    assert og.dtype == np.uint8 and dm.dtype == np.float64 and og.shape[0] == 7
    for k, i in enumerate(range(2, 9)):
        assert same(og[k], singles[i][0]) and same(dm[k], singles[i][1]), i
    og2 = ds.og_img[0:12:3]                                           # strided: frame by frame, as before
    assert all(same(og2[k], singles[3 * k][0]) for k in range(4))
    assert ds.og_img[5:5].shape == (0,) + og.shape[1:]


def test_make_synthetic_dataset_matches_the_lazy_frames(tmp_path):
    from rope_s3d_amd.data.dataset import Dataset, SyntheticDataset, make_synthetic_dataset
    d = make_synthetic_dataset(str(tmp_path / 'syn'), 5, '1280_720_color', seed=77)
    ds, lazy = Dataset(d), SyntheticDataset(5, '1280_720_color', seed=77)
    for i in range(5):
        assert same(np.asarray(ds.og_img[i]), lazy.og_img[i]) and same(np.asarray(ds.depthmaps[i]), lazy.depthmaps[i]), i


def test_lookup_creator_file(tmp_path):
    from rope_s3d_amd.crop import applyBatchCrop
    from rope_s3d_amd.data import hdf5
    from rope_s3d_amd.projection import Intrinsics
    from rope_s3d_amd.simulation import RobotLookupCreator
    from rope_s3d_amd.simulation.render import Renderer
    if not hdf5.available():
        pytest.skip("no libhdf5 on this machine")
    intr = Intrinsics('1280_720_color')
    intr.downscale(8)
    lc = RobotLookupCreator(np.array(DEFAULT_CAMERA_POSE, float), intr)
    lc.load_config(4, 'SLU', [4, 3, 3, 1, 1, 1])
    path = str(tmp_path / 'table.h5')
    lc.run(path, preview=True)
    full = lc._generate_depth_array()
    assert full.shape == (36, 90, 160) and full.dtype == np.float64
    ref = Renderer('seg', DEFAULT_CAMERA_POSE, intr)
    ref.setMaxParts(4)
    crop = lc.crop
    with hdf5.H5File(path) as f:
        a = f.attrs
        assert a['num_links_rendered'] == 4 and np.array_equal(a['divisions'], [4, 3, 3, 1, 1, 1])
        assert np.array_equal(a['angles_changed'], [1, 1, 1, 0, 0, 0]) and a['intrinsics'] == str(lc.intrinsics)
        assert np.array_equal(a['pose'], DEFAULT_CAMERA_POSE) and a['urdf'] == lc.u_reader.name
        angles, depth = f['angles'][:], f['depth'][:]
    assert depth.dtype == np.float64 and depth.shape == (36, crop[1] - crop[0] + 1, crop[3] - crop[2] + 1)
    assert np.array_equal(angles, lc.angles)
    for k in range(36):
        ref.setJointAngles(angles[k])
        d = ref.render()[1]
        assert same(depth[k], applyBatchCrop(d[None].astype(np.float64), crop)[0].copy()), k
        assert same(full[k], d.astype(np.float64)), k
    assert (depth > 0).any()
