"""GPU: rope_shade_frames (csrc/rope_shade.hip) against the numpy restatement of its contract (tests/shade_ref.py), byte for byte
and word for word, at the shapes where its tiles (16 rows x 256 columns), its 4-pixel chunks and its alignment rules change path;
then the layers above it: Renderer.render_photo_batch_device, PhotoDataset, and the annotator and evaluator on a 'photo:' set."""
import glob
import json
import os

import numpy as np
import pytest

import shade_ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

INTR = (310.0, 305.0, 7.25, 4.5)
SEED = 0x123456789ABCDEF
# 1-pixel edges; chunk - 1, chunk, chunk + 1 columns; tile - 1, tile, tile + 1 in both; several tiles with an odd plane size
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 9), (2, 3), (2, 4), (3, 5), (15, 255), (16, 256), (17, 257), (33, 515)]


@pytest.fixture(scope='module')
def engine():
    from rope_s3d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _records(n, n_bg=2):
    """Records that differ in everything: flat colour / picture 0 / picture 1, with and without noise, lights on and off axis."""
    from rope_s3d_amd.simulation.shading import draw_params, default_params, unit_light
    p = draw_params(77, np.arange(n), 6, n_bg)
    p['bg_index'] = np.arange(n) % (n_bg + 1) - 1
    p['noise_q'] = [0 if m % 3 == 0 else (1023 if m % 3 == 1 else 37) for m in range(n)]
    p[0]['light'] = unit_light([0, 0, 1])
    if n > 1:
        p[1]['light'] = unit_light([.8, -.5, .3])
    p[n - 1]['gain'] = (1.6, .4, 1.0)                      # clamps at 255
    p[0]['albedo'] = default_params(1)[0]['albedo']
    return p


def _scene(H, W, n=3, seed=0):
    rng = np.random.default_rng((seed, H, W))
    planes = [shade_ref.blob_scene(rng, H, W) for _ in range(n)]
    backs = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    return np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes]), backs


def _offset(a, off):
    """The array's bytes on the device at `off` bytes past an aligned allocation."""
    flat = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    buf = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device='cuda')
    buf[off:off + flat.numel()] = flat.cuda()
    return buf[off:off + flat.numel()].view(a.shape)


def _gpu(engine, depth, ids, params, backs, frame0=0, seed=SEED, off=0, alias=False):
    N, H, W = depth.shape
    d = torch.from_numpy(depth).cuda()
    out = torch.zeros(N * H * W * 3 + 16, dtype=torch.uint8, device='cuda')[off:off + N * H * W * 3].view(N, H, W, 3)
    bgr, dout = engine.shade_frames(d, _offset(ids, off), params, INTR, 6, _offset(backs, off) if backs is not None else None, frame0, seed,
                                    depth_out=d if alias else True, out=out)
    torch.cuda.synchronize()
    assert bgr.data_ptr() % 4 == off % 4 and (not alias or dout.data_ptr() == d.data_ptr())
    return bgr.cpu().numpy(), dout.cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert got[1].view(np.uint32).tobytes() == want[1].view(np.uint32).tobytes()


@pytest.mark.parametrize('H,W', SHAPES)
def test_kernel_equals_reference(engine, H, W):
    depth, ids, backs = _scene(H, W)
    params = _records(3)
    want = shade_ref.shade_frames(depth, ids, INTR, params, 6, backs, 5, SEED)
    _same(_gpu(engine, depth, ids, params, backs, 5), want)
    _same(_gpu(engine, depth, ids, params, backs, 5, alias=True), want)          # depth_out written over depth_dev
    if (H, W) in ((5, 9), (17, 257), (16, 256)):
        for off in (1, 3):                                                        # byte planes at odd base addresses
            _same(_gpu(engine, depth, ids, params, backs, 5, off=off), want)


def test_nan_depth_and_no_depth_out(engine):
    depth, ids, backs = _scene(9, 21)
    depth[1, 5, 5], ids[1, 4:7, 4:7] = np.nan, 2
    params = _records(3)
    want = shade_ref.shade_frames(depth, ids, INTR, params, 6, backs, 0, SEED)
    assert (want[0][1, 5, 5] == 0).all() or params[1]['noise_q'] > 0
    got = _gpu(engine, depth, ids, params, backs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
    d = torch.from_numpy(depth).cuda()
    bgr, none = engine.shade_frames(d, torch.from_numpy(ids).cuda(), params, INTR, 6, torch.from_numpy(backs).cuda(), 0, SEED, depth_out=False)
    assert none is None and np.array_equal(bgr.cpu().numpy(), want[0]) and np.array_equal(d.cpu().numpy(), depth, equal_nan=True)
    empty = engine.shade_frames(d[:0], torch.from_numpy(ids).cuda()[:0], params[:0], INTR, 6)
    assert empty[0].shape == (0, 9, 21, 3) and empty[1].shape == (0, 9, 21)
    with pytest.raises(ValueError):
        engine.shade_frames(d, torch.from_numpy(ids).cuda(), params, INTR, 6, None, 0, SEED)       # bg_index >= 0 without pictures


def test_batches_do_not_change_a_pixel(engine):
    depth, ids, backs = _scene(19, 37, n=36)                                       # more frames than one launch carries records for
    params = _records(36)
    whole = _gpu(engine, depth, ids, params, backs)
    for a, b in ((0, 2), (2, 4), (30, 36)):
        part = _gpu(engine, depth[a:b], ids[a:b], params[a:b], backs, frame0=a)
        _same(part, (whole[0][a:b], whole[1][a:b]))
    _same((whole[0][30:], whole[1][30:]), shade_ref.shade_frames(depth[30:], ids[30:], INTR, params[30:], 6, backs, 30, SEED))
    other = _gpu(engine, depth[:2], ids[:2], params[:2], backs, frame0=1)
    assert not np.array_equal(other[0][1], whole[0][1])                             # frame 1 has noise: another frame index, other noise


@pytest.fixture(scope='module')
def renderer():
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.simulation.render import Renderer
    return Renderer('seg', DEFAULT_CAMERA_POSE, '640_480_color', intrinsic_ds_factor=4)


def test_render_photo_equals_reference_on_real_renders(renderer):
    from rope_s3d_amd.simulation.shading import draw_params, make_backgrounds
    r = renderer
    H, W = r.resolution
    angles = np.array([[0.3, 0.2, -0.4, 0, 0.5, 0], [-1.1, 0.6, 0.3, 0.2, -0.3, 0]])
    params, backs = draw_params(3, [4, 5], 6, 2), make_backgrounds(3, 2, H, W)
    params['noise_q'] = (0, 60)
    depth, ids = (t.cpu().numpy() for t in r.render_ids_batch_device(angles))
    assert (ids < 6).sum() > 200
    intr = (r.intrinsics.fx, r.intrinsics.fy, r.intrinsics.cx, r.intrinsics.cy)
    want = shade_ref.shade_frames(depth, ids, intr, params, 6, backs, 4, 3)
    bgr, dout, ids_t = r.render_photo_batch_device(angles, None, params, backs, frame0=4, seed=3)
    _same((bgr.cpu().numpy(), dout.cpu().numpy()), want)
    assert np.array_equal(ids_t.cpu().numpy(), ids)
    host = r.render_photo_batch(angles, None, params, backs, frame0=4, seed=3)
    assert np.array_equal(host[0], want[0]) and host[1].dtype == np.float32 and host[2].dtype == np.uint8
    # the default scene is shade_depth's: the pictures of mode 'real', to a grey level — except where the depth steps inside one link
    # so far that the estimated normal faces away from the camera: shade_depth lights both sides (|n.z|), the contract one
    # (light from behind leaves the ambient level, rint(200 * 0.12) = 24)
    from rope_s3d_amd.simulation.render import shade_depth
    grey = r.render_photo_batch(angles)[0]
    for k in range(2):
        off = np.abs(grey[k].astype(int) - shade_depth(depth[k], ids[k], r.intrinsics).astype(int)).max(axis=-1) > 1
        assert (grey[k][off] == 24).all() and not off.all()


@pytest.fixture(scope='module')
def photo6():
    from rope_s3d_amd.data.dataset import open_dataset
    return open_dataset('photo:6')


def test_photo_dataset_frames_are_the_same_bytes_however_read(photo6):
    from rope_s3d_amd.data.dataset import PhotoDataset, SyntheticDataset
    ds = photo6
    assert isinstance(ds, PhotoDataset) and ds.attrs['synthetic'] is False and ds.attrs['rendered'] is True and 'color_dict' not in ds.attrs
    assert len(ds) == 6 and ds.og_img.shape == (6, 480, 640, 3) and ds.depthmaps.dtype == np.float64
    one, run = ds.og_img[2], ds.og_img[1:4]
    assert np.array_equal(one, run[1]) and np.array_equal(ds.depthmaps[2], ds.depthmaps[1:4][1])
    again = PhotoDataset.from_name('photo:6')
    assert np.array_equal(again.og_img[2], one) and np.array_equal(again.angles, ds.angles)
    assert np.array_equal(ds.angles, SyntheticDataset.from_name('synthetic:6').angles)
    assert not np.array_equal(PhotoDataset.from_name('photo:6:5').og_img[2], one)
    from rope_s3d_amd.simulation.shading import draw_params
    ids = ds._r.render_ids_batch(ds.angles[1:4])[1]
    dm, bg_depth = ds.depthmaps[1:4], draw_params(ds.seed, [1, 2, 3], 6, ds.n_backgrounds)['bg_depth']
    for k in range(3):
        assert (dm[k][ids[k] >= 6] == np.float64(bg_depth[k])).all() and (dm[k][ids[k] < 6] < 3.0).all()
    assert len(np.unique(one.reshape(-1, 3), axis=0)) > 500                          # a picture, not a colour table
    holed = PhotoDataset(6, holes=True)
    assert np.array_equal(holed.og_img[2], one) and (holed.depthmaps[2] == 0).any() and not (ds.depthmaps[2] == 0).any()
    assert np.array_equal(holed.depthmaps[2], holed.depthmaps[2:4][0])


def test_annotator_on_photo_set_traces_the_synthetic_sets_polygons(tmp_path):
    from rope_s3d_amd.data import annotation as ann
    shapes = {}
    for name in ('photo:4', 'synthetic:4'):
        dest = str(tmp_path / name.split(':')[0])
        ann.AutomaticAnnotator(name, preview=False, dest_path=dest).run()
        files = sorted(glob.glob(os.path.join(dest, '*', '*.json')), key=os.path.basename)
        assert [os.path.basename(f) for f in files] == [f'{i:05d}.json' for i in range(4)]
        shapes[name] = [json.load(open(f))['shapes'] for f in files]
    assert shapes['photo:4'] == shapes['synthetic:4'] and all(len(s) for s in shapes['photo:4'])


class _RenderSegmenter:
    """batches_device of MaskRCNNSegmenter answering with the render's own masks, frame after frame."""
    device = 'cuda:0'

    def __init__(self, gt, n_classes):
        self.gt, self.n = gt, n_classes

    def batches_device(self, groups):
        at = 0
        for g in groups:
            out = []
            for plane in self.gt[at:at + len(g)]:
                labels = [b for b in range(self.n) if ((plane >> b) & 1).any()]
                masks = np.stack([((plane >> b) & 1).astype(bool) for b in labels]) if labels else np.zeros((0,) + plane.shape, bool)
                out.append({'class_ids': np.array([b + 1 for b in labels], np.int32), 'scores': np.array([.9 - .01 * b for b in labels], np.float32),
                            'masks_device': torch.from_numpy(masks).cuda(), 'masks_stacked': None})
            at += len(g)
            yield out


def test_evaluator_on_photo_set_with_the_renders_own_masks():
    from rope_s3d_amd import evaluation as ev
    from rope_s3d_amd.data.dataset import open_dataset
    from rope_s3d_amd.robot import RobotModel
    names = list(RobotModel.from_urdf().link_names[:6])
    gt = ev.gt_from_renders('photo:4', np.arange(4))
    colors = np.asarray(open_dataset('photo:4').og_img[:])
    got = ev.SegmentationEvaluator(_RenderSegmenter(gt, 6), names, 2).run(colors, gt)
    assert got['frames'] == 4 and got['frames_skipped'] == 0 and got['AP'] == got['AP50'] == got['AP75'] == 1.0
