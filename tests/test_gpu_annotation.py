"""Annotation on the device: rope_render_masks (Engine.render_masks, Renderer.render_masks_batch) against the host dilation of
the ids rope_render_batch draws, and AutomaticAnnotator.run against Annotator.annotate on colour renders, file for file."""
import os

import numpy as np
import pytest

from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR
from rope_s3d_amd.data import annotation as ann
from rope_s3d_amd.projection import camera_matrix

import helpers

pytestmark = pytest.mark.gpu

# a camera 0.12 m from the upper arm: triangles cross the near plane, the clipping kernels draw (tests/test_gpu_render_batch.py)
NEAR_POSE = [0.3, -0.12, 0.77, 0, 0.2, 0.3]
SIZES = [('1280_720_color', 8), ('640_480_color', 1), ('1280_720_color', 1)]
LABELINGS = [(4, np.arange(4)), (6, np.arange(6)), (6, np.zeros(6))]        # 'seg' with setMaxParts(4), 'seg', 'seg_full'


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


def views(intr, n, seed):
    rng = np.random.default_rng(seed)
    poses = np.asarray(DEFAULT_CAMERA_POSE, float) + rng.uniform(-0.15, 0.15, (n, 6)) * [1, 1, 1, 0.3, 0.3, 0.3]
    return np.stack([camera_matrix(p, intr, ZNEAR, ZFAR) for p in poses])


def host_masks(ids, labels, pad):
    """What Annotator._mask_color gives for every label at once: id -> label bits, then cv2's dilation."""
    lut = np.zeros(256, np.uint8)
    lut[:len(labels)] = 1 << np.asarray(labels, np.uint8)
    return np.stack([ann.dilate(lut[i], pad) for i in ids])


def host_boxes(masks):
    out = np.full((len(masks), 8, 4), -1, np.int32)
    for k, m in enumerate(masks):
        for b in range(8):
            r, c = np.nonzero((m >> b) & 1)
            if len(r):
                out[k, b] = (r.min(), r.max(), c.min(), c.max())
    return out


def check(e, q, n_render, labels, pad, PV=None):
    masks, boxes = e.render_masks(q, n_render, labels, pad, PV)
    _, ids = e.render_batch(q, n_render, PV, depth=False)
    want = host_masks(ids, labels, pad)
    assert masks.shape == want.shape and masks.tobytes() == want.tobytes(), (n_render, pad, PV is not None)
    assert np.array_equal(boxes, host_boxes(want)), (n_render, pad)
    return masks


@pytest.mark.parametrize('preset,ds', SIZES)
def test_masks_equal_host_dilation(preset, ds):
    """Every pad, labelling and camera choice: the device planes and boxes equal the host dilation of the same ids."""
    e, intr, _ = make_engine(preset, ds)
    n = 4 if intr.width > 640 else 10
    q = slu_poses(n, 3)
    PVs = views(intr, n, 4)
    seen = 0
    for pad in (1, 3, 4, 5, 9):
        for n_render, labels in LABELINGS:
            for PV in (None, PVs):
                seen |= np.bitwise_or.reduce(check(e, q, n_render, labels, pad, PV), axis=None)
    assert seen == 0b111111                                   # every link's bit was drawn somewhere


@pytest.mark.parametrize('W,H', [(131, 37), (126, 45)])
def test_masks_at_widths_off_a_multiple_of_four(W, H):
    """Sizes no preset produces (rope_set_camera admits any): at W % 4 != 0 the label planes are stored byte by byte and the last
    word of a row is partial; pad 64 is the tallest halo."""
    from rope_s3d_amd.projection import Intrinsics, view_matrix
    e, _, _ = make_engine('640_480_color', 1)
    it = Intrinsics('640_480_color')
    dx, dy = 640 / W, 480 / H                                 # the preset's whole view on W x H pixels that are not square
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2 * it.fx / dx / W, 2 * it.fy / dy / H
    P[0, 2], P[1, 2] = 1 - 2 * it.cx / dx / W, 2 * it.cy / dy / H - 1
    P[2, 2], P[2, 3], P[3, 2] = (ZFAR + ZNEAR) / (ZNEAR - ZFAR), 2 * ZFAR * ZNEAR / (ZNEAR - ZFAR), -1
    e.set_camera(P @ view_matrix(np.asarray(DEFAULT_CAMERA_POSE, float)), W, H, ZNEAR, ZFAR)
    assert (e.W, e.H) == (W, H) and W % 4
    q = slu_poses(5, 9)
    seen = 0
    for pad in (3, 64):
        seen |= np.bitwise_or.reduce(check(e, q, 6, np.arange(6), pad), axis=None)
    assert seen == 0b111111


def test_chunk_boundary_fullsize():
    """160 poses at 1280x720 need two chunks (256 MiB for the id and label planes of each pose)."""
    e, intr, _ = make_engine('1280_720_color', 1)
    q = slu_poses(160, 5)
    masks, boxes = e.render_masks(q, 6, np.arange(6), 5)
    _, ids = e.render_batch(q, 6, depth=False)
    for k in (0, 1, 144, 145, 146, 159):
        want = host_masks(ids[k:k + 1], np.arange(6), 5)
        assert masks[k].tobytes() == want[0].tobytes(), k
        assert np.array_equal(boxes[k:k + 1], host_boxes(want)), k
    assert (masks != 0).any(axis=(1, 2)).all()


def test_near_camera_selects_clipping():
    """A camera close enough to the arm for triangles to reach the near plane: the clipping raster path, same masks."""
    e, intr, PV = make_engine('640_480_color', 1, NEAR_POSE)
    q = slu_poses(8, 6)
    check(e, q, 6, np.arange(6), 3)
    e2, _, _ = make_engine('640_480_color', 1)
    check(e2, q, 6, np.arange(6), 3, np.stack([PV] * len(q)))


def test_render_batch_unchanged_after_masks():
    e, intr, _ = make_engine('640_480_color', 1)
    q = slu_poses(6, 7)
    d0, i0 = e.render_batch(q, 6)
    e.render_masks(q[::-1], 4, np.arange(4), 9, views(intr, 6, 8))
    d1, i1 = e.render_batch(q, 6)
    assert d0.tobytes() == d1.tobytes() and i0.tobytes() == i1.tobytes()


def test_arguments_refused():
    e, _, _ = make_engine('1280_720_color', 8)
    q = slu_poses(2, 1)
    with pytest.raises(eng.EngineError):
        e.render_masks(q, 6, np.arange(6), 0)
    with pytest.raises(eng.EngineError):
        e.render_masks(q, 6, np.arange(6), 65)
    with pytest.raises(eng.EngineError):
        e.render_masks(q, 6, [0, 1, 2, 3, 4, 8], 3)


def test_automatic_annotator_matches_host_path(tmp_path):
    """24 synthetic frames at 640x480: the device path writes 24 JSON + PNG pairs, split, byte for byte what Annotator.annotate
    writes from Renderer.render colours at the same poses and paths; the renderer's own pose is as it was."""
    from rope_s3d_amd.simulation.render import DatasetRenderer, Renderer
    dest = str(tmp_path / 'link_annotations')
    rend = DatasetRenderer('synthetic:24')
    rend.setJointAngles([0.2, 0.1, 0.3, 0, 0, 0])
    before = (rend._angles.copy(), rend._camera_pose6.copy(), rend.render()[0])
    auto = ann.AutomaticAnnotator('synthetic:24', rend, preview=True, dest_path=dest)
    auto.run()
    assert np.array_equal(rend._angles, before[0]) and np.array_equal(rend._camera_pose6, before[1])
    assert np.array_equal(rend.render()[0], before[2])
    assert os.path.isfile(os.path.join(dest, 'split.json'))
    where = {}
    for sub in ('train', 'test', 'ignore'):
        for f in os.listdir(os.path.join(dest, sub)):
            where.setdefault(f, sub)
    assert len(where) == 48 and sum(f.endswith('.json') for f in where) == 24
    assert len(os.listdir(os.path.join(dest, 'train'))) == 2 * int(24 * .4)
    ds = auto.ds
    host = Renderer('seg', ds.camera_pose[0], ds.intrinsics)
    a = ann.Annotator(pad_size=3, color_dict=host.color_dict)
    assert a.color_dict == auto.anno.color_dict
    og = np.asarray(ds.og_img[:])
    n_shapes = 0
    for f in range(24):
        host.setJointAngles(ds.angles[f])
        host.setCameraPose(ds.camera_pose[f])
        color, _ = host.render()
        path = os.path.join(dest, f'{f:05d}')                  # the same path string as the device run wrote into the JSON
        a.annotate(og[f], color, path)
        for ext in ('.json', '.png'):
            got = open(os.path.join(dest, where[f'{f:05d}{ext}'], f'{f:05d}{ext}'), 'rb').read()
            assert got == open(path + ext, 'rb').read(), (f, ext)
        n_shapes += open(path + '.json').read().count('"shape_type"')
    assert n_shapes >= 24
