"""Mask R-CNN training on the device: the target kernels against their host restatements, the float32 RoIAlign pair against the
tensor formulation and autograd, a short overfit run, and train.py's function end to end into the prediction path's loader."""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def frames(tmp_path_factory):
    """8 annotated synthetic frames at 640x480 (AutomaticAnnotator output, read back through data/labelme.py) plus one frame
    without any instance."""
    torch.cuda.init()                                   # torch's context before the engine's
    from rope_s3d_amd.data.annotation import AutomaticAnnotator
    from rope_s3d_amd.data.labelme import read_annotation
    from rope_s3d_amd.robot import RobotModel
    dest = str(tmp_path_factory.mktemp('anno') / 'link_annotations')
    AutomaticAnnotator('synthetic:8', preview=False, dest_path=dest).run()
    names = list(RobotModel.from_urdf().link_names[:6])
    files = sorted(os.path.join(dest, s, f) for s in ('train', 'test', 'ignore') for f in os.listdir(os.path.join(dest, s)) if f.endswith('.json'))
    out = [read_annotation(f, names) for f in files]
    assert sum(len(o[2]) for o in out) >= 8
    img = out[0][0].copy()
    out.append((img, np.zeros((0,) + img.shape[:2], bool), np.zeros(0, np.int32)))
    return out


def _ulp_close(a, b, ulps=1):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        ia, ib = a.view(np.int64), b.view(np.int64)
    else:
        ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return bool(np.all(np.abs(ia - ib) <= ulps))


def test_target_kernels_equal_host(frames):
    from rope_s3d_amd import maskrcnn as mr
    from rope_s3d_amd import training as tr
    torch.manual_seed(0)
    net = mr.MaskRCNN(7).cuda()
    trainer = tr.MaskRCNNTrainer(net, layers='heads', seed=1, augmentation=False)
    x, gt, cls, gm, cnt = trainer._prepare(frames, False)
    assert cnt[-1] == 0 and cnt[:-1].min() > 0
    B, A = len(frames), len(trainer._anchors)
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 2 ** 32, (B, A), dtype=np.uint32)
    match, bbox, _ = tr.rpn_targets_device(trainer._anchors, torch.from_numpy(gt.astype(np.float64)).cuda(), torch.from_numpy(cnt).cuda(),
                                           torch.from_numpy(keys.view(np.int32)).cuda())
    match, bbox = match.cpu().numpy(), bbox.cpu().numpy()
    an = trainer._anchors.cpu().numpy()
    for f in range(B):
        m, b, _ = tr.rpn_targets_host(an, gt[f, :cnt[f]].astype(np.float64), keys[f])
        assert np.array_equal(match[f], m), f
        assert np.array_equal(bbox[f, :, :2].view(np.int64), b[:, :2].view(np.int64)), f
        assert _ulp_close(bbox[f, :, 2:], b[:, 2:]), f                 # log: the device's and the host's libm, 1 ulp apart at most
    # detection targets: proposals scattered around the GT boxes plus random ones, 2000 per frame, fewer in one frame
    gtn = np.stack([tr.norm_boxes(gt[f], (512, 512)) for f in range(B)])
    props = np.zeros((B, 2000, 4), np.float32)
    count = np.full(B, 2000, np.int32)
    count[1] = 777
    for f in range(B):
        c = rng.uniform(0, 1, (2000, 2)).astype(np.float32)
        s = rng.uniform(0.02, 0.4, (2000, 2)).astype(np.float32)
        p = np.concatenate([c - s / 2, c + s / 2], 1).clip(0, 1)
        if cnt[f]:
            near = gtn[f, rng.integers(0, cnt[f], 600)] + rng.normal(0, 0.01, (600, 4)).astype(np.float32)
            p[:600] = near.clip(0, 1)
        props[f] = p.astype(np.float32)
        props[f, count[f]:] = 0
    pkeys = rng.integers(0, 2 ** 32, (B, 2000), dtype=np.uint32)
    d = [torch.from_numpy(a).cuda() for a in (props, count, gtn, cls, cnt, gm, pkeys.view(np.int32))]
    rois, tcls, deltas, masks = [t.cpu().numpy() for t in tr.roi_targets_device(*d)]
    n_pos = 0
    for f in range(B):
        r, c, dl, mk = tr.roi_targets_host(props[f, :count[f]], gtn[f, :cnt[f]], cls[f, :cnt[f]], gm[f, :cnt[f]], pkeys[f])
        assert np.array_equal(rois[f].view(np.int32), r.view(np.int32)), f
        assert np.array_equal(tcls[f], c), f
        assert np.array_equal(deltas[f].view(np.int32), dl.view(np.int32)), f
        assert np.array_equal(masks[f], mk), f
        n_pos += int((c > 0).sum())
    assert n_pos > 0 and not rois[-1].any()
    # an IoU of 0/0: a zero-area GT (a one-pixel-thin mask) against zero-area proposals that miss it counts as no overlap
    g = np.array([[[0.2, 0.2, 0.2, 0.6], [0.5, 0.5, 0.7, 0.7]]], np.float32)
    pr = np.zeros((1, 2000, 4), np.float32)
    pr[0, :10] = [0.9, 0.1, 0.9, 0.3]
    pr[0, 10:20] = g[0, 1] + 0.001
    k = rng.integers(0, 2 ** 32, (1, 2000), dtype=np.uint32)
    gmk = np.zeros((1, 2, 512, 512), np.uint8)
    gmk[0, 0, 102, 102:307] = 1
    gmk[0, 1, 256:358, 256:358] = 1
    d = [torch.from_numpy(a).cuda() for a in (pr, np.array([20], np.int32), g, np.array([[2, 4]], np.int32), np.array([2], np.int32), gmk,
                                                k.view(np.int32))]
    got = [t.cpu().numpy()[0] for t in tr.roi_targets_device(*d)]
    want = tr.roi_targets_host(pr[0, :20], g[0], np.array([2, 4], np.int32), gmk[0], k[0])
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert (want[1] == 4).sum() == 10 and want[0][10:20].any(1).all()        # 10 positives, the 10 0/0 proposals negatives


def _pyramid(B, C=256, size=512, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [torch.randn(B, C, size // s, size // s, device='cuda', generator=g) for s in (4, 8, 16, 32, 64)]


def _boxes_all_levels(K, seed=0):
    rng = np.random.default_rng(seed)
    sides = np.array([0.08, 0.22, 0.44, 0.9])[rng.integers(0, 4, K)]        # levels 2..5 by area
    c = rng.uniform(-0.1, 1.1, (K, 2))                                      # some samples off the map
    b = np.concatenate([c - sides[:, None] / 2, c + sides[:, None] / 2], 1).astype(np.float32)
    return torch.from_numpy(b).cuda()


def test_roi_align_f32_forward_and_backward():
    """Forward: bit-equal to maskrcnn._roi_align's tensor formulation on float32 rows (the same IEEE operations in the same
    order).  Backward: within relative 1e-5 of autograd through that formulation (atomic adds sum in another order); the tight
    per-element bound, other channel counts and non-square levels are in tests/test_gpu_train_kernels.py."""
    from rope_s3d_amd import maskrcnn as mr
    from rope_s3d_amd import training as tr
    torch.cuda.init()
    B, K = 2, 300
    feats = _pyramid(B)
    boxes = _boxes_all_levels(K)
    frame = torch.arange(K, device='cuda') % B
    h = boxes[:, 2] - boxes[:, 0]
    lv = (4 + torch.log2((h * h).sqrt() / (224.0 / 512)).round()).clamp(2, 5)
    assert set(lv.long().tolist()) == {2, 3, 4, 5}
    for pool in (7, 14):
        f1 = [f.clone().requires_grad_(True) for f in feats]
        ref = mr._roi_align(f1, boxes, pool, 512, frame)
        f2 = [f.clone().requires_grad_(True) for f in feats]
        got = tr.roi_align_train(f2, boxes, pool, 512, frame)
        assert torch.equal(got, ref), pool
        w = torch.randn_like(ref)
        (ref * w).sum().backward()
        (got * w).sum().backward()
        for a, b in zip(f1[:4], f2[:4]):
            scale = a.grad.abs().max()
            assert float((a.grad - b.grad).abs().max()) <= 1e-5 * float(scale), pool


def test_overfit_four_frames(frames):
    """4 annotated frames, layers='heads', 60 steps of batch 4 at 512: the total loss ends (mean of the last 5 steps) at most
    half the mean of the first 5, every loss finite.  The curve is printed."""
    from rope_s3d_amd import maskrcnn as mr
    from rope_s3d_amd import training as tr
    torch.manual_seed(0)
    net = mr.MaskRCNN(7).cuda()
    trainer = tr.MaskRCNNTrainer(net, layers='heads', seed=0, augmentation=False)
    batch = [f for f in frames if len(f[2])][:4]
    t0, curve = time.time(), []
    for _ in range(60):
        out = trainer.step(batch)
        assert all(np.isfinite(out[k]) for k in tr.LOSS_NAMES), out
        curve.append(out['loss'])
    torch.cuda.synchronize()
    dt = time.time() - t0
    print("overfit curve:", ' '.join(f'{v:.3f}' for v in curve), f"({dt:.1f} s)")
    assert dt < 60
    assert np.mean(curve[-5:]) <= 0.5 * np.mean(curve[:5])


def test_train_end_to_end(frames, tmp_path, monkeypatch):
    """train.py's function: 1 epoch on a tiny annotated synthetic set writes a checkpoint into a new model folder;
    Predictor(model_ds=<that set>) loads it through its unchanged _load_segmenter and predicts a frame through the segmentation
    path."""
    monkeypatch.setenv('ROPE_MODELS', str(tmp_path / 'models'))
    monkeypatch.setenv('ROPE_OUTPUT', str(tmp_path / 'output'))
    import importlib.util
    from rope_s3d_amd import Predictor
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    from rope_s3d_amd.data.annotation import AutomaticAnnotator
    from rope_s3d_amd.maskrcnn import MaskRCNNSegmenter, load_matterport_weights
    from rope_s3d_amd.models import ModelData, ModelManager
    auto = AutomaticAnnotator('synthetic:20', preview=False)
    auto.run()
    spec = importlib.util.spec_from_file_location('train_cli', os.path.join(os.path.dirname(os.path.dirname(__file__)), 'train.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    dest = cli.train('synthetic:20', batch=2, epochs=1)
    assert any(f.startswith('mask_rcnn_model.001-') for f in os.listdir(dest))
    md = ModelData(dest)
    assert md.dataset_size == 20 and md.train_size == int(20 * .4) and md.valid_size > 0
    path = ModelManager().dynamicLoad(dataset='synthetic:20')
    assert path is not None and os.path.dirname(path) == os.path.abspath(dest)
    p = Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', model_ds='synthetic:20', lookup_divisions=4)
    assert isinstance(p.seg, MaskRCNNSegmenter)
    want = load_matterport_weights(path, 7)['mask.14.weight'].to(p.seg.net.mask[14].weight.dtype)
    assert torch.equal(p.seg.net.mask[14].weight.detach().cpu(), want)          # the trained head, not a random one
    ds = auto.ds
    color, depth = np.asarray(ds.og_img[0]), np.asarray(ds.depthmaps[0]).astype(np.float64)
    angles = p.run(color, depth)
    assert np.asarray(angles).shape == (6,) and np.all(np.isfinite(angles))
