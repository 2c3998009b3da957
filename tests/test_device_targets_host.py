"""CPU: the host side of the device-built targets (rope_stage_targets_segmented): the ABI is declared and bound, the network can
leave its masks where they were computed, and Predictor(device_targets=True) without a segmenter that does so is the host path."""
import os
import re

import numpy as np

from rope_s3d_amd import engine as eng

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))


def test_header_declares_and_the_binding_knows_both_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'rope_s3d.h')).read()
    decl = re.search(r'int rope_stage_targets_segmented\(([^;]*)\);', hdr)
    assert decl and len(decl.group(1).split(',')) == 12
    for arg in ('int n_total', 'int slot0', 'int n_frames', 'const void *depth_dev', 'int depth_kind', 'const uint8_t *masks_dev',
                'const int32_t *inst_first', 'const int32_t *link_of', 'int n_lookup_links', 'int want_tsweep', 'void *stream'):
        assert arg in decl.group(1), arg
    assert re.search(r'int rope_debug_targets\(rope_ctx \*ctx, uint64_t \*tq, float \*t32, float \*t32_tsweep, uint8_t \*flags\);', hdr)
    lib = eng.load_library()
    assert {'rope_stage_targets_segmented', 'rope_debug_targets'} <= set(eng.ABI_SYMBOLS)
    assert len(lib.rope_stage_targets_segmented.argtypes) == 12 and len(lib.rope_debug_targets.argtypes) == 5
    assert hasattr(eng.Engine, 'stage_targets_segmented') and hasattr(eng.Engine, 'debug_targets')
    # a null context is refused before anything touches a device
    assert lib.rope_stage_targets_segmented(None, 1, 0, 1, None, 1, None, None, None, 0, 0, None) == -1
    assert lib.rope_debug_targets(None, None, None, None, None) == -1


def test_tile_constants_are_the_kernels():
    src = open(os.path.join(ROOT, 'rope_s3d_amd', 'csrc', 'rope_kernels.h')).read()
    assert int(re.search(r'#define ROPE_TARGET_TILE_W (\d+)', src).group(1)) == eng.TARGET_TILE_W
    assert int(re.search(r'#define ROPE_TARGET_TILE_H (\d+)', src).group(1)) == eng.TARGET_TILE_H
    from rope_s3d_amd import build
    assert 'rope_targets.hip' in build._SOURCES and 'rope_targets.hip' in build._DEPS


def test_detect_batch_on_device_returns_the_same_masks():
    import torch
    from rope_s3d_amd.maskrcnn import MaskRCNNSegmenter
    seg = MaskRCNNSegmenter(7, device='cpu', seed=3, min_confidence=0.0)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 255, (45, 80, 3), dtype=np.uint8) for _ in range(2)]
    images = seg._upload(frames)
    host = seg.net.detect_batch(images)
    dev = seg.net.detect_batch(images, on_device=True)
    assert len(host) == len(dev) == 2 and sum(len(h[0]) for h in host) > 0
    at = 0
    for (cls_h, score_h, masks_h), (cls_d, score_d, masks_d, (stacked, first)) in zip(host, dev):
        assert torch.equal(cls_h, cls_d) and torch.equal(score_h, score_d)
        assert first == at and stacked is dev[0][3][0] and torch.equal(stacked[first:first + len(cls_d)], masks_d)
        at += len(cls_d)
        assert masks_d.dtype == torch.bool and tuple(masks_d.shape) == (len(cls_d), 45, 80)
        assert torch.equal(masks_h, masks_d.permute(1, 2, 0))
    res = seg.batch_device(frames)
    assert [sorted(r) for r in res] == [['class_ids', 'masks_device', 'masks_stacked', 'scores']] * 2
    from rope_s3d_amd.prediction.predict import Predictor
    together = Predictor._stacked(res)
    assert together.data_ptr() == res[0]['masks_stacked'][0].data_ptr() and together.shape[0] == sum(len(r['class_ids']) for r in res)
    plain = [{'class_ids': r['class_ids'], 'masks_device': r['masks_device']} for r in res]           # a segmenter that hands out frames only
    assert torch.equal(Predictor._stacked(plain), together) and Predictor._stacked(plain).data_ptr() != together.data_ptr()
    for r, (cls_h, _, masks_h) in zip(res, host):
        assert isinstance(r['class_ids'], np.ndarray) and np.array_equal(r['class_ids'], cls_h.numpy())
        assert torch.equal(r['masks_device'].permute(1, 2, 0), masks_h)
    again = list(seg.batches_device([frames[:1], frames[1:]]))
    assert len(again) == 2 and all(len(g) == 1 and 'masks_device' in g[0] for g in again)
    # nothing found: an empty stack of planes of the frame's size
    seg.net.min_conf = 2.0
    none = seg.net.detect_batch(images, on_device=True)
    assert all(tuple(m.shape) == (0, 45, 80) and m.dtype == torch.bool and st is None for _, _, m, st in none)
    assert Predictor._stacked(seg._results_device(none)) is None


class _Stub:
    """What Predictor's target preparation touches, without an engine."""
    synthetic = False
    ds_factor = 2

    class intrinsics:
        height, width = 4, 6


def test_device_targets_without_batch_device_is_the_host_path():
    """The flag takes the device route only with a segmenter that offers batch_device; otherwise run_many prepares on the host as
    ever (checked on the route decision and the numpy preparation: no GPU here)."""
    from rope_s3d_amd.prediction.predict import Predictor
    import inspect
    assert inspect.signature(Predictor.__init__).parameters['device_targets'].default is False
    depths = [np.zeros((8, 12), np.float32)] * 3
    plain = lambda color: None                                               # noqa: E731

    class Offers:
        def __call__(self, color): return None
        def batch_device(self, frames): return []

    def applies(flag, seg, depths=depths, **kw):
        s = _Stub()
        s.device_targets, s.seg = flag, seg
        for k, v in kw.items():
            setattr(s, k, v)
        return Predictor._device_targets_apply(s, depths)

    assert applies(True, Offers())
    assert not applies(False, Offers())
    assert not applies(True, plain), "no batch_device: as device_targets=False"
    assert not applies(True, None)
    assert not applies(True, Offers(), synthetic=True)
    assert not applies(True, Offers(), depths=[np.zeros((8, 12), np.int32)] * 2), "a depth type the kernels do not take"
    assert not applies(True, Offers(), depths=[np.zeros((8, 10), np.float32)] * 2), "not the camera's size"
    assert not applies(True, Offers(), ds_factor=3)
    # the decision as _run_many_batched takes it: the device route is entered only when the predicate holds
    class Routed(Exception):
        pass

    def route(flag, seg):
        s = _Stub()
        s.device_targets, s.seg = flag, seg
        s._device_targets_apply = lambda d: Predictor._device_targets_apply(s, d)
        s._run_many_device = lambda *a: 'device'

        def host(*a):
            raise Routed
        s._groups = host                                                      # the first thing the host route does
        try:
            return Predictor._run_many_batched(s, [None] * 3, depths, None, 2)
        except Routed:
            return 'host'

    assert route(True, Offers()) == 'device'
    assert route(True, plain) == 'host' and route(False, Offers()) == 'host' and route(False, plain) == 'host'
