"""label_mask_kernel (rope_masks.hip) on synthetic id planes, through tests/masks_shim.hip: the widths rope_render_masks never
sees from a preset (W % 4 != 0: the byte stores and the partial last word), pads up to the permitted 64, single pixels in the
corners and on the tile seams, a label only in one half of a tile's columns, all eight bits in one pixel, empty and dense
planes — byte for byte against the host dilation (annotation.dilate) and its boxes (tests/seg_ref.py builds the planes;
tests/test_seg_refs.py asserts on the CPU that they reach the branches they are named for)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import seg_ref as R
from rope_s3d_amd.data import annotation as ann
from test_gpu_annotation import host_boxes, host_masks

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
GUARD = 0xA5


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    torch.cuda.init()                                   # one HIP runtime in the process: torch's, loaded first
    from rope_s3d_amd import build
    out = str(tmp_path_factory.mktemp('masks_shim') / 'libmasks_shim.so')
    subprocess.check_call([build.shutil.which('hipcc') or '/opt/rocm/bin/hipcc'] + build.HIPCC_FLAGS +
                          [os.path.join(ROOT, 'tests', 'masks_shim.hip'), '-o', out])
    lib = C.CDLL(out)
    vp, i32 = C.c_void_p, C.c_int
    lib.shim_label_masks.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, vp]
    return lib


def run(shim, ids, lut, pad):
    """ids (n, H, W) uint8 -> (masks, boxes); the mask planes lie between guard bytes, which must come back untouched."""
    n, H, W = ids.shape
    size = n * H * W
    d_ids, d_lut = torch.from_numpy(np.ascontiguousarray(ids)).cuda(), torch.from_numpy(lut).cuda()
    buf = torch.full((size + 512,), GUARD, dtype=torch.uint8, device='cuda')
    boxes = torch.full((n, 8, 4), -1, dtype=torch.int32, device='cuda')             # as rope_render_masks starts them
    rc = shim.shim_label_masks(d_ids.data_ptr(), n, H, W, d_lut.data_ptr(), pad, buf.data_ptr() + 256, boxes.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    host = buf.cpu().numpy()
    assert (host[:256] == GUARD).all() and (host[256 + size:] == GUARD).all(), (H, W, pad)
    return host[256:256 + size].reshape(n, H, W), boxes.cpu().numpy()


@pytest.mark.parametrize('pad', R.MASK_PADS)
def test_label_masks_odd_widths_every_height(shim, pad):
    seen = 0
    for H in R.MASK_HEIGHTS:
        for W in R.MASK_WIDTHS:
            ids, names = R.mask_planes(H, W)
            masks, boxes = run(shim, ids, R.mask_lut(), pad)
            want = host_masks(ids, R.MASK_LABELS, pad)
            bad = np.argwhere(masks != want)
            assert not len(bad), (H, W, pad, names, bad[:4])
            want_boxes = host_boxes(want)
            assert np.array_equal(boxes, want_boxes), (H, W, pad, names)
            if 'empty' in names:
                k = names.index('empty')
                assert not masks[k].any() and (boxes[k] == -1).all()
            sp = masks[names.index('sparse')]
            assert sp[0, 0] & sp[0, W - 1] & sp[H - 1, 0] & sp[H - 1, W - 1] & 1        # the four corner pixels
            if W >= 127 and H in (1, 15):                                               # tile 0: bit 2 only in columns 64..127, bit 3 only below
                t0 = sp[:16, :128]
                c2, c3 = np.nonzero(((t0 >> 2) & 1).any(0))[0], np.nonzero(((t0 >> 3) & 1).any(0))[0]
                assert len(c2) and c2.min() >= 64 and len(c3) and c3.max() < 64
            seen |= int(np.bitwise_or.reduce(masks, axis=None))
    assert seen == 0xFF


def test_label_masks_all_eight_bits_in_one_pixel(shim):
    """A table that gives one id every label: the byte-wise OR carries all eight masks at once."""
    lut = R.mask_lut()
    lut[8] = 0xFF
    for H, W, pad in ((17, 131, 3), (33, 257, 64), (1, 5, 2), (15, 3, 9)):
        ids = np.full((3, H, W), R.BACKGROUND, np.uint8)
        ids[0, H - 1, W - 1] = ids[1, 0, 0] = ids[2, H // 2, W // 2] = 8
        ids[2, 0, W - 1] = 3
        masks, boxes = run(shim, ids, lut, pad)
        want = np.stack([ann.dilate(lut[i], pad) for i in ids])
        assert masks.tobytes() == want.tobytes() and (masks == 0xFF).any(axis=(1, 2)).all()
        assert np.array_equal(boxes, host_boxes(want))


def test_label_masks_refuses_pads_and_sizes_out_of_range(shim):
    buf = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    p = buf.data_ptr()
    for n, H, W, pad in ((1, 4, 4, 0), (1, 4, 4, 65), (0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 3)):
        assert shim.shim_label_masks(p, n, H, W, p, pad, p, p, None) != 0
    torch.cuda.synchronize()
    assert not bool(buf.any())
