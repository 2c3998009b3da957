"""The inference kernels of rope_seg.hip against plain references at the edges tests/test_maskrcnn.py's shapes do not reach:
the two NMS kernels against a sequential greedy NMS (chains across block seams, the limit on a seam, invalid sets, the strict
threshold, degenerate boxes, 66 mask words), RoIAlign on non-square pyramids at every channel count and pool size bit for bit
against a numpy restatement and under a derived bound against float64, bias / residual / ReLU off the block and channel
multiples, and the refusals of the three entry points (tests/seg_ref.py, where the references and inputs are built;
tests/test_seg_refs.py asserts on the CPU that every input reaches the edge it is named for, and the asserts on the host
results below say so again)."""
import ctypes

import numpy as np
import pytest
import torch

import seg_ref as R

pytestmark = pytest.mark.gpu

ROPE_E_ARG = -1


@pytest.fixture(scope='module')
def lib():
    torch.cuda.init()                                   # torch's context before the engine's
    from rope_s3d_amd import maskrcnn as mr
    return mr._seg_lib()


def _cuda(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


# ------------------------------------------------------------------------------------------------ NMS
def _nms_device(lib, case, limit=None):
    """A direct call: the limit goes through as it is (maskrcnn._nms_batched clamps it to n).  The scratch starts as all ones, so
    a word of it that the mask kernel does not write and the scan reads would show."""
    boxes = _cuda(case['boxes'])
    S, n = boxes.shape[:2]
    groups = None if case['groups'] is None else _cuda(case['groups'])
    valid = None if case['valid'] is None else _cuda(case['valid'])
    scratch = torch.full((S, n, (n + 63) // 64), -1, dtype=torch.int64, device='cuda')
    guard = torch.full((S * n + 256,), 7, dtype=torch.uint8, device='cuda')
    out = guard[:S * n]
    rc = lib.rope_seg_nms(boxes.data_ptr(), None if groups is None else groups.data_ptr(), None if valid is None else valid.data_ptr(),
                          S, n, ctypes.c_float(case['thr']), int(case['limit'] if limit is None else limit), scratch.data_ptr(),
                          out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((guard[S * n:] == 7).all())                                      # nothing past the last set
    return out.cpu().numpy().reshape(S, n)


def _nms_check(lib, case):
    want = R.nms_ref_sets(case)
    got = _nms_device(lib, case)
    assert got.tobytes() == want.tobytes(), [np.nonzero(g != w)[0][:8] for g, w in zip(got, want)]
    assert (got.sum(1) <= case['limit']).all()
    if case['valid'] is not None:
        assert not (got & (1 - case['valid'])).any()
    exp = case['meta'].get('expect')
    for s, e in enumerate(exp or ()):
        if e is not None:
            assert want[s].sum() == min(e, case['limit'])
    return got


@pytest.mark.parametrize('n', R.NMS_SIZES)
def test_nms_staircase_chain_across_block_seams(lib, n):
    got = _nms_check(lib, R.nms_staircase(n))
    assert np.array_equal(np.nonzero(got[0])[0], np.arange(0, n, 2)) and got[1].all()
    assert np.array_equal(np.nonzero(got[2])[0], np.arange(0, n, 3))


@pytest.mark.parametrize('n', [129, 4161])
def test_nms_limit_on_block_seams(lib, n):
    for limit, last in ((1, 0), (32, 31), (33, 32), (64, 63), (65, 64), (66, 65), (n, n - 1), (n + 7, n - 1)):
        got = _nms_check(lib, R.nms_staircase(n, limit))
        assert np.nonzero(got[1])[0][-1] == last and got[1].sum() == min(limit, n)
        assert got[0].sum() == min(limit, (n + 1) // 2)


@pytest.mark.parametrize('n', R.NMS_SIZES)
def test_nms_identical_disjoint_groups_validity(lib, n):
    assert _nms_check(lib, R.nms_identical(n)).sum(1).tolist() == [1, min(n, 2), 1]
    for limit in (n, max(n // 2, 1)):
        assert (_nms_check(lib, R.nms_disjoint(n, limit)).sum(1) == limit).all()
    assert _nms_check(lib, R.nms_seven_groups(n)).sum(1)[0] == min(n, 7)
    case = R.nms_one_set_invalid(n)
    assert not _nms_check(lib, case)[1].any() and not case['valid'][1].any()
    case = R.nms_invalid_suppressor(n)
    assert np.array_equal(_nms_check(lib, case)[0], case['valid'][0])              # an invalid box struck nothing


def test_nms_far_victim_threshold_and_degenerate_boxes(lib):
    case = R.nms_far_victim()
    got = _nms_check(lib, case)
    assert (case['boxes'].shape[1] + 63) // 64 == 66
    assert not got[0][-1] and got[0][:-1].all() and not got[1][-1] and got[2].all()
    assert _nms_check(lib, R.nms_exact_threshold(False)).sum() == 6                 # IoU == thr: not over it
    assert _nms_check(lib, R.nms_exact_threshold(True)).sum() == 3
    case = R.nms_degenerate()
    got = _nms_check(lib, case)
    b = case['boxes']
    assert got[(b[..., 2] <= b[..., 0]) | (b[..., 3] <= b[..., 1])].all() and got[2][:2].all()


# ------------------------------------------------------------------------------------------------ RoIAlign
@pytest.mark.parametrize('pyramid,channels,pool', R.ROI_CASES)
def test_roi_align_bits_and_float64_bound(lib, pyramid, channels, pool):
    """Bit for bit the numpy restatement (the sign of the zero outside the map included: x * 0), and every element
    within the bound of tests/seg_ref.py of the float64 crop_and_resize.  Worst err / bound measured on an MI355X: 0.70
    (the restatement itself: 0.70; they are the same bits)."""
    levels, rows = R.roi_features(pyramid, channels, seed=channels + pool)
    boxes, frame = R.roi_boxes(R.roi_box_count(channels, pool))
    t = R.roi_sample_t(pool)
    hw, off = R.roi_levels_abi(pyramid)
    arg = R.roi_level_arg64(boxes)
    assert np.abs(arg - np.floor(arg) - 0.5).min() >= 1e-3 and set(np.clip(np.rint(arg), 2, 5).tolist()) == {2, 3, 4, 5}
    K = len(boxes)
    guard = torch.full((K * pool * pool * channels + 512,), 0x5A5A, dtype=torch.int16, device='cuda')
    d_rows, d_boxes, d_frame, d_t = _cuda(rows), _cuda(boxes), _cuda(frame), _cuda(t)
    rc = lib.rope_seg_roi_align(d_rows.data_ptr(), d_boxes.data_ptr(), d_frame.data_ptr(), hw.ctypes.data, off.ctypes.data, K, channels, pool,
                                ctypes.c_float(float(R.roi_inv_unit())), d_t.data_ptr(), guard.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((guard[K * pool * pool * channels:] == 0x5A5A).all())
    got = guard[:K * pool * pool * channels].cpu().numpy().view(np.uint16).reshape(K, pool, pool, channels)
    want = R.roi_align_ref_bits(pyramid, rows, boxes, frame, pool, t)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:4]
    r = R.roi_align_ref64(pyramid, levels, rows, boxes, frame, pool, t)
    worst, skipped = R.check_roi_bound(got, r)
    print(f"roi_align {pyramid} C {channels} pool {pool} K {K}: worst err/bound {worst:.3f}, skipped {skipped:.4f}")
    assert worst <= 1.0 and skipped <= 0.01 and r['dmax'] < R.EDGE_EPS
    assert r['inside'][0].all() and bool(R.bf16_value(got[0, -1, -1]).any())       # [0,0,1,1]: the last sample, on hm and wm, is inside
    assert not got[9].any() or not (got[9] & 0x7FFF).any()                          # the box wholly beyond the map


# ------------------------------------------------------------------------------------------------ bias / residual / ReLU
@pytest.mark.parametrize('shape', R.BIAS_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_bias_act_bits(lib, shape):
    """Bit for bit the separate bfloat16 operations; where those give a zero, the kernel's ReLU may give a zero of either sign."""
    layout, B, C, hw = shape
    y, bias, res = R.bias_act_inputs(*shape)
    chan = R.bias_channel_index(*shape)
    n = len(y)
    d_bias, d_res = _cuda(bias), _cuda(res)
    for use_res in (False, True):
        for relu in (False, True):
            buf = torch.full((n + 256,), 0x5A5A, dtype=torch.int16, device='cuda')
            buf[:n] = _cuda(y)
            rc = lib.rope_seg_bias_act(buf.data_ptr(), d_bias.data_ptr(), d_res.data_ptr() if use_res else None, n, C, hw if layout == 'nchw' else 1,
                                       int(relu), None)
            torch.cuda.synchronize()
            assert rc == 0
            assert bool((buf[n:] == 0x5A5A).all())
            got = buf[:n].cpu().numpy().view(np.uint16)
            want = R.bias_act_ref(y, bias, res if use_res else None, chan, relu)
            bad = np.nonzero(~((got == want) | (((want & 0x7FFF) == 0) & ((got & 0x7FFF) == 0))))[0]
            assert not len(bad), (shape, use_res, relu, bad[:4], got[bad[:4]], want[bad[:4]])
            assert R.bias_act_equal(got, want)


# ------------------------------------------------------------------------------------------------ ABI refusals (no launch)
def test_abi_refuses_out_of_range_arguments(lib):
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    p = buf.data_ptr()
    hw = np.array([[4, 4], [2, 2], [1, 1], [1, 1]], np.int32)
    hw0 = np.array([[4, 4], [0, 2], [1, 1], [1, 1]], np.int32)
    off = np.array([0, 16, 20, 21], np.int64)
    one = ctypes.c_float(1.0)

    def nms(boxes=p, scratch=p, keep=p, n_sets=1, n=8, limit=8):
        return lib.rope_seg_nms(boxes, None, None, n_sets, n, ctypes.c_float(0.5), limit, scratch, keep, None)

    def align(rows=p, boxes=p, frame=p, level_hw=hw.ctypes.data, level_off=off.ctypes.data, n_boxes=1, channels=8, pool=2, t=p, out=p):
        return lib.rope_seg_roi_align(rows, boxes, frame, level_hw, level_off, n_boxes, channels, pool, one, t, out, None)

    def act(y=p, bias=p, n=64, channels=8, inner=8):
        return lib.rope_seg_bias_act(y, bias, None, n, channels, inner, 1, None)
    for kw in (dict(boxes=None), dict(scratch=None), dict(keep=None), dict(n_sets=0), dict(n=0), dict(limit=0), dict(n=-1)):
        assert nms(**kw) == ROPE_E_ARG, kw
    for kw in (dict(rows=None), dict(boxes=None), dict(frame=None), dict(level_hw=None), dict(level_off=None), dict(t=None), dict(out=None),
               dict(n_boxes=0), dict(pool=0), dict(channels=12), dict(channels=4), dict(channels=4096), dict(level_hw=hw0.ctypes.data)):
        assert align(**kw) == ROPE_E_ARG, kw
    for kw in (dict(y=None), dict(bias=None), dict(n=0), dict(n=12), dict(channels=0), dict(inner=12), dict(channels=12, inner=1)):
        assert act(**kw) == ROPE_E_ARG, kw
    torch.cuda.synchronize()
    assert not bool(buf.any())                                                  # nothing was launched on it
