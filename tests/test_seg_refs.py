"""The references and input builders of tests/seg_ref.py, held to account without a GPU: the references against each other, against
the product's tensor formulation on the CPU and against the sequential oracle, and every builder against the edge it is named for
(tests/test_gpu_seg_kernels.py and tests/test_gpu_label_masks.py run the kernels on the same inputs)."""
import numpy as np
import pytest
import torch

import seg_ref as R
from oracle import maskrcnn_ref as orc
from rope_s3d_amd import maskrcnn as mr
from rope_s3d_amd.data import annotation as ann


# ------------------------------------------------------------------------------------------------ bfloat16 helper
def test_bf16_rounding_equals_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-40, 38, 4000), [0.0, -0.0, np.inf, -np.inf, 3.3895314e38, 1e-40, -1e-45],
                        R.bf16_value(np.arange(0, 0x7F80, 7, dtype=np.uint16)).astype(np.float64) * (1 + 2.0 ** -9)]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x), want)
    halves = (np.arange(0x3F80, 0x3FA0, dtype=np.uint32) << 16 | 0x8000).view(np.float32)          # exact ties: to even
    assert np.array_equal(R.bf16_bits(halves), ((np.arange(0x3F80, 0x3FA0) + 1) & ~1).astype(np.uint16))
    assert R.bf16_bits(np.float32([np.nan]))[0] == 0x7FC0


# ------------------------------------------------------------------------------------------------ NMS
def _product_nms(case):
    """maskrcnn._nms_batched on the CPU (scores descending in the given order; blocks of 256 above 200 boxes, so that the staircase
    settles in hundreds of rounds, not thousands, and the block-to-block thinning runs too)."""
    b = torch.from_numpy(case['boxes'])
    S, n = b.shape[:2]
    scores = torch.arange(n, 0, -1, dtype=torch.float32).expand(S, n).contiguous()
    keep = mr._nms_batched(b, scores, case['thr'], case['limit'], block=256 if n > 200 else 2048,
                           valid=None if case['valid'] is None else torch.from_numpy(case['valid']).bool(),
                           groups=None if case['groups'] is None else torch.from_numpy(case['groups']).long())
    return keep.numpy().astype(np.uint8)


def _check_case(case, oracle_too=True):
    want = R.nms_ref_sets(case)
    n = case['boxes'].shape[1]
    assert np.array_equal(_product_nms(case), want)
    assert (want.sum(1) <= case['limit']).all()
    if case['valid'] is not None:
        assert not (want & (1 - case['valid'])).any()
    if oracle_too and case['groups'] is None and case['valid'] is None and n <= 129:
        for s in range(len(want)):
            kept = orc.non_max_suppression(case['boxes'][s], -np.arange(n, dtype=np.float32), case['limit'], case['thr'])
            assert np.array_equal(np.nonzero(want[s])[0], np.array(kept))
    exp = case['meta'].get('expect')
    if exp is not None:
        for s, e in enumerate(exp):
            if e is not None:
                assert want[s].sum() == min(e, case['limit']), (s, e)
    return want


@pytest.mark.parametrize('n', R.NMS_SIZES)
def test_nms_staircase_keeps_the_even_boxes(n):
    want = _check_case(R.nms_staircase(n))
    assert np.array_equal(np.nonzero(want[0])[0], np.arange(0, n, 2))              # kept by the removal of the predecessor
    assert np.array_equal(np.nonzero(want[2])[0], np.arange(0, n, 3))
    if n == 4161:
        assert want[0].sum() == 2081 and (n + 63) // 64 == 66


@pytest.mark.parametrize('n', [129, 4161])
def test_nms_limit_lands_on_block_seams(n):
    """Set 1 keeps every box, so limit L is reached at box L - 1: 63 (the last of block 0), 64 (the first of block 1), 65; set 0
    keeps the even ones: limit 32 ends on box 62, limit 33 on box 64."""
    for limit, last1, last0 in ((1, 0, 0), (32, 31, 62), (33, 32, 64), (64, 63, 126), (65, 64, 128), (66, 65, None), (n, n - 1, None), (n + 7, n - 1, None)):
        want = _check_case(R.nms_staircase(n, limit))
        assert np.nonzero(want[1])[0][-1] == last1 and want[1].sum() == min(limit, n)
        if last0 is not None:
            assert np.nonzero(want[0])[0][-1] == last0 and want[0].sum() == limit


@pytest.mark.parametrize('n', R.NMS_SIZES)
def test_nms_identical_disjoint_groups_validity(n):
    _check_case(R.nms_identical(n))
    for limit in (n, max(n // 2, 1)):
        _check_case(R.nms_disjoint(n, limit))
    _check_case(R.nms_seven_groups(n))
    case = R.nms_one_set_invalid(n)
    want = _check_case(case)
    assert not case['valid'][1].any() and not want[1].any()
    case = R.nms_invalid_suppressor(n)
    want = _check_case(case)
    assert np.array_equal(want[0], case['valid'][0])                                # every valid box stays: its strikers were invalid
    if n > 1:
        assert R.iou_over_ref(case['boxes'][0][:1], case['boxes'][0][1], 0.5)[0].all()


def test_nms_far_victim_needs_the_second_trip():
    case = R.nms_far_victim()
    n = case['boxes'].shape[1]
    assert (n + 63) // 64 == 66 and (n - 1) // 64 == 65                             # lane 0 of block 0 reads words 1 and 65
    want = _check_case(case)
    assert not want[0][-1] and want[0][:-1].all() and not want[1][-1] and want[2].all()
    over, _ = R.iou_over_ref(case['boxes'][0][1:], case['boxes'][0][0], 0.5)
    assert np.array_equal(np.nonzero(over)[0], [n - 2])                             # box 0 strikes the last box and nothing else


def test_nms_exact_threshold_is_strict():
    at, below = R.nms_exact_threshold(False), R.nms_exact_threshold(True)
    for s in range(3):
        _, iou = R.iou_over_ref(at['boxes'][s][:1], at['boxes'][s][1], 0.5)
        assert iou.view(np.uint32)[0] == np.float32(0.5).view(np.uint32)            # bit for bit
    assert np.float32(below['thr']) < np.float32(0.5) and np.float32(below['thr']) == np.nextafter(np.float32(0.5), np.float32(0))
    assert _check_case(at).sum() == 6 and _check_case(below).sum() == 3


def test_nms_degenerate_boxes_never_suppress():
    """Not compared with the oracle: TF swaps inverted corners and has no floor under the union; the product clamps (rope_seg.hip)."""
    case = R.nms_degenerate()
    want = _check_case(case, oracle_too=False)
    b = case['boxes']
    flat = (b[..., 2] <= b[..., 0]) | (b[..., 3] <= b[..., 1])
    assert flat.sum() >= 10 and want[flat].all()                                    # zero-area and inverted boxes all stay
    _, iou = R.iou_over_ref(b[2][:1], b[2][1], 0.5)
    assert np.isclose(iou[0], 0.01) and want[2][:2].all()                           # union 1e-14 under the 1e-12 floor


# ------------------------------------------------------------------------------------------------ RoIAlign
def _roi_inputs(pyramid, channels, pool):
    levels, rows = R.roi_features(pyramid, channels, seed=channels + pool)
    boxes, frame = R.roi_boxes(R.roi_box_count(channels, pool))
    return levels, rows, boxes, frame, R.roi_sample_t(pool)


def test_roi_boxes_reach_every_level_and_edge():
    boxes, frame = R.roi_boxes()
    arg = R.roi_level_arg64(boxes)
    assert np.abs(arg - np.floor(arg) - 0.5).min() >= 1e-3                          # log2f may differ in its last digit: same level
    for count in (12, 48):
        lv = np.clip(np.rint(arg[:count]), 2, 5)
        assert set(lv.tolist()) == {2, 3, 4, 5}
    assert set(frame[:12].tolist()) == {0, 1, 2}
    assert (boxes[:, 2] == boxes[:, 0]).any() and (boxes.min() < 0) and (boxes.max() > 1)
    assert {c for _, c, _ in R.ROI_CASES} == {8, 16, 64, 512, 2048} and {p for _, _, p in R.ROI_CASES} == {1, 2, 7, 14, 33}
    assert any(p > 256 // (c // 8) for _, c, p in R.ROI_CASES if c == 64)
    hw = np.array([R.ROI_PYRAMIDS[k] for k in R.ROI_PYRAMIDS])
    assert (hw[..., 0] != hw[..., 1]).all() and (hw[2:, :, 0] == 1).any() and (hw[2:, :, 1] == 1).any()
    assert R.roi_sample_t(1).tolist() == [0.0] and R.roi_sample_t(33)[-1] == 1.0


@pytest.mark.parametrize('pyramid,channels,pool', R.ROI_CASES)
def test_roi_references_agree(pyramid, channels, pool):
    """Form (a) equals maskrcnn._roi_align on CPU bfloat16 features bit for bit, and lies within the derived bound of form (b)."""
    levels, rows, boxes, frame, t = _roi_inputs(pyramid, channels, pool)
    got = R.roi_align_ref_bits(pyramid, rows, boxes, frame, pool, t)
    feats = [R.torch_bf16(lv) for lv in levels]
    prod = mr._roi_align(feats, torch.from_numpy(boxes), pool, R.ROI_SIZE, torch.from_numpy(frame).long())
    prod = prod.permute(0, 2, 3, 1).contiguous().view(torch.int16).numpy().view(np.uint16)
    assert prod.tobytes() == got.tobytes(), np.argwhere(prod != got)[:4]           # the sign of x * 0 outside the map included
    r = R.roi_align_ref64(pyramid, levels, rows, boxes, frame, pool, t)
    worst, skipped = R.check_roi_bound(got, r)
    print(f"roi_align ref (a) vs (b) {pyramid} C {channels} pool {pool}: worst err/bound {worst:.3f}, skipped {skipped:.4f}")
    assert worst <= 1.0 and skipped <= 0.01 and r['dmax'] < R.EDGE_EPS
    assert r['inside'].any() and not r['inside'].all()
    assert r['inside'][0].all() and bool(R.bf16_value(got[0, -1, -1]).any())
    if pool > 1:                                                                    # [0,0,1,1]: the last sample exactly on hm, wm
        assert r['ys'][0, -1] == r['hm'][0, 0] and r['xs'][0, -1] == r['wm'][0, 0]


@pytest.mark.parametrize('pyramid,channels,pool', [('tall', 8, 7), ('wide', 16, 14), ('thin', 64, 2), ('thin', 64, 33)])
def test_roi_float64_form_equals_the_oracle_crop(pyramid, channels, pool):
    levels, rows, boxes, frame, t = _roi_inputs(pyramid, channels, pool)
    r = R.roi_align_ref64(pyramid, levels, rows, boxes, frame, pool, t)
    on_edge = ((r['ys'] == r['hm']) & (r['hm'] > 0))[:, :, None] | ((r['xs'] == r['wm']) & (r['wm'] > 0))[:, None, :]
    for k in range(len(boxes)):
        fmap = R.bf16_value(levels[r['level'][k] - 2][frame[k]]).astype(np.float64).transpose(1, 2, 0)
        want = orc.crop_and_resize(fmap, boxes[k], pool)
        ok = ~(r['skip'][k] | on_edge[k])                     # the oracle steps by (y2 - y1) hm / (pool - 1): may miss hm by an ulp
        # t is the float32 linspace, off k / (pool - 1) by at most 2^-25: the sample moves by that times the box's extent (at most 2)
        # times hm (at most 40), the value by that times the steepest neighbour difference (at most twice the largest value), per axis
        atol = 2.0 ** -25 * 2 * 40 * 2 * np.abs(fmap).max() * 2
        assert np.allclose(r['ref'][k][ok], want[ok], rtol=0, atol=atol), k


# ------------------------------------------------------------------------------------------------ bias / residual / ReLU
def test_bias_shapes_cover_the_tails():
    n8 = {s: s[1] * s[2] * s[3] // 8 for s in R.BIAS_SHAPES}
    assert all(s[1] * s[2] * s[3] % 8 == 0 for s in R.BIAS_SHAPES)
    assert any(n8[s] % 256 for s in R.BIAS_SHAPES if s[0] == 'nchw') and any(n8[s] % 256 for s in R.BIAS_SHAPES if s[0] == 'nhwc')
    assert 1 in n8.values()
    assert {(s[2], s[3]) for s in R.BIAS_SHAPES if s[0] == 'nchw'} == {(c, hw) for c in (1, 3, 64) for hw in (8, 24, 960)}
    assert {s[2] for s in R.BIAS_SHAPES if s[0] == 'nhwc'} == {8, 24, 128}
    assert any(n8[s] * 8 > s[2] and s[2] == 24 for s in R.BIAS_SHAPES if s[0] == 'nhwc')    # (i * 8) % 24 wraps off a power of two


@pytest.mark.parametrize('shape', R.BIAS_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_bias_act_ref_equals_the_separate_tensor_operations(shape):
    layout, B, C, hw = shape
    y, bias, res = R.bias_act_inputs(*shape)
    chan = R.bias_channel_index(*shape)
    yv = R.bf16_value(y)
    assert ((y & 0x7F80) == 0).any() and ((y == R.BF_NEG_ZERO).any() or len(y) < 64)
    seen_inf = False
    for use_res in (False, True):
        for relu in (False, True):
            want = R.bias_act_ref(y, bias, res if use_res else None, chan, relu)
            assert not np.isnan(R.bf16_value(want)).any()
            seen_inf |= bool(np.isinf(R.bf16_value(want)).any())

            def shaped(bits):
                tt = R.torch_bf16(bits)
                return tt.view(B, C, hw, 1) if layout == 'nchw' else tt.view(B, hw, 1, C).permute(0, 3, 1, 2)
            out = shaped(y) + R.torch_bf16(bias).view(1, -1, 1, 1)
            if use_res:
                out = out + shaped(res)
            if relu:
                out = torch.relu(out)
            out = out.contiguous() if layout == 'nchw' else out.permute(0, 2, 3, 1).contiguous()
            got = out.view(torch.int16).numpy().view(np.uint16).reshape(-1)
            assert R.bias_act_equal(got, want) and R.bias_act_equal(want, got)
    assert np.isfinite(yv).all()
    if (C >= 3 or hw == 24) and len(y) >= 64:
        assert seen_inf


# ------------------------------------------------------------------------------------------------ label masks
def test_mask_planes_reach_the_named_branches():
    lut = R.mask_lut()
    assert any(w & 3 for w in R.MASK_WIDTHS) and {1, 2, 3} <= {w % 4 for w in R.MASK_WIDTHS} and min(R.MASK_WIDTHS) < 4
    assert max(R.MASK_PADS) == 64 and any(8 < p for p in R.MASK_PADS)
    kinds_at = {}
    for H in R.MASK_HEIGHTS:
        for W in R.MASK_WIDTHS:
            planes, names = R.mask_planes(H, W)
            assert planes.shape == (3, H, W) and (len({p.tobytes() for p in planes}) == 3 or H * W < 8)
            for k, name in enumerate(names):
                kinds_at.setdefault(name, set()).add(k)
            sp = planes[names.index('sparse')]
            assert sp[0, 0] == sp[0, W - 1] == sp[H - 1, 0] == sp[H - 1, W - 1] == 0
            assert (planes[names.index('empty')] == R.BACKGROUND).all() if 'empty' in names else True
            if W > 128 and H > 16:
                assert sp[15, 127] == 1 and ((sp[15:17, 127:129] == 1).all() or (H, W) == (17, 129))     # there (16, 128) is a corner
            for pad in R.MASK_PADS:
                out = ann.dilate(lut[sp], pad)
                if W >= 127:                                   # tile 0: bit 2 only in columns 64..127, bit 3 only in 0..63
                    t0 = out[:16, :128]
                    c2, c3 = np.nonzero(((t0 >> 2) & 1).any(0))[0], np.nonzero(((t0 >> 3) & 1).any(0))[0]
                    if len(c2):
                        assert c2.min() >= 64
                    if len(c3):
                        assert c3.max() < 64
                    if H in (1, 15):
                        assert len(c2) and len(c3)
                if 'eight' in names and pad >= 4 and W >= 5 and H >= 15:
                    assert (ann.dilate(lut[planes[names.index('eight')]], pad) == 0xFF).any()     # all eight bits in one pixel
    assert all(v == {0, 1, 2} for k, v in kinds_at.items() if k in ('sparse', 'dense')) and kinds_at['empty'] == {0, 1, 2}
