"""CPU: the depth holes' integer contract — the numpy restatement tests/holes_ref.py against the public definition of
its generator, the library's host-only thresholds, the statistics of the seeds, and NoiseMaker.holes, the code it stands in for."""
import ctypes as C
import math

import numpy as np
import pytest

from rope_s3d_amd import build
from rope_s3d_amd import engine as eng
from rope_s3d_amd.simulation.noise import NoiseMaker

import holes_ref

SETTINGS = [(.22, 1, 25), (.35, 1.5, 19), (.3, 2, 33)]         # NoiseMaker.holes' defaults and two others (10 dilations, d up to 30)


def test_generator_known_answers():
    """Philox4x32-10 of Random123's known-answer file: zero counter and key, all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in holes_ref.philox4x32_10(*ctr, *key)) == want


def test_abi_and_sources():
    assert {'rope_render_batch_device', 'rope_stage_targets_synthetic', 'rope_hole_thresholds', 'rope_depth_holes'} <= set(eng.ABI_SYMBOLS)
    assert 'rope_synth.hip' in build._SOURCES and 'rope_synth.hip' in build._DEPS


@pytest.mark.parametrize('std,thresh_factor,max_size', SETTINGS)
def test_thresholds_equal_the_written_expression(std, thresh_factor, max_size):
    d, T = eng.hole_thresholds(std, thresh_factor, max_size)
    sizes, want = holes_ref.thresholds(std, thresh_factor, max_size)
    assert d.tolist() == sizes == list(range(3, max_size, 3))
    assert [int(t) for t in T] == want
    assert want == [math.floor(math.erfc((1 - thresh_factor / k) / (std * math.sqrt(2))) * 2 ** 32) for k in sizes]
    assert all(0 < t < 2 ** 32 for t in want)


def test_thresholds_refuse_what_the_kernel_cannot_take():
    lib = eng.load_library()
    n = C.c_int(-1)
    assert lib.rope_hole_thresholds(.22, 1.0, 3, None, C.byref(n)) == 0 and n.value == 0          # np.arange(3, 3, 3) is empty
    assert lib.rope_hole_thresholds(.22, 1.0, 34, None, C.byref(n)) == -1                        # a window of 33
    assert lib.rope_hole_thresholds(0.0, 1.0, 25, None, C.byref(n)) == -1
    assert lib.rope_hole_thresholds(.22, 1.0, 25, None, None) == -1


def test_seed_count_is_binomial():
    """The seeds of d = 3 on a 512 x 512 field: within five standard deviations of p 2^18."""
    _, T = holes_ref.thresholds()
    p = T[0] / 2 ** 32
    n = 512 * 512
    assert p * n > 100
    count = int(holes_ref.seeds(512, 512, 0, 0x0123456789ABCDEF, T[:1])[0].sum())
    assert abs(count - p * n) <= 5 * math.sqrt(n * p * (1 - p)), (count, p * n)


class _SeedsAsNormals:
    """Stands in for numpy's generator inside NoiseMaker.holes: call j of normal() returns 1.0 at the reference's seeds of dilation j
    and 0 elsewhere, so the thresholding of holes() keeps exactly those pixels."""

    def __init__(self, seeds):
        self.seeds, self.calls = seeds, 0

    def normal(self, mean, std, shape):
        s = self.seeds[self.calls]
        self.calls += 1
        assert shape == s.shape
        return s.astype(np.float64)


@pytest.mark.parametrize('std,frame', [(.22, 0), (.24, 3)])
def test_noisemaker_fed_the_reference_seeds_zeroes_the_same_pixels(std, frame):
    H, W, seed = 75, 110, 0xFEEDFACE12345678
    sizes, T = holes_ref.thresholds(std)
    s = holes_ref.seeds(H, W, frame, seed, T)
    stub = _SeedsAsNormals(s)
    depth = np.random.default_rng(1).uniform(.5, 3., (H, W))
    got = NoiseMaker(stub).holes(depth, std=std)
    assert stub.calls == len(sizes) == 8
    mask = holes_ref.hole_mask(H, W, frame, seed, std=std)
    assert mask.any() and not mask.all()
    assert np.array_equal(got == 0, mask)
    assert np.array_equal(got[~mask], depth[~mask])
    assert np.array_equal(holes_ref.holes(depth, frame, seed, std=std), got)


# ---- the raw reference, its second restatement, and the cases of tests/test_gpu_hole_edges.py

ENDS = (1, 2, 3, 4, 31, 32)                                     # window sizes: the smallest, both parities, the largest the kernel holds
CASES = holes_ref.HOLE_EDGE_CASES
NEEDS = holes_ref.HOLE_CASE_NEEDS


def _first_mixed_frame(H, W, sizes, T, k, limit=64):
    """The first frame whose reference mask has set and clear pixels."""
    for frame in range(limit):
        m = holes_ref.hole_mask_raw(H, W, frame, holes_ref.SEED, sizes, T, k)
        if m.any() and not m.all():
            return frame, m
    raise AssertionError(f"no frame below {limit} with set and clear pixels: sizes {sizes}, T {T}, window {k} on {W}x{H}")


@pytest.mark.parametrize('k', ENDS)
def test_raw_reference_equals_the_loops(k):
    """Every (k, d) of ENDS² on 41 x 37, one to two seeds expected for the large blocks and a few dozen for the small ones, at the
    first frame whose mask is neither empty nor full (there is one for every pair)."""
    H, W = 37, 41
    for d in ENDS:
        sizes, T = [d], holes_ref.T_count(H, W, 1.5 if max(k, d) > 4 else 40)
        frame, want = _first_mixed_frame(H, W, sizes, T, k)
        got = holes_ref.hole_mask_loops(H, W, frame, holes_ref.SEED, sizes, T, k)
        assert np.array_equal(got, want), f"k {k}, d {d}, frame {frame}: {np.argwhere(got != want)[:4].tolist()}"


@pytest.mark.parametrize('H,W', [(1, 1), (1, 9), (9, 1), (5, 7), (33, 31)])
def test_raw_reference_equals_the_loops_on_small_images_and_several_calls(H, W):
    """Six dilations (two generator calls, the second cut short) and an even and an odd close, frames 0 .. 3."""
    sizes, T = [2, 1, 4, 3, 5, 2], holes_ref.T_count(H, W, *([.4] * 6))
    for k in (2, 5):
        for frame in range(4):
            want = holes_ref.hole_mask_raw(H, W, frame, holes_ref.SEED, sizes, T, k)
            assert np.array_equal(holes_ref.hole_mask_loops(H, W, frame, holes_ref.SEED, sizes, T, k), want), (k, frame)


@pytest.mark.parametrize('switch', ['mirror_d', 'mirror_k', 'erode_outside_clear', 'dilate_outside_set'])
def test_the_wrong_switches_mean_the_same_in_both_restatements(switch):
    """hole_mask_raw mirrors and pads through imgproc, hole_mask_loops moves its window bounds: the same wrong masks."""
    H, W = 23, 26
    differs = False
    for k, d in ((2, 4), (4, 2), (3, 5), (32, 2)):
        sizes, T = [d], holes_ref.T_count(H, W, 3)
        for frame in range(3):
            wrong = holes_ref.hole_mask_raw(H, W, frame, holes_ref.SEED, sizes, T, k, **{switch: True})
            assert np.array_equal(holes_ref.hole_mask_loops(H, W, frame, holes_ref.SEED, sizes, T, k, **{switch: True}), wrong), (k, d, frame)
            differs = differs or not np.array_equal(wrong, holes_ref.hole_mask_raw(H, W, frame, holes_ref.SEED, sizes, T, k))
    assert differs


def test_hole_mask_is_the_raw_mask_of_its_thresholds():
    sizes, T = holes_ref.thresholds(.24)
    assert np.array_equal(holes_ref.hole_mask(40, 70, 7, 12345, std=.24), holes_ref.hole_mask_raw(40, 70, 7, 12345, sizes, T, 20))
    depth = np.random.default_rng(2).uniform(.5, 3., (40, 70)).astype(np.float32)
    assert np.array_equal(holes_ref.holes(depth, 7, 12345, std=.24), holes_ref.holes_raw(depth, 7, 12345, sizes, T, 20))


@pytest.fixture(scope='module')
def case_masks():
    """name -> the reference masks of the case's frames; computed once, never written to."""
    out = {}
    for name, (n, H, W, frame0, seed, sizes, T, k) in CASES.items():
        out[name] = [holes_ref.hole_mask_raw(H, W, frame0 + m, seed, sizes, T, k) for m in range(n)]
        for m in out[name]:
            m.setflags(write=False)
    return out


def _wrong_masks(name, **wrong):
    n, H, W, frame0, seed, sizes, T, k = CASES[name]
    return [holes_ref.hole_mask_raw(H, W, frame0 + m, seed, sizes, T, k, **wrong) for m in range(n)]


def _differs(name, case_masks, **wrong):
    return any(not np.array_equal(a, b) for a, b in zip(_wrong_masks(name, **wrong), case_masks[name]))


def test_the_table_holds_what_the_kernel_has_not_run():
    """The parameters themselves: the ends of k, d and n_d, the generator calls, the image sizes around a tile, and the limits of
    the test file (at most 200 pixels a side, at most three frames)."""
    ks = {c[7] for c in CASES.values()}
    ds = {d for c in CASES.values() for d in c[5]}
    n_ds = {len(c[5]) for c in CASES.values()}
    shapes = {(c[1], c[2]) for c in CASES.values()}
    assert {1, 2, 3, 31, 32} <= ks and {1, 2, 31, 32} <= ds and {0, 1, 4, 5, 9, 12, 13, 16} <= n_ds
    assert {(1, 1), (1, 200), (200, 1), (5, 7), (31, 33), (63, 63), (64, 64), (65, 65), (70, 129), (129, 70), (70, 130), (130, 70)} <= shapes
    assert any(c[7] == 32 and 32 in c[5] for c in CASES.values()), "every plane in LDS used to its last row and column"
    assert any(c[3] + c[0] > 2 ** 32 for c in CASES.values())
    for name, (n, H, W, frame0, seed, sizes, T, k) in CASES.items():
        assert 1 <= n <= 3 and 1 <= H <= 200 and 1 <= W <= 200, name
        assert len(sizes) == len(T) <= 16 and 1 <= k <= 32 and all(1 <= d <= 32 for d in sizes) and all(0 <= t <= 0xFFFFFFFF for t in T), name
    assert set(NEEDS) <= set(CASES)


@pytest.mark.parametrize('name', list(CASES))
def test_case_is_worth_running(case_masks, name):
    """Set and clear pixels in every mask.  Exempt are only the cases whose point is the opposite, each held to that: no dilations
    and T = 0 set nothing, T = 0xFFFFFFFF sets everything.  A 1 x 1 image can only be all or nothing: its three frames hold both."""
    n, H, W, frame0, seed, sizes, T, k = CASES[name]
    masks, needs = case_masks[name], NEEDS.get(name, ())
    if 'nothing' in needs:
        assert (len(sizes) == 0 or not any(T)) and not any(m.any() for m in masks)
    elif 'everything' in needs:
        assert T == [0xFFFFFFFF] * len(T) and all(m.all() for m in masks)
    elif H * W == 1:
        assert {bool(m[0, 0]) for m in masks} == {False, True}
    else:
        assert all(m.any() and not m.all() for m in masks)
    m = masks[0]
    if 'borders' in needs:
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    if 'cross_x' in needs:
        assert (m[:, 63] & m[:, 64]).any(), "no hole across column 64"
    if 'cross_y' in needs:
        assert (m[63] & m[64]).any(), "no hole across row 64"
    if n > 1:
        assert any(not np.array_equal(masks[0], b) for b in masks[1:])


@pytest.mark.parametrize('name', [n for n in CASES if len(CASES[n][5]) and not set(NEEDS.get(n, ())) & {'nothing', 'everything', 'extreme'}])
def test_every_dilation_of_a_case_matters(case_masks, name):
    """With T[j] = 0 for any single j the reference mask changes: no dilation's seeds, word or size can go wrong unseen."""
    n, H, W, frame0, seed, sizes, T, k = CASES[name]
    for j in range(len(T)):
        without = [holes_ref.hole_mask_raw(H, W, frame0 + m, seed, sizes, T[:j] + [0] + T[j + 1:], k) for m in range(n)]
        assert any(not np.array_equal(a, b) for a, b in zip(without, case_masks[name])), f"dilation {j} (d = {sizes[j]}) changes nothing"


# a wrong statement of the contract -> the switches that make it, and cases that tell it from the contract
WRONG = {
    'the blocks\' even anchor mirrored': (dict(mirror_d=True), ['130x70, one dilation of 2', '130x70, one dilation of 32']),
    'the close\'s even anchor mirrored': (dict(mirror_k=True), ['130x70, close window 2', '130x70, close window 32']),
    'outside clear for the erosion': (dict(erode_outside_clear=True), ['130x70, close window 32', '130x70, close window 31']),
    'outside set for the dilation': (dict(dilate_outside_set=True), ['130x70, close window 3', '1x200, small windows']),
    'word <= T': (dict(le=True), ['threshold equal to a word']),
    'every word from the first call': (dict(first_call_only=True), ['200x120, 5 dilations', '200x120, 16 dilations']),
    'a last call of fewer than four dropped': (dict(drop_partial_call=True), ['200x120, 5 dilations', '200x120, 9 dilations', '200x120, 13 dilations']),
    'the frame counter not wrapped': (dict(carry_frame=True), ['three frames from 0xFFFFFFFE']),
    'tiles that do not see each other': (dict(tile_halo=(0, 0)), ['130x70, close window 32', '70x130, close window 32', '200x120, 13 dilations']),
}


@pytest.mark.parametrize('what', list(WRONG))
def test_wrong_variant_is_told_apart_by_a_named_case(case_masks, what):
    wrong, names = WRONG[what]
    for name in names:
        assert _differs(name, case_masks, **wrong), f"{what}: the case {name!r} does not show it"


def test_threshold_zero_and_the_compare():
    """No word of these images is 0 (a word is with probability 2^-32, and all the table's images together draw under 2^24), so
    T = 0 cannot tell `<` from `<=`: it is held to setting nothing.  `<=` is told apart by a threshold that is a pixel's own word:
    that pixel is no seed, and with d = k = 1 the mask is the seed plane."""
    n, H, W, frame0, seed, sizes, T, k = CASES['threshold 0']
    assert min(int(w.min()) for w in holes_ref.words(H, W, frame0, seed, 0)) > 0
    assert not any(m.any() for m in _wrong_masks('threshold 0', le=True))
    n, H, W, frame0, seed, sizes, T, k = CASES['threshold equal to a word']
    w0 = holes_ref.words(H, W, frame0, seed, 0)[0]
    assert (w0 == T[0]).sum() == 1 and (w0 < T[0]).sum() == 6 and (sizes, k) == ([1], 1)
    assert np.array_equal(holes_ref.hole_mask_raw(H, W, frame0, seed, sizes, T, k), w0 < T[0])
    # T = 0xFFFFFFFF: every word but 0xFFFFFFFF itself is a seed, and none of this image's is
    n, H, W, frame0, seed, sizes, T, k = CASES['threshold 0xFFFFFFFF']
    assert max(int(w.max()) for w in holes_ref.words(H, W, frame0, seed, 0)) < 0xFFFFFFFF


def test_frame_counter_wraps(case_masks):
    n, H, W, frame0, seed, sizes, T, k = CASES['three frames from 0xFFFFFFFE']
    assert (n, frame0) == (3, 0xFFFFFFFE)
    masks = case_masks['three frames from 0xFFFFFFFE']
    assert np.array_equal(masks[1], holes_ref.hole_mask_raw(H, W, 0xFFFFFFFF, seed, sizes, T, k))
    assert np.array_equal(masks[2], holes_ref.hole_mask_raw(H, W, 0, seed, sizes, T, k))
    assert not np.array_equal(masks[2], masks[0]) and not np.array_equal(masks[2], masks[1])


@pytest.mark.parametrize('name', [n for n in CASES if max(CASES[n][1], CASES[n][2]) > 64])
def test_tiles_with_the_exact_halo_give_the_mask(case_masks, name):
    """Each 64 x 64 tile closed from the seeds within 2 k/2 + max d/2 before and 2 (k - 1 - k/2) + max (d - 1 - d/2) after it alone:
    the reference itself, so a tile-local kernel can be right."""
    n, H, W, frame0, seed, sizes, T, k = CASES[name]
    assert not _differs(name, case_masks, tile_halo=holes_ref.exact_halo(sizes, k))


def test_a_halo_one_pixel_short_shows():
    """Not a property the table as a whole has: with windows of 20 and more a halo short by one pixel changed no mask in 150 frames.
    Two cases were found for it — k = 2, d = 3 at p = 2e-3 for the side before the tile, and at p = 2e-2 for both sides."""
    for name, short_before, short_after in (('70x130, halo before', True, False), ('130x70, halo before and after', True, True)):
        n, H, W, frame0, seed, sizes, T, k = CASES[name]
        before, after = holes_ref.exact_halo(sizes, k)
        want = holes_ref.hole_mask_raw(H, W, frame0, seed, sizes, T, k)
        assert np.array_equal(holes_ref.hole_mask_raw(H, W, frame0, seed, sizes, T, k, tile_halo=(before, after)), want)
        assert np.array_equal(holes_ref.hole_mask_raw(H, W, frame0, seed, sizes, T, k, tile_halo=(before - 1, after)), want) != short_before, name
        assert np.array_equal(holes_ref.hole_mask_raw(H, W, frame0, seed, sizes, T, k, tile_halo=(before, after - 1)), want) != short_after, name
