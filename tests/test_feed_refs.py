"""CPU: the plain reference of the depth conditioning (tests/feed_ref.py) against cases worked by hand and written out here.
The GPU tests (tests/test_gpu_feed.py) hold the kernels to the reference word for word; these hold the reference to the rule
include/rope_s3d.h writes down."""
import numpy as np

import feed_ref


def _from_patches(patches, k, grid):
    """grid x grid patches of k x k values (row-major lists) -> one (1, grid k, grid k) frame."""
    raw = np.zeros((1, grid * k, grid * k), np.uint16)
    for i, p in enumerate(patches):
        r, c = divmod(i, grid)
        raw[0, r * k:r * k + k, c * k:c * k + k] = np.array(p, np.uint16).reshape(k, k)
    return raw


def test_decimation_lower_median_of_the_valid_values():
    # (patch, expected): 0 to 4 valid values; sorted ascending, index (m - 1) // 2
    cases = [([0, 0, 0, 0], 0), ([0, 7, 0, 0], 7), ([9, 0, 0, 4], 4), ([5, 1, 0, 3], 3),
             ([8, 2, 6, 4], 4), ([65535, 65535, 1, 0], 65535), ([10, 10, 10, 10], 10), ([0, 0, 0, 65535], 65535),
             ([3, 0, 0, 0], 3), ([0, 2, 1, 0], 1), ([1, 2, 3, 0], 2), ([4, 3, 2, 1], 2),
             ([0, 0, 5, 5], 5), ([1, 65535, 0, 0], 1), ([7, 8, 9, 0], 8), ([0, 0, 0, 0], 0)]
    raw = _from_patches([p for p, _ in cases], 2, 4)
    assert feed_ref.decimated_shape(8, 8, 2) == (4, 4)
    assert feed_ref.decimate(raw, 2)[0].ravel().tolist() == [e for _, e in cases]
    # k = 3: nine valid 1..9 -> index 4; four valid -> index 1; the rest empty
    nine = [[9, 1, 8, 2, 7, 3, 6, 4, 5], [0, 4, 0, 3, 0, 2, 0, 1, 0]] + [[0] * 9] * 14
    out = feed_ref.decimate(_from_patches(nine, 3, 4), 3)
    assert out.shape == (1, 4, 4) and out[0].ravel().tolist() == [5, 2] + [0] * 14


def test_decimation_mean_of_the_valid_values_from_four_up():
    z = [0] * 16
    cases = [(z, 0), ([9] + z[1:], 9), ([1, 2] + z[2:], 1), ([65535] * 16, 65535), ([10, 0, 11, 0, 12] + z[5:], 11), ([1, 1, 2] + z[3:], 1),
             (list(range(1, 17)), 8), ([0] * 15 + [65535], 65535)] + [(z, 0)] * 8              # 136 // 16 = 8
    out = feed_ref.decimate(_from_patches([p for p, _ in cases], 4, 4), 4)
    assert out.shape == (1, 4, 4) and out[0].ravel().tolist() == [e for _, e in cases]


def test_decimated_shape_drops_to_a_multiple_of_four():
    assert feed_ref.decimated_shape(10, 22, 2) == (4, 8) and feed_ref.decimated_shape(13, 29, 3) == (4, 8)
    assert feed_ref.decimated_shape(33, 67, 4) == (8, 16) and feed_ref.decimated_shape(7, 64, 2) == (0, 32)
    assert feed_ref.decimated_shape(720, 1280, 2) == (360, 640)
    raw = np.arange(1, 2 * 10 * 22 + 1, dtype=np.uint16).reshape(2, 10, 22)
    out = feed_ref.decimate(raw, 2)                   # increasing values: the lower median of a patch is its top right pixel
    assert out.shape == (2, 4, 8) and np.array_equal(out, raw[:, 0:8:2, 1:16:2])


def test_spatial_pass_on_a_line_with_every_threshold_and_a_hole():
    """delta 20, alpha 0.5 (every float32 step exact): neighbour differences 0, 1, 20 (after the update before it), a hole, 21, 20."""
    line = np.array([100, 100, 101, 121, 0, 200, 221, 241], np.uint16)
    # forward: 100 | d 0: stays | d 1: 50.5 + 50 + .5 = 101 | a = 101, d 20: 60.5 + 50.5 + .5 = 111.5 -> 111 | hole stays |
    #          a = 0: stays | d 21: stays | d 20: 120.5 + 110.5 + .5 = 231.5 -> 231
    assert feed_ref.spatial_pass(line, 0.5, 20).tolist() == [100, 100, 101, 111, 0, 200, 221, 231]
    # backward from the right: 231 | d 10: 110.5 + 115.5 + .5 -> 226 | a = 226, d 26: stays | hole | a = 0: stays |
    #          a = 111, d 10: 50.5 + 55.5 + .5 -> 106 | a = 106, d 6: 50 + 53 + .5 -> 103 | a = 103, d 3: 50 + 51.5 + .5 = 102
    assert feed_ref.spatial_pass(line, 0.5, 20, backward=True).tolist() == [102, 103, 106, 111, 0, 200, 226, 231]
    again = np.array([100, 100, 101, 121, 0, 200, 221, 241], np.uint16)
    assert feed_ref.spatial_sweep(again, 0.5, 20).tolist() == line.tolist()
    assert feed_ref.spatial_sweep(np.array([7], np.uint16), 0.5, 20).tolist() == [7]
    # alpha 0.3 rounds: 110 x 0.3f = 33.0000013 -> 33, 100 x (1 - 0.3f) = 69.9999988 -> 70, 103 + .5 -> 103
    assert feed_ref.spatial_pass(np.array([100, 110], np.uint16), 0.3, 20).tolist() == [100, 103]
    # alpha 1: the value itself
    assert feed_ref.spatial_pass(np.array([100, 110], np.uint16), 1.0, 20).tolist() == [100, 110]


def test_spatial_rows_then_columns():
    p = np.array([[[100, 110], [120, 0]]], np.uint16)
    # rows: [100, 110] -> forward [100, 105], backward [103, 105] (52.5 + 50 + .5); [120, 0] stays
    # columns: [103, 120] d 17 -> forward [103, 112] (60 + 51.5 + .5), backward [108, 112] (51.5 + 56 + .5 = 108); [105, 0] stays
    assert feed_ref.spatial(p, 0.5, 20, 1)[0].tolist() == [[108, 105], [112, 0]]
    assert p[0].tolist() == [[100, 110], [120, 0]]                        # a copy is filtered


TEMPORAL_IN = [100, 110, 0, 0, 0, 0, 131, 0, 140, 0]
# frame 1: d 10 -> 55 + 50 + .5 = 105.5 -> 105.  Frames 2-4 see two valid frames among the last four (history 0b11, 0b110, 0b1100),
# frame 5 one (0b11000).  Frame 6: d 26 > 20 -> last = 131.  Frame 7: history 0b1100001, one of the last four.  Frame 8: d 9 ->
# 70 + 65.5 + .5 = 136; the shift drops the bit of frame 0.  Frame 9: history 0b10000101, two of the last four.
TEMPORAL_OUT = {0: [100, 105, 0, 0, 0, 0, 131, 0, 136, 0],
                3: [100, 105, 105, 105, 105, 0, 131, 0, 136, 136],
                8: [100, 105, 105, 105, 105, 105, 131, 131, 136, 136]}


def test_temporal_rule_on_one_pixel_over_ten_frames():
    for pers, want in TEMPORAL_OUT.items():
        last, hist = np.zeros((1, 1), np.uint16), np.zeros((1, 1), np.uint8)
        frames = np.array(TEMPORAL_IN, np.uint16).reshape(10, 1, 1)
        out = feed_ref.temporal(frames, 0.5, 20, pers, last, hist)
        assert out.ravel().tolist() == want, pers
        assert last[0, 0] == 136 and hist[0, 0] == 0b00001010          # 1, 3, 6, 12, 24, 48, 97, 194, 133, 10
        # frame by frame, the same
        last1, hist1 = np.zeros((1, 1), np.uint16), np.zeros((1, 1), np.uint8)
        one = [int(feed_ref.temporal(frames[i:i + 1], 0.5, 20, pers, last1, hist1)[0, 0, 0]) for i in range(10)]
        assert one == want and last1[0, 0] == 136 and hist1[0, 0] == 10


# Sensors for which every step of the alignment is exact: focal lengths and the depth scale are powers of two.
SCALE = 2.0 ** -10
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
# The corners (x - 0.5, y - 0.5) and (x + 0.5, y + 0.5) of a pixel round to x and x + 1: with identical sensors a pixel covers
# [x .. x + 1] x [y .. y + 1], pixels of the last row and column reach outside and are skipped, and a colour pixel takes the
# minimum of the depth pixels at, left of, above and left above it.  So the output equals the input on a plane that does not
# rise to the right or downwards and whose last row and column repeat the ones before:
ALIGN_SAME = [[900, 800, 700, 600, 600], [850, 750, 650, 550, 550], [800, 700, 600, 500, 500], [800, 700, 600, 500, 500]]
# ... and on any other plane it is that minimum, zeros standing aside:
ALIGN_ANY = [[5, 9, 0, 4], [7, 0, 3, 8], [6, 2, 1, 9]]
ALIGN_ANY_OUT = [[5, 5, 9, 0], [5, 5, 3, 3], [7, 7, 3, 3]]             # contributors: (0,0) 5, (1,0) 9, (0,1) 7, (2,1) 3 — (1,1), (2,0) are holes
# Colour terms doubled (fx, fy, cx, cy x 2), colour image 6 x 6: pixel (x, y) covers [2x - 1 .. 2x + 1] x [2y - 1 .. 2y + 1]; row 0
# and column 0 reach to -1 and are skipped.  (1,1) = 5 covers 1..3 x 1..3, (2,1) = 60 columns 3..5, (1,2) = 80 rows 3..5, (2,2) = 9.
ALIGN_DOUBLE = [[10, 20, 30], [40, 5, 60], [70, 80, 9]]
ALIGN_DOUBLE_OUT = [[0, 0, 0, 0, 0, 0], [0, 5, 5, 5, 60, 60], [0, 5, 5, 5, 60, 60], [0, 5, 5, 5, 9, 9], [0, 80, 80, 9, 9, 9], [0, 80, 80, 9, 9, 9]]
# A translation of 2^-4 m along x, fx = 64: a pixel at 1 m (1024 units) moves 4 columns, one at 2 m (2048) moves 2.  Pixel 0 at
# 1 m and pixel 2 at 2 m both cover columns 4..5, rows 0..1: the nearer wins.  Pixel 5 at 2 m covers columns 7..8.
ALIGN_SHIFT = [[1024, 0, 2048, 0, 0, 2048]]
ALIGN_SHIFT_T = [1, 0, 0, 0, 1, 0, 0, 0, 1, 2.0 ** -4, 0, 0]
ALIGN_SHIFT_OUT = [[0, 0, 0, 0, 1024, 1024, 0, 2048, 2048, 0]] * 2 + [[0] * 10]


def test_alignment_between_identical_sensors():
    same = np.array([ALIGN_SAME], np.uint16)
    intr = [64.0, 64.0, 2.0, 1.5]
    assert feed_ref.align(same, intr, intr, IDENTITY, SCALE, 4, 5)[0].tolist() == ALIGN_SAME
    stats = {}
    assert feed_ref.align(np.array([ALIGN_ANY], np.uint16), intr, intr, IDENTITY, SCALE, 3, 4, stats)[0].tolist() == ALIGN_ANY_OUT
    assert stats['outside'] == 6                                          # (3,0) 4, (3,1) 8 and the four pixels of the last row


def test_alignment_to_a_sensor_of_twice_the_resolution():
    d, c = [64.0, 64.0, 1.0, 1.0], [128.0, 128.0, 2.0, 2.0]
    stats = {}
    assert feed_ref.align(np.array([ALIGN_DOUBLE], np.uint16), d, c, IDENTITY, SCALE, 6, 6, stats)[0].tolist() == ALIGN_DOUBLE_OUT
    assert stats['outside'] == 5 and stats['collided'] > 0


def test_alignment_with_a_translation_keeps_the_nearer_of_two():
    intr = [64.0, 64.0, 0.0, 0.0]
    got = feed_ref.align(np.array([ALIGN_SHIFT], np.uint16), intr, intr, ALIGN_SHIFT_T, SCALE, 3, 10)
    assert got[0].tolist() == ALIGN_SHIFT_OUT
    # behind the colour sensor (Z' <= 0) nothing contributes; a footprint beyond 16 pixels is skipped
    back = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, -4.0]
    assert not feed_ref.align(np.array([ALIGN_SHIFT], np.uint16), intr, intr, back, SCALE, 3, 10).any()
    wide = [64.0 * 32, 64.0 * 32, 0.0, 0.0]
    assert not feed_ref.align(np.array([[[0, 0], [0, 1024]]], np.uint16), intr, wide, IDENTITY, SCALE, 100, 100).any()


def test_chain_applies_the_steps_in_order_and_keeps_state():
    rng = np.random.default_rng(5)
    raw = rng.integers(1000, 1040, (3, 8, 16)).astype(np.uint16)
    raw[rng.random(raw.shape) < 0.1] = 0
    d = [8.0, 8.0, 8.0, 4.0]
    ch = feed_ref.Chain(d, [4.0, 4.0, 4.0, 2.0], IDENTITY, SCALE, (4, 8))
    many = ch.process_many(raw)
    x = feed_ref.spatial(feed_ref.decimate(raw, 2), 0.5, 20, 2)
    x = feed_ref.temporal(x, 0.5, 20, 3, np.zeros((4, 8), np.uint16), np.zeros((4, 8), np.uint8))
    assert many.shape == (3, 4, 8) and np.array_equal(many, feed_ref.align(x, [4.0, 4.0, 4.0, 2.0], [4.0, 4.0, 4.0, 2.0], IDENTITY, SCALE, 4, 8))
    ch.reset()
    assert np.array_equal(np.stack([ch.process(f) for f in raw]), many)
    ch.reset()
    assert np.array_equal(ch.average(raw), many.astype(np.float64).sum(axis=0) * SCALE / 3)
    assert ch.metres(many[0]).dtype == np.float64 and np.array_equal(ch.metres(many[0]), many[0] * SCALE)
