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
