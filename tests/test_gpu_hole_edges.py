"""GPU: depth_holes_kernel (csrc/rope_synth.hip) at the ends of its parameters — rope_depth_holes called with explicit thresholds,
dilation sizes and close window, on the cases of holes_ref.HOLE_EDGE_CASES: windows of 1, 2, 31 and 32, none to sixteen dilations,
thresholds 0 and 0xFFFFFFFF, images that end one pixel before, on and after a tile's edge or are smaller than every window, and a
frame counter that passes 2^32.  What each case is for is asserted on the reference alone in tests/test_holes_host.py.

Reference: holes_ref.holes_raw, the integer contract of DESIGN.md §3a in numpy.  Every comparison is bit for bit, NaN payloads and
the sign of zero included: where no hole is set the kernel does not touch the word."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import holes_ref

pytestmark = pytest.mark.gpu

E_ARG = -1
CASES = holes_ref.HOLE_EDGE_CASES
SPECIAL = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001], np.uint32)   # NaNs, -0.0, infinities, a denormal


@pytest.fixture(scope='module')
def lib():
    torch.cuda.init()
    return eng.load_library()


def _plane(rng, n, H, W):
    """As the planes of test_gpu_synth_targets.py, with a render's background zeros; one pixel in twelve a special bit pattern.  An
    image of under 16 pixels: plain depths."""
    d = rng.uniform(0.3, 3.0, (n, H, W)).astype(np.float32)
    if H * W < 16:                                              # every pixel of a tiny image must show its hole
        return d
    d[rng.random((n, H, W)) < 0.2] = 0.0
    pick = rng.random((n, H, W)) < 1 / 12
    d.view(np.uint32)[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return d


def _holes(lib, t, frame0, seed, sizes, T, k, n_d=None, null_T=False, null_d=False):
    """rope_depth_holes on the (n, H, W) tensor t, in place, on torch's current stream -> the return code."""
    Ta, da = np.array(T, np.uint32), np.array(sizes, np.int32)
    n, H, W = t.shape
    with torch.cuda.device(t.device):
        rc = lib.rope_depth_holes(C.c_void_p(t.data_ptr()), n, H, W, frame0, seed, None if null_T or not len(Ta) else Ta.ctypes.data_as(C.c_void_p),
                                  None if null_d or not len(da) else da.ctypes.data_as(C.c_void_p), len(sizes) if n_d is None else n_d, k,
                                  C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream))
        torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('name', list(CASES))
def test_holes_equal_the_raw_reference(lib, name):
    n, H, W, frame0, seed, sizes, T, k = CASES[name]
    depth = _plane(np.random.default_rng(H * 1000 + W + len(sizes)), n, H, W)
    want = np.stack([holes_ref.holes_raw(depth[m], frame0 + m, seed, sizes, T, k) for m in range(n)])
    if H * W >= 1000 and (want != 0).any():                     # the bits that must survive are there to survive
        kept = want.view(np.uint32)
        assert (kept == 0x80000000).any() and (kept == 0x7FC12345).any() and (kept == 0xFFA00001).any()
    t = torch.from_numpy(depth).cuda()
    assert _holes(lib, t, frame0, seed, sizes, T, k) == 0
    got = t.cpu().numpy()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), (f"{len(bad)} of {got.size} pixels differ; first (frame, y, x) {bad[:6].tolist()}: "
                          f"got {[hex(int(got.view(np.uint32)[tuple(b)])) for b in bad[:6]]}, want {[hex(int(want.view(np.uint32)[tuple(b)])) for b in bad[:6]]}")


def test_refusals_leave_the_plane_as_it_was(lib):
    H, W, seed = 40, 70, 12345
    depth = _plane(np.random.default_rng(0), 1, H, W)
    T16, d16 = [1 << 26] * 17, [3] * 17
    refused = {
        'a dilation of 0': dict(sizes=[3, 0], T=T16[:2], k=5),
        'a dilation of 33': dict(sizes=[33, 3], T=T16[:2], k=5),
        'seventeen dilations': dict(sizes=d16, T=T16, k=5),
        'a close window of 0': dict(sizes=[3], T=T16[:1], k=0),
        'no thresholds for two dilations': dict(sizes=[3, 6], T=T16[:2], k=5, null_T=True),
        'no sizes for two dilations': dict(sizes=[3, 6], T=T16[:2], k=5, null_d=True),
    }
    for what, kw in refused.items():
        t = torch.from_numpy(depth).cuda()
        assert _holes(lib, t, 0, seed, **kw) == E_ARG, what
        assert np.array_equal(t.cpu().numpy().view(np.uint32), depth.view(np.uint32)), what
    # the same arguments are taken once they are in range, and change the plane
    t = torch.from_numpy(depth).cuda()
    assert _holes(lib, t, 0, seed, sizes=[3, 6], T=T16[:2], k=5) == 0
    assert np.array_equal(t.cpu().numpy().view(np.uint32), holes_ref.holes_raw(depth[0], 0, seed, [3, 6], T16[:2], 5)[None].view(np.uint32))
    assert (t.cpu().numpy().view(np.uint32) != depth.view(np.uint32)).any()
    # no dilations need no tables
    t = torch.from_numpy(depth).cuda()
    assert _holes(lib, t, 0, seed, sizes=[], T=[], k=5, null_T=True, null_d=True) == 0
    assert np.array_equal(t.cpu().numpy().view(np.uint32), depth.view(np.uint32))
