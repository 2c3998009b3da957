"""GPU: the depth conditioning (rope_depth_* of csrc/rope_feed.hip, prediction/conditioning.py, feed.RawRecordingCamera) against
tests/feed_ref.py, equal word for word, at the smallest shapes at which each kernel's partitioning can go wrong: the horizontal
sweep moves 16 rows x 128 columns a tile, the vertical sweep 64 columns x 32 rows a chunk, the others 256 pixels a workgroup.
Outputs are filled with garbage before a call; inputs are seeded and built so that both sides of every threshold occur."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import feed_ref
import test_feed_refs as hand

pytestmark = pytest.mark.gpu

E_ARG = -1
GARBAGE16, GARBAGE8 = 0x5A5A, 0x5A
DELTA = 20


def _dev(a):
    """A uint16 / uint8 / uint32 array on the GPU (16-bit words as torch.int16, 32-bit as int32: the same bytes)."""
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view).copy()).cuda()


def _host(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def _garbage(shape, dtype=np.uint16):
    return _dev(np.full(shape, GARBAGE16 if dtype == np.uint16 else GARBAGE8, dtype))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    return eng.load_library()


STEPS = np.array([0, 1, DELTA - 1, DELTA, DELTA + 1, 5000])


def _walk(rng, shape, axis, zeros=0.12):
    """Planes whose neighbour differences along `axis` are drawn from {0, 1, delta - 1, delta, delta + 1, large} with either
    sign, values up to 65535 (the walk is held to 1 .. 65535, so it touches the top), 10 to 15 % of the pixels then set to 0."""
    shape = tuple(shape)
    moved = np.moveaxis(np.empty(shape), axis, 0).shape
    steps = rng.choice(STEPS, moved) * rng.choice([-1, 1], moved)
    x = np.empty(moved, np.int64)
    x[0] = rng.choice([3, 30000, 65535], moved[1:])
    for i in range(1, moved[0]):
        x[i] = np.clip(x[i - 1] + steps[i], 1, 65535)
    x = np.moveaxis(x, 0, axis).astype(np.uint16)
    x[rng.random(shape) < zeros] = 0
    return np.ascontiguousarray(x)


def _assert_thresholds_occur(x, axis):
    """Among neighbours along `axis` that are both valid: every difference of the set, so both sides of 1 and of delta."""
    a, b = np.moveaxis(x, axis, 0)[:-1].astype(np.int64), np.moveaxis(x, axis, 0)[1:].astype(np.int64)
    d = np.abs(a - b)[(a != 0) & (b != 0)]
    for v in (0, 1, DELTA - 1, DELTA, DELTA + 1):
        assert (d == v).any(), (axis, v)
    assert (d > 1000).any() and (x == 65535).any()
    assert 0.10 <= (x == 0).mean() <= 0.15


# ------------------------------------------------------------------------------------------------------------------ decimation
def _decimate(raw, k, out=None, null=None, shape=None):
    n, H, W = raw.shape if shape is None else shape
    h, w = feed_ref.decimated_shape(H, W, k) if k >= 1 else (0, 0)
    if out is None:
        out = _garbage((n, max(h, 1), max(w, 1)))
    ptrs = [_p(_dev(raw)), _p(out)]
    if null is not None:
        ptrs[null] = None
    rc = _lib().rope_depth_decimate(ptrs[0], n, H, W, k, ptrs[1], _stream())
    torch.cuda.synchronize()
    return rc, _host(out)


@pytest.mark.parametrize('shape,k', [((1, 8, 8), 2), ((2, 10, 22), 2), ((1, 13, 29), 3), ((1, 33, 67), 4), ((3, 40, 300), 2), ((1, 70, 70), 8)])
def test_decimate_equals_the_reference(shape, k):
    rng = np.random.default_rng(sum(shape) + k)
    raw = _walk(rng, shape, 2, zeros=0.3)                    # many zeros: patches with every count of valid values
    want = feed_ref.decimate(raw, k)
    rc, got = _decimate(raw, k)
    assert rc == 0 and got.shape == want.shape and np.array_equal(got, want)
    if k == 2 and raw.size >= 10000:
        valid = (raw[:, :want.shape[1] * 2, :want.shape[2] * 2].reshape(shape[0], want.shape[1], 2, want.shape[2], 2) != 0).sum(axis=(2, 4))
        assert set(np.unique(valid)) == {0, 1, 2, 3, 4}


def test_decimate_the_hand_patches():
    cases = [([0, 0, 0, 0], 0), ([0, 7, 0, 0], 7), ([9, 0, 0, 4], 4), ([5, 1, 0, 3], 3), ([8, 2, 6, 4], 4), ([65535, 65535, 1, 0], 65535)]
    raw = hand._from_patches([p for p, _ in cases] + [[0] * 4] * 10, 2, 4)
    rc, got = _decimate(raw, 2)
    assert rc == 0 and got[0].ravel().tolist()[:6] == [e for _, e in cases]


def test_decimate_argument_errors_leave_the_output_alone():
    raw = _walk(np.random.default_rng(1), (1, 7, 64), 2)
    rc, got = _decimate(raw, 2)                               # (7 / 2) / 4 * 4 = 0 rows
    assert rc == E_ARG and (got == GARBAGE16).all()
    raw = _walk(np.random.default_rng(2), (1, 16, 16), 2)
    for kw in (dict(k=1), dict(k=9), dict(k=2, null=0), dict(k=2, null=1), dict(k=2, shape=(0, 16, 16)), dict(k=2, shape=(1, 0, 16)),
               dict(k=2, shape=(1, 16, -4)), dict(k=2, shape=(2, 40000, 40000))):
        k = kw.pop('k')
        rc, got = _decimate(raw, k, out=_garbage((1, 4, 4)), **kw)
        assert rc == E_ARG and (got == GARBAGE16).all(), kw


# --------------------------------------------------------------------------------------------------------------------- spatial
def _spatial(x, alpha, delta, iterations, null=False, shape=None):
    n, h, w = x.shape if shape is None else shape
    t = _dev(x)
    rc = _lib().rope_depth_spatial(None if null else _p(t), n, h, w, alpha, delta, iterations, _stream())
    torch.cuda.synchronize()
    return rc, _host(t)


# (1, 1, 1), (1, 1, 2), (1, 2, 1): lines of length 1 and 2.  (3, 5, 67): a row band of 15 rows across three frames' boundaries.
# (2, 70, 9): 140 rows = 8 full bands and one of 12; three chunks of 32 rows, the last of 6.  (1, 130, 131): two column tiles (128 + 3),
# three column groups of 64 lanes, five row chunks.  (1, 3, 300): three column tiles, the carry crossing two tile borders each way.
SPATIAL_SHAPES = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (3, 5, 67), (2, 70, 9), (1, 130, 131), (1, 3, 300)]


@pytest.fixture(scope='module')
def spatial_planes():
    """Per shape: frames walked along the rows and frames walked along the columns, stacked (so both sweeps meet every difference)."""
    out = {}
    for shape in SPATIAL_SHAPES:
        rng = np.random.default_rng(shape[1] * 1000 + shape[2])
        out[shape] = np.concatenate([_walk(rng, shape, 2), _walk(rng, shape, 1)])
    return out


@pytest.mark.parametrize('shape', SPATIAL_SHAPES)
@pytest.mark.parametrize('iterations', [1, 2])
@pytest.mark.parametrize('alpha', [0.5, 0.3])
def test_spatial_equals_the_reference(spatial_planes, shape, iterations, alpha):
    x = spatial_planes[shape]
    n = shape[0]
    if shape[2] >= 60:
        _assert_thresholds_occur(x[:n], 2)
    if shape[1] >= 60:
        _assert_thresholds_occur(x[n:], 1)
    want = feed_ref.spatial(x, alpha, DELTA, iterations)
    rc, got = _spatial(x, alpha, DELTA, iterations)
    assert rc == 0 and np.array_equal(got, want), (shape, iterations, alpha)
    assert np.array_equal(got == 0, x == 0)                   # zeros are never written over, and nothing becomes one
    if x.size > 100:
        assert (got != x).any()


def test_spatial_the_hand_line_as_a_row_and_as_a_column():
    line = np.array([100, 100, 101, 121, 0, 200, 221, 241], np.uint16)
    want = [102, 103, 106, 111, 0, 200, 226, 231]
    rc, got = _spatial(line.reshape(1, 1, 8), 0.5, 20, 1)
    assert rc == 0 and got.ravel().tolist() == want
    rc, got = _spatial(line.reshape(1, 8, 1), 0.5, 20, 1)
    assert rc == 0 and got.ravel().tolist() == want
    rc, got = _spatial(np.array([[[100, 110], [120, 0]]], np.uint16), 0.5, 20, 1)
    assert rc == 0 and got[0].tolist() == [[108, 105], [112, 0]]


def test_spatial_other_deltas():
    x = _walk(np.random.default_rng(77), (1, 20, 70), 2)
    for delta in (1, 19, 65535):
        rc, got = _spatial(x, 0.5, delta, 1)
        assert rc == 0 and np.array_equal(got, feed_ref.spatial(x, 0.5, delta, 1)), delta


def test_spatial_argument_errors_leave_the_planes_alone():
    x = _walk(np.random.default_rng(3), (2, 8, 16), 2)
    for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float('nan')), dict(alpha=-0.5), dict(delta=0), dict(delta=65536), dict(iterations=0),
               dict(iterations=6), dict(null=True), dict(shape=(0, 8, 16)), dict(shape=(2, 0, 16)), dict(shape=(2, 8, 0)), dict(shape=(70000, 1, 1))):
        a = dict(alpha=0.5, delta=DELTA, iterations=2)
        a.update(kw)
        rc, got = _spatial(x, a.pop('alpha'), a.pop('delta'), a.pop('iterations'), **a)
        assert rc == E_ARG and np.array_equal(got, x), kw


# -------------------------------------------------------------------------------------------------------------------- temporal
def _temporal(frames, alpha, delta, pers, last, hist, null=None):
    """One call on device state `last` / `hist` (updated in place) -> (rc, the filtered frames)."""
    t = _dev(frames)
    ptrs = [_p(t), _p(last), _p(hist)]
    if null is not None:
        ptrs[null] = None
    n, h, w = frames.shape
    rc = _lib().rope_depth_temporal(ptrs[0], n, h, w, alpha, delta, pers, ptrs[1], ptrs[2], _stream())
    torch.cuda.synchronize()
    return rc, _host(t)


@pytest.fixture(scope='module')
def temporal_frames():
    x = _walk(np.random.default_rng(12), (12, 6, 70), 0)
    _assert_thresholds_occur(x, 0)
    x[2:11, :, 5] = 0                                         # one pixel column empty for 9 frames: its history runs out
    assert (x[1, :, 5] != 0).any() and (x[11, :, 5] != 0).any()
    return x


@pytest.mark.parametrize('pers', [0, 3, 8])
@pytest.mark.parametrize('alpha', [0.5, 0.3])
def test_temporal_equals_the_reference_however_the_frames_are_cut(temporal_frames, pers, alpha):
    x = temporal_frames
    last_ref, hist_ref = np.zeros((6, 70), np.uint16), np.zeros((6, 70), np.uint8)
    want = feed_ref.temporal(x, alpha, DELTA, pers, last_ref, hist_ref)
    assert (hist_ref[:, 5] <= 1).all()                        # nine empty frames, then the last: only bit 0 can be set
    for cuts in ([12], [1] * 12, [5, 7]):
        last, hist = _dev(np.zeros((6, 70), np.uint16)), _dev(np.zeros((6, 70), np.uint8))
        got, at = [], 0
        for n in cuts:
            rc, part = _temporal(x[at:at + n], alpha, DELTA, pers, last, hist)
            assert rc == 0
            got.append(part)
            at += n
        assert np.array_equal(np.concatenate(got), want), (pers, alpha, cuts)
        assert np.array_equal(_host(last), last_ref) and np.array_equal(_host(hist), hist_ref), (pers, alpha, cuts)
    filled = (x == 0) & (want != 0)
    assert filled.any() == (pers != 0) and (pers == 8 or ((x == 0) & (want == 0))[1:].any())


def test_temporal_the_hand_sequence():
    frames = np.array(hand.TEMPORAL_IN, np.uint16).reshape(10, 1, 1)
    for pers, want in hand.TEMPORAL_OUT.items():
        last, hist = _dev(np.zeros((1, 1), np.uint16)), _dev(np.zeros((1, 1), np.uint8))
        rc, got = _temporal(frames, 0.5, 20, pers, last, hist)
        assert rc == 0 and got.ravel().tolist() == want and _host(last)[0, 0] == 136 and _host(hist)[0, 0] == 10


def test_temporal_every_persistence_and_a_plane_past_one_workgroup():
    x = _walk(np.random.default_rng(13), (10, 3, 111), 0, zeros=0.4)
    for pers in range(9):
        last_ref, hist_ref = np.zeros((3, 111), np.uint16), np.zeros((3, 111), np.uint8)
        want = feed_ref.temporal(x, 0.5, DELTA, pers, last_ref, hist_ref)
        last, hist = _dev(last_ref * 0), _dev(hist_ref * 0)
        rc, got = _temporal(x, 0.5, DELTA, pers, last, hist)
        assert rc == 0 and np.array_equal(got, want) and np.array_equal(_host(hist), hist_ref), pers


def test_temporal_argument_errors_leave_frames_and_state_alone():
    x = _walk(np.random.default_rng(4), (2, 4, 8), 0)
    for kw in (dict(alpha=0.0), dict(alpha=2.0), dict(delta=0), dict(delta=65536), dict(pers=-1), dict(pers=9), dict(null=0), dict(null=1), dict(null=2)):
        a = dict(alpha=0.5, delta=DELTA, pers=3, null=None)
        a.update(kw)
        last, hist = _garbage((4, 8)), _garbage((4, 8), np.uint8)
        rc, got = _temporal(x, a['alpha'], a['delta'], a['pers'], last, hist, null=a['null'])
        assert rc == E_ARG and np.array_equal(got, x) and (_host(last) == GARBAGE16).all() and (_host(hist) == GARBAGE8).all(), kw


# ------------------------------------------------------------------------------------------------------------------- alignment
def _align(planes, d, c, ext, scale, Hc, Wc, null=None, out=None):
    n, h, w = planes.shape
    t = _dev(planes)
    scratch = _dev(np.full((n, max(Hc, 1), max(Wc, 1)), 0x5A5A5A5A, np.uint32))
    if out is None:
        out = _garbage((n, Hc, Wc))
    arr = lambda v, k: None if v is None else (C.c_double * k)(*[float(q) for q in v])     # noqa: E731
    args = [_p(t), arr(d, 4), arr(c, 4), arr(ext, 12), _p(scratch), _p(out)]
    if null is not None:
        args[null] = None
    rc = _lib().rope_depth_align(args[0], n, h, w, args[1], args[2], args[3], scale, Hc, Wc, args[4], args[5], _stream())
    torch.cuda.synchronize()
    return rc, _host(out)


def test_align_the_hand_cases():
    same = [64.0, 64.0, 2.0, 1.5]
    rc, got = _align(np.array([hand.ALIGN_SAME], np.uint16), same, same, hand.IDENTITY, hand.SCALE, 4, 5)
    assert rc == 0 and got[0].tolist() == hand.ALIGN_SAME
    rc, got = _align(np.array([hand.ALIGN_ANY], np.uint16), same, same, hand.IDENTITY, hand.SCALE, 3, 4)
    assert rc == 0 and got[0].tolist() == hand.ALIGN_ANY_OUT
    rc, got = _align(np.array([hand.ALIGN_DOUBLE], np.uint16), [64.0, 64.0, 1.0, 1.0], [128.0, 128.0, 2.0, 2.0], hand.IDENTITY, hand.SCALE, 6, 6)
    assert rc == 0 and got[0].tolist() == hand.ALIGN_DOUBLE_OUT
    zero = [64.0, 64.0, 0.0, 0.0]
    rc, got = _align(np.array([hand.ALIGN_SHIFT], np.uint16), zero, zero, hand.ALIGN_SHIFT_T, hand.SCALE, 3, 10)
    assert rc == 0 and got[0].tolist() == hand.ALIGN_SHIFT_OUT
    rc, got = _align(np.array([hand.ALIGN_SHIFT], np.uint16), zero, zero, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, -4.0], hand.SCALE, 3, 10)
    assert rc == 0 and not got.any()                          # behind the colour sensor
    rc, got = _align(np.array([[[0, 0], [0, 1024]]], np.uint16), zero, [2048.0, 2048.0, 0.0, 0.0], hand.IDENTITY, hand.SCALE, 100, 100)
    assert rc == 0 and not got.any()                          # a footprint of 33 x 33


def _tilted():
    """A colour sensor of twice the resolution, turned 3 degrees about y and 2 about x, 3 cm to the side and 1 cm up."""
    ay, ax = np.deg2rad(3.0), np.deg2rad(-2.0)
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    return [40.0, 41.0, 20.3, 11.7], [80.5, 79.5, 40.2, 23.9], list((Ry @ Rx).ravel()) + [0.03, -0.01, 0.002]


def test_align_to_a_tilted_sensor_equals_the_reference():
    rng = np.random.default_rng(2440)
    planes = rng.integers(600, 3000, (2, 24, 40)).astype(np.uint16)
    planes[rng.random(planes.shape) < 0.12] = 0
    planes[0, 3, 3], planes[1, 20, 30] = 65535, 1
    d, c, ext = _tilted()
    stats = {}
    want = feed_ref.align(planes, d, c, ext, 0.001, 48, 80, stats)
    assert stats['outside'] > 0 and stats['collided'] > 0 and (want != 0).sum() > 1000 and (want == 0).any()
    rc, got = _align(planes, d, c, ext, 0.001, 48, 80)
    assert rc == 0 and np.array_equal(got, want)
    rc, got = _align(np.zeros((2, 24, 40), np.uint16), d, c, ext, 0.001, 48, 80)
    assert rc == 0 and not got.any()                          # a plane of all zeros


def test_align_argument_errors_leave_the_output_alone():
    planes = np.full((1, 4, 4), 1000, np.uint16)
    d, c, ext = _tilted()
    for kw in (dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=4), dict(null=5), dict(scale=0.0), dict(scale=-1.0),
               dict(scale=float('nan')), dict(d=[0.0, 40.0, 2.0, 2.0]), dict(d=[40.0, float('inf'), 2.0, 2.0]), dict(c=[float('nan'), 1, 1, 1]),
               dict(ext=[float('nan')] * 12), dict(Hc=0), dict(Wc=-3)):
        a = dict(d=d, c=c, ext=ext, scale=0.001, Hc=8, Wc=8, null=None)
        a.update(kw)
        out = _garbage((1, 8, 8))
        rc, got = _align(planes, a['d'], a['c'], a['ext'], a['scale'], a['Hc'], a['Wc'], null=a['null'], out=out)
        assert rc == E_ARG and (got == GARBAGE16).all(), kw


# ----------------------------------------------------------------------------------------------------------------------- chain
CHAIN_DEPTH = {'width': 88, 'height': 48, 'fx': 70.0, 'fy': 70.5, 'cx': 44.3, 'cy': 23.8}
CHAIN_EXT = {'rotation': [1, 0, 0, 0, 1, 0, 0, 0, 1], 'translation': [0.015, 0, 0]}


@pytest.fixture(scope='module')
def chain():
    """(5, 48, 88) raw frames: a slowly moving surface (steps within delta from frame to frame) with holes -> the reference chain's
    planes and average, computed once."""
    rng = np.random.default_rng(4888)
    base = _walk(rng, (1, 48, 88), 2, zeros=0)[0].astype(np.int64) % 3000 + 500
    raw = np.stack([np.clip(base + rng.integers(-15, 16, base.shape) * (i + 1) // 2, 1, 65535) for i in range(5)]).astype(np.uint16)
    raw[rng.random(raw.shape) < 0.12] = 0
    terms = [CHAIN_DEPTH[k] for k in ('fx', 'fy', 'cx', 'cy')]
    ext = CHAIN_EXT['rotation'] + CHAIN_EXT['translation']
    ref = feed_ref.Chain(terms, terms, ext, 0.001, (48, 88))
    planes = ref.process_many(raw)
    ref.reset()
    return raw, planes, ref.average(raw)


def _conditioner(**kw):
    from rope_s3d_amd.prediction.conditioning import DepthConditioner
    return DepthConditioner(CHAIN_DEPTH, CHAIN_DEPTH, CHAIN_EXT, 0.001, **kw)


def test_conditioner_equals_the_reference_chain(chain):
    raw, want, want_mean = chain
    assert (want != 0).mean() > 0.5
    c = _conditioner()
    many = c.process_many(raw)
    assert many.dtype == np.uint16 and many.shape == (5, 48, 88) and np.array_equal(many, want)
    c.reset()
    assert np.array_equal(np.stack([c.process(f) for f in raw]), many)              # frame by frame
    assert not np.array_equal(c.process(raw[0]), many[0])                            # the state is kept ...
    c.reset()
    assert np.array_equal(c.process(raw[0]), many[0])                                # ... until it is reset: a fresh instance
    assert np.array_equal(_conditioner().process(raw[0]), many[0])
    c.reset()
    mean = c.average(raw)
    assert mean.dtype == np.float64 and np.array_equal(mean, want_mean)
    assert np.array_equal(c.metres(many[1]), np.array(many[1], dtype=float) * 0.001)
    dev = _conditioner().process_many_device(_dev(raw))
    assert dev.dtype == torch.uint16 and dev.is_cuda and np.array_equal(_host(dev.view(torch.int16)), many)
    with pytest.raises(ValueError):
        c.process_many(raw[:, :40])                                                  # not the sensor's size
    with pytest.raises(ValueError):
        c.process(raw.astype(np.int32)[0])


def test_conditioner_with_filters_switched_off(chain):
    raw = chain[0][:2]
    terms = [CHAIN_DEPTH[k] for k in ('fx', 'fy', 'cx', 'cy')]
    ext = CHAIN_EXT['rotation'] + CHAIN_EXT['translation']
    for kw in (dict(decimation=None), dict(spatial=None), dict(temporal=None), dict(decimation=None, spatial=None, temporal=None)):
        ref = feed_ref.Chain(terms, terms, ext, 0.001, (48, 88), **{**dict(decimation=2, spatial=(2, 0.5, 20), temporal=(0.5, 20, 3)), **kw})
        keep = raw.copy()
        assert np.array_equal(_conditioner(**kw).process_many(raw), ref.process_many(raw)), kw
        assert np.array_equal(raw, keep)


# ------------------------------------------------------------------------------------------------------------------ end to end
E2E_SCALE = 0.001


@pytest.fixture(scope='module')
def raw_folder(tmp_path_factory):
    """Four frames of a synthetic set at 320 x 240 (the Renderer's depth, metres) written as a raw capture: depth quantised to z16
    at 1 mm, holes punched by a seeded mask, the colour frames as they are; equal sensors, identity extrinsics."""
    from rope_s3d_amd.data.dataset import Dataset, make_synthetic_dataset
    from rope_s3d_amd.projection import Intrinsics
    intr = Intrinsics('640_480_color')
    intr.downscale(2)
    root = tmp_path_factory.mktemp('feed')
    ds = Dataset(make_synthetic_dataset(str(root / 'parent4'), 4, base_intrin=str(intr), seed=7919))
    folder = str(root / 'raw4')
    os.makedirs(folder)
    rng = np.random.default_rng(240)
    sensor = {k: float(getattr(intr, k)) for k in ('fx', 'fy', 'cx', 'cy')}
    sensor.update(width=intr.width, height=intr.height, coeffs=[0.0] * 5)
    depths = []
    for i in range(4):
        z = np.clip(np.floor(np.asarray(ds.depthmaps[i], np.float64) / E2E_SCALE + 0.5), 0, 65535).astype(np.uint16)
        z[rng.random(z.shape) < 0.05] = 0
        depths.append(z)
        np.save(os.path.join(folder, f'depth_{i:06d}.npy'), z)
        np.save(os.path.join(folder, f'color_{i:06d}.npy'), np.asarray(ds.og_img[i]))
    with open(os.path.join(folder, 'sensor.json'), 'w') as f:
        json.dump({'depth': sensor, 'color': sensor, 'extrinsics': {'rotation': [1, 0, 0, 0, 1, 0, 0, 0, 1], 'translation': [0, 0, 0]},
                   'depth_scale': E2E_SCALE, 'angles': np.asarray(ds.angles).tolist()}, f)
    terms = [sensor[k] for k in ('fx', 'fy', 'cx', 'cy')]
    ref = feed_ref.Chain(terms, terms, hand.IDENTITY, E2E_SCALE, (intr.height, intr.width))
    conditioned = [ref.metres(ref.process(z)) for z in depths]
    return ds, folder, conditioned


def test_raw_recording_camera_equals_the_reference_chain(raw_folder):
    from rope_s3d_amd.prediction.feed import RawRecordingCamera
    ds, folder, conditioned = raw_folder
    assert (conditioned[0] != 0).any()
    cam = RawRecordingCamera(folder)
    cam.start()
    for i in range(4):
        color, depth = cam.get()
        assert np.array_equal(color, np.asarray(ds.og_img[i])) and depth.dtype == np.float64 and np.array_equal(depth, conditioned[i]), i
    assert cam.get() is None


def test_live_loop_over_a_raw_folder_predicts_what_the_reference_frames_give(raw_folder, tmp_path, monkeypatch):
    import importlib
    from rope_s3d_amd.prediction.feed import RawRecordingCamera
    ds, folder, conditioned = raw_folder
    monkeypatch.chdir(tmp_path)
    pl = importlib.import_module('predict_live')
    cam = RawRecordingCamera(folder)
    live = pl.Live(str(ds.intrinsics), ds, 'SLU', 2, camera=cam, link=cam.claims(), save_to=None, color_dict=ds.attrs['color_dict'],
                   lookup_divisions=4)
    assert live.run() == 4
    live.stop()
    assert np.array_equal(np.array(live.running_claims), np.asarray(ds.angles))
    want = np.array([live.pred.run(np.copy(ds.og_img[i]), conditioned[i]) for i in range(4)])
    assert np.array_equal(np.array(live.running_predictions), want)
