"""GPU: a synthetic run's frames kept on the device — rope_render_batch_device, rope_depth_holes, rope_stage_targets_synthetic
(csrc/rope_synth.hip) and SyntheticPredictor.run_batch_poses(batch=...).  Every comparison is bit for bit; the one exception is a NaN
in a float plane, where NaN-ness is compared and not the payload.

References: rope_render_batch for the renders; tests/holes_ref.py (the integer contract in numpy) for the holes; the host function
rope_prepare_synthetic on the colour plane blue_of_id[ids] for the targets; the per-frame loop and Predictor.run_many for the run."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import BACKGROUND_ID, DEFAULT_CAMERA_POSE, DEFAULT_RENDER_COLORS, ZFAR, ZNEAR
from rope_s3d_amd.projection import camera_matrix

import helpers
import holes_ref

pytestmark = pytest.mark.gpu

E_ARG = -1
LUT = np.zeros(256, np.uint8)                                     # Renderer's table in mode 'seg': channel 0 of every link's colour
LUT[:6] = [DEFAULT_RENDER_COLORS[i][0] for i in range(6)]
LINK_BLUE = [int(DEFAULT_RENDER_COLORS[i][0]) for i in range(6)]
POSES = np.array([[0.4, 0.3, 0.8, 0, 0, 0], [-0.9, 0.7, 0.2, 0.5, -0.4, 0.3], [1.3, -0.2, 1.1, 0, 0.6, 0], [0, 0, 0, 0, 0, 0],
                  [-0.3, 0.9, -0.5, 1.0, 0.2, -0.7]])


@pytest.fixture(scope='module')
def engines():
    """Two contexts on one GPU, as SyntheticPredictor holds them: one draws the full-size frames, one takes the targets."""
    out = []
    for _ in range(2):
        e = eng.Engine(0)
        e.set_robot(helpers.robot())
        out.append(e)
    return out


def _camera(e, H, W, ds=4):
    _, PV = helpers.camera('640_480_color', ds)
    e.set_camera(PV, W, H, ZNEAR, ZFAR)


def _same_floats(got, want):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return np.array_equal(nan_g, nan_w) and np.array_equal(got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w])


# ---- renders that stay on the device

def test_device_renders_equal_host_renders(engines):
    e = engines[0]
    _camera(e, 120, 160)
    intr, PV = helpers.camera('640_480_color', 4)
    away = camera_matrix([0, -1.5, .75, 0, 0, np.pi], intr, ZNEAR, ZFAR)          # turned round: nothing of the robot in the frame
    views = np.stack([PV, PV, PV, away, PV])
    for pv in (None, views):
        want_d, want_i = e.render_batch(POSES, 6, pv)
        got_d, got_i = e.render_batch_device(POSES, 6, pv)
        assert got_d.device.type == 'cuda' and got_d.dtype == torch.float32 and got_i.dtype == torch.uint8
        assert np.array_equal(got_i.cpu().numpy(), want_i)
        assert np.array_equal(got_d.cpu().numpy().view(np.uint32), want_d.view(np.uint32))
    assert (want_i[3] == BACKGROUND_ID).all() and not want_d[3].any(), "the fourth view was to leave its frame empty"
    assert all((want_i[k] != BACKGROUND_ID).any() for k in (0, 1, 2, 4))


# ---- depth holes

def _plane(rng, n, H, W):
    d = rng.uniform(0.3, 3.0, (n, H, W)).astype(np.float32)
    d[rng.random((n, H, W)) < 0.2] = 0.0                        # a render's background
    return d


HOLE_CASES = {                                                    # n, H, W, frame0, std
    '150x100, defaults': (1, 100, 150, 0, .22),
    '150x100, blocks merge and touch the borders': (1, 100, 150, 0, .24),
    '1280x720': (1, 720, 1280, 0, .22),
    'three frames from frame 2': (3, 100, 150, 2, .22),
}


@pytest.mark.parametrize('case', list(HOLE_CASES))
def test_holes_equal_the_numpy_contract(engines, case):
    n, H, W, frame0, std = HOLE_CASES[case]
    seed = 0x9E3779B97F4A7C15
    depth = _plane(np.random.default_rng(H + n), n, H, W)
    masks = [holes_ref.hole_mask(H, W, frame0 + m, seed, std=std) for m in range(n)]
    for m in masks:                                             # asserted on the reference alone: the comparison must show something
        assert m.any() and not m.all()
    if 'borders' in case:
        m = masks[0]
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and m.mean() > .5
    if n > 1:
        # frame0 moves the stream: what the device is held to below is not the run's first frames
        assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[0], holes_ref.hole_mask(H, W, 0, seed, std=std))
    want = np.stack([holes_ref.holes(depth[m], frame0 + m, seed, std=std) for m in range(n)])
    t = torch.from_numpy(depth).cuda()
    engines[0].depth_holes(t, seed, frame0=frame0, std=std)
    got = t.cpu().numpy()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), f"{len(bad)} pixels differ, first {bad[:4].tolist()}"


def test_holes_take_a_single_plane_and_refuse_what_the_kernel_cannot_hold(engines):
    H, W, seed = 40, 70, 12345
    depth = _plane(np.random.default_rng(0), 1, H, W)[0]
    t = torch.from_numpy(depth).cuda()
    engines[0].depth_holes(t, seed, frame0=7, std=.24)
    want = holes_ref.holes(depth, 7, seed, std=.24)
    assert (want != depth).any()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(eng.EngineError):
        engines[0].depth_holes(t, seed, connection_factor=33)
    with pytest.raises(ValueError):
        engines[0].depth_holes(t.double(), seed)


# ---- targets from device planes

def _reference(depth, ids, f, n_lookup, link_blue=LINK_BLUE):
    """rope_prepare_synthetic per frame on the colour plane LUT[ids] -> (tq, t32, tsweep, flags)."""
    n, H0, W0 = depth.shape
    H, W = H0 // f, W0 // f
    tq, t32, ts, flags = np.empty((n, H, W), np.uint64), np.empty((n, H, W), np.float32), np.empty((n, H, W), np.float32), np.zeros((n, 8), np.uint8)
    for i in range(n):
        color = np.zeros((H0, W0, 3), np.uint8)
        color[..., 0] = LUT[ids[i]]
        tgt = np.empty((H, W), np.float64)
        assert eng.prepare_synthetic(color, depth[i], f, link_blue, n_lookup, tq[i], t32[i], flags[i], tgt)
        with np.errstate(all='ignore'):
            ts[i] = tgt
    return tq, t32, ts, flags


def _device(e, depth, ids, f, n_lookup, want_ts, calls, link_blue=LINK_BLUE):
    n = len(depth)
    for lo, hi in calls:
        e.stage_targets_synthetic(torch.from_numpy(depth[lo:hi]).cuda(), torch.from_numpy(ids[lo:hi]).cuda(), f, LUT, link_blue, n_lookup, n, lo, want_ts)
    e.commit_targets()
    return e.debug_targets(want_ts)


def _check(got, want, want_ts):
    for i in range(len(want[0])):
        assert np.array_equal(got[0][i], want[0][i]), f"frame {i}: packed plane differs at {np.argwhere(got[0][i] != want[0][i])[:4].tolist()}"
        assert _same_floats(got[1][i], want[1][i]), f"frame {i}: lookup plane"
        if want_ts:
            assert _same_floats(got[2][i], want[2][i]), f"frame {i}: TensorSweep plane"
        assert np.array_equal(got[3][i], want[3][i]), f"frame {i}: flags {got[3][i]} vs {want[3][i]}"


def _made_up(rng, H, W, f):
    """Three frames (depth, ids) of H f x W f: random links in blocks with single pixels strewn in (so that the down-sampled colour
    also takes values that are no link's) and depths full of special values; the 5 % rule from both sides with a link absent;
    depth 0 inside every mask."""
    up = np.ones((f, f), np.uint8)
    choice = np.array([0, 1, 2, 3, 4, 5, BACKGROUND_ID], np.uint8)
    ids = np.kron(choice[rng.integers(0, 7, (H // 4 + 1, W // 4 + 1))], np.ones((4 * f, 4 * f), np.uint8))[:H * f, :W * f]
    strew = rng.random(ids.shape) < 0.1
    ids[strew] = choice[rng.integers(0, 7, int(strew.sum()))]
    depth = rng.uniform(0.3, 3.0, ids.shape).astype(np.float32)
    pick = rng.random(ids.shape) < 0.3
    depth[pick] = rng.choice(np.array([0.0, -1.5, np.nan, np.inf, 1e-12, 127.9999, 200.0], np.float32), int(pick.sum()))
    # links 2 and 3 with 100 pixels each, 5 and 6 of them with depth; link 5 (and 1, 4) absent
    ids_lo = np.full((H, W), BACKGROUND_ID, np.uint8)
    ids_lo[2:12, 3:13] = 2
    ids_lo[12:22, 20:30] = 3
    depth_lo = np.zeros((H, W), np.float32)
    depth_lo[4, 5:10] = 1.25
    depth_lo[14, 21:27] = 0.75
    depth_lo[0, 0] = 2.0
    ids_r, depth_r = np.kron(ids_lo, up), np.kron(depth_lo, up.astype(np.float32))
    ids_z = np.kron(choice[rng.integers(0, 7, (H // 8 + 1, W // 8 + 1))], np.ones((8 * f, 8 * f), np.uint8))[:H * f, :W * f]
    depth_z = np.where(ids_z == BACKGROUND_ID, np.float32(1.5), np.float32(0.0))
    return np.stack([depth, depth_r, depth_z]), np.stack([ids, ids_r, ids_z])


# context size, f: the issue's three, and two whose pixel count is no multiple of the kernel's 256 pixels per workgroup (160 x 120 is);
# factors 4 and 6 (the taps f/2 - 1 and f/2 at a factor that is no power of two) on a context of 30 x 24
GEOMETRIES = [(120, 160, 1), (120, 160, 2), (24, 40, 8), (100, 150, 1), (118, 158, 2), (24, 30, 4), (24, 30, 6)]


@pytest.mark.parametrize('want_ts', [False, True], ids=['lookup plane only', 'with the TensorSweep plane'])
@pytest.mark.parametrize('H,W,f', GEOMETRIES, ids=[f'{w}x{h} from {w * f}x{h * f}' for h, w, f in GEOMETRIES])
def test_staged_planes_equal_the_host_function(engines, H, W, f, want_ts):
    """A set of five frames — two renders, three made up — filled in calls of 2 + 2 + 1 slots."""
    e_r, e_t = engines
    _camera(e_r, H * f, W * f, ds=max(1, 4 // f))
    _camera(e_t, H, W)
    rd, ri = e_r.render_batch(POSES[:2], 6)
    md, mi = _made_up(np.random.default_rng(H * f + W), H, W, f)
    depth, ids = np.ascontiguousarray(np.concatenate([rd, md])), np.ascontiguousarray(np.concatenate([ri, mi]))
    want = _reference(depth, ids, f, 4)
    got = _device(e_t, depth, ids, f, 4, want_ts, [(0, 2), (2, 4), (4, 5)])
    _check(got, want, want_ts)
    assert got[2] is None or want_ts
    # the cases must bite (asserted on the reference): link pixels in the renders, NaN and zero depths, the flag values
    assert all((want[0][i] >> np.uint64(40)).any() for i in range(5)) and np.isnan(want[2][2]).any() and (want[1] != want[2])[~np.isnan(want[2])].any()
    assert want[3][3].tolist()[1:6] == [0, 1, 3, 0, 0], f"absent, five of a hundred, six of a hundred: {want[3][3]}"
    assert not (want[3][4][1:6] & 2).any() and want[3][4].any(), "depth 0 inside every mask: no link has depth"


# context size, f: outputs of one pixel, one row and one column — a single workgroup whose live lanes are fewer than a wave
SLIVERS = [(1, 1, 1), (1, 1, 2), (1, 1, 6), (1, 37, 1), (1, 37, 2), (23, 1, 4), (23, 1, 1)]


@pytest.mark.parametrize('H,W,f', SLIVERS, ids=[f'{w}x{h} from {w * f}x{h * f}' for h, w, f in SLIVERS])
def test_staged_slivers_equal_the_host_function(engines, H, W, f):
    """Twelve windows of H f x W f cut out of each of _made_up's three frames, spread over them, so that the 36 tiny frames between
    them hold pixels of several links, with and without depth, and special depths."""
    e_t = engines[1]
    _camera(e_t, H, W)
    md, mi = _made_up(np.random.default_rng(100 * H + W + f), 24, 40, f)
    cuts = [np.s_[:, y * f:(y + H) * f, x * f:(x + W) * f] for y in (0, (24 - H) // 2, 24 - H) for x in (0, (40 - W) // 3, 2 * (40 - W) // 3, 40 - W)]
    depth, ids = np.ascontiguousarray(np.concatenate([md[c] for c in cuts])), np.ascontiguousarray(np.concatenate([mi[c] for c in cuts]))
    want = _reference(depth, ids, f, 4)
    got = _device(e_t, depth, ids, f, 4, True, [(0, 5), (5, 36)])
    _check(got, want, True)
    assert got[0].shape == (36, H, W)
    # asserted on the reference: pixels of three links at the least, a NaN depth; links absent, without depth and with it
    assert len(np.unique(want[0] >> np.uint64(40))) >= 4 and np.isnan(want[2]).any()
    assert {0, 1, 3} <= set(want[3].ravel().tolist())


# link_blue, n_lookup_links: tables other than the six links of the renderer with four lookup links
LINK_TABLES = {
    'links 1 and 2 share a colour': ([LINK_BLUE[0], LINK_BLUE[1], LINK_BLUE[1], LINK_BLUE[3], LINK_BLUE[4], LINK_BLUE[5]], 4),
    'a lookup link and a later link share a colour': ([LINK_BLUE[0], LINK_BLUE[1], LINK_BLUE[2], LINK_BLUE[3], LINK_BLUE[4], LINK_BLUE[2]], 4),
    'one link': ([LINK_BLUE[2]], 1),
    'one link, no lookup link': ([LINK_BLUE[2]], 0),
    'no lookup links': (LINK_BLUE, 0),
    'every link a lookup link': (LINK_BLUE, 6),
    'three links, two of them lookup links': (LINK_BLUE[3:], 2),
}


@pytest.mark.parametrize('table', list(LINK_TABLES))
def test_staged_planes_follow_the_link_table(engines, table):
    link_blue, n_lookup = LINK_TABLES[table]
    e_t = engines[1]
    H, W, f = 24, 40, 2
    _camera(e_t, H, W)
    md, mi = _made_up(np.random.default_rng(17), H, W, f)
    want = _reference(md, mi, f, n_lookup, link_blue)
    got = _device(e_t, md, mi, f, n_lookup, True, [(0, 2), (2, 3)], link_blue)
    _check(got, want, True)
    # what the table changes, asserted on the reference
    bits = want[0] >> np.uint64(40)
    assert bits.any() and not (bits >> np.uint64(len(link_blue))).any() and not want[3][:, len(link_blue):].any()
    if 'share' in table:
        a, b = [l for l in range(6) if link_blue.count(link_blue[l]) == 2]
        both = np.uint64((1 << a) | (1 << b))
        assert ((bits & both) == both).any() and not ((bits & both) == np.uint64(1 << a)).any(), "both bits or neither"
        assert np.array_equal(want[3][:, a], want[3][:, b]) and want[3][:, a].any(), "both links are counted"
    if n_lookup == 0:
        t32 = want[1]
        assert np.isnan(t32).any() and not t32[~np.isnan(t32)].any(), "zeros where the depth is finite, NaN where it is not"
    else:
        assert want[1][~np.isnan(want[1])].any()
    if n_lookup == len(link_blue):
        hit = bits != 0
        assert np.array_equal(want[1].view(np.uint32)[hit], want[2].view(np.uint32)[hit]), "every link pixel keeps its depth"
    default = _reference(md, mi, f, 4)
    assert not all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(want, default)), "the table changes nothing"


def test_staging_refusals_are_those_of_the_segmented_call(engines):
    e_r, e_t = engines
    H, W, f = 24, 40, 2
    _camera(e_t, H, W)
    md, mi = _made_up(np.random.default_rng(9), H, W, f)
    before = _device(e_t, md, mi, f, 4, True, [(0, 3)])
    lib, ctx = e_t._lib, e_t._ctx
    depth_t, ids_t = torch.from_numpy(md).cuda(), torch.from_numpy(mi).cuda()
    torch.cuda.synchronize()
    lb = np.array(LINK_BLUE, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                               # noqa: E731

    def call(n_total=3, slot0=0, n_frames=3, H0=H * f, W0=W * f, f_=f, depth_p=C.c_void_p(depth_t.data_ptr()), n_links=6, n_lookup=4, ts=1):
        return lib.rope_stage_targets_synthetic(ctx, n_total, slot0, n_frames, depth_p, C.c_void_p(ids_t.data_ptr()), H0, W0, f_, p(LUT), p(lb),
                                                n_links, n_lookup, ts, None)

    refused = {
        'a size that is not the context\'s': dict(H0=H * f + f),
        'the size without the factor': dict(f_=1),
        'an odd factor': dict(H0=H * 3, W0=W * 3, f_=3),
        'slots beyond the set': dict(slot0=1),
        'slot0 beyond the set': dict(slot0=4, n_frames=1),
        'no frames': dict(n_frames=0),
        'null depth': dict(depth_p=None),
        'n_lookup_links beyond the links': dict(n_lookup=7),
        'too many links': dict(n_links=7),
    }
    for what, kw in refused.items():
        assert call(**kw) == E_ARG, what
        assert lib.rope_commit_targets(ctx) == E_ARG, f"{what}: nothing complete is staged"
    # a set that is not complete yet, and a changed n_total in mid-set
    assert call(n_total=4, n_frames=3) == 0
    assert lib.rope_commit_targets(ctx) == E_ARG, "three of four slots filled"
    assert call(n_total=5, slot0=3, n_frames=1) == E_ARG, "n_total changed in mid-set"
    assert call(n_total=4, slot0=3, n_frames=1, ts=0) == E_ARG, "want_tsweep changed in mid-set"
    assert lib.rope_commit_targets(ctx) == E_ARG
    assert b'rope_stage_targets_synthetic' in lib.rope_last_error(ctx)
    after = e_t.debug_targets(True)                             # the resident set is what it was
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # a refused call changes nothing: the half-filled set can be continued, then committed
    assert call(n_total=4, slot0=3, n_frames=1) == 0
    assert lib.rope_commit_targets(ctx) == 0
    e_t.n_targets = 4
    got = e_t.debug_targets(True)
    want = _reference(md, mi, f, 4)
    _check([g[:3] for g in got], want, True)
    _check([g[3:] for g in got], [w[:1] for w in want], True)


# ---- end to end

@pytest.fixture(scope='module')
def synth():
    from rope_s3d_amd.prediction.synthetic import SyntheticPredictor
    intr, _ = helpers.camera('640_480_color', 4)                 # 160 x 120 renders, predicted at 80 x 60
    sp = SyntheticPredictor(DEFAULT_CAMERA_POSE, intr, 2, 'SLU', noise=False, seed=3, lookup_divisions=4)
    sp.SUB_BATCH = 2                                             # several staging calls per group
    lim = sp.urdf_reader.joint_limits
    poses = np.random.default_rng(11).uniform(lim[:, 0], lim[:, 1], (7, 6)) * np.array([1, 1, 1, 0, 0, 0])
    return sp, poses


def test_batched_run_without_noise_equals_the_loop(synth, tmp_path):
    sp, poses = synth
    sp.do_noise = False
    want = sp.run_batch_poses(list(poses), str(tmp_path / 'loop'))
    staged = []
    inner = sp.predictor.engine.stage_targets_synthetic
    sp.predictor.engine.stage_targets_synthetic = lambda d, *a, **k: (staged.append(d.shape[0]), inner(d, *a, **k))[1]
    try:
        got = sp.run_batch_poses(list(poses), str(tmp_path / 'batched'), batch=3)
    finally:
        del sp.predictor.engine.stage_targets_synthetic
    assert staged == [2, 1, 2, 1, 1], "two full groups of three and one frame, in sub-batches of two: the device path was not taken"
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(np.load(str(tmp_path / 'batched.npy')), got) and got.shape == (2, 7, 6) and np.array_equal(got[0], poses)


def test_batched_run_with_noise_equals_run_many_on_host_built_frames(synth, tmp_path):
    sp, poses = synth
    sp.do_noise = True
    try:
        sp.rng = np.random.default_rng(5)
        seed = int(np.random.default_rng(5).integers(0, 1 << 64, dtype=np.uint64))
        got = sp.run_batch_poses(list(poses), str(tmp_path / 'noise'), batch=3)
    finally:
        sp.do_noise = False
    depth, ids = sp.renderer.render_ids_batch(poses)
    holed = [holes_ref.holes(depth[i], i, seed) for i in range(len(poses))]
    assert all((h != d).any() for h, d in zip(holed, depth)), "a frame without a hole in the robot"
    want = sp.predictor.run_many([sp.renderer._lut[i] for i in ids], holed, batch=3)
    assert np.array_equal(got[1].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(got[0], poses)
