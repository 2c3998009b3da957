"""GPU: the segmentation path's targets built on the device from device-resident instance masks (rope_stage_targets_segmented,
csrc/rope_targets.hip; Engine.stage_targets_segmented, Predictor(device_targets=True)).

The reference throughout is the host function rope_prepare_segmented, per frame with f = 1: the resident planes after
rope_commit_targets (rope_debug_targets) equal its output bit for bit — the packed plane, both float planes viewed as uint32,
the 8 flag bytes.  The one exception is a NaN in a float plane: NaN-ness is compared there, not the payload."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR

import helpers

pytestmark = pytest.mark.gpu

TW, TH = eng.TARGET_TILE_W, eng.TARGET_TILE_H
E_ARG = -1
SPECIAL = np.array([0.0, -1.5, np.nan, np.inf, 1e-12, 127.9999, 200.0])      # 200.0 clips to 2^39 - 1


@pytest.fixture(scope='module')
def engine():
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    return e


def _camera(e, H, W):
    _, PV = helpers.camera('640_480_color')
    e.set_camera(PV, W, H, ZNEAR, ZFAR)


def _depth(rng, n, H, W, dtype):
    """Positive depths with the special values strewn in thickly: under and outside every body mask."""
    d = rng.uniform(0.3, 3.0, (n, H, W))
    pick = rng.random((n, H, W)) < 0.3
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return np.ascontiguousarray(d.astype(dtype))


def _bars(H, W, axis):
    """Bars two pixels wide separated by gaps of 1..9, across `axis`."""
    line = np.zeros(W if axis == 1 else H, np.uint8)
    at, gap = 1, 1
    while at < len(line):
        line[at:at + 2] = 1
        at += 2 + gap
        gap = gap % 9 + 1
    return np.broadcast_to(line[None, :] if axis == 1 else line[:, None], (H, W)).copy()


def _mask_cases(rng, H, W):
    """name -> (masks (K, H, W) uint8, link_of (K,)): one frame each."""
    z = lambda: np.zeros((H, W), np.uint8)                                   # noqa: E731
    cases = {'no instance': (np.zeros((0, H, W), np.uint8), [])}
    cases['all ones'] = (np.ones((1, H, W), np.uint8), [0])
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    single = np.zeros((len(pts), H, W), np.uint8)
    for k, (y, x) in enumerate(pts):
        single[k, y, x] = 1
    cases['corners and edge middles'] = (single, [k % 6 for k in range(len(pts))])
    cases['bars'] = (np.stack([_bars(H, W, 1), _bars(H, W, 0)]), [1, 2])
    cases['bernoulli'] = (np.stack([(rng.random((H, W)) < 0.02) * np.uint8(255), (rng.random((H, W)) < 0.5) * np.uint8(2)]).astype(np.uint8), [0, 3])
    sparse = (rng.random((H, W)) < 0.02).astype(np.uint8)
    cases['sparse alone'] = (sparse[None], [5])
    left, right = z(), z()
    left[H // 4:H // 2 + 1, :W // 2] = 1
    right[H // 3:, W // 2:] = 1
    cases['two instances of one link'] = (np.stack([left, right]), [2, 2])
    blob, other = z(), z()
    blob[:H // 2 + 1, W // 3:] = 1
    other[H // 2:, :W // 2 + 1] = 1
    cases['an instance of no link widens the body'] = (np.stack([blob, other]), [-1, 0])
    cases['only an instance of no link'] = (blob[None].copy(), [-1])
    cases['link with an all-zero mask'] = (np.stack([z(), other]), [1, 4])
    return cases


def _reference(depth, masks, link_of, n_lookup):
    """rope_prepare_segmented per frame, f = 1 -> (tq, t32, tsweep, flags)."""
    n, H, W = depth.shape
    tq, t32, ts, flags = np.empty((n, H, W), np.uint64), np.empty((n, H, W), np.float32), np.empty((n, H, W), np.float32), np.zeros((n, 8), np.uint8)
    for i in range(n):
        tgt = np.empty((H, W), np.float64)
        hwk = np.ascontiguousarray(masks[i].transpose(1, 2, 0))
        assert eng.prepare_segmented(depth[i], 1, hwk, link_of[i], 6, n_lookup, tq[i], t32[i], flags[i], tgt)
        with np.errstate(all='ignore'):
            ts[i] = tgt
    return tq, t32, ts, flags


def _stage(e, depth, masks, link_of, n_lookup, want_ts, lo, hi, n_total):
    """Frames lo .. hi - 1 into their slots."""
    first = np.concatenate([[0], np.cumsum([len(masks[i]) for i in range(lo, hi)])])
    links = [l for i in range(lo, hi) for l in link_of[i]]
    planes = np.concatenate([masks[i] for i in range(lo, hi)])
    depth_t = torch.from_numpy(depth[lo:hi]).cuda()
    masks_t = torch.from_numpy(planes).cuda() if len(planes) else None
    e.stage_targets_segmented(depth_t, masks_t, first, links, n_lookup, n_total, lo, want_ts)


def _device(e, depth, masks, link_of, n_lookup, want_ts=True, calls=None):
    n = len(depth)
    for lo, hi in calls or [(0, n)]:
        _stage(e, depth, masks, link_of, n_lookup, want_ts, lo, hi, n)
    e.commit_targets()
    return e.debug_targets(want_ts)


def _same_floats(got, want):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return np.array_equal(nan_g, nan_w) and np.array_equal(got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w])


def _check(got, want, names=None, want_ts=True):
    for i in range(len(want[0])):
        label = f"frame {i}" + (f" ({names[i]})" if names else "")
        assert np.array_equal(got[0][i], want[0][i]), f"{label}: packed plane differs at {np.argwhere(got[0][i] != want[0][i])[:4].tolist()}"
        assert _same_floats(got[1][i], want[1][i]), f"{label}: lookup plane"
        if want_ts:
            assert _same_floats(got[2][i], want[2][i]), f"{label}: TensorSweep plane"
        assert np.array_equal(got[3][i], want[3][i]), f"{label}: flags {got[3][i]} vs {want[3][i]}"


# 1x1; smaller than both windows; about the windows' size; a frame of several tiles; and around the tile in each axis
SIZES = [(1, 1), (5, 6), (7, 8), (8, 7), (90, 160), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1),
         (TH - 1, 2 * TW + 1), (2 * TH + 1, TW - 1), (TH + 1, TW), (TH, TW + 1)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('H,W', SIZES, ids=[f'{h}x{w}' for h, w in SIZES])
def test_every_mask_case_equals_the_host_function(engine, H, W, dtype):
    """One call over a frame per mask case (K from 0 to 8 in one call), depths full of special values."""
    rng = np.random.default_rng(H * 1000 + W)
    cases = _mask_cases(rng, H, W)
    names = list(cases)
    masks, link_of = [cases[k][0] for k in names], [cases[k][1] for k in names]
    depth = _depth(rng, len(names), H, W, dtype)
    _camera(engine, H, W)
    want = _reference(depth, masks, link_of, 4)
    got = _device(engine, depth, masks, link_of, 4)
    _check(got, want, names)
    i = names.index('link with an all-zero mask')
    assert got[3][i][1] == 1, "a link that has an instance with an empty mask has flag value 1"
    assert not got[3][names.index('no instance')].any()
    if H * W > 64:                                              # the cases must bite: set and clear pixels, NaN under a cleared body pixel
        assert (want[0] >> np.uint64(40)).any() and np.isnan(want[2]).any() and (want[2] == 0).any() and (want[1] != want[2])[~np.isnan(want[2])].any()


@pytest.mark.parametrize('n_lookup', [0, 2, 6])
def test_lookup_links_absent_and_all(engine, n_lookup):
    """body_look empty (no lookup links at all, or only instances of the other links) up to every link a lookup link."""
    H, W = TH + 5, TW + 9
    rng = np.random.default_rng(77 + n_lookup)
    cases = _mask_cases(rng, H, W)
    names = list(cases)
    masks, link_of = [cases[k][0] for k in names], [cases[k][1] for k in names]
    depth = _depth(rng, len(names), H, W, np.float32)
    _camera(engine, H, W)
    want = _reference(depth, masks, link_of, n_lookup)
    _check(_device(engine, depth, masks, link_of, n_lookup), want, names)
    if n_lookup == 0:
        assert not np.nan_to_num(want[1], nan=0.0).any(), "no lookup links: the lookup plane holds zeros (and NaN where inf or NaN met a zero)"


@pytest.mark.parametrize('n_depth,flag', [(5, 1), (6, 3)])
def test_five_per_cent_rule(engine, n_depth, flag):
    """n_mask = 100: five pixels with depth are not MORE than 5 % (bit 1 clear), six are."""
    H, W = 16, 24
    m = np.zeros((1, H, W), np.uint8)
    m[0, 3:13, 5:15] = 1
    depth = np.zeros((1, H, W), np.float32)
    depth[0, 4, 6:6 + n_depth] = 1.25
    depth[0, 0, 0] = 2.0                                        # outside the body: does not count
    _camera(engine, H, W)
    want = _reference(depth, [m], [[0]], 4)
    got = _device(engine, depth, [m], [[0]], 4)
    _check(got, want)
    assert got[3][0][0] == flag and want[3][0][0] == flag


@pytest.mark.parametrize('want_ts', [False, True], ids=['lookup plane only', 'with the TensorSweep plane'])
def test_a_set_filled_by_two_calls(engine, want_ts):
    """Five frames, slots [0, 2) and [2, 5) (three frames with K = 2, 0, 8 in one call)."""
    H, W = 40, 70
    rng = np.random.default_rng(5)
    cases = _mask_cases(rng, H, W)
    names = ['bernoulli', 'bars', 'two instances of one link', 'no instance', 'corners and edge middles']
    masks, link_of = [cases[k][0] for k in names], [cases[k][1] for k in names]
    depth = _depth(rng, 5, H, W, np.float64)
    _camera(engine, H, W)
    got = _device(engine, depth, masks, link_of, 4, want_ts, calls=[(0, 2), (2, 5)])
    _check(got, _reference(depth, masks, link_of, 4), names, want_ts)
    assert got[2] is None or want_ts


def test_kernels_run_behind_the_work_that_wrote_the_masks(engine):
    """The masks are the result of a torch operation on a stream of its own, enqueued behind a long one right before the call;
    the test does not synchronise: the staging kernels are on that stream, and rope_commit_targets waits for them."""
    H, W = 90, 160
    rng = np.random.default_rng(11)
    cases = _mask_cases(rng, H, W)
    names = ['bernoulli', 'an instance of no link widens the body', 'bars']
    masks, link_of = [cases[k][0] for k in names], [cases[k][1] for k in names]
    depth = _depth(rng, 3, H, W, np.float32)
    _camera(engine, H, W)
    planes = np.concatenate(masks)
    half_a = torch.from_numpy(planes & np.uint8(0x0F)).cuda()
    half_b = torch.from_numpy(planes & np.uint8(0xF0)).cuda()
    depth_src = torch.from_numpy(depth).cuda()
    busy = torch.randn(4096, 4096, device='cuda')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(8):
            busy = busy @ busy * 1e-3
        masks_t = half_a | half_b
        depth_t = depth_src + 0
        first = np.concatenate([[0], np.cumsum([len(m) for m in masks])])
        engine.stage_targets_segmented(depth_t, masks_t, first, [l for ls in link_of for l in ls], 4, 3, 0, True)
    engine.commit_targets()
    _check(engine.debug_targets(True), _reference(depth, masks, link_of, 4), names)
    torch.cuda.synchronize()


def test_refusals_leave_the_resident_set_alone(engine):
    H, W = 20, 30
    rng = np.random.default_rng(3)
    cases = _mask_cases(rng, H, W)
    masks, link_of = [cases['bars'][0], cases['bernoulli'][0]], [cases['bars'][1], cases['bernoulli'][1]]
    depth = _depth(rng, 2, H, W, np.float32)
    _camera(engine, H, W)
    before = _device(engine, depth, masks, link_of, 4)
    lib, ctx = engine._lib, engine._ctx
    depth_t = torch.from_numpy(depth).cuda()
    masks_t = torch.from_numpy(np.concatenate(masks)).cuda()
    torch.cuda.synchronize()
    dp, mp = C.c_void_p(depth_t.data_ptr()), C.c_void_p(masks_t.data_ptr())
    i32 = lambda *v: np.array(v, np.int32)                                   # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)                               # noqa: E731
    first, links = i32(0, 2, 4), i32(1, 2, 0, 3)

    def call(n_total=2, slot0=0, n_frames=2, depth_p=dp, kind=1, masks_p=mp, first_a=first, links_a=links, n_lookup=4):
        return lib.rope_stage_targets_segmented(ctx, n_total, slot0, n_frames, depth_p, kind, masks_p, None if first_a is None else p(first_a),
                                                None if links_a is None else p(links_a), n_lookup, 1, None)

    refused = {
        'null masks where instances exist': dict(masks_p=None),
        'null link_of where instances exist': dict(links_a=None),
        'null inst_first': dict(first_a=None),
        'null depth': dict(depth_p=None),
        'slots beyond the set': dict(slot0=1),
        'slot0 beyond the set': dict(slot0=3, n_frames=1),
        'non-monotone inst_first': dict(first_a=i32(0, 3, 2)),
        'negative first offset': dict(first_a=i32(-1, 2, 4)),
        'link_of beyond the links': dict(links_a=i32(1, 2, 6, 3)),
        'link_of below -1': dict(links_a=i32(1, -2, 0, 3)),
        'n_lookup_links negative': dict(n_lookup=-1),
        'n_lookup_links beyond the links': dict(n_lookup=7),
        'unknown depth_kind': dict(kind=3),
        'no frames': dict(n_frames=0),
    }
    for what, kw in refused.items():
        assert call(**kw) == E_ARG, what
        assert lib.rope_commit_targets(ctx) == E_ARG, f"{what}: nothing complete is staged"
    # a changed n_total in mid-set, and a set that is simply not complete yet
    assert call(n_total=3, n_frames=2) == 0
    assert lib.rope_commit_targets(ctx) == E_ARG, "two of three slots filled"
    assert call(n_total=3, n_frames=2) == 0
    assert call(n_total=4, slot0=2, n_frames=1, first_a=i32(0, 2), links_a=i32(1, 2)) == E_ARG, "n_total changed in mid-set"
    assert lib.rope_commit_targets(ctx) == E_ARG
    assert b'rope_stage_targets_segmented' in lib.rope_last_error(ctx)
    # the resident set is what it was, and still serves evaluations
    after = engine.debug_targets(True)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    cand = np.zeros((2, 6))
    err = engine.eval_targets(cand, [0, 1], 6, eng.LOSS_DEPTH)
    assert err.shape == (2,)
    # a refused call changes nothing: a complete staging that waits for its commit is still taken
    _stage(engine, depth, masks, link_of, 4, True, 0, 2, 2)
    assert call(kind=3) == E_ARG and call(n_total=5, slot0=1, n_frames=1, first_a=i32(0, 2), links_a=i32(1, 2)) == E_ARG
    engine.commit_targets()
    _check(engine.debug_targets(True), before)
    # and so is a half-filled set: slot 0, a refusal, slot 1
    _stage(engine, depth, masks, link_of, 4, True, 0, 1, 2)
    assert call(slot0=1, n_frames=1, first_a=i32(0, 2), links_a=i32(1, 9)) == E_ARG
    _stage(engine, depth, masks, link_of, 4, True, 1, 2, 2)
    engine.commit_targets()
    _check(engine.debug_targets(True), before)


# ---- end to end: Predictor(device_targets=True)

class _DeviceColorSegmenter:
    """ColorSegmenter whose masks can also be had on the GPU, as a network's would be."""
    stateless = True

    def __init__(self, inner):
        self.inner, self.device_batches = inner, []

    def __call__(self, color):
        return self.inner(color)

    def batch_device(self, frames):
        self.device_batches.append(len(frames))
        out = []
        for f in frames:
            r = self.inner(f)
            out.append({'class_ids': r['class_ids'], 'scores': r['scores'],
                        'masks_device': torch.from_numpy(np.ascontiguousarray(r['masks'].transpose(2, 0, 1))).cuda()})
        return out


@pytest.fixture(scope='module')
def pipeline():
    from rope_s3d_amd import Predictor, Renderer
    from rope_s3d_amd.segmentation import ColorSegmenter
    rb = helpers.robot()
    lim = rb.joint_limits
    r = Renderer('seg', DEFAULT_CAMERA_POSE, '640_480_color')
    rng = np.random.default_rng(2024)
    colors, depths = [], []
    for _ in range(12):
        r.setJointAngles(rng.uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0]))
        color, depth = r.render()
        colors.append(color)
        depths.append(np.asarray(depth, np.float64))
    seg = _DeviceColorSegmenter(ColorSegmenter(['BG'] + rb.link_names[:6], split_instances=True))
    make = lambda flag: Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', segmenter=seg, lookup_divisions=4, device_targets=flag)  # noqa: E731
    off, on = make(False), make(True)
    on.SEG_BATCH = 2                                            # several staging calls per group
    return off, on, seg, colors, depths


@pytest.mark.parametrize('batch,dtype', [(12, np.float64), (5, np.float64), (5, np.float32)], ids=['one group', 'short last group', 'float32 depth'])
def test_predictor_with_device_targets_gives_the_same_angles_and_traces(pipeline, batch, dtype):
    off, on, seg, colors, depths = pipeline
    depths = [d.astype(dtype) for d in depths]
    want = off.run_many(colors, [d.copy() for d in depths], batch=batch)
    want_trace = off.traces._trace.copy()
    del seg.device_batches[:]
    got = on.run_many(colors, [d.copy() for d in depths], batch=batch)
    assert seg.device_batches and max(seg.device_batches) <= 2 and sum(seg.device_batches) == 12, "the device path was not taken"
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(on.traces._trace.view(np.uint64), want_trace.view(np.uint64))        # the last group's frames, stage by stage


def test_mask_rcnn_masks_go_from_the_network_to_the_planes_on_the_device():
    """MaskRCNNSegmenter with random weights in front: the planes the device path leaves resident equal rope_prepare_segmented's
    over the same detections (the masks the network left on the GPU, copied down by the test)."""
    from rope_s3d_amd import Predictor, Renderer
    from rope_s3d_amd.maskrcnn import MaskRCNNSegmenter
    net = MaskRCNNSegmenter(7, device='cuda:0', seed=1, min_confidence=0.7)
    r = Renderer('seg', DEFAULT_CAMERA_POSE, '640_480_color')
    colors, depths = [], []
    for q in ([0.3, 0.4, 0.9, 0, 0, 0], [-0.5, 0.2, 0.4, 0, 0, 0]):
        r.setJointAngles(q)
        color, depth = r.render()
        colors.append(color)
        depths.append(np.asarray(depth, np.float32))
    p = Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', segmenter=net, lookup_divisions=4, device_targets=True)
    small = [p._downsample(c, 4) for c in colors]
    for conf in (0.7, 0.5, 0.3, 0.2, 0.15, 0.0):                # lowered until the host path finds something in every frame
        net.net.min_conf = conf
        host = net.batch(small)
        if all(len(h['class_ids']) >= 1 for h in host):
            break
    assert all(len(h['class_ids']) >= 1 and h['masks'].shape == (120, 160, len(h['class_ids'])) for h in host), "no detections at any confidence"

    seen = []
    inner = net.batch_device

    def recording(frames):
        out = inner(frames)
        if out[0]['masks_device'].shape[0]:                     # the network's own tensor goes to the engine, not a copy of it
            assert Predictor._stacked(out).data_ptr() == out[0]['masks_device'].data_ptr()
            assert Predictor._stacked(out).shape[0] == sum(len(o['class_ids']) for o in out)
        seen.extend((o['class_ids'].copy(), o['masks_device'].cpu().numpy().view(np.uint8)) for o in out)
        return out
    net.batch_device = recording
    net.batches_device = lambda groups: (recording(g) for g in groups)
    p.run_many(colors, [d.copy() for d in depths], batch=2)
    assert len(seen) == 2 and all(len(ids) >= 1 for ids, _ in seen)
    got = p.engine.debug_targets(p._has_tsweep())
    depth = np.stack([p._downsample(d, 4) for d in depths])
    link_of = [[p.link_names.index(p.classes[c]) if p.classes[c] in p.link_names else -1 for c in ids] for ids, _ in seen]
    want = _reference(depth, [m for _, m in seen], link_of, 6)
    _check(got, want, want_ts=p._has_tsweep())
    assert (want[0] >> np.uint64(40)).any(), "the detections cover no pixel: the comparison would be empty"
