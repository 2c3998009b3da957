"""GPU: every instantiation of the raster kernels against its scratch-free twin and the oracle.

raster_tile<LOSS, MODE, CLIP> is compiled into 46 kernels (raster_score_kernel x 28, raster_queue_kernel x 18), each
register-allocated on its own; the plain queue kernels — the default hot path — spill into scratch, the score kernels never do
(tests/test_kernel_resources.py, profiles/kernel_resources_gfx950.txt).  A kernel wrong in one instantiation only is what
DESIGN.md §6a records.  So each case here builds a batch for which the host code must pick the kernel in question and

  * runs it with strategy 0, with NO_QUEUE (raster_score_kernel instead of raster_queue_kernel), with NO_LAYERS | NO_QUEUE
    (no shared layers either) and with strategy 0 a second time — two default passes, no loop — and wants the same bits;
  * holds about ten sampled rows to the CPU oracle, bit for bit;
  * where the camera is near, counts on the CPU (cut_triangles) that triangles of the sampled rows do cross the near plane.

Which kernel a batch gets is plan_pass() of csrc/rope_passplan.h, where the rules and their thresholds are: the cases below name
them Q (the scoring queue, raster_queue_kernel<.., SCORE, ..>), L (the layer queue, raster_queue_kernel<.., LAYER, ..>), S (the split
path, raster_score_kernel<DEPTH, SPLIT, ..> + score_gtile_kernel) and C (the CLIP kernels: use_clip of rope_abi.hip, the camera within
the robot's reach of the near plane — on the camera-pose path, ANY view of the call).  tests/test_passplan_host.py pins the plan of
every batch built here, at the borders the cases count on.
profiles/kernel_trace_instantiations.txt lists the kernels a run of the GPU suite launched.
"""
import os

import numpy as np
import pytest

from oracle import camera_ref, oracle as orc
from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, ZFAR, ZNEAR

import helpers

pytestmark = pytest.mark.gpu

# the near cameras of test_robot_partly_and_wholly_out_of_view (tests/test_gpu_fullsize.py) with the robot pose each looks at
NEAR = [([0.3, -0.12, 0.77, 0, 0.2, 0.3], [0, 0, 0, 0, 0, 0]), ([0.2, -0.1, 0.6, 0.3, 0.1, -0.4], [0.5, 0.4, 0.6, 0.2, 0.3, 0.1])]
# the one of those cameras that also sees the base link at the home pose, which the Predictor's crops are made from (crop.py)
NEAR_BASE = ([0.05, -0.12, 0.25, 0, -0.4, 0.1], [0, 0, 0, 0, 0, 0])
TWINS = ('NO_QUEUE', 'NO_LAYERS|NO_QUEUE', 'NO_LAYERS', 'again')


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def cut_triangles(o, q, n=6) -> int:
    """Triangles of pose q with vertices on both sides of the near plane under o.PV (z < -w in clip space, the oracle's own test,
    rope_oracle.c shade_vertex) — the ones a renderer has to cut."""
    mvp = o.mvp(q, n).astype(np.float64).reshape(n, 4, 4)
    verts = o.verts.reshape(-1, 3).astype(np.float64)
    faces = o.faces.reshape(-1, 3)
    cut = 0
    for l in range(n):
        v = verts[o.vtx_off[l]:o.vtx_off[l + 1]]
        clip = v @ mvp[l, :, :3].T + mvp[l, :, 3]
        behind = clip[:, 2] < -clip[:, 3]
        nb = behind[faces[o.tri_off[l]:o.tri_off[l + 1]]].sum(axis=1)
        cut += int(((nb > 0) & (nb < 3)).sum())
    return cut


def beyond_reach(rb, PV) -> bool:
    """True when no vertex of the robot can get behind the near plane of PV whatever the joint angles: near_plane_in_reach of
    rope_abi.hip with a reach taken from whole links' boxes, which is no smaller than the engine's (from meshlet boxes) — so
    True here means the engine chooses the plain kernels for this camera."""
    jf = np.asarray(rb.joint_fixed, np.float64).reshape(-1, 12)
    verts = np.asarray(rb.verts, np.float64).reshape(-1, 3)
    reach = chain = 0.0
    for l in range(len(rb.vtx_off) - 1):
        if l > 0:
            chain += float(np.sqrt(jf[l - 1, 3] ** 2 + jf[l - 1, 7] ** 2 + jf[l - 1, 11] ** 2))
        v = verts[rb.vtx_off[l]:rb.vtx_off[l + 1]]
        reach = max(reach, chain + float(np.sqrt((np.abs(v).max(axis=0) ** 2).sum())))
    PV = np.asarray(PV, np.float64).reshape(4, 4)
    g, h = PV[2, :3] + PV[3, :3], PV[2, 3] + PV[3, 3]
    return bool(h - np.sqrt((g * g).sum()) * (reach + 0.01) > 0.0)


def twins(e, run, same, flags=TWINS):
    """run() under strategy 0, then under each of `flags` (the last: strategy 0 again); same(base, other, what) asserts.  With
    ROPE_KEEP_ARRAYS=<directory> in the environment, a pair that differs is written there before the test fails."""
    base = run()
    for name in flags:
        flag = 0 if name == 'again' else sum(getattr(e, n) for n in name.split('|'))
        e.set_strategy(flag)
        try:
            other = run()
        finally:
            e.set_strategy(0)
        try:
            same(base, other, name)
        except AssertionError:                           # a spilled kernel against its twin: keep both results to look at
            keep = os.environ.get('ROPE_KEEP_ARRAYS')
            if keep:
                arrays = {}
                for which, result in (('base', base), ('other', other)):
                    for i, x in enumerate(result if isinstance(result, tuple) else (result,)):
                        if x is not None:
                            arrays[f'{which}{i}'] = np.asarray(x)
                case = os.environ.get('PYTEST_CURRENT_TEST', 'case').split('::')[-1].split(' ')[0]
                np.savez(os.path.join(keep, f"mismatch_{case}_{name.replace('|', '+')}.npz"), **arrays)
            raise
    return base


def shared_grid(q0, pairs, per_pair, rng, spread=.25):
    """`pairs` (S, L) pairs about q0, `per_pair` values of U under each: rows that share their first two joint angles -> layers"""
    q0 = np.asarray(q0, float)
    sl = q0[:2] + rng.uniform(-spread, spread, (pairs, 2))
    cand = np.zeros((pairs * per_pair, 6))
    cand[:, :2] = np.repeat(sl, per_pair, axis=0)
    cand[:, 2] = np.tile(q0[2] + np.linspace(-.4, .4, per_pair), pairs)
    cand[:, 3:] = q0[3:]
    return cand


def single_scene(pose, q0, ds=2):
    """Engine and oracle at 640x480 / ds under camera `pose`, the target rendered at q0 by the oracle."""
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=ds, pose=pose)
    e = eng.Engine(0)
    e.set_robot(rb)
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    o = helpers.make_oracle(rb, intr, PV)
    d_ref, id_ref = o.render(q0, 6)
    tq, t32, flags, tgt, _, _ = helpers.synthetic_target(d_ref, id_ref)
    full32 = np.ascontiguousarray(tgt, np.float32)
    e.set_target(tq, t32, flags)
    e.set_target_tsweep(full32)
    H, W = intr.height, intr.width
    crop = [int(H * .15), int(H * .9), int(W * .1), int(W * .95)]
    return dict(rb=rb, e=e, o=o, PV=PV, intr=intr, tq=tq, t32=t32, flags=flags, full32=full32, crop=crop)


# ---------------------------------------------------------------- rope_eval_views: CAMFULL and TSWEEP, far / near / mixed cameras
VIEW_FRAMES = 4


@pytest.fixture(scope='module')
def views_scene():
    """160x120 (four tiles, busy_tiles 2).  Four frames of the robot about NEAR[0]'s pose, as seen from a far and from the near
    camera; trial cameras about both."""
    rb = helpers.robot()
    intr, PV0 = helpers.camera('640_480_color', ds=4)
    o = helpers.make_oracle(rb, intr, PV0)
    P = intr.gl_projection(ZNEAR, ZFAR)
    rng = np.random.default_rng(77)
    near_pose, q0 = np.array(NEAR[0][0], float), np.array(NEAR[0][1], float)
    far_pose = np.array(DEFAULT_CAMERA_POSE, float) + np.array([.06, -.05, .04, .01, -.015, .02])
    qs = q0 + rng.uniform(-.15, .15, (VIEW_FRAMES, 6))
    names = rb.link_names[:6]
    refs = {}
    for kind, true_pose in (('far', far_pose), ('near', near_pose)):
        o.PV = np.ascontiguousarray(P @ camera_ref.view_of_pose(true_pose))
        frames = [o.render(q, 6) for q in qs]
        tgt = np.stack([d for d, _ in frames]).astype(np.float64)
        seg = [{n: {'mask': frames[i][1] == l} for l, n in enumerate(names) if (frames[i][1] == l).any()} for i in range(VIEW_FRAMES)]
        refs[kind] = (camera_ref.CameraReference(o, P, 'segmented', qs, tgt, seg, names), tgt)
    e = eng.Engine(0)
    e.set_robot(rb)
    e.set_camera(PV0, intr.width, intr.height, ZNEAR, ZFAR)
    far_views = far_pose + rng.uniform(-1, 1, (260, 6)) * np.array([.08, .08, .08, .05, .05, .05])      # all beyond the robot's reach
    near_views = near_pose + rng.uniform(-1, 1, (260, 6)) * np.array([.02, .02, .02, .05, .05, .05])
    return dict(rb=rb, o=o, P=P, e=e, qs=qs, refs=refs, far=far_views, near=near_views)


@pytest.mark.parametrize('loss', [eng.LOSS_CAMFULL, eng.LOSS_TSWEEP])
@pytest.mark.parametrize('cams,K', [
    ('far', 260),      # 1040 rows, rule Q, no camera in reach: raster_queue_kernel<LOSS, SCORE, plain>; twin raster_score_kernel<LOSS, SCORE, plain>
    ('near', 260),     # 1040 rows, rules Q + C: raster_queue_kernel<LOSS, SCORE, CLIP>; twin raster_score_kernel<LOSS, SCORE, CLIP>
    ('near', 12),      # 48 rows, rules S + C: raster_score_kernel<DEPTH, SPLIT, CLIP> + score_gtile_kernel<LOSS>
    ('mixed', 12),     # 48 rows, one near camera among eleven far ones: clip_views holds for the whole call (rules S + C)
    ('mixed', 260),    # 1040 rows, one near camera among 259 far ones: rules Q + C
])
def test_eval_views(views_scene, cams, K, loss):
    s = views_scene
    e, o, P, rb = s['e'], s['o'], s['P'], s['rb']
    ref, tgt = s['refs']['near' if cams == 'near' else 'far']
    N = VIEW_FRAMES
    e.set_frames(s['qs'], np.stack([eng.pack_target(d) for d in tgt]), tgt.astype(np.float32), np.tile(ref.planes[None], (N, 1, 1, 1)))
    poses = s['near' if cams == 'near' else 'far'][:K].copy()
    near_idx = list(range(K)) if cams == 'near' else []
    if cams == 'mixed':
        poses[1] = s['near'][0]
        near_idx = [1]
    PV = np.stack([P @ camera_ref.view_of_pose(p) for p in poses])
    far_idx = [k for k in range(K) if k not in near_idx]
    assert all(beyond_reach(rb, PV[k]) for k in far_idx), "a far camera within the robot's reach of the near plane"
    sample = sorted({0, 1, K - 1})                       # three views x four frames = twelve rows for the oracle
    for k in sample:
        o.PV = np.ascontiguousarray(PV[k])
        cut = sum(cut_triangles(o, q) for q in s['qs'])
        assert (cut > 0) == (k in near_idx), f"view {k}: {cut} triangles cross the near plane"
    assert K * N > 1024 or K * N <= 256                  # rule Q or rule S, as the case says

    def same(a, b, what):
        assert np.array_equal(a, b), f"sums differ from strategy 0 under {what}"
    got = twins(e, lambda: e.eval_views(PV, 6, loss), same, ('NO_QUEUE', 'NO_LAYERS|NO_QUEUE', 'again'))
    assert got.shape == (K, N, 23)
    for k in sample:
        want = ref.frame_sums(poses[k], 'full' if loss == eng.LOSS_CAMFULL else 'sweep')
        if loss == eng.LOSS_CAMFULL:
            assert np.array_equal(got[k], want), f"CAMFULL sums of view {k} differ from the oracle's"
        else:
            assert np.array_equal(got[k][:, :5], want[:, :5]), f"sweep sums of view {k} differ from the oracle's"
    if cams == 'mixed':                                  # the far views through the CLIP kernels == the same views through the plain ones
        alone = e.eval_views(PV[far_idx], 6, loss)
        assert np.array_equal(got[far_idx], alone), "far views scored beside a near one differ from the far views alone"


# ---------------------------------------------------------------- rope_eval: LOOKUP with a crop and TSWEEP under a far camera
@pytest.fixture(scope='module')
def far_scene():
    return single_scene(DEFAULT_CAMERA_POSE, [0.4, 0.3, 0.8, 0, 0, 0])


@pytest.mark.parametrize('loss', [eng.LOSS_LOOKUP, eng.LOSS_TSWEEP])
def test_eval_far_queue_and_layer_queue(far_scene, loss):
    """768 rows under 64 (S, L) pairs at 320x240: layers engaged (256 <= 768), rules Q and L -> raster_queue_kernel<LOSS, LAYER,
    plain> then raster_queue_kernel<LOSS, SCORE, plain>.  NO_QUEUE: raster_score_kernel<LOSS, LAYER / SCORE, plain>; NO_LAYERS |
    NO_QUEUE: raster_score_kernel<LOSS, SCORE, plain> drawing all six links (768 x 3 > 2048: no split); NO_LAYERS: the queue alone."""
    s = far_scene
    e, o = s['e'], s['o']
    assert beyond_reach(s['rb'], s['PV'])
    rng = np.random.default_rng(43)
    cand = shared_grid([0.4, 0.3, 0.8, 0, 0, 0], 64, 12, rng)
    cr = s['crop'] if loss == eng.LOSS_LOOKUP else None

    def same(a, b, what):
        assert np.array_equal(a[1], b[1]), f"sums differ from strategy 0 under {what}"
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[2] == b[2], f"errors or argmin differ from strategy 0 under {what}"
    err, sums, bi, _ = twins(e, lambda: e.eval(cand, 6, loss, crop=cr, want_sums=True), same)
    pick = np.sort(rng.choice(len(cand), 10, replace=False))
    t_plane = s['full32'] if loss == eng.LOSS_TSWEEP else s['t32']
    err_ref, sums_ref = o.eval(cand[pick], loss, 6, s['tq'], t_plane, cr, s['flags'], threads=8, want_sums=True)
    assert np.array_equal(sums[pick], sums_ref) and np.array_equal(_bits(err[pick]), _bits(err_ref))
    assert bi == int(np.nanargmin(err))


# ---------------------------------------------------------------- near cameras: a frame per row, the stored table, coverage
@pytest.fixture(scope='module', params=[0, 1])
def near_scene(request):
    pose, q0 = NEAR[request.param]
    s = single_scene(pose, q0)
    s['q0'] = np.array(q0, float)
    # three frames for rope_eval_targets: the robot at and about q0 under the same near camera
    rng = np.random.default_rng(51 + request.param)
    frames = []
    for f in range(3):
        q = s['q0'] + (0 if f == 0 else rng.uniform(-.2, .2, 6))
        d, ids = s['o'].render(q, 6)
        tq, t32, flags, tgt, _, _ = helpers.synthetic_target(d, ids)
        frames.append(dict(q=q, tq=tq, t32=t32, flags=flags, full=np.ascontiguousarray(tgt, np.float32)))
    s['frames'] = frames
    return s


@pytest.mark.parametrize('loss', [eng.LOSS_DEPTH, eng.LOSS_FULL, eng.LOSS_LOOKUP, eng.LOSS_TSWEEP])
def test_eval_targets_near(near_scene, loss):
    """864 rows over three frames' targets, 24 (S, L) pairs x 12 under each frame, at 320x240 under a near camera: layers inside
    every frame (288 <= 864), rules Q, L and C -> raster_queue_kernel<LOSS, LAYER, CLIP> and <LOSS, SCORE, CLIP> with a frame per
    row; the twins are raster_score_kernel<LOSS, LAYER / SCORE, CLIP>.  Errors only come back from rope_eval_targets: they must also
    be the bits rope_eval gives row by row with that frame as the one target, and the oracle's on ten rows."""
    s = near_scene
    e, o, frames = s['e'], s['o'], s['frames']
    rng = np.random.default_rng(61)
    B = len(frames)
    cand = np.concatenate([shared_grid(s['q0'], 24, 12, rng) for _ in range(B)])
    frame_of = np.repeat(np.arange(B), 24 * 12).astype(np.int32)
    perm = rng.permutation(len(cand))                    # frames interleaved
    cand, frame_of = cand[perm], frame_of[perm]
    cr = s['crop'] if loss == eng.LOSS_LOOKUP else None
    ts = loss == eng.LOSS_TSWEEP
    pick = np.sort(rng.choice(len(cand), 10, replace=False))
    assert sum(cut_triangles(o, q) for q in cand[pick]) > 0, "the near camera cuts no triangles of the sampled rows"
    e.set_targets(np.stack([f['tq'] for f in frames]), np.stack([f['t32'] for f in frames]), np.stack([f['flags'] for f in frames]),
                  np.stack([f['full'] for f in frames]) if ts else None)

    def same(a, b, what):
        assert np.array_equal(_bits(a), _bits(b)), f"errors differ from strategy 0 under {what}"
    got = twins(e, lambda: e.eval_targets(cand, frame_of, 6, loss, cr), same)
    for f, fr in enumerate(frames):
        sel = frame_of == f
        e.set_target(fr['tq'], fr['t32'], fr['flags'])
        e.set_target_tsweep(fr['full'] if ts else None)
        want = e.eval(cand[sel], 6, loss, crop=cr)[0]
        assert np.array_equal(_bits(got[sel]), _bits(want)), f"frame {f}: rows differ from rope_eval against that target"
        rows = pick[frame_of[pick] == f]
        if len(rows):
            ref = o.eval(cand[rows], loss, 6, fr['tq'], fr['full'] if ts else fr['t32'], cr, fr['flags'], threads=8)
            assert np.array_equal(_bits(got[rows]), _bits(ref)), f"frame {f}: rows differ from the oracle"
    e.set_target(s['tq'], s['t32'], s['flags'])          # the module's scene as the other tests expect it
    e.set_target_tsweep(s['full32'])


def test_stored_table_near(near_scene):
    """rope_lookup_build under a near camera: raster_score_kernel<LOOKUP, TABLE, CLIP> (launch_raster, whatever the strategy).
    768 rows under 64 (S, L) pairs; the stored table's scores == LOOKUP on the fly under strategy 0 (rules Q, L, C) and with
    neither layers nor queue == the oracle's on ten rows; built and scored a second time, the same bits."""
    s = near_scene
    e, o = s['e'], s['o']
    rng = np.random.default_rng(71)
    cand = shared_grid(s['q0'], 64, 12, rng)
    pick = np.sort(rng.choice(len(cand), 10, replace=False))
    assert sum(cut_triangles(o, q) for q in cand[pick]) > 0, "the near camera cuts no triangles of the sampled rows"
    crop = s['crop']
    e.lookup_build(cand, 6, crop)
    scores, bi, be = e.lookup_score(want_scores=True)

    def same(a, b, what):
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[2] == b[2] and a[3] == b[3], f"on-the-fly LOOKUP differs from strategy 0 under {what}"
    fly, _, bi_fly, be_fly = twins(e, lambda: e.eval(cand, 6, eng.LOSS_LOOKUP, crop=crop), same, ('NO_LAYERS|NO_QUEUE',))
    assert np.array_equal(_bits(scores), _bits(fly)) and bi == bi_fly and be == be_fly
    ref = o.eval(cand[pick], orc.LOSS_LOOKUP, 6, s['tq'], s['t32'], crop, s['flags'], threads=8)
    assert np.array_equal(_bits(scores[pick]), _bits(ref))
    e.lookup_build(cand, 6, crop)
    scores2, bi2, be2 = e.lookup_score(want_scores=True)
    assert np.array_equal(_bits(scores2), _bits(scores)) and bi2 == bi and be2 == be


def test_coverage_near(near_scene):
    """rope_coverage under a near camera: raster_score_kernel<DEPTH, COVER, CLIP> (launch_raster, whatever the strategy) against
    the oracle's drawn-pixel mask over the same 48 poses, four links and six."""
    s = near_scene
    e, o = s['e'], s['o']
    rng = np.random.default_rng(81)
    cand = shared_grid(s['q0'], 4, 12, rng)
    assert sum(cut_triangles(o, q) for q in cand[::5]) > 0, "the near camera cuts no triangles of the sampled rows"
    for n in (4, 6):
        cover = e.coverage(cand, n)
        want = o.coverage(cand, n, threads=8) != 0
        assert want.any() and np.array_equal(cover != 0, want), f"coverage of {n} links differs from the oracle's"
        assert np.array_equal(e.coverage(cand, n), cover)


@pytest.mark.parametrize('table', [True, False])
def test_predict_batch_near(table):
    """rope_predict_batch under a near camera (160x120): six frames in lockstep through the whole stage list — Lookup (the stored
    table, or LOOKUP on the fly with a frame per row), Descent (FULL / DEPTH rows of all frames in one launch) and TensorSweep —
    all through CLIP kernels; angles and per-stage traces equal rope_predict's on every frame."""
    from rope_s3d_amd import SyntheticPredictor
    pose, q0 = NEAR_BASE
    sp = SyntheticPredictor(pose, '640_480_color', 4, 'SLU', noise=False, seed=5, lookup_divisions=4)
    p = sp.predictor
    if not table:
        p.lookup_table_budget = 0
        p._loadLookup()
        assert not p._lookup_table
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=4, pose=pose, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    rng = np.random.default_rng(91)
    qs = np.array(q0, float) + rng.uniform(-.2, .2, (6, 6)) * np.array([1, 1, 1, 0, 0, 0])
    assert all(cut_triangles(o, q) > 0 for q in qs), "the near camera cuts no triangles of a frame's pose"
    colors, depths = [], []
    for q in qs:
        sp.renderer.setJointAngles(q)
        c, d = sp.renderer.render()
        colors.append(c)
        depths.append(d)
    got = p.run_batch([p.prepare(c, d) for c, d in zip(colors, depths)])
    traces = p.traces
    assert got.shape == (6, 6) and len(traces) == 6
    for i in range(6):
        one = p.run(colors[i], depths[i])
        assert np.array_equal(_bits(one), _bits(got[i])), f"frame {i}"
        for (k1, a1), (k2, a2) in zip(p.trace, traces[i]):
            assert k1 == k2 and np.array_equal(_bits(a1), _bits(a2)), f"frame {i} stage {k1}"
