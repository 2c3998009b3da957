"""GPU: the context's owned buffers (csrc/rope_buffers.h) through growth, reuse at a smaller size, reuse by another entry, the swap
of the staged and the resident targets, and creation and destruction — at 80x60 (four tiles), every result bit for bit what a
call the other suites already hold to their references gives."""
import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import ZFAR, ZNEAR

import helpers

pytestmark = pytest.mark.gpu

LABELS, PAD = [0, 1, 1, 2, 255, 3], 5


def _engine():
    intr, PV = helpers.camera('640_480_color', ds=8)
    e = eng.Engine(0)
    e.set_robot(helpers.robot())
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    return e


def _poses(n, seed, joints=3):
    lim = helpers.robot().joint_limits
    q = np.zeros((n, 6))
    q[:, :joints] = np.random.default_rng(seed).uniform(lim[:joints, 0], lim[:joints, 1], (n, joints))
    return q


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_render_planes_shared_across_entries_and_sizes():
    """render_batch, render_masks and render_batch_device in turn on one engine, the batch growing and shrinking: d_rids serves
    both kinds of entry, d_rdepth, d_rmask, d_rboxes and the staging block grow and are then used below their size."""
    e = _engine()
    assert (e.W, e.H) == (80, 60)
    q = _poses(21, 5)
    single = [e.render(r, 6) for r in q]
    assert any((i != 255).any() for _, i in single)

    def check(rows, depth, ids):
        for k, r in enumerate(rows):
            if depth is not None:
                assert _same(np.asarray(depth[k]), single[r][0]), r
            if ids is not None:
                assert _same(np.asarray(ids[k]), single[r][1]), r

    def fresh_masks(rows):
        f = _engine()
        out = f.render_masks(q[rows], 6, LABELS, PAD)
        f.close()
        return out

    rows = list(range(0, 3))
    check(rows, *e.render_batch(q[rows], 6))                                       # 1. depth and ids, 3 poses
    rows = list(range(3, 8))
    m, b = e.render_masks(q[rows], 6, LABELS, PAD)                                 # 2. masks, 5 poses
    want_m, want_b = fresh_masks(rows)
    assert _same(m, want_m) and _same(b, want_b) and m.any()
    rows = [8]
    check(rows, *e.render_batch(q[rows], 6, depth=False))                          # 3. ids only, 1 pose
    rows = list(range(9, 13))
    d, i = e.render_batch_device(q[rows], 6)                                       # 4. planes left on the device, 4 poses
    check(rows, d.cpu().numpy(), i.cpu().numpy())
    rows = list(range(13, 15))
    m, b = e.render_masks(q[rows], 6, LABELS, PAD)                                 # 5. masks, 2 poses
    want_m, want_b = fresh_masks(rows)
    assert _same(m, want_m) and _same(b, want_b)
    rows = list(range(15, 21))
    check(rows, *e.render_batch(q[rows], 6, ids=False))                            # 6. depth only, 6 poses


def test_staged_and_resident_targets_change_places_at_different_sizes():
    """Sets of 3, 1, 5 and 2 frames, with and without the TensorSweep planes: after every commit the resident set is the staged
    one, plane for plane, and rows score against it as they do on a fresh engine after rope_set_targets."""
    e = _engine()
    q = _poses(8, 9, joints=5)
    frames = []
    for r in q:
        depth, ids = e.render(r, 6)
        tq, t32, flags, tgt, _, _ = helpers.synthetic_target(depth, ids)
        frames.append((tq, t32, flags, np.ascontiguousarray(tgt, np.float32)))

    def planes(idx, ts):
        return (np.stack([frames[i][0] for i in idx]), np.stack([frames[i][1] for i in idx]), np.stack([frames[i][2] for i in idx]),
                np.stack([frames[i][3] for i in idx]) if ts else None)

    e.set_targets(*planes([0, 1, 2], False))
    for idx, ts in [([3], True), ([4, 5, 6, 7, 0], False), ([1, 2], True)]:
        tq, t32, flags, full = planes(idx, ts)
        e.stage_targets(tq, t32, flags, full)
        e.commit_targets()
        assert e.n_targets == len(idx)
        got_tq, got_t32, got_ts, got_flags = e.debug_targets(ts)
        assert _same(got_tq, tq) and _same(got_t32, t32) and _same(got_flags, flags)
        if ts:
            assert _same(got_ts, full)
        else:
            with pytest.raises(eng.EngineError):                                   # no such planes in this set
                e.debug_targets(True)
    cand = _poses(4, 10, joints=5)
    frame_of = np.array([0, 1, 1, 0], np.int32)
    fresh = _engine()
    fresh.set_targets(*planes([1, 2], True))
    for loss in (eng.LOSS_FULL, eng.LOSS_TSWEEP):
        got, want = e.eval_targets(cand, frame_of, 6, loss), fresh.eval_targets(cand, frame_of, 6, loss)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.isfinite(got).all(), loss


def test_per_candidate_group_regrows():
    """8 rows, then 300 (past the rows scored through mapped host memory, and past the first allocation of 64), then 8 again."""
    e = _engine()
    depth, ids = e.render(_poses(1, 3)[0], 6)
    tq, t32, flags, _, _, _ = helpers.synthetic_target(depth, ids)
    e.set_target(tq, t32, flags)
    for n, seed in [(8, 1), (300, 2), (8, 3)]:
        cand = _poses(n, seed, joints=5)
        fresh = _engine()
        fresh.set_target(tq, t32, flags)
        got, want = e.eval(cand, 6, eng.LOSS_FULL), fresh.eval(cand, 6, eng.LOSS_FULL)
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1:] == want[1:], n
        fresh.close()


def test_created_and_destroyed_contexts_give_their_memory_back():
    """Twenty engines made, used and closed: free device memory ends no lower than it started by more than ONE engine's footprint
    (the drop across making and using the first) — a buffer per context left behind would show twenty times over.  An engine is
    made, used and closed before the first reading, so that what the runtime keeps for itself after first use is in neither figure."""
    free = lambda: torch.cuda.mem_get_info(0)[0]                                    # noqa: E731
    q = _poses(2, 7)

    def use():
        e = _engine()
        e.render_batch(q, 6)
        return e

    warm = use()                                                                   # the runtime's own first-use allocations
    warm.close()
    torch.cuda.synchronize()
    before = free()
    first = use()
    footprint = before - free()
    first.close()
    for _ in range(19):
        use().close()
    torch.cuda.synchronize()
    lost = before - free()
    print(f'footprint {footprint} bytes, lost after 20 engines {lost} bytes')
    assert lost <= footprint
    e = use()
    d, i = e.render(q[0], 6)
    assert (i != 255).any() and d.max() > 0


def test_the_kinds_of_target_in_turn_on_one_context():
    """A single target, a resident set, camera-pose frames, two staged sets (the first without float32 planes) and the single
    target's TensorSweep plane, one after the other on ONE context: every answer is byte for byte what a fresh engine gives
    that has only ever seen that kind.  80x60, 64 candidates (a 4x4x4 grid), 3 target frames, 2 camera-pose frames x 2 views."""
    import re
    from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE
    rb = helpers.robot()
    intr, PV0 = helpers.camera('640_480_color', ds=8)

    def make():
        f = eng.Engine(0)
        f.set_robot(rb)
        f.set_camera(PV0, intr.width, intr.height, ZNEAR, ZFAR)
        return f

    def fresh(setup, *calls):
        f = make()
        setup(f)
        out = [call(f) for call in calls]
        f.close()
        return out

    def same(got, want):                                                            # arrays, scalars, None, or tuples of them
        if isinstance(got, tuple):
            return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
        if isinstance(got, np.ndarray):
            return _same(got, want)
        return got == want or (got != got and want != want)

    e = make()
    cand = helpers.slu_grid(rb.joint_limits, 4)
    grid = helpers.slu_grid(rb.joint_limits, 3)
    assert len(cand) == 64
    crop, frame_of = (8, 51, 12, 71), (np.arange(64) % 3).astype(np.int32)
    frames = []
    for r in _poses(6, 31, joints=5):
        depth, ids = e.render(r, 6)
        tq, t32, flags, tgt, _, _ = helpers.synthetic_target(depth, ids)
        full = np.ascontiguousarray(tgt, np.float32)
        frames.append((tq, t32, flags, np.where(full > 0, full + np.float32(0.125), np.float32(0)).astype(np.float32)))
    assert all((f[1] != f[3]).any() for f in frames)                                # the TensorSweep planes are planes of their own

    def planes(idx, t32=True, ts=False):
        return (np.stack([frames[i][0] for i in idx]), np.stack([frames[i][1] for i in idx]) if t32 else None,
                np.stack([frames[i][2] for i in idx]), np.stack([frames[i][3] for i in idx]) if ts else None)

    def ev(loss, cr=None):
        return lambda f: tuple(x for x in f.eval(cand, 6, loss, cr) if x is not None)   # errors, argmin, its error

    def evt(loss, cr=None):
        return lambda f: f.eval_targets(cand, frame_of, 6, loss, cr)

    def refused(call, message):
        with pytest.raises(eng.EngineError, match=re.escape(f'failed (-1): {message}')):
            call(e)

    tq0, t320, flags0, ts0 = frames[0]
    single = lambda f: f.set_target(tq0, t320, flags0)                              # noqa: E731
    # 1. the single target
    single(e)
    calls1 = [ev(eng.LOSS_FULL), ev(eng.LOSS_LOOKUP, crop), ev(eng.LOSS_TSWEEP)]
    want1 = fresh(single, *calls1)
    assert same(tuple(c(e) for c in calls1), tuple(want1)) and np.isfinite(want1[0][0]).all()
    # 2. a resident set with its float32 planes, and the stored table against it
    set2 = lambda f: f.set_targets(*planes([1, 2, 3]))                              # noqa: E731
    table = lambda f: (f.lookup_build(grid, 3, crop), f.lookup_score_targets(True))[1]   # noqa: E731
    calls2 = [evt(eng.LOSS_FULL), evt(eng.LOSS_LOOKUP, crop), evt(eng.LOSS_TSWEEP), table]
    set2(e)
    assert same(tuple(c(e) for c in calls2), tuple(fresh(set2, *calls2)))
    # 3. camera-pose frames in the same planes: the resident set is gone
    qs = _poses(2, 32, joints=5)
    views = np.stack([PV0, helpers.camera('640_480_color', ds=8, pose=np.array(DEFAULT_CAMERA_POSE, float) + .05)[1]])
    set3 = lambda f: f.set_frames(qs, *planes([4, 5])[:2])                          # noqa: E731
    calls3 = [lambda f: f.eval_views(views, 6, eng.LOSS_DEPTH), lambda f: f.eval_views(views, 6, eng.LOSS_TSWEEP)]
    set3(e)
    assert same(tuple(c(e) for c in calls3), tuple(fresh(set3, *calls3)))
    refused(evt(eng.LOSS_DEPTH), 'rope_eval_targets: no targets set (rope_set_targets)')
    # 4. a staged set WITHOUT float32 planes becomes the resident one: the planes of step 3 are still in the buffers, and not read
    def staged(idx, t32, ts):
        def setup(f):
            tq, a, flags, b = planes(idx, t32, ts)
            f.stage_targets(tq, a, flags, b)
            f.commit_targets()
        return setup
    staged([3, 0, 5], False, False)(e)
    refused(evt(eng.LOSS_LOOKUP, crop), "rope_eval_targets: this loss needs the targets' float32 planes")
    refused(evt(eng.LOSS_TSWEEP), 'rope_eval_targets: this loss needs float32 planes')
    assert same(evt(eng.LOSS_DEPTH)(e), fresh(lambda f: f.set_targets(*planes([3, 0, 5], False)), evt(eng.LOSS_DEPTH))[0])
    # 5. a staged set with both kinds of float32 plane: TensorSweep reads its own
    staged([2, 4, 1], True, True)(e)
    calls5 = [evt(eng.LOSS_LOOKUP, crop), evt(eng.LOSS_TSWEEP), evt(eng.LOSS_FULL)]
    got5 = tuple(c(e) for c in calls5)
    assert same(got5, tuple(fresh(lambda f: f.set_targets(*planes([2, 4, 1], True, True)), *calls5)))
    tq5, t325, flags5, ts5 = planes([2, 4, 1], True, True)
    as_t32, plain = (fresh(lambda f: f.set_targets(tq5, p, flags5), evt(eng.LOSS_TSWEEP))[0] for p in (ts5, t325))
    assert same(got5[1], as_t32) and not same(got5[1], plain)
    # 6. the single target's TensorSweep plane, which the next rope_set_target takes away again
    e.set_target_tsweep(ts0)
    with_ts = ev(eng.LOSS_TSWEEP)(e)
    assert same(with_ts, fresh(lambda f: (single(f), f.set_target_tsweep(ts0)), ev(eng.LOSS_TSWEEP))[0]) and not same(with_ts, want1[2])
    assert same(ev(eng.LOSS_LOOKUP, crop)(e), want1[1])                             # that plane is TensorSweep's alone
    single(e)
    assert same(ev(eng.LOSS_TSWEEP)(e), want1[2])
    # 7. the single target as in step 1: it never depended on the sets
    assert same(tuple(c(e) for c in calls1), tuple(want1))
    e.close()
