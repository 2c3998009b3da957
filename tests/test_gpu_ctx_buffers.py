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
