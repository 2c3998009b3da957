"""GPU: the frame-agreement sums (rope_frame_agreement, csrc/rope_verify.hip; Engine.frame_agreement) against verify_ref.py, equal
word for word, at the smallest shapes where the kernel's cut of a frame into head, 16-byte body and tail takes every form and at
the smallest at which a workgroup's share of a frame runs through the unrolled body loop, the remainder loop and the hand-over
between them; then the Verifier end to end on a synthetic set in which three frames carry a wrong recorded pose."""
import ctypes as C

import numpy as np
import pytest
import torch

from rope_s3d_amd import engine as eng

import verify_ref
from verify_ref import HAND_WORDS, TOL, hand_planes

pytestmark = pytest.mark.gpu

E_ARG = -1
GARBAGE = 0x5A5A5A5A5A5A5A5A


def _device(a, offset_elems=0):
    """The array on the GPU, starting offset_elems elements into an allocation."""
    flat = torch.empty(a.size + offset_elems + 16, dtype=torch.from_numpy(a).dtype, device='cuda')
    view = flat[offset_elems:offset_elems + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return view.reshape(a.shape)


def _call(R, ids, T, n_links, tol, sums=None, offsets=(0, 0, 0), null=None, n_frames=None, hw=None):
    """The C entry point on a sums buffer filled with garbage (or the one given) -> (rc, sums as uint64, the buffer)."""
    N, H, W = R.shape
    tensors = [_device(a, o) for a, o in zip((R, ids, T), offsets)]
    if sums is None:
        sums = torch.full((N, 28), GARBAGE, dtype=torch.int64, device='cuda')
    ptrs = [C.c_void_p(t.data_ptr()) for t in tensors] + [C.c_void_p(sums.data_ptr())]
    if null is not None:
        ptrs[null] = None
    H, W = hw if hw is not None else (H, W)
    rc = eng.load_library().rope_frame_agreement(ptrs[0], ptrs[1], ptrs[2], N if n_frames is None else n_frames, H, W, n_links, tol, ptrs[3],
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, sums.cpu().numpy().view(np.uint64), sums


def _planes(rng, N, H, W, n_links):
    """Seeded planes built so that the tolerance is met exactly: R a multiple of 2^-20 in [0.5, 4), T = R + k 2^-5 for k in
    -2 .. 2 (|q(R) - q(T)| = q(tol) exactly for k = +-1), for a part of the pixels one float32 step further from or nearer to R;
    a tenth of T not valid (0, negative, NaN, inf, 128, 300); ids the links, the background, and a few of no link; a few render
    depths outside [0, 128) under links.  With three frames or more, frame 0 is all background and the last has T all zero."""
    R = (rng.integers(2 ** 19, 2 ** 22, (N, H, W)) * 2.0 ** -20).astype(np.float32)
    T = (R + rng.integers(-2, 3, R.shape) * np.float32(TOL)).astype(np.float32)
    step = rng.integers(0, 4, R.shape)
    T = np.where(step == 1, np.nextafter(T, np.float32(np.inf)), np.where(step == 2, np.nextafter(T, np.float32(-np.inf)), T)).astype(np.float32)
    bad = rng.random(R.shape) < 0.1
    T[bad] = rng.choice(np.array([0.0, -1.5, np.nan, np.inf, -np.inf, 128.0, 300.0], np.float32), int(bad.sum()))
    ids = rng.choice(np.array(list(range(n_links)) + [255, 255, 255], np.uint8), R.shape)
    odd = rng.random(R.shape) < 0.03
    ids[odd] = rng.integers(n_links, 255, int(odd.sum()), dtype=np.uint8)
    out = rng.random(R.shape) < 0.02
    R[out] = rng.choice(np.array([np.nan, -2.0, 128.0, 1e30, np.inf], np.float32), int(out.sum()))
    if N > 2:
        ids[0] = 255
        T[-1] = 0.0
    return R, ids, T


# N = 1 at 1 x 1: one tail pixel.  3 x 23 x 37: H W = 851 is odd, the float planes of frames 1 and 2 start 12 and 8 bytes
# past a 16-byte boundary: heads of 1 and 2 pixels, a body, tails (a head of 3 comes with the shifted allocations below).  2 x 16 x 64: all aligned, no head, no tail.  5 x 120 x 160: several workgroups a frame.
SHAPES = [(1, 1, 1), (3, 23, 37), (2, 16, 64), (5, 120, 160)]


@pytest.mark.parametrize('N,H,W', SHAPES)
@pytest.mark.parametrize('n_links', [1, 6])
def test_sums_equal_the_reference_word_for_word(N, H, W, n_links):
    R, ids, T = _planes(np.random.default_rng(1000 * H + W + n_links), N, H, W, n_links)
    want = verify_ref.frame_sums(R, ids, T, n_links, TOL)
    rc, got, buf = _call(R, ids, T, n_links, TOL)
    assert rc == 0 and got.shape == want.shape and np.array_equal(got, want), (N, H, W, n_links)
    if H * W > 1:
        per = want[:, 4:4 + 4 * n_links].reshape(N, n_links, 4).astype(np.int64)
        assert (per[:, :, 2] > 0).any() and (per[:, :, 3] > 0).any() and (per[:, :, 1] > per[:, :, 2] + per[:, :, 3]).any() and want[:, 3].any()
    if N > 2:
        assert want[0, 1] == 0 and want[0, 0] > 0 and want[-1, 0] == 0 and want[-1, 1] > 0
    # a second call into the same buffer: the same words, so the call zeroes them itself
    rc2, again, _ = _call(R, ids, T, n_links, TOL, sums=buf)
    assert rc2 == 0 and again.tobytes() == got.tobytes()


def test_a_workgroup_share_long_enough_for_both_body_loops():
    """The entry point cuts frames until a launch has about 2 048 workgroups, so a workgroup sees more than one pass of 256 quads
    only when there are many frames: 2 048 frames of 14 x 457 (6 398 pixels; frames start 0 and 8 bytes past a boundary in turn)
    give one workgroup a frame, 1 599 quads.  Every lane then takes the four-fold unrolled pass once (quads t, t + 256, t + 512,
    t + 768), hands over to the remainder loop at quad t + 1 024 and runs it twice, lanes 0-62 a third time."""
    N, H, W = 2048, 14, 457
    assert (H * W - 2) // 4 == 1599 and (2048 + N - 1) // N == 1
    R, ids, T = _planes(np.random.default_rng(2048), N, H, W, 6)
    rc, got, _ = _call(R, ids, T, 6, TOL)
    assert rc == 0 and np.array_equal(got, verify_ref.frame_sums(R, ids, T, 6, TOL))


def test_single_frame_all_background_and_all_unmeasured():
    R, ids, T = _planes(np.random.default_rng(3), 1, 23, 37, 6)
    for I2, T2 in ((np.full_like(ids, 255), T), (ids, np.zeros_like(T))):
        rc, got, _ = _call(R, I2, T2, 6, TOL)
        assert rc == 0 and np.array_equal(got, verify_ref.frame_sums(R, I2, T2, 6, TOL))
        assert got[0, 2] == 0 and not got[0, 5::4].any()


def test_the_hand_made_planes():
    rc, got, _ = _call(*hand_planes(), 2, TOL)
    assert rc == 0 and got[0].tolist() == HAND_WORDS


@pytest.mark.parametrize('offsets', [(1, 0, 1), (2, 3, 3), (3, 1, 0), (0, 2, 1)])
def test_planes_that_start_off_a_16_byte_boundary(offsets):
    """The three stacks begin 4, 8 or 12 bytes (ids: 1 to 3 bytes) past a boundary, the render and the recording differently."""
    R, ids, T = _planes(np.random.default_rng(50 + sum(offsets)), 3, 23, 37, 6)
    rc, got, _ = _call(R, ids, T, 6, TOL, offsets=offsets)
    assert rc == 0 and np.array_equal(got, verify_ref.frame_sums(R, ids, T, 6, TOL))


def test_other_tolerances():
    R, ids, T = _planes(np.random.default_rng(8), 2, 16, 64, 6)
    for tol in (0.0, 2.0 ** -6, 2.0 ** -4, float(np.float32(0.01)), 1000.0):
        rc, got, _ = _call(R, ids, T, 6, tol)
        assert rc == 0 and np.array_equal(got, verify_ref.frame_sums(R, ids, T, 6, tol)), tol


def test_argument_errors_return_their_code_without_a_launch():
    R, ids, T = _planes(np.random.default_rng(9), 2, 16, 64, 6)
    cases = [dict(n_frames=0), dict(n_frames=-1), dict(hw=(0, 64)), dict(hw=(16, 0)), dict(hw=(-1, -1)), dict(n_links=0), dict(n_links=7),
             dict(tol=-2.0 ** -5), dict(tol=float('nan')), dict(tol=float('inf')), dict(null=0), dict(null=1), dict(null=2), dict(null=3)]
    for case in cases:
        kw = dict(n_links=6, tol=TOL)
        kw.update(case)
        n_links, tol = kw.pop('n_links'), kw.pop('tol')
        rc, got, _ = _call(R, ids, T, n_links, tol, **kw)
        assert rc == E_ARG and (got == np.uint64(GARBAGE)).all(), case       # refused before anything was enqueued: the garbage is still there
    rc, got, _ = _call(R, ids, T, 6, TOL, hw=(4097, 4096))                   # more than 2^24 pixels a frame
    assert rc == E_ARG and (got == np.uint64(GARBAGE)).all()


def test_engine_frame_agreement_takes_tensors_and_refuses_others():
    R, ids, T = _planes(np.random.default_rng(10), 3, 23, 37, 6)
    e = eng.Engine(0)
    try:
        dR, dI, dT = (torch.from_numpy(a).cuda() for a in (R, ids, T))
        got = e.frame_agreement(dR, dI, dT, 6, TOL)
        assert got.dtype == np.uint64 and got.shape == (3, 28) and np.array_equal(got, verify_ref.frame_sums(R, ids, T, 6, TOL))
        assert e.frame_agreement(dR[:0], dI[:0], dT[:0], 6, TOL).shape == (0, 28)
        for bad in ((dR.double(), dI, dT), (dR, dI.int(), dT), (dR, dI, dT[:2]), (dR.cpu(), dI, dT), (dR[:, :, ::2], dI[:, :, ::2], dT[:, :, ::2])):
            with pytest.raises(ValueError):
                e.frame_agreement(*bad, 6, TOL)
        with pytest.raises(ValueError):
            e.frame_agreement(dR, dI, dT, 7, TOL)
        with pytest.raises(ValueError):
            e.frame_agreement(dR, dI, dT, 6, -1.0)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- the Verifier, end to end
@pytest.fixture(scope='module')
def shifted_set(tmp_path_factory):
    """make_synthetic_dataset at 160 x 120, no noise, E2E_FRAMES frames; then the recorded L angle of the frames E2E_SHIFTED moved by
    E2E_SHIFT_RAD = 0.3 rad (tests/test_verify_refs.py checks on CPU renders that the rule flags exactly those at that shift)."""
    from rope_s3d_amd.data.dataset import make_synthetic_dataset
    from rope_s3d_amd.projection import Intrinsics
    import os

    import helpers
    intr = Intrinsics('640_480_color')
    intr.downscale(4)
    d = make_synthetic_dataset(str(tmp_path_factory.mktemp('verify') / 'shifted'), verify_ref.E2E_FRAMES, base_intrin=str(intr), seed=verify_ref.E2E_SEED)
    true, recorded = verify_ref.e2e_angles(helpers.robot().joint_limits)
    assert np.array_equal(np.load(os.path.join(d, 'angles.npy')), true)
    np.save(os.path.join(d, 'angles.npy'), recorded)
    return d


def test_verifier_names_the_frames_with_a_wrong_pose(shifted_set, tmp_path):
    from rope_s3d_amd.data.dataset import Dataset
    from rope_s3d_amd.data.verification import Verifier
    v = Verifier(shifted_set)
    assert v.batch == 64 and v.tol == 2.0 ** -5
    table = v.run()
    shifted = list(verify_ref.E2E_SHIFTED)
    assert v.flagged().tolist() == shifted and v.unrendered().tolist() == []
    rest = np.setdiff1d(np.arange(verify_ref.E2E_FRAMES), shifted)
    assert table['mean_abs_diff'].shape == (24,) and (table['mean_abs_diff'][rest] == 0).all() and (table['close'][rest] == 1).all()
    assert (table['coverage'][rest] == 1).all() and (table['front'][rest] == 0).all() and (table['behind'][rest] == 0).all()
    assert (table['mean_abs_diff'][shifted] > 0).all() and (table['bad_ids'] == 0).all() and (table['rendered'] > 0).all()
    assert table['links']['close'].shape == (24, 6) and np.array_equal(table['links']['both'].sum(axis=1), table['both'])
    assert str(shifted) in v.summary()
    # the sums are those of the reference on the same renders and recordings
    ds = Dataset(shifted_set)
    depth_t, ids_t = v._renderer('seg').render_ids_batch_device(ds.angles[:], ds.camera_pose[:])
    want = verify_ref.frame_sums(depth_t.cpu().numpy(), ids_t.cpu().numpy(), np.asarray(ds.depthmaps[:], np.float32), 6, v.tol)
    assert np.array_equal(v.sums, want) and verify_ref.flagged(want, 6)[0].tolist() == shifted
    # groups of 5 (24 = 4 x 5 + 4): row for row the same
    five = Verifier(shifted_set, batch=5)
    five.run()
    assert five.sums.tobytes() == v.sums.tobytes() and five.flagged().tolist() == shifted
    five._rend.close()
    # contact sheets of the flagged frames, and the set without them
    paths = v.sheets(str(tmp_path / 'sheets'), v.flagged())
    h, w = v.thumbnail_size
    assert (h, w) == (30, 39) and len(paths) == 1 and open(paths[0], 'rb').read(8) == b'\x89PNG\r\n\x1a\n'
    ov = v.overlays(shifted)
    colours, _ = v._renderer('seg_full').render_indices(np.array(shifted))
    from rope_s3d_amd.imgproc import resize_linear
    assert np.array_equal(ov[1], verify_ref.add_weighted(resize_linear(np.asarray(ds.og_img[11]), w, h), .7, resize_linear(colours[1], w, h), 1 - .7))
    out = v.remove(v.flagged())
    clean = Verifier(out)
    clean.run()
    assert clean.ds.length == 21 and clean.flagged().tolist() == [] and (clean.table['mean_abs_diff'] == 0).all()
    assert np.array_equal(clean.sums, v.sums[rest])
    clean._rend.close()
    v._rend.close()
    ds.close()


def test_synthetic_names_and_the_caller(tmp_path, capsys):
    """'synthetic:<frames>' through Verifier and through verify.py: a set rendered as it is read agrees with itself; with the
    renderer's copy of one recorded L angle moved by 0.3 rad that frame is named; -remove is refused before anything runs."""
    import argparse
    import json

    import verify
    from rope_s3d_amd.data.dataset import SyntheticDataset
    from rope_s3d_amd.data.verification import Verifier
    from rope_s3d_amd.simulation.render import DatasetRenderer
    name = f'synthetic:6:{verify_ref.E2E_SEED}'
    args = argparse.Namespace(dataset=name, batch=4, tol=2.0 ** -5, sheets=str(tmp_path / 'sheets'), remove=False, json=str(tmp_path / 'table.json'))
    assert verify.verify(args).tolist() == []
    out = capsys.readouterr().out
    assert '6 frames, 6 scored' in out and 'flagged (0): []' in out
    table = json.load(open(args.json))
    assert table['flagged'] == [] and table['table']['mean_abs_diff'] == [0.0] * 6 and len(table['sums']) == 6 and len(table['sums'][0]) == 28
    with pytest.raises(SystemExit):
        verify.verify(argparse.Namespace(**dict(vars(args), remove=True)))
    ds = SyntheticDataset.from_name(name)
    rend = DatasetRenderer(ds, 'seg')
    rend._ds_angles = rend._ds_angles.copy()                             # a view of ds.angles, which the frames themselves are rendered from
    rend._ds_angles[2, 1] += verify_ref.E2E_SHIFT_RAD                    # the pose the frame is compared at, not the one it is rendered at
    v = Verifier(ds, batch=4, ds_renderer=rend)
    assert v.flagged().tolist() == [2] and (np.delete(v.table['mean_abs_diff'], 2) == 0).all()
    assert len(v.sheets(str(tmp_path / 'one'), v.flagged())) == 1
    with pytest.raises(ValueError):
        v.remove([2])                                                    # stored nowhere: it needs a name
    kept = Verifier(v.remove([2], name=str(tmp_path / 'kept')))
    assert kept.ds.length == 5 and kept.flagged().tolist() == []
    kept._rend.close()
    rend.close()
