"""CPU: the plain restatements of the dataset verification (verify_ref.py) on hand cases with the answers written out, the host
side of rope_s3d_amd/data/verification.py against them, Verifier.remove on both storage forms, and — before the GPU test relies
on it — the flag rule on CPU renders of the end-to-end set (oracle renders, verify_ref sums)."""
import json
import os

import numpy as np
import pytest

from rope_s3d_amd import constants
from rope_s3d_amd.data import hdf5
from rope_s3d_amd.data import verification as ver
from rope_s3d_amd.data.dataset import Dataset, write_dataset

import verify_ref

from verify_ref import A, HAND_WORDS, TOL, U, hand_planes  # noqa: E402


def test_q_is_a_floor_and_exact():
    assert verify_ref.q(np.float32(1.0)) == 2 ** 32 and verify_ref.q(A) == 2 ** 27 + 16
    assert verify_ref.q(np.float32(15.5 * U)) == 15 and verify_ref.q(np.float32(0.0)) == 0
    assert verify_ref.q(verify_ref.LAST_BELOW_128) == 2 ** 39 - 2 ** 15


def test_hand_made_planes_give_the_words_written_out():
    got = verify_ref.frame_sums(*hand_planes(), 2, TOL)
    assert got.dtype == np.uint64 and got.shape == (1, 28) and got[0].tolist() == HAND_WORDS
    # the tolerance is a float32: the next one below 2^-5 (q = 2^27 - 8) leaves nothing close, A itself (q = 2^27 + 16) makes all close
    less, more = (verify_ref.frame_sums(*hand_planes(), 2, t)[0].tolist() for t in (np.float32(TOL - 2.0 ** -29), A))
    assert less[4:12] == [5, 3, 0, 3, 5, 2, 0, 0] and more[4:12] == [5, 3, 3, 0, 5, 2, 2, 0]
    assert less[:4] == more[:4] == HAND_WORDS[:4]
    table = ver.agreement_table(got, 2)
    assert table['both'].tolist() == [5] and table['valid'].tolist() == [7] and table['bad_ids'].tolist() == [1]
    assert table['mean_abs_diff'][0] == (5 * 2 ** 27 + 1) / 5 / 2 ** 32
    assert table['coverage'][0] == 0.5 and table['close'][0] == 0.6 and table['front'][0] == 0.2 and table['behind'][0] == 0.2
    assert table['links']['behind'][0].tolist() == [0.0, 0.5] and table['links']['coverage'][0].tolist() == [0.6, 0.4]


def test_blend_rounds_half_to_even_and_saturates():
    a = np.array([1, 3, 5, 255, 250, 2, 255, 0, 100], np.uint8)
    b = np.array([0, 0, 0, 255, 250, 2, 0, 255, 200], np.uint8)
    half = [0, 2, 2, 255, 250, 2, 128, 128, 150]                  # .5 -> 0, 1.5 -> 2, 2.5 -> 2, 127.5 -> 128
    assert verify_ref.add_weighted(a, .5, b, .5).tolist() == half == ver.blend(a, .5, b, .5).tolist()
    assert verify_ref.add_weighted(a, .5, b, .5, 10).tolist()[3:6] == [255, 255, 12] == ver.blend(a, .5, b, .5, 10).tolist()[3:6]
    assert verify_ref.add_weighted(a, .5, b, .5, -10).tolist()[:3] == [0, 0, 0] == ver.blend(a, .5, b, .5, -10).tolist()[:3]
    assert ver.blend(a, 1.5, b, 1.5).tolist()[3:5] == [255, 255]
    # the Verifier's own weights, in float32 as OpenCV holds them: 255 float32(.7) and 255 float32(.3) round to 178.5 and 76.5, ties that
    # go to the even 178 and 76 (float64 weights would give 178.49999.. -> 178 but 76.50000.. -> 77); 5 float32(.7) rounds to 3.5 -> 4
    al = constants.VERIFIER_ALPHA
    assert (al, constants.VERIFIER_SCALER, constants.VERIFIER_ROWS, constants.VERIFIER_COLUMNS, constants.THUMBNAIL_DS_FACTOR) == (.7, 1.5, 4, 4, 6)
    want = [1, 2, 4, 255, 250, 2, 178, 76, 130]
    assert verify_ref.add_weighted(a, al, b, 1 - al).tolist() == want == ver.blend(a, al, b, 1 - al, 0).tolist()
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, 256, (2, 9, 7, 3), dtype=np.uint8)
    assert np.array_equal(ver.blend(x, al, y, 1 - al), verify_ref.add_weighted(x, al, y, 1 - al))


def test_contact_sheets_fill_row_by_row():
    ov = np.arange(1, 19, dtype=np.uint8)[:, None, None, None] * np.ones((18, 2, 3, 3), np.uint8)
    sheets = ver.contact_sheets(ov)
    assert len(sheets) == 2 and sheets[0].shape == (4 * 2, 4 * 3, 3)
    assert sheets[0][::2, ::3, 0].tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]]
    assert sheets[1][::2, ::3, 0].tolist() == [[17, 18, 0, 0]] + [[0] * 4] * 3


def _sums_of(means_units, both=4):
    """Frames whose four `both` pixels (link 0) differ by means_units units each."""
    s = np.zeros((len(means_units), 28), np.uint64)
    s[:, 0] = s[:, 1] = s[:, 4] = s[:, 5] = both
    s[:, 2] = [both * int(m) for m in means_units]
    return s


def test_flag_rule_on_a_hand_checked_vector():
    # 1 2 3 4 100: Q1 = 2, Q3 = 4, IQR = 2, fence = 7 -> only 100 lies above it
    assert verify_ref.iqr_upper_fence(np.array([1.0, 2, 3, 4, 100])) == 7.0 == ver.upper_fence([1.0, 2, 3, 4, 100])
    # eight values: np.percentile interpolates: Q3 = 6.25, Q1 = 2.75 -> fence 11.5; 11 stays, 12 goes
    assert ver.upper_fence([1, 2, 3, 4, 5, 6, 7, 11]) == verify_ref.iqr_upper_fence(np.array([1, 2, 3, 4, 5, 6, 7, 11])) == 6.25 + 1.5 * 3.5
    s = _sums_of([2 ** 20, 2 * 2 ** 20, 3 * 2 ** 20, 4 * 2 ** 20, 100 * 2 ** 20, 0, 0])
    s[5, [0, 5]] = 0                                              # frame 5: rendered, nothing valid under the render -> flagged
    s[6, [1, 4, 5]] = 0                                           # frame 6: nothing rendered -> reported, not flagged
    table = ver.agreement_table(s, 6)
    flagged, unrendered = ver.flag_frames(table)
    assert flagged.tolist() == [4, 5] and unrendered.tolist() == [6]
    assert verify_ref.flagged(s, 6)[0].tolist() == [4, 5]
    assert np.array_equal(table['mean_abs_diff'][:5], np.array([1, 2, 3, 4, 100]) * 2.0 ** -12) and np.isnan(table['mean_abs_diff'][5:]).all()
    # all equal: IQR 0, the fence is the value itself, nothing lies above it
    assert ver.flag_frames(ver.agreement_table(_sums_of([7] * 6), 6))[0].tolist() == []
    assert ver.flag_frames(ver.agreement_table(_sums_of([0] * 9 + [1]), 6))[0].tolist() == [9]


# ---------------------------------------------------------------------------------------------- remove
class NoEngine:
    """Stands where the DatasetRenderer would: remove() must not draw anything; it may let go of the renderer of a set it replaced."""

    def __init__(self, ds):
        self.ds, self.closed = ds, False

    def close(self):
        self.closed = True
        self.ds.close()

    def __getattr__(self, name):
        raise AssertionError(f"remove() reached for the renderer's {name}")


def _tiny_set(root, n=5):
    rng = np.random.default_rng(31)
    og = rng.integers(0, 256, (n, 6, 8, 3), dtype=np.uint8)
    arrays = dict(og=og, depth=rng.uniform(0.5, 2, (n, 6, 8)), angles=rng.uniform(-1, 1, (n, 6)), poses=rng.uniform(-1, 1, (n, 6)),
                  positions=rng.uniform(-1, 1, (n, 6, 3)), preview=og[:, ::2, ::2].copy())
    d = write_dataset(str(root / 'tiny'), og, arrays['depth'], arrays['angles'], arrays['poses'], '640_480_color', positions=arrays['positions'],
                      extra_attrs={'synthetic': True, 'color_dict': {'base': [0, 0, 255]}, 'note': 'kept'}, preview=arrays['preview'])
    return d, arrays


def _same_frames(ds, arrays, keep):
    for attr, key in (('og_img', 'og'), ('depthmaps', 'depth'), ('angles', 'angles'), ('camera_pose', 'poses'), ('positions', 'positions'),
                      ('preview_img', 'preview')):
        got = np.asarray(getattr(ds, attr)[:])
        assert got.dtype == arrays[key].dtype and np.array_equal(got, arrays[key][keep]), attr


def test_remove_on_a_npy_set(tmp_path):
    d, arrays = _tiny_set(tmp_path)
    before = {fn: open(os.path.join(d, fn), 'rb').read() for fn in sorted(os.listdir(d))}
    ds = Dataset(d)
    v = ver.Verifier(ds, ds_renderer=NoEngine(ds))
    out = v.remove([3, 1, 3])
    assert out == d + '_verified' and sorted(os.listdir(out)) == sorted(before)
    new = Dataset(out)
    assert new.length == len(new) == 3 and new.file is None
    _same_frames(new, arrays, [0, 2, 4])
    assert new.attrs == dict(ds.attrs, length=3, name='tiny_verified')
    assert {fn: open(os.path.join(d, fn), 'rb').read() for fn in sorted(os.listdir(d))} == before      # the original is untouched
    assert v.ds is ds and ds.length == 5
    # another name; nothing removed is a copy; an index outside the set is refused
    other = v.remove([], name=str(tmp_path / 'copy'))
    _same_frames(Dataset(other), arrays, [0, 1, 2, 3, 4])
    with pytest.raises(IndexError):
        v.remove([5])
    with pytest.raises(ValueError):
        v.remove([0], inplace=True, name=str(tmp_path / 'x'))
    # in place is refused while the folder holds data made for the old numbering, and nothing is touched
    os.makedirs(os.path.join(d, 'link_annotations'))
    with pytest.raises(ValueError, match='link_annotations'):
        v.remove([0, 4], inplace=True)
    assert {fn: open(os.path.join(d, fn), 'rb').read() for fn in sorted(before)} == before and v.ds is ds and not os.path.exists(d + '.verifier_tmp')
    os.rmdir(os.path.join(d, 'link_annotations'))
    # in place: the same folder, the same name, the Verifier holds the new set
    assert v.remove([0, 4], inplace=True) == d
    assert sorted(os.listdir(d)) == sorted(before) and not os.path.exists(d + '.verifier_tmp')
    assert v.ds is not ds and v.ds.length == 3 and v.ds.attrs == dict(json.load(open(os.path.join(out, 'attrs.json'))), name='tiny')
    _same_frames(v.ds, arrays, [1, 2, 3])
    _same_frames(Dataset(d), arrays, [1, 2, 3])


@pytest.mark.skipif(not hdf5.available(), reason="no libhdf5 on this machine")
def test_remove_on_the_hand_made_h5_set(tmp_path):
    import shutil
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, 'golden'))
    import make_h5_by_hand as byhand
    og, depth, angles, positions, poses, preview = byhand.frames()
    arrays = dict(og=og, depth=depth, angles=angles, poses=poses, positions=positions, preview=preview)
    src = str(tmp_path / 'refset_by_hand')
    shutil.copytree(os.path.join(here, 'golden', 'refset_by_hand'), src)
    golden = open(os.path.join(src, 'refset_by_hand.h5'), 'rb').read()
    ds = Dataset(src)
    v = ver.Verifier(ds, ds_renderer=NoEngine(ds))
    out = v.remove([1])
    assert out == src + '_verified' and os.listdir(out) == ['refset_by_hand_verified.h5']
    new = Dataset(out)
    try:
        assert new.file is not None and new.length == 2
        _same_frames(new, arrays, [0, 2])
        for k, want in dict(byhand.ATTRS, length=2, name='refset_by_hand_verified').items():
            assert (list(new.attrs[k]) == list(want)) if k == 'resolution' else (new.attrs[k] == want), k
        assert new.intrinsics == byhand.ATTRS['color_intrinsics']
    finally:
        new.close()
    assert open(os.path.join(src, 'refset_by_hand.h5'), 'rb').read() == golden
    assert v.remove([0, 2], inplace=True) == src and os.listdir(src) == ['refset_by_hand.h5']
    try:
        assert v.ds.length == 1 and v.ds.attrs['name'] == 'refset_by_hand' and v.ds.file is not None
        _same_frames(v.ds, arrays, [1])
    finally:
        v.ds.close()


# ---------------------------------------------------------------------------------------------- the end-to-end input, on the CPU
def test_the_rule_flags_exactly_the_shifted_frames_on_cpu_renders():
    """What tests/test_gpu_verify.py relies on: with the recorded L angle of three frames moved by E2E_SHIFT_RAD = 0.3 rad, the
    sums of verify_ref on the oracle's renders flag those three and nothing else; every other frame differs from itself by 0."""
    import helpers
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', 4, as_predictor=True)      # through its string form, as a stored set's camera
    assert (intr.width, intr.height) == (160, 120)
    o = helpers.make_oracle(rb, intr, PV)
    true, recorded = verify_ref.e2e_angles(rb.joint_limits)
    T = np.stack([o.render(q, 6)[0] for q in true])
    renders = [o.render(q, 6) for q in recorded]
    sums = verify_ref.frame_sums(np.stack([d for d, _ in renders]), np.stack([i for _, i in renders]), T, 6, TOL)
    flagged, m = verify_ref.flagged(sums, 6)
    assert flagged.tolist() == list(verify_ref.E2E_SHIFTED) and verify_ref.E2E_SHIFT_RAD == 0.3
    rest = np.setdiff1d(np.arange(verify_ref.E2E_FRAMES), flagged)
    assert (m[rest] == 0).all() and (m[flagged] > 0.01).all() and (sums[:, 1] > 0).all()
    assert ver.flag_frames(ver.agreement_table(sums, 6))[0].tolist() == list(verify_ref.E2E_SHIFTED)
