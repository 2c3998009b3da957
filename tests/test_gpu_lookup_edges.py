"""The stored lookup table end to end through the engine at the crops its other tests never take (they all have cw % 4 == 1):
one crop per cw % 4, one column, one row, a corner no pose draws on (every row empty), the whole image and a crop some poses miss
— rope_lookup_build + rope_lookup_score against rope_eval(ROPE_LOSS_LOOKUP) and the oracle, bit for bit, with three rows that tie;
rope_lookup_score_targets at 1, 33 and 65 frames against rope_lookup_score frame by frame; and the table rebuilt at a smaller and
then a larger crop on one context.  tests/test_table_refs.py shows on the CPU that the crops are what they are named."""
import numpy as np
import pytest

from oracle import oracle as orc
from rope_s3d_amd import engine as eng
from rope_s3d_amd.constants import ZFAR, ZNEAR

import helpers
from table_ref import argmin, bits
from test_table_refs import ENGINE_CROPS, TARGET_ROW, engine_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def scene():
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=4)
    o = helpers.make_oracle(rb, intr, PV)
    e = eng.Engine(0)
    e.set_robot(rb)
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    cand = engine_rows(rb.joint_limits)
    d, ids = o.render(cand[TARGET_ROW])
    tq, _, flags, *_ = helpers.synthetic_target(d, ids)
    t32 = np.sqrt(d)                                    # the tying rows' own table row: they score 0 wherever they draw
    return rb, o, e, cand, tq, t32, flags


def frames_of(e, rb, n):
    """n targets of different poses -> (tq (n, H, W), t32 (n, H, W), flags (n, 8))."""
    lim = rb.joint_limits
    rng = np.random.default_rng(n)
    out = []
    for _ in range(n):
        depth, ids = e.render(rng.uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0.3, 0.3, 0]), 6)
        out.append(helpers.synthetic_target(depth, ids)[:3])
    return tuple(np.stack([f[k] for f in out]) for k in range(3))


@pytest.mark.parametrize('name', list(ENGINE_CROPS))
def test_lookup_build_and_score_at_the_crops_edges(scene, name):
    rb, o, e, cand, tq, t32, flags = scene
    crop = ENGINE_CROPS[name]
    e.set_target(tq, t32, flags)
    e.lookup_build(cand, 6, crop)
    scores, bi, be = e.lookup_score(want_scores=True)
    err_fly, _, bi_fly, be_fly = e.eval(cand, 6, eng.LOSS_LOOKUP, crop)
    ref = o.eval(cand, orc.LOSS_LOOKUP, 6, tq, t32, crop, flags, threads=8)
    assert np.array_equal(bits(scores), bits(ref)) and np.array_equal(bits(err_fly), bits(ref))
    first = argmin(ref)
    assert bi == bi_fly == first and bits(be) == bits(be_fly) == bits(ref[first])
    assert bits(ref[TARGET_ROW]) == bits(ref[27]) == bits(ref[28])
    if name == 'empty corner':
        assert len(set(bits(ref).tolist())) == 1 and first == 0
    else:
        assert first == TARGET_ROW and ref[TARGET_ROW] == 0.0              # the first of the three duplicates


@pytest.mark.parametrize('n', [1, 33, 65])
def test_lookup_score_targets_equals_per_frame_at_the_crops_edges(scene, n):
    rb, o, e, cand, *_ = scene
    tqs, t32s, flags = frames_of(e, rb, n)
    for name in ('cw%4==2', 'cw%4==3', 'cw%4==0', 'one column', 'some poses miss'):
        e.lookup_build(cand, 6, ENGINE_CROPS[name])
        e.set_targets(tqs, t32s, flags)
        scores, best, best_score = e.lookup_score_targets(want_scores=True)
        for f in range(n):
            e.set_target(tqs[f], t32s[f], flags[f])
            s1, b1, bs1 = e.lookup_score(want_scores=True)
            assert np.array_equal(bits(scores[f]), bits(s1)) and best[f] == b1 and bits(best_score[f]) == bits(bs1), (name, f)
        ref = o.eval(cand, orc.LOSS_LOOKUP, 6, tqs[n - 1], t32s[n - 1], ENGINE_CROPS[name], flags[n - 1], threads=8)
        assert np.array_equal(bits(scores[n - 1]), bits(ref)) and best[n - 1] == argmin(ref), name


def test_table_rebuilt_smaller_then_larger_on_one_context(scene):
    """The context's table, cropped-target and per-frame buffers only grow: a smaller table after a larger one leaves them longer
    than it needs, a larger one after that has them grown again."""
    rb, o, e0, cand, tq, t32, flags = scene
    intr, PV = helpers.camera('640_480_color', ds=4)
    e = eng.Engine(0)                                   # a context of its own: the order of growth is this test's
    e.set_robot(rb)
    e.set_camera(PV, intr.width, intr.height, ZNEAR, ZFAR)
    tqs, t32s, fl = frames_of(e, rb, 3)
    try:
        for name in ('cw%4==3', 'empty corner', 'one column', 'whole image', 'cw%4==2', 'one row', 'whole image'):
            crop = ENGINE_CROPS[name]
            e.lookup_build(cand, 6, crop)
            e.set_target(tq, t32, flags)
            scores, bi, _ = e.lookup_score(want_scores=True)
            ref = o.eval(cand, orc.LOSS_LOOKUP, 6, tq, t32, crop, flags, threads=8)
            assert np.array_equal(bits(scores), bits(ref)) and bi == argmin(ref), name
            e.set_targets(tqs, t32s, fl)
            many, best, _ = e.lookup_score_targets(want_scores=True)
            for f in range(3):
                ref_f = o.eval(cand, orc.LOSS_LOOKUP, 6, tqs[f], t32s[f], crop, fl[f], threads=8)
                assert np.array_equal(bits(many[f]), bits(ref_f)) and best[f] == argmin(ref_f), (name, f)
    finally:
        e.close()
