"""GPU: the batched Predictor against the oracle's sequential restatement, decision by decision."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import predictor_ref
from rope_s3d_amd.constants import DEFAULT_CAMERA_POSE, LINK_BLUE
from rope_s3d_amd.crop import Crop, crop_pose_grid
from rope_s3d_amd.imgproc import resize_linear

import helpers

pytestmark = pytest.mark.gpu
THREADS = min(os.cpu_count() or 1, 16)


@pytest.fixture(scope='module')
def synth():
    from rope_s3d_amd import SyntheticPredictor
    # 640x480 frames, predicted at 160x120 (ds_factor 4), 4^3 lookup grid: small enough for the CPU oracle
    return SyntheticPredictor(DEFAULT_CAMERA_POSE, '640_480_color', 4, 'SLU', noise=False, seed=11, lookup_divisions=4)


def test_crop_matches_oracle(synth):
    p = synth.predictor
    rb = helpers.robot()
    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    crop = Crop(DEFAULT_CAMERA_POSE, intr, renderer=p.renderer, use_disk_cache=False)
    for n in (1, 4, 6):
        angles = np.zeros((1, 6)) if n == 1 else crop_pose_grid(rb.joint_limits, intr.size, n)[0]
        cover = o.coverage(angles, n, threads=THREADS) != 0
        r, c = np.where(cover)
        want = [max(r.min() - 10, 0), min(r.max() + 10, intr.height - 1), max(c.min() - 10, 0), min(c.max() + 10, intr.width - 1)]
        assert list(crop[n]) == want
    assert list(crop[0]) == list(crop[6])


@pytest.mark.parametrize('seed', [7919 + k for k in range(int(os.environ.get('ROPE_TRACE_SEEDS', '3')))])
def test_predictor_trace_matches_sequential_reference(synth, seed):
    p = synth.predictor
    rb = helpers.robot()
    lim = rb.joint_limits
    q_true = np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
    synth.renderer.setJointAngles(q_true)
    color, depth = synth.renderer.render()
    got = p.run(color, depth)

    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
    tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
    names = rb.link_names
    link_blue = {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}
    want, trace, n_eval = predictor_ref.predict_reference(
        o, tgt_depth, tgt_blue, names, link_blue, lim, DEFAULT_CAMERA_POSE,
        helpers.slu_grid(lim, 4), p.lookup_crop, 'SLU')
    assert len(trace) == len(p.trace)
    for (k_ref, a_ref), (k_got, a_got) in zip(trace, p.trace):
        assert np.array_equal(a_ref, a_got), f"stage {k_got}: {a_got} vs reference {a_ref}"
    assert np.array_equal(got, want)
    # the synthetic pose is recovered to within the descent's terminal resolution
    if seed < 7922:                                    # 4^3 lookup grid: coarse start, sanity bound on the standing seeds only
        assert np.abs(got - q_true)[:3].max() < 0.25


@pytest.mark.parametrize('fseed', [123 + 11 * k for k in range(int(os.environ.get('ROPE_TRACE_SEEDS', '1')))])
def test_segmentation_path_trace_matches_reference(synth, fseed):
    """Non-synthetic mode: a segmenter supplies instance masks (two per link here), Predictor._segmentLoad merges
    them, masks the depth with the dilate-8/erode-7 body and the stage machine runs on that target."""
    from rope_s3d_amd import Predictor
    from rope_s3d_amd.prediction.predict import segment_targets
    from rope_s3d_amd.segmentation import ColorSegmenter
    rb = helpers.robot()
    lim = rb.joint_limits
    names = ['BG'] + rb.link_names
    seg_fn = ColorSegmenter(names, split_instances=True)
    p = Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', segmenter=seg_fn, lookup_divisions=4)
    q_true = np.random.default_rng(fseed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
    synth.renderer.setJointAngles(q_true)
    color, depth = synth.renderer.render()
    depth_in = depth.astype(np.float64)
    got = p.run(color, depth_in)

    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    small = resize_linear(color, intr.width, intr.height)
    seg = Predictor._reorganize_by_link(p, seg_fn(small))
    tgt = resize_linear(depth.astype(np.float64), intr.width, intr.height)
    lookup = segment_targets(seg, tgt, rb.link_names)
    want, trace, _ = predictor_ref.predict_reference(
        o, tgt, None, rb.link_names, {}, lim, DEFAULT_CAMERA_POSE, helpers.slu_grid(lim, 4), p.lookup_crop, 'SLU',
        seg_masks={k: v['mask'] for k, v in seg.items()}, lookup_depth=lookup)
    for i, ((k_ref, a_ref), (k_got, a_got)) in enumerate(zip(trace, p.trace)):
        if not np.array_equal(a_ref, a_got):
            # what the two sides saw at the pose they parted at and at each other's answer: the engine's errors against the
            # current target, the oracle's against the target this test prepared
            rows = np.array([trace[i - 1][1] if i else a_ref, a_ref, a_got])
            from oracle import oracle as orc
            tq_ref = orc.pack_target(tgt, sum((np.asarray(seg[n]['mask'], np.uint64) << np.uint64(l)) for l, n in enumerate(rb.link_names) if n in seg))
            print("engine errors n=4:", p.engine.eval(rows, 4, 1)[0], " n=6:", p.engine.eval(rows, 6, 1)[0])
            print("oracle errors n=4:", o.eval(rows, 1, 4, tq_ref, link_flags=p._target.flags, threads=4), " n=6:", o.eval(rows, 1, 6, tq_ref, link_flags=p._target.flags, threads=4))
            print("target planes equal:", np.array_equal(tq_ref, p._target.tq), "flags", p._target.flags)
        assert np.array_equal(a_ref, a_got), f"stage {i} {k_got}: {a_got} vs reference {a_ref}"
    assert np.array_equal(got, want)
    if fseed == 123:
        assert np.abs(got - q_true)[:3].max() < 0.25


def test_predict_dataset_cli_end_to_end(tmp_path, monkeypatch):
    """make_synthetic_dataset -> Dataset -> predict_dataset.run (the reference's caller) -> predictions_<ds>.npy."""
    import argparse
    import importlib
    from rope_s3d_amd.data.dataset import Dataset, make_synthetic_dataset
    d = make_synthetic_dataset(str(tmp_path / 'synth4'), 4, base_intrin='640_480_color', seed=7919)
    ds = Dataset(d)
    assert ds.length == 4 and ds.og_img.shape == (4, 480, 640, 3) and ds.attrs['synthetic']
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('WORLD_SIZE', '1')
    pd = importlib.import_module('predict_dataset')
    full = pd.run(argparse.Namespace(dataset=d, angs='SLU', ds_factor=4))
    saved = np.load(tmp_path / 'predictions_synth4.npy')
    assert full.shape == (4, 6) and np.array_equal(saved, full)
    err = np.abs(full - np.asarray(ds.angles))[:, :3]
    assert err.max() < 0.3 and err.mean() < 0.08          # coarse default grid at 160x120; sanity only
    # frame 0 is the golden frame (seed 7919), but with the default lookup size rule instead of 4^3: same ballpark
    assert np.abs(full[0] - np.asarray(ds.angles)[0])[:3].max() < 0.1


def test_predict_dataset_two_ranks_shard_and_gather(tmp_path):
    """Two processes (gloo, both on GPU 0) predict halves of a 4-frame dataset; the gathered array equals a 1-rank run."""
    import socket
    import subprocess
    import sys
    from rope_s3d_amd.data.dataset import make_synthetic_dataset
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
    d = make_synthetic_dataset(str(tmp_path / 'synth4r'), 4, base_intrin='640_480_color', seed=8000)
    env = dict(os.environ, PYTHONPATH=root, ROPE_FORCE_DEVICE='0', ROPE_DIST_BACKEND='gloo', OMP_NUM_THREADS='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    one = subprocess.run([sys.executable, os.path.join(root, 'predict_dataset.py'), d, '-ds_factor', '4'],
                         cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stdout + one.stderr
    single = np.load(tmp_path / 'predictions_synth4r.npy')
    os.remove(tmp_path / 'predictions_synth4r.npy')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    two = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                          '--master-port', str(port), os.path.join(root, 'predict_dataset.py'), d, '-ds_factor', '4'],
                         cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert two.returncode == 0, two.stdout + two.stderr
    assert np.array_equal(np.load(tmp_path / 'predictions_synth4r.npy'), single)      # frames are independent: same bits


def test_tensor_sweep_stage_matches_reference(synth):
    """TensorSweep (predict.py:340-373) is in no default stage list; run it inside a custom list on both sides."""
    from rope_s3d_amd.prediction.stages import Descent, Lookup, SFlip, TensorSweep
    p = synth.predictor
    rb = helpers.robot()
    lim = rb.joint_limits
    q_true = np.random.default_rng(77).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
    synth.renderer.setJointAngles(q_true)
    color, depth = synth.renderer.render()
    stages = [Lookup(), TensorSweep(6, 12, 'U'), SFlip(4), TensorSweep(4, 9, 'SL', 0.2), Descent(6, 5, 'SLU', early_stop=.0075)]
    orig = p._setStages
    p._setStages = lambda: setattr(p, 'stages', stages)
    try:
        got = p.run(color, depth)
    finally:
        p._setStages = orig
    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
    tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
    names = rb.link_names
    link_blue = {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}
    ref_stages = [('lookup',), ('tsweep', 6, 12, 'U', None), ('sflip', 4), ('tsweep', 4, 9, 'SL', 0.2),
                  ('descent', 6, 5, 'SLU', [None] * 6, 0.5, 0.0075)]
    want, trace, _ = predictor_ref.predict_reference(o, tgt_depth, tgt_blue, names, link_blue, lim, DEFAULT_CAMERA_POSE,
                                                     helpers.slu_grid(lim, 4), p.lookup_crop, 'SLU', stages=ref_stages)
    assert len(trace) == len(p.trace)
    for (k_ref, a_ref), (k_got, a_got) in zip(trace, p.trace):
        assert np.array_equal(a_ref, a_got), f"stage {k_got}: {a_got} vs reference {a_ref}"
    assert np.array_equal(got, want)


@pytest.mark.parametrize('seed', [5, 6])
def test_sl_stage_list_trace_matches_reference(seed):
    """do_angles='SL' (stages.py:138-150): Lookup, SFlip, two interpolative sweeps, SFlip — and the 'SL' lookup grid."""
    from rope_s3d_amd import SyntheticPredictor
    sp = SyntheticPredictor(DEFAULT_CAMERA_POSE, '640_480_color', 4, 'SL', noise=False, seed=3, lookup_divisions=6)
    p = sp.predictor
    rb = helpers.robot()
    lim = rb.joint_limits
    q_true = np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 0, 0, 0, 0])
    sp.renderer.setJointAngles(q_true)
    color, depth = sp.renderer.render()
    got = p.run(color, depth)
    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
    tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
    names = rb.link_names
    link_blue = {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}
    want, trace, _ = predictor_ref.predict_reference(o, tgt_depth, tgt_blue, names, link_blue, lim, DEFAULT_CAMERA_POSE,
                                                     p.lookup_angles, p.lookup_crop, 'SL')
    assert [k for k, _ in trace] == ['lookup', 'sflip', 'isweep', 'isweep', 'sflip'] and len(trace) == len(p.trace)
    for (k_ref, a_ref), (k_got, a_got) in zip(trace, p.trace):
        assert np.array_equal(a_ref, a_got), f"stage {k_got}: {a_got} vs reference {a_ref}"
    assert np.array_equal(got, want)


def test_camera_pose_change_between_frames(synth):
    """run(..., camera_pose) with a new pose rebuilds crops and the lookup table (predict.py:105-117,127-130); the trace
    under the new camera matches the restatement, and going back to the first pose reproduces the first answer."""
    p = synth.predictor
    rb = helpers.robot()
    lim = rb.joint_limits
    q_true = np.random.default_rng(31).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
    synth.renderer.setCameraPose(DEFAULT_CAMERA_POSE)
    synth.renderer.setJointAngles(q_true)
    color0, depth0 = synth.renderer.render()
    first = p.run(color0, depth0, DEFAULT_CAMERA_POSE)
    pose = np.array([0.25, -1.4, 0.9, 0.0, -0.12, 0.2])
    synth.renderer.setCameraPose(pose)
    color, depth = synth.renderer.render()
    synth.renderer.setCameraPose(DEFAULT_CAMERA_POSE)
    got = p.run(color, depth, pose)
    assert np.array_equal(p.camera_pose, pose)
    intr, PV = helpers.camera('640_480_color', ds=4, pose=pose, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
    tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
    names = rb.link_names
    link_blue = {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}
    want, trace, _ = predictor_ref.predict_reference(o, tgt_depth, tgt_blue, names, link_blue, lim, pose,
                                                     helpers.slu_grid(lim, 4), p.lookup_crop, 'SLU')
    for (k_ref, a_ref), (k_got, a_got) in zip(trace, p.trace):
        assert np.array_equal(a_ref, a_got), f"stage {k_got}: {a_got} vs reference {a_ref}"
    assert np.array_equal(got, want)
    assert np.array_equal(p.run(color0, depth0, DEFAULT_CAMERA_POSE), first)


def test_synth_cli_with_noise_then_plot_errors(tmp_path, monkeypatch, capsys):
    """synth.py (render -> holes noise -> predict, partial saves) and plot_errors.py on its result file."""
    import argparse
    import importlib
    monkeypatch.chdir(tmp_path)
    sy = importlib.import_module('synth')
    sy.run(argparse.Namespace(dataset='none', num=5, file='synth_test', noise=True, ds_factor=8, angs='SLU', intrinsics='1280_720_color'))
    res = np.load(tmp_path / 'synth_test.npy')
    assert res.shape == (2, 5, 6) and np.isfinite(res).all()
    assert np.abs(res[1] - res[0])[:, :3].mean() < 0.25            # holes in the depth map: loose sanity bound
    pe = importlib.import_module('plot_errors')
    pe.run(argparse.Namespace(file=str(tmp_path / 'synth_test'), sort_by='S', angs='SLU', dataset=None))
    out = capsys.readouterr().out
    assert out.count('Err Stats (deg)') >= 2 and 'Err Stats (cm)' in out


def test_other_robot_as_active_urdf():
    """Paths.set('URDF', ...) switches the active robot (the reference edits data/paths.json): motoman mh50, camera
    pulled back, 1280x720 / 8 — the whole Predictor trace against the restatement built from the same URDF."""
    from rope_s3d_amd import SyntheticPredictor
    from rope_s3d_amd.config import Paths
    from rope_s3d_amd.urdf import URDFReader
    urdf = 'urdfs/motoman_mh50_support/urdf/mh50.urdf'
    old = Paths().URDF
    Paths().set('URDF', urdf)
    try:
        pose = [0, -4.0, 1.5, 0, 0, 0]
        sp = SyntheticPredictor(pose, '1280_720_color', 8, 'SLU', noise=False, seed=5, lookup_divisions=4)
        p = sp.predictor
        assert URDFReader().name == 'mh50' and p.renderer.robot.link_names[1] == URDFReader().mesh_names[1]
        rb = helpers.robot(urdf)
        lim = URDFReader().joint_limits
        q_true = np.random.default_rng(9).uniform(lim[:, 0] * .4, lim[:, 1] * .4) * np.array([1, 1, 1, 0, 0, 0])
        sp.renderer.setJointAngles(q_true)
        color, depth = sp.renderer.render()
        got = p.run(color, depth)
        intr, PV = helpers.camera('1280_720_color', ds=8, pose=pose, as_predictor=True)
        o = helpers.make_oracle(rb, intr, PV)
        tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
        tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
        names = rb.link_names
        link_blue = {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}
        want, trace, _ = predictor_ref.predict_reference(o, tgt_depth, tgt_blue, names, link_blue, lim, pose,
                                                         p.lookup_angles, p.lookup_crop, 'SLU')
        for (k_ref, a_ref), (k_got, a_got) in zip(trace, p.trace):
            assert np.array_equal(a_ref, a_got), f"stage {k_got}: {a_got} vs reference {a_ref}"
        assert np.array_equal(got, want)
    finally:
        Paths().set('URDF', old)


def test_preview_shows_the_reference_render_sequence(synth, tmp_path):
    """preview=True (ProjectionViz, predict.py:153-157,510-602): same angles as without it, one preview frame per
    pose the reference's serial loop renders, those poses in its order (the oracle's evaluations after the lookup),
    and a video file holding exactly those frames."""
    from rope_s3d_amd import Predictor
    p0 = synth.predictor
    rb = helpers.robot()
    lim = rb.joint_limits
    q_true = np.random.default_rng(7919).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
    synth.renderer.setJointAngles(q_true)
    color, depth = synth.renderer.render()
    want = p0.run(color, depth)

    video = tmp_path / 'preview.avi'
    p = Predictor(DEFAULT_CAMERA_POSE, 4, True, str(video), 'SLU', base_intrin='640_480_color',
                  color_dict=p0.color_dict, lookup_divisions=4)
    shown, parts = [], [None]
    set_parts, set_angles = p.renderer.setMaxParts, p.renderer.setJointAngles
    p.renderer.setMaxParts = lambda n: (parts.__setitem__(0, n), set_parts(n))[1]
    p.renderer.setJointAngles = lambda q: (shown.append((parts[0], np.array(q, float))), set_angles(q))[1]
    got = p.run(color, depth)
    assert np.array_equal(got, want)

    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
    tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
    names = rb.link_names
    evaluated = []
    _, _, n_eval = predictor_ref.predict_reference(
        o, tgt_depth, tgt_blue, names, {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}, lim, DEFAULT_CAMERA_POSE,
        helpers.slu_grid(lim, 4), p.lookup_crop, 'SLU', evaluated=evaluated)
    assert p.viz.shown == n_eval - len(p.lookup_angles)             # the lookup stage renders nothing per frame
    assert len(shown) == len(evaluated) == p.viz.shown
    for i, ((n_got, q_got), (n_ref, q_ref)) in enumerate(zip(shown, evaluated)):
        assert n_got == n_ref and np.array_equal(q_got, q_ref), (i, n_got, q_got, n_ref, q_ref)
    frame = p.viz.frame
    assert frame.shape == (720, 1280, 3) and frame[:360, 640:].any() and frame[360:, :640].any()
    p.viz.close()
    size = os.path.getsize(video)
    per_frame = 8 + 1280 * 720 * 3
    assert (size - p.viz.shown * per_frame) < 4096 and size > p.viz.shown * per_frame


@pytest.mark.parametrize('do_angles', ['SLU', 'SL'])
def test_native_stage_machine_matches_the_reference(do_angles):
    """rope_predict (the stage loop in librope_hip.so) against the sequential restatement of the reference on the same frames,
    with the reference's serial descent order and with the speculative batches: same angles after every stage.  Serially it
    evaluates exactly the reference's poses in its order (its on_eval log, with the lower-limit renders SFlip throws away put back
    as the preview does); the speculative batches evaluate those poses among others."""
    from rope_s3d_amd import SyntheticPredictor
    from rope_s3d_amd.prediction.predict import preview_rows
    from rope_s3d_amd.prediction.stages import SFlip
    sp = SyntheticPredictor(DEFAULT_CAMERA_POSE, '640_480_color', 4, do_angles, noise=False, seed=3, lookup_divisions=5)
    p = sp.predictor
    rb = helpers.robot()
    lim = rb.joint_limits
    names = rb.link_names
    link_blue = {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}
    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    log = []
    predict = p.engine.predict
    p.engine.predict = lambda *a, **k: predict(*a, **{**k, 'on_eval': lambda stage, n_render, rows: log.append((stage, n_render, rows))})
    try:
        for seed in range(int(os.environ.get('ROPE_NATIVE_SEEDS', '6'))):
            q = np.random.default_rng(1000 + seed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
            sp.renderer.setJointAngles(q)
            color, depth = sp.renderer.render()
            tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
            tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
            evaluated = []
            with np.errstate(all='ignore'):
                want, trace, n_eval = predictor_ref.predict_reference(o, tgt_depth, tgt_blue, names, link_blue, lim, DEFAULT_CAMERA_POSE,
                                                                      p.lookup_angles, p.lookup_crop, do_angles, evaluated=evaluated)
            runs = {}
            for spec in (3, 1):
                p.SPECULATE, p.evaluations = spec, 0
                log.clear()
                got = p.run(color, depth)
                assert len(trace) == len(p.trace)
                for k, ((k_ref, a_ref), (k_got, a_got)) in enumerate(zip(trace, p.trace)):
                    assert np.array_equal(a_ref, a_got), (seed, spec, k, k_got, a_got, a_ref)
                assert np.array_equal(got, want)
                runs[spec] = got, [(n, r) for stage, n, rows in log for r in rows], p.evaluations
                if spec == 1:
                    shown = [(n, r) for stage, n, rows in log for r in preview_rows(type(p.stages[stage]) is SFlip, rows, lim)]
                    assert len(shown) == len(evaluated) == n_eval - len(p.lookup_angles)
                    for i, ((n_got, q_got), (n_ref, q_ref)) in enumerate(zip(shown, evaluated)):
                        assert n_got == n_ref and np.array_equal(q_got, q_ref), (seed, i, n_got, q_got, n_ref, q_ref)
                    # evaluations: the reference's renders less the lower-limit ones SFlip throws away
                    assert p.evaluations == n_eval - (len(shown) - len(runs[1][1]))
            spec3 = {(n, r.tobytes()) for n, r in runs[3][1]}
            assert all((n, r.tobytes()) in spec3 for n, r in runs[1][1]), seed
            assert np.array_equal(runs[3][0], runs[1][0])
    finally:
        p.SPECULATE = 3
        del p.engine.predict


def test_native_stage_machine_argument_errors(synth):
    from rope_s3d_amd.engine import STAGE_ISWEEP, STAGE_LOOKUP, EngineError, StageDesc
    p = synth.predictor
    lim = helpers.robot().joint_limits
    bad = StageDesc(STAGE_ISWEEP, 6, 3, 4)                    # three divisions: no cubic through them
    with pytest.raises(EngineError, match='at least 4 divisions'):
        p.engine.predict([bad], lim, DEFAULT_CAMERA_POSE, p.min_ang_inc)
    with pytest.raises(EngineError, match='needs the pose grid'):
        p.engine.predict([StageDesc(STAGE_LOOKUP, 6)], lim, DEFAULT_CAMERA_POSE, p.min_ang_inc)
    with pytest.raises(EngineError, match='unknown stage kind'):
        p.engine.predict([StageDesc(9, 6)], lim, DEFAULT_CAMERA_POSE, p.min_ang_inc)


def test_run_many_prefetch_equals_frame_by_frame(synth):
    """Predictor.run_many prepares frame i+1 on a worker thread while frame i is on the GPU: same angles as a loop of
    run(), with and without the thread, on the colour path and on the segmenter path."""
    from rope_s3d_amd import Predictor
    from rope_s3d_amd.segmentation import ColorSegmenter
    p = synth.predictor
    lim = helpers.robot().joint_limits
    colors, depths = [], []
    for seed in range(5):
        q = np.random.default_rng(50 + seed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
        synth.renderer.setJointAngles(q)
        c, d = synth.renderer.render()
        colors.append(c); depths.append(d)
    want = np.array([p.run(c, d) for c, d in zip(colors, depths)])
    assert np.array_equal(p.run_many(colors, depths), want)
    assert np.array_equal(p.run_many(colors, depths, [DEFAULT_CAMERA_POSE] * 5, prefetch=False), want)
    assert p.run_many([], []).shape == (0, 6)
    seg = Predictor(DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', segmenter=ColorSegmenter(p.classes, split_instances=True),
                    lookup_divisions=4)
    want_seg = np.array([seg.run(c, d.astype(np.float64)) for c, d in zip(colors, depths)])
    assert np.array_equal(seg.run_many(colors, [d.astype(np.float64) for d in depths]), want_seg)


def test_predict_live_replay_monitors_deviation(tmp_path, monkeypatch, capsys):
    """predict_live.Live (predict_live.py:94-185) over a replayed dataset: predictions equal Predictor.run's, the
    (2, n, 6) log is saved every frame, and a controller that lies about its pose flips the state after LENGTH frames."""
    import importlib
    from rope_s3d_amd.data.dataset import Dataset, make_synthetic_dataset
    from rope_s3d_amd.prediction.feed import DatasetCamera
    d = make_synthetic_dataset(str(tmp_path / 'live5'), 5, base_intrin='640_480_color', seed=7919)
    ds = Dataset(d)
    monkeypatch.chdir(tmp_path)
    pl = importlib.import_module('predict_live')
    cam = DatasetCamera(ds)
    live = pl.Live(str(ds.intrinsics), ds, 'SLU', 4, camera=cam, link=cam.claims(), color_dict=ds.attrs['color_dict'], lookup_divisions=4)
    assert live.run() == 5
    live.stop()
    log = np.load(tmp_path / 'live_preds.npy')
    assert log.shape == (2, 5, 6) and np.array_equal(log[0], np.asarray(ds.angles))
    want = np.array([live.pred.run(np.copy(ds.og_img[i]), np.copy(ds.depthmaps[i])) for i in range(5)])
    assert np.array_equal(log[1], want)
    assert not live.state and 'in range' in capsys.readouterr().out

    class Lying:                                    # claims a pose a quarter turn of S away from the truth
        def __init__(self, inner): self.inner = inner
        def get_pose(self, timeout=None):
            q = self.inner.get_pose()
            return None if q is None else q + np.array([1.2, 0, 0, 0, 0, 0])
        def reset(self, timeout=None): pass
    cam = DatasetCamera(ds)
    live = pl.Live(str(ds.intrinsics), ds, 'SLU', 4, camera=cam, link=Lying(cam.claims()), save_to=None,
                   color_dict=ds.attrs['color_dict'], lookup_divisions=4)
    states = []
    while live.step():
        states.append(live.state)
    assert states == [False, False, True, True, True]


def test_predict_dataset_reads_the_reference_hdf5_form(tmp_path, monkeypatch):
    """The same frames as .npy directory and as the reference's <name>/<name>.h5 (gzip-chunked): same predictions."""
    import argparse
    import importlib
    from rope_s3d_amd.data import hdf5
    from rope_s3d_amd.data.dataset import Dataset, make_synthetic_dataset, write_h5_dataset
    if not hdf5.available():
        pytest.skip("no libhdf5 on this machine")
    d = make_synthetic_dataset(str(tmp_path / 'synth3'), 3, base_intrin='640_480_color', seed=7919)
    a = Dataset(d)
    h5 = write_h5_dataset(str(tmp_path / 'synth3h'), np.asarray(a.og_img), np.asarray(a.depthmaps), np.asarray(a.angles),
                          np.asarray(a.camera_pose), a.intrinsics, extra_attrs={'synthetic': True, 'color_dict': a.attrs['color_dict']})
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('WORLD_SIZE', '1')
    pd = importlib.import_module('predict_dataset')
    want = pd.run(argparse.Namespace(dataset=d, angs='SLU', ds_factor=4))
    got = pd.run(argparse.Namespace(dataset=os.path.dirname(h5), angs='SLU', ds_factor=4, predictors=2))      # and two Predictors on the GPU
    assert np.array_equal(got, want)
    assert np.array_equal(np.load(tmp_path / 'predictions_synth3h.npy'), want)


def test_predictor_pool_equals_one_predictor(synth):
    """PredictorPool: three Predictors on one GPU fed by three threads give, frame by frame, what one Predictor gives."""
    from rope_s3d_amd.prediction.pool import PredictorPool
    p = synth.predictor
    lim = helpers.robot().joint_limits
    colors, depths = [], []
    for seed in range(10):
        q = np.random.default_rng(80 + seed).uniform(lim[:, 0], lim[:, 1]) * np.array([1, 1, 1, 0, 0, 0])
        synth.renderer.setJointAngles(q)
        c, d = synth.renderer.render()
        colors.append(c); depths.append(d)
    want = np.array([p.run(c, d) for c, d in zip(colors, depths)])
    pool = PredictorPool(3, DEFAULT_CAMERA_POSE, 4, base_intrin='640_480_color', color_dict=p.color_dict, lookup_divisions=4)
    for _ in range(2):                                                  # twice: the contexts are reused across calls
        assert np.array_equal(pool.run_many(colors, depths, [DEFAULT_CAMERA_POSE] * 10), want)
    assert np.array_equal(pool.run_many(colors[:2], depths[:2]), want[:2]) and pool.run_many([], []).shape == (0, 6)
    assert pool.evaluations > 0 and len(pool) == 3
    # many Predictors on one GPU take the geometry launch of its own back (PredictorPool._tune): the same angles
    assert all(q.renderer.engine._strategy == 0 for q in pool.predictors)
    pool.THROUGHPUT_FROM = 2
    pool._tune()
    assert all(q.renderer.engine._strategy == q.renderer.engine.SEPARATE_GEOMETRY for q in pool.predictors)
    assert np.array_equal(pool.run_many(colors, depths), want)


def test_reference_table_aliasing_over_a_sequence(synth):
    """Predictor(reference_table_aliasing=True): the reference's drifting angle table (predict.py:171,212-215) over five
    frames of an arm that barely moves — stage by stage against the restatement that lets numpy do the aliasing; frame 1
    equals the default mode, later frames start from drifted rows."""
    from rope_s3d_amd import Predictor
    rb = helpers.robot()
    lim = rb.joint_limits
    names = rb.link_names
    link_blue = {n: int(LINK_BLUE[i]) for i, n in enumerate(names)}
    kw = dict(base_intrin='640_480_color', color_dict=synth.predictor.color_dict, lookup_divisions=4)
    p = Predictor(DEFAULT_CAMERA_POSE, 4, reference_table_aliasing=True, **kw)
    q = Predictor(DEFAULT_CAMERA_POSE, 4, **kw)                        # default: independent frames
    intr, PV = helpers.camera('640_480_color', ds=4, as_predictor=True)
    o = helpers.make_oracle(rb, intr, PV)
    grid = helpers.slu_grid(lim, 4)
    live = grid.copy()
    rng = np.random.default_rng(31)
    q0 = np.array([0.30, 0.25, 0.95, 0, 0, 0])
    differs = 0
    for f in range(5):
        q_true = q0 + rng.uniform(-.02, .02, 6) * np.array([1, 1, 1, 0, 0, 0])
        synth.renderer.setJointAngles(q_true)
        color, depth = synth.renderer.render()
        got = np.array(p.run(color, depth))
        tgt_depth = resize_linear(depth, intr.width, intr.height).astype(np.float64)
        tgt_blue = resize_linear(color, intr.width, intr.height)[..., 0]
        want, trace, _ = predictor_ref.predict_reference(o, tgt_depth, tgt_blue, names, link_blue, lim, DEFAULT_CAMERA_POSE, grid, p.lookup_crop,
                                                         'SLU', lookup_live=live)
        for (k_ref, a_ref), (k_got, a_got) in zip(trace, p.trace):
            assert np.array_equal(a_ref, a_got), f"frame {f} stage {k_got}: {a_got} vs reference {a_ref}"
        assert np.array_equal(got, np.array(want)) and np.array_equal(p._lookup_live, live), f
        ind = q.run(color, depth)
        if f == 0:
            assert np.array_equal(ind, got)
        elif not np.array_equal(q.trace[0][1], p.trace[0][1]):
            differs += 1
    assert differs >= 1 and (live != grid).any() and np.array_equal(p.lookup_angles, grid)
    # a new camera pose reloads the table (changeCameraPose -> _loadLookup, predict.py:105-117)
    p.changeCameraPose(np.array(DEFAULT_CAMERA_POSE) + [0.01, 0, 0, 0, 0, 0])
    assert np.array_equal(p._lookup_live, p.lookup_angles)


def test_renderer_modes_share_one_depth_image():
    """Renderer 'seg' / 'seg_full' / 'real' (render.py:100-105): the same depth; flat link colours, one colour, or the head-lit
    shading of mode 'real' (grey, zero on the background, brightest where the surface faces the camera)."""
    from rope_s3d_amd import Renderer
    from rope_s3d_amd.constants import DEFAULT_RENDER_COLORS
    r = Renderer('seg', DEFAULT_CAMERA_POSE, '640_480_color')
    r.setJointAngles([0.3, 0.4, 0.9, 0, 0, 0])
    col_seg, d_seg = r.render()
    r.setMode('seg_full')
    col_full, d_full = r.render()
    r.setMode('real')
    col_real, d_real = r.render()
    assert np.array_equal(d_seg, d_full) and np.array_equal(d_seg, d_real)
    on = d_seg > 0
    assert (col_full[on] == np.array(DEFAULT_RENDER_COLORS[0], np.uint8)).all() and len(np.unique(col_seg[on], axis=0)) > 3
    assert col_real.shape == col_seg.shape and col_real.dtype == np.uint8
    assert (col_real[~on] == 0).all() and (col_real[on, 0] > 0).all() and col_real.max() <= 200
    assert (col_real[..., 0] == col_real[..., 2]).all() and len(np.unique(col_real[on, 0])) > 20
    with pytest.raises(AssertionError):
        r.setMode('wireframe')
