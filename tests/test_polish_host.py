"""CPU: the host side of the native polish (prediction/refinement.py: PoseRefiner(native=); prediction/predict.py:
Predictor(refine='native')) over a stub engine, as tests/test_silhouette_host.py does for the silhouette term — native=True goes
through Engine.refine_poses and nothing else, native=False never touches it, the Predictor builds the refiner its switch asks for,
and an empty batch asks the engine for nothing.  The tensors stay on the host: Tensor.to is patched to drop the device."""
import numpy as np
import pytest
import torch

from rope_s3d_amd.prediction import refinement as rf
from rope_s3d_amd.projection import Intrinsics


class StubEngine:
    """Records the calls.  The host loop's words make every trial cheaper than the last, so every step is accepted."""
    device, n_links = 0, 6

    def __init__(self, workspace=1 << 20):
        self.calls, self.workspace = [], workspace

    def render_batch_device(self, angles, n_links, PV):
        self.calls.append('render')
        return torch.zeros((len(angles), 6, 8)), torch.zeros((len(angles), 6, 8), dtype=torch.uint8)

    def pose_normal_equations(self, rd, ri, depth_t, joints, n_links, clip, intr):
        self.calls.append('equations')
        w = np.zeros((len(rd), 32))
        w[:, 0] = w[:, 2] = 40.0
        w[:, 1] = w[:, 3] = 40.0 * 1e-4 / (1 + self.calls.count('equations'))
        A = np.eye(6) * 50.0 + 1.0
        w[:, 10:31] = A[np.triu_indices(6)]
        w[:, 4:10] = 1e-3
        return w

    def refine_workspace(self, n):
        return self.workspace * n

    def refine_poses(self, q, depth_t, camera_pose, intr, active_mask, limits, clip, iterations, damping, want_words=False):
        N = len(q)
        self.calls.append(('refine_poses', N, tuple(depth_t.shape), active_mask, clip, iterations, damping))
        var = np.full((N, 6), np.nan)
        var[:, [j for j in range(6) if (active_mask >> j) & 1]] = 4e-6
        return dict(angles=np.asarray(q) + 1e-3, var=var, cost_before=np.full(N, 2e-4), cost_after=np.full(N, 1e-4),
                    steps=np.full(N, 3, np.int32), inliers=np.full(N, 40.0))


@pytest.fixture
def on_the_host(monkeypatch):
    real = torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, 'to', lambda self, *a, **k: real(self, *[x for x in a if not isinstance(x, torch.device)],
                                                                        **{n: v for n, v in k.items() if n != 'device'}))


def _intr():
    intr = Intrinsics('640_480_color')
    intr.downscale(4)
    return intr


POSE = np.array([.1, -1.4, .6, 0.0, 0.2, 1.5])
ANGLES = np.zeros((3, 6))
DEPTH = np.ones((3, 6, 8), np.float32)


def test_native_routes_to_refine_poses_and_nothing_else(on_the_host):
    e = StubEngine()
    r = rf.PoseRefiner(e, POSE, _intr(), 'SLU', iterations=4, damping=1e-2, native=True)
    assert r.native is True
    res = r.refine(ANGLES, DEPTH)
    assert e.calls == [('refine_poses', 3, (3, 6, 8), 0b111, 2 ** -5, 4, 1e-2)]
    assert isinstance(res, rf.RefineResult) and len(res) == 3
    assert np.array_equal(res.angles, ANGLES + 1e-3) and np.allclose(res.sigma[:, :3], 2e-3) and np.isnan(res.sigma[:, 3:]).all()
    assert res.steps_taken.dtype == np.int64 and (res.steps_taken == 3).all() and (res.inliers == 40.0).all()
    assert (res.cost_before == 2e-4).all() and (res.cost_after == 1e-4).all()
    # the joints of do_angles become the mask
    e2 = StubEngine()
    rf.PoseRefiner(e2, POSE, _intr(), 'SBT', native=True).refine(ANGLES, DEPTH)
    assert e2.calls[0][3] == 0b110001                      # S, B and T of 'SLURBT'


def test_native_cuts_the_frames_to_the_workspace_budget(on_the_host):
    e = StubEngine(workspace=rf.PoseRefiner.NATIVE_WORK_BYTES // 2)       # two frames a call
    res = rf.PoseRefiner(e, POSE, _intr(), 'SLU', native=True).refine(ANGLES, DEPTH)
    assert [c[1] for c in e.calls] == [2, 1] and len(res) == 3 and res.sigma.shape == (3, 6)


def test_default_never_touches_refine_poses(on_the_host):
    e = StubEngine()
    r = rf.PoseRefiner(e, POSE, _intr(), 'SLU', iterations=2)
    assert r.native is False
    res = r.refine(ANGLES, DEPTH)
    assert e.calls == ['render', 'equations'] * 3 and (res.steps_taken == 2).all()


def test_empty_batch_asks_the_engine_for_nothing(on_the_host):
    for native in (False, True):
        e = StubEngine()
        res = rf.PoseRefiner(e, POSE, _intr(), 'SLU', native=native).refine(np.zeros((0, 6)), np.zeros((0, 6, 8), np.float32))
        assert e.calls == [] and len(res) == 0 and res.sigma.shape == (0, 6) and res.steps_taken.dtype == np.int64


def test_predictor_switch_builds_the_refiner_it_asks_for(on_the_host):
    from rope_s3d_amd.prediction.predict import Predictor
    for bad in ('host', 'Native'):
        with pytest.raises(ValueError, match='refine'):
            Predictor(POSE, 4, refine=bad)
    for refine, native in ((True, False), ('native', True)):
        p = Predictor.__new__(Predictor)
        e = StubEngine()
        # what Predictor.__init__ sets before it touches the engine, and what _polish reads
        p.refine, p.refine_native, p.last_refinement, p._refiner = bool(refine), refine == 'native', None, None
        p.renderer, p.camera_pose, p.intrinsics, p.do_angles = e, POSE, _intr(), 'SLU'
        out = p._polish(ANGLES, DEPTH)
        assert p._refiner.native is native and out.shape == (3, 6) and len(p.last_refinement) == 3
        assert any(isinstance(c, tuple) and c[0] == 'refine_poses' for c in e.calls) is native
