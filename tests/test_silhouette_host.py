"""CPU: the host side of the silhouette term (prediction/refinement.py: BundleRefiner(silhouette=, radius=)) over a stub engine —
what it refuses, that silhouette=0 walks the old path and touches neither new call, and which calls silhouette > 0 makes.  The
tensors stay on the host: Tensor.to is patched to drop the device."""
import numpy as np
import pytest
import torch

from rope_s3d_amd.prediction import refinement as rf
from rope_s3d_amd.projection import Intrinsics


class StubEngine:
    """Records the calls; the words it hands back make every trial cheaper than the last, so every step is accepted."""
    device, n_links = 0, 6

    def __init__(self):
        self.calls = []

    def _words(self, N, count, cost):
        w = np.zeros((N, 96))
        w[:, 0], w[:, 2] = count, count
        w[:, 1] = w[:, 3] = cost * count
        A = np.zeros((12, 12))
        live = [0, 1, 2] + list(range(6, 12))
        A[np.ix_(live, live)] = np.eye(9) * 50.0 + 1.0
        w[:, 16:94] = A[np.triu_indices(12)]
        w[:, 4:16] = np.where(np.isin(np.arange(12), live), 1e-3, 0.0)
        return w

    def render_batch_device(self, angles, n_links, PV):
        self.calls.append('render')
        return torch.zeros((len(angles), 6, 8)), torch.zeros((len(angles), 6, 8), dtype=torch.uint8)

    def bundle_normal_equations(self, rd, ri, depth_t, axes, twists, n_links, clip, intr):
        self.calls.append('bundle')
        return self._words(len(rd), 40.0, 1e-4 / (1 + self.calls.count('bundle')))

    def mask_distance(self, mask_t, radius):
        self.calls.append(('mask_distance', mask_t.dtype, tuple(mask_t.shape), radius))
        return torch.zeros(mask_t.shape, dtype=torch.int32)

    def silhouette_normal_equations(self, rd, ri, sd2, axes, twists, n_links, radius, intr):
        self.calls.append('silhouette')
        return self._words(len(rd), 10.0, 9.0 / (1 + self.calls.count('silhouette')))


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
MASK = np.zeros((3, 6, 8), bool)


def test_arguments_are_checked():
    e, intr = StubEngine(), _intr()
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError):
            rf.BundleRefiner(e, intr, silhouette=1.0, radius=bad)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            rf.BundleRefiner(e, intr, silhouette=bad)
    r = rf.BundleRefiner(e, intr, silhouette=0.5, radius=16)
    assert r.silhouette == 0.5 and r.radius == 16
    r = rf.BundleRefiner(e, intr)
    assert r.silhouette == 0.0 and r.radius == 8
    with pytest.raises(ValueError, match='mask'):
        rf.BundleRefiner(e, intr, silhouette=1.0).refine(POSE, ANGLES, DEPTH)
    with pytest.raises(ValueError, match='mask'):
        rf.BundleRefiner(e, intr, silhouette=1.0).refine(POSE, ANGLES, None)
    assert e.calls == []


@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_without_the_term_the_old_path_runs_and_nothing_new_is_called(on_the_host, mode):
    e1, e2, intr = StubEngine(), StubEngine(), _intr()
    a = rf.BundleRefiner(e1, intr, joints=mode, iterations=3).refine(POSE, ANGLES, DEPTH)
    b = rf.BundleRefiner(e2, intr, joints=mode, iterations=3, silhouette=0.0, radius=3).refine(POSE, ANGLES, DEPTH, MASK)
    assert e1.calls == e2.calls == ['render', 'bundle'] * 4
    assert a.pose.tobytes() == b.pose.tobytes() and a.angles.tobytes() == b.angles.tobytes() and a.sigma_pose.tobytes() == b.sigma_pose.tobytes()
    assert a.steps_taken == b.steps_taken == 3 and a.cost_after == b.cost_after < a.cost_before
    assert np.isnan(b.cost_silhouette_before) and np.isnan(b.cost_silhouette_after) and b.inliers_silhouette == 0


@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_with_the_term_the_field_is_made_once_and_both_kernels_see_every_render(on_the_host, mode):
    e, intr = StubEngine(), _intr()
    res = rf.BundleRefiner(e, intr, joints=mode, iterations=2, silhouette=2.0, radius=5).refine(POSE, ANGLES, DEPTH, MASK.astype(np.uint8) * 255)
    assert e.calls[0] == ('mask_distance', torch.uint8, (3, 6, 8), 5)
    assert e.calls[1:] == ['render', 'bundle', 'silhouette'] * 3
    assert res.steps_taken == 2 and res.cost_silhouette_before == 9.0 / 2 and res.cost_silhouette_after == 9.0 / 4
    assert res.cost_before == 1e-4 / 2 and res.cost_after == 1e-4 / 4 and res.inliers == 120 and res.inliers_silhouette == 30
    assert np.isfinite(res.sigma_pose).all() and res.frame_cost.shape == (3,)
    # the outline alone
    e = StubEngine()
    res = rf.BundleRefiner(e, intr, joints=mode, iterations=2, silhouette=1.0).refine(POSE, ANGLES, None, torch.from_numpy(MASK))
    assert e.calls[0] == ('mask_distance', torch.uint8, (3, 6, 8), 8) and e.calls[1:] == ['render', 'silhouette'] * 3
    assert np.isnan(res.cost_before) and np.isnan(res.cost_after) and res.inliers == 0 and np.isnan(res.frame_cost).all()
    assert res.cost_silhouette_after < res.cost_silhouette_before and res.steps_taken == 2 and np.isfinite(res.sigma_pose).all()
    with pytest.raises(ValueError):
        rf.BundleRefiner(e, intr, silhouette=1.0).refine(POSE, ANGLES, DEPTH[:, :5], MASK)
    with pytest.raises(ValueError):
        rf.BundleRefiner(e, intr, silhouette=1.0).refine(POSE, ANGLES, DEPTH, MASK[:2])


def test_the_information_of_both_terms_adds_up():
    """One frame, one live camera column: sigma^-2 = A_d / s_d^2 + A_s / s_s^2 with each term's own s^2 = [3] / ([2] - 1)."""
    wd, ws = np.zeros((1, 96)), np.zeros((1, 96))
    wd[0, [2, 3]], ws[0, [2, 3]] = (101.0, 4.0), (11.0, 5.0)
    k = 16 + list(zip(*np.triu_indices(12))).index((6, 6))
    wd[0, k], ws[0, k] = 8.0, 3.0
    info = np.zeros((1, 96))
    info[0, k] = 8.0 / (4.0 / 100.0) + 3.0 / (5.0 / 10.0)
    info[0, 2], info[0, 3] = 2.0, 1.0
    _, sc = rf.schur_sigma(info, [], [0])
    assert abs(sc[0] - 1.0 / np.sqrt(200.0 + 6.0)) < 1e-15
