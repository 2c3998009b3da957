"""A continuous last step for a predicted pose, and how sure it is: Gauss-Newton on the depth residual.

Every stage of the Predictor is a search over discrete candidates, so its answer sits on the step lattice the last Descent ended
on, and it says nothing about which of the six angles the view pins down.  `PoseRefiner` polishes a batch of poses against their
depth frames: per round one batched render at the current angles, the joint axes at those angles in camera axes (the float64 FK
mirror, simulation/kinematics.py), one rope_pose_normal_equations call (csrc/rope_refine.hip: J^T J, J^T r and the residual sums
over all pixels, on the GPU) and, on the host, a Levenberg step per frame.  A step is kept only when the next round's cost is
strictly smaller, so a refined pose is never worse than its start under the refiner's own cost.  Inverting the final system
gives the formal covariance of the angles.

The reference has no such step (robotpose/prediction/predict.py ends with its last Descent)."""
from dataclasses import dataclass

import numpy as np

from ..constants import NUM_RENDER_LINKS
from ..projection import camera_pose_matrix
from ..simulation.kinematics import ForwardKinematics
from ..utils import str_to_arr

NEQ_WORDS = 32


@dataclass
class RefineResult:
    """What PoseRefiner.refine returns, one row per frame."""
    angles: np.ndarray          # (N, 6) the refined angles; joints outside do_angles as they came
    sigma: np.ndarray           # (N, 6) formal standard deviation, rad: inf = the view does not pin the joint down, nan = not refined
    cost_before: np.ndarray     # (N,) mean truncated squared residual at the start, m^2 (inf: nothing to compare)
    cost_after: np.ndarray      # (N,) the same at the refined pose; never larger than cost_before
    steps_taken: np.ndarray     # (N,) accepted steps, 0 .. iterations
    inliers: np.ndarray         # (N,) pixels that carried the final system

    def __len__(self):
        return len(self.angles)

    @staticmethod
    def concatenate(results) -> 'RefineResult':
        results = list(results)
        return RefineResult(*(np.concatenate([getattr(r, k) for r in results]) for k in
                              ('angles', 'sigma', 'cost_before', 'cost_after', 'steps_taken', 'inliers')))


def unpack_normal_equations(words: np.ndarray):
    """One frame's 32 words -> (A (6, 6) = J^T J, g (6,) = J^T r)."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = words[10:31]
    return A + np.triu(A, 1).T, np.array(words[4:10], np.float64)


def levenberg_step(words: np.ndarray, active, lam: float) -> np.ndarray:
    """(A + lam diag A) d = -g on the active joints whose diagonal entry is positive -> d (6,); zero for every other joint, and
    zero altogether when the system is singular."""
    A, g = unpack_normal_equations(words)
    idx = [j for j in active if A[j, j] > 0]
    d = np.zeros(6)
    if not idx:
        return d
    S = A[np.ix_(idx, idx)]
    try:
        sol = np.linalg.solve(S + lam * np.diag(np.diag(S)), -g[idx])
    except np.linalg.LinAlgError:
        return d
    if np.isfinite(sol).all():
        d[idx] = sol
    return d


def formal_sigma(words: np.ndarray, active) -> np.ndarray:
    """sqrt(s^2 diag(A^-1)) with s^2 = [3] / ([2] - p), p the active joints with a positive diagonal -> (6,) rad.  inf for an active
    joint with a zero diagonal (no inlier pixel moves with it), for fewer inliers than p + 1 and for a singular A; nan for joints
    that are not active.  This is a FORMAL sigma: it treats the pixels as independent measurements, and neighbouring pixels of a
    depth frame are not, so it is optimistic — good for telling an observable joint from a hidden one and for ranking, not an
    error bar to be taken at its face value."""
    A, _ = unpack_normal_equations(words)
    out = np.full(6, np.nan)
    out[list(active)] = np.inf
    idx = [j for j in active if A[j, j] > 0]
    p = len(idx)
    if p == 0 or words[2] < p + 1:
        return out
    try:
        cov = np.linalg.inv(A[np.ix_(idx, idx)])
    except np.linalg.LinAlgError:
        return out
    var = (words[3] / (words[2] - p)) * np.diag(cov)
    if np.isfinite(var).all() and (var >= 0).all():
        out[idx] = np.sqrt(var)
    return out


def mean_cost(words: np.ndarray) -> np.ndarray:
    """(N, 32) -> (N,): [1] / [0], the mean of min(r^2, clip^2) over the pixels both rendered and measured; inf where there are none."""
    w = np.asarray(words, np.float64)
    return np.where(w[:, 0] > 0, w[:, 1] / np.where(w[:, 0] > 0, w[:, 0], 1.0), np.inf)


class PoseRefiner:
    """renderer_or_engine  a simulation.render.Renderer (its camera is moved to camera_pose here unless it stands there) — or an
                        Engine on which robot and camera are set already, all links rendered
    camera_pose         [x, y, z, a3, a4, a5] as the Predictor takes it
    intrinsics          projection.Intrinsics of the frames (the working resolution)
    do_angles           the joints to refine, letters of 'SLUBRT'
    clip                metres at which a residual is truncated (the Verifier's tol means the same)
    iterations          rounds at most: iterations + 1 renders and kernel calls a batch
    damping             the Levenberg factor a frame starts with; multiplied by 10 for a frame whenever its step is refused"""

    def __init__(self, renderer_or_engine, camera_pose, intrinsics, do_angles: str = 'SLU', clip: float = 2 ** -5, iterations: int = 5,
                 damping: float = 1e-3):
        if not (np.isfinite(clip) and clip > 0):
            raise ValueError(f"clip must be finite and positive, got {clip}")
        if iterations < 0 or not (np.isfinite(damping) and damping >= 0):
            raise ValueError("iterations and damping must not be negative")
        self.renderer = renderer_or_engine if hasattr(renderer_or_engine, 'render_ids_batch_device') else None
        self.engine = self.renderer.engine if self.renderer is not None else renderer_or_engine
        self.intrinsics = intrinsics
        self.active = [int(j) for j in np.flatnonzero(str_to_arr(do_angles.upper()))]
        self.clip, self.iterations, self.damping = float(clip), int(iterations), float(damping)
        self.fk = ForwardKinematics()
        self.limits = np.asarray(self.fk.reader.joint_limits, np.float64)
        self.setCameraPose(camera_pose)

    def setCameraPose(self, camera_pose):
        self.camera_pose = np.asarray(camera_pose, np.float64).copy()
        # a renderer that stands at this pose already is left alone: setting a camera anew drops what its engine built for it
        # (the Predictor's lookup table)
        if self.renderer is not None and not np.array_equal(getattr(self.renderer, '_camera_pose6', None), self.camera_pose):
            self.renderer.setCameraPose(self.camera_pose)
        M = camera_pose_matrix(self.camera_pose)                       # camera to world; the GL camera looks along -z with y up
        flip = np.diag([1.0, -1.0, -1.0])                              # to the kernel's axes: x right, y down, z forward
        self._Rwc, self._tc = flip @ M[:3, :3].T, M[:3, 3].copy()

    @property
    def n_links(self) -> int:
        """Links the refiner draws: all that are ever drawn, whatever limit the renderer stands at (setMaxParts)."""
        return min(int(self.engine.n_links), NUM_RENDER_LINKS)

    def joint_axes(self, angles: np.ndarray) -> np.ndarray:
        """(N, 6) angles -> (N, 6, 6): per joint its unit axis and a point on it, in camera axes, at those angles."""
        angles = np.asarray(angles, np.float64).reshape(-1, 6)
        N = len(angles)
        out = np.empty((N, 6, 6))
        R = np.broadcast_to(np.eye(3), (N, 3, 3))          # ForwardKinematics.calc's chain, all frames at once
        t = np.zeros((N, 3))
        eye = np.eye(3)
        for j in range(6):
            a = self.fk.axes[j]
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            s, c = np.sin(angles[:, j])[:, None, None], np.cos(angles[:, j])[:, None, None]
            rot = c * eye + s * K + (1 - c) * np.outer(a, a)
            t = t + R @ self.fk.fixed[j, :, 3]
            R = R @ (self.fk.fixed[j, :, :3] @ rot)
            out[:, j, :3] = (R @ a) @ self._Rwc.T
            out[:, j, 3:] = (t - self._tc) @ self._Rwc.T
        return out

    def _render(self, angles):
        return self.engine.render_batch_device(np.ascontiguousarray(angles, np.float64), self.n_links, None)

    def equations(self, angles: np.ndarray, depth_t) -> np.ndarray:
        """One render and one kernel call: the normal equations of the poses `angles` against the frames depth_t (a float32 tensor
        on the engine's device) -> (N, 32)."""
        intr = self.intrinsics
        rd, ri = self._render(angles)
        return self.engine.pose_normal_equations(rd, ri, depth_t, self.joint_axes(angles), self.n_links, self.clip,
                                                 (intr.fx, intr.fy, intr.cx, intr.cy))

    def refine(self, angles, depth) -> RefineResult:
        """angles (N, 6); depth (N, H, W) metres at the refiner's resolution, a numpy array or a torch tensor on the host or the
        device, 0 / NaN where nothing was measured -> RefineResult."""
        import torch
        q = np.array(angles, np.float64).reshape(-1, 6)
        N = len(q)
        if N == 0:
            e = np.zeros(0)
            return RefineResult(q, np.zeros((0, 6)), e, e.copy(), np.zeros(0, np.int64), e.copy())
        device = torch.device('cuda', self.engine.device)
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32))
        depth_t = depth.to(device=device, dtype=torch.float32).contiguous()
        if depth_t.dim() != 3 or depth_t.shape[0] != N:
            raise ValueError(f"depth: ({N}, H, W), got {tuple(depth_t.shape)}")
        lam = np.full(N, self.damping)
        words = self.equations(q, depth_t)
        cost = mean_cost(words)
        cost_before, steps = cost.copy(), np.zeros(N, np.int64)
        for _ in range(self.iterations):
            trial = np.stack([np.clip(q[f] + levenberg_step(words[f], self.active, lam[f]), self.limits[:, 0], self.limits[:, 1])
                              for f in range(N)])
            w_t = self.equations(trial, depth_t)
            c_t = mean_cost(w_t)
            ok = c_t < cost                                             # strictly smaller, or the angles are put back
            q[ok], words[ok], cost[ok] = trial[ok], w_t[ok], c_t[ok]
            steps += ok
            lam[~ok] *= 10.0
        return RefineResult(q, np.stack([formal_sigma(w, self.active) for w in words]), cost_before, cost, steps, words[:, 2].copy())
