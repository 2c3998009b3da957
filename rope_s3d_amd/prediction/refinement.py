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


# ---------------------------------------------------------------------------------------------- the camera pose
@dataclass
class CameraRefineResult:
    """What CameraPoseRefiner.refine returns: one camera, pooled over the frames."""
    pose: np.ndarray            # (6,) the refined [x, y, z, a3, a4, a5]; parameters outside do_params as they came
    sigma: np.ndarray           # (6,) formal standard deviation, m and rad: inf = the views do not pin the parameter down, nan = not refined
    cost_before: float          # pooled mean truncated squared residual at the start, m^2 (inf: nothing to compare)
    cost_after: float           # the same at the refined pose; never larger than cost_before
    steps_taken: int            # accepted steps, 0 .. iterations
    inliers: float              # pixels of all frames that carried the final system
    frame_cost: np.ndarray      # (N,) every frame's own mean truncated cost at the refined pose: a frame whose recorded joint
    #                             angles do not fit the others stands out


def camera_twists(pose6) -> np.ndarray:
    """[x, y, z, a3, a4, a5] -> (6, 6): row k is the twist (w, v), in the kernel's camera axes (x right, y down, z forward), with
    which a world-fixed point moves per unit of pose parameter k: dX_c / dp_k = w x X_c + v.

    With M = camera_pose_matrix(pose) = [R | t], Rwc = diag(1, -1, -1) R^T and X_c = Rwc (X_w - t):
      a translation t_k gives dX_c = -Rwc e_k: w = 0, v = -Rwc[:, k];
      an angle turns R = Rz(yaw) Ry(pitch) Rx(roll) about a world axis a (yaw: z; pitch: Rz y; roll: Rz Ry x), dR = [a]x R, so
      dX_c = -diag(1, -1, -1) R^T (a x (X_w - t)) = -(Rwc a) x X_c (diag(1, -1, -1) is a rotation, it goes through the cross
      product): w = -Rwc a, v = 0."""
    p = np.asarray(pose6, np.float64).reshape(6)
    Rwc = np.diag([1.0, -1.0, -1.0]) @ camera_pose_matrix(p)[:3, :3].T
    yaw, pitch = p[5], p[3]
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    axis = {5: np.array([0.0, 0.0, 1.0]), 3: np.array([-sy, cy, 0.0]), 4: np.array([cy * cp, sy * cp, -sp])}      # z; Rz y; Rz Ry x
    out = np.zeros((6, 6))
    for k in range(3):
        out[k, 3:] = -Rwc[:, k]
    for k in (3, 4, 5):
        out[k, :3] = -(Rwc @ axis[k])
    return out


def pool_frames(words: np.ndarray) -> np.ndarray:
    """(N, 32) -> (32,): the frames' words added in frame order, one float64 addition after the other (no pairwise summation: the
    order is part of what tests/camera_refine_ref.py restates)."""
    pooled = np.zeros(NEQ_WORDS)
    for w in np.asarray(words, np.float64).reshape(-1, NEQ_WORDS):
        pooled = pooled + w
    return pooled


class CameraPoseRefiner:
    """A continuous last step for a CAMERA pose seen in N frames at known joint angles, and how sure it is: PoseRefiner's loop
    with the six pose parameters as columns (camera_twists, rope_camera_normal_equations) and ONE system pooled over the frames.

    renderer_or_engine  a simulation.render.Renderer or an Engine on which robot and camera are set (the camera's resolution is
                        what counts: every render here brings its own P V, projection.camera_matrix's, the renderer's own camera
                        is neither read nor moved)
    intrinsics          projection.Intrinsics of the frames (the working resolution)
    do_params           the parameters of [x, y, z, a3, a4, a5] to refine
    clip, iterations, damping   as PoseRefiner's; damping is multiplied by 10 whenever a step is refused"""

    def __init__(self, renderer_or_engine, intrinsics, do_params=(True,) * 6, clip: float = 2 ** -5, iterations: int = 5, damping: float = 1e-3):
        if not (np.isfinite(clip) and clip > 0):
            raise ValueError(f"clip must be finite and positive, got {clip}")
        if iterations < 0 or not (np.isfinite(damping) and damping >= 0):
            raise ValueError("iterations and damping must not be negative")
        do_params = np.asarray(do_params, bool).reshape(-1)
        if len(do_params) != 6:
            raise ValueError("do_params: six flags, one per pose parameter")
        self.engine = renderer_or_engine.engine if hasattr(renderer_or_engine, 'render_ids_batch_device') else renderer_or_engine
        self.intrinsics = intrinsics
        self.active = [int(k) for k in np.flatnonzero(do_params)]
        self.clip, self.iterations, self.damping = float(clip), int(iterations), float(damping)

    @property
    def n_links(self) -> int:
        return min(int(self.engine.n_links), NUM_RENDER_LINKS)

    def equations(self, pose, angles: np.ndarray, depth_t) -> np.ndarray:
        """One render of the N frames' angles under the camera `pose` and one kernel call -> (N, 32), per frame."""
        from ..projection import camera_matrix
        intr = self.intrinsics
        N = len(angles)
        PV = np.tile(camera_matrix(pose, intr)[None], (N, 1, 1))
        rd, ri = self.engine.render_batch_device(angles, self.n_links, PV)
        twists = np.tile(camera_twists(pose)[None], (N, 1, 1))
        return self.engine.camera_normal_equations(rd, ri, depth_t, twists, self.n_links, self.clip, (intr.fx, intr.fy, intr.cx, intr.cy))

    def refine(self, camera_pose, angles, depth) -> CameraRefineResult:
        """camera_pose (6,); angles (N, 6) the robot's joint angles in the frames; depth (N, H, W) metres at the refiner's
        resolution, a numpy array or a torch tensor on the host or the device, 0 / NaN where nothing was measured.

        sigma is formal_sigma's of the pooled system: it treats the pixels as independent measurements, and neighbouring pixels
        of a depth frame are not, so it is FORMAL and optimistic — good for telling a parameter the views pin down from one they
        do not (a camera seen head-on barely fixes its distance) and for ranking, not an error bar to be taken at face value."""
        import torch
        pose = np.array(camera_pose, np.float64).reshape(6)
        q = np.ascontiguousarray(np.asarray(angles, np.float64).reshape(-1, 6))
        N = len(q)
        if N == 0:
            sig = np.full(6, np.nan)
            sig[self.active] = np.inf
            return CameraRefineResult(pose, sig, np.inf, np.inf, 0, 0.0, np.zeros(0))
        device = torch.device('cuda', self.engine.device)
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32))
        depth_t = depth.to(device=device, dtype=torch.float32).contiguous()
        if depth_t.dim() != 3 or depth_t.shape[0] != N:
            raise ValueError(f"depth: ({N}, H, W), got {tuple(depth_t.shape)}")
        lam = self.damping
        words = self.equations(pose, q, depth_t)
        pooled = pool_frames(words)
        cost = float(mean_cost(pooled[None])[0])
        cost_before, steps = cost, 0
        for _ in range(self.iterations):
            trial = pose + levenberg_step(pooled, self.active, lam)
            w_t = self.equations(trial, q, depth_t)
            p_t = pool_frames(w_t)
            c_t = float(mean_cost(p_t[None])[0])
            if c_t < cost:                                              # strictly smaller, or the pose is put back
                pose, words, pooled, cost = trial, w_t, p_t, c_t
                steps += 1
            else:
                lam *= 10.0
        return CameraRefineResult(pose, formal_sigma(pooled, self.active), cost_before, cost, steps, float(pooled[2]), mean_cost(words))
