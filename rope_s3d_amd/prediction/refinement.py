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


def _intr4(intr):
    return intr.fx, intr.fy, intr.cx, intr.cy


def _check_loop_args(clip, iterations, damping):
    if not (np.isfinite(clip) and clip > 0):
        raise ValueError(f"clip must be finite and positive, got {clip}")
    if iterations < 0 or not (np.isfinite(damping) and damping >= 0):
        raise ValueError("iterations and damping must not be negative")


def _active_params(do_params):
    do_params = np.asarray(do_params, bool).reshape(-1)
    if len(do_params) != 6:
        raise ValueError("do_params: six flags, one per pose parameter")
    return [int(k) for k in np.flatnonzero(do_params)]


def _stage_depth(engine, depth, N):
    """depth (N, H, W), a numpy array or a torch tensor on the host or the device -> a contiguous float32 tensor on the engine's device."""
    import torch
    if not isinstance(depth, torch.Tensor):
        depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32))
    depth_t = depth.to(device=torch.device('cuda', engine.device), dtype=torch.float32).contiguous()
    if depth_t.dim() != 3 or depth_t.shape[0] != N:
        raise ValueError(f"depth: ({N}, H, W), got {tuple(depth_t.shape)}")
    return depth_t


def _camera_axes(pose):
    """[x, y, z, a3, a4, a5] -> (Rwc, tc) of the kernel's camera axes X_c = Rwc (X_w - tc): x right, y down, z forward."""
    M = camera_pose_matrix(np.asarray(pose, np.float64).reshape(6))    # camera to world; the GL camera looks along -z with y up
    return np.diag([1.0, -1.0, -1.0]) @ M[:3, :3].T, M[:3, 3].copy()


class _DrawsEveryLink:
    @property
    def n_links(self) -> int:
        """Links the refiner draws: all that are ever drawn, whatever limit the renderer stands at (setMaxParts)."""
        return min(int(self.engine.n_links), NUM_RENDER_LINKS)


def _levenberg_loop(evaluate, propose, state, iterations: int, damping: float):
    """The Levenberg loop with ONE damping and ONE cost: evaluate(state) -> (payload, cost) and propose(state, payload, lam) ->
    the trial state.  A trial is kept only when its cost is strictly smaller; refused, it multiplies lam by 10.
    -> (the state held at the end, its payload, the start's payload, accepted steps)."""
    lam = damping
    payload, cost = evaluate(state)
    first, steps = payload, 0
    for _ in range(iterations):
        trial = propose(state, payload, lam)
        p_t, c_t = evaluate(trial)
        if c_t < cost:                                                  # strictly smaller, or everything is put back
            state, payload, cost, steps = trial, p_t, c_t, steps + 1
        else:
            lam *= 10.0
    return state, payload, first, steps


def _unpack(words: np.ndarray, slots: int):
    """[4 ..] of a system of `slots` unknowns -> (A (slots, slots) = J^T J from its upper triangle, g (slots,) = J^T r)."""
    A = np.zeros((slots, slots))
    A[np.triu_indices(slots)] = words[4 + slots:4 + slots + slots * (slots + 1) // 2]
    return A + np.triu(A, 1).T, np.array(words[4:4 + slots], np.float64)


def _pool(words: np.ndarray, width: int) -> np.ndarray:
    """(N, width) -> (width,): the frames' words added in frame order, one float64 addition after the other (no pairwise summation:
    the order is part of what tests/camera_refine_ref.py and tests/bundle_ref.py restate)."""
    pooled = np.zeros(width)
    for w in np.asarray(words, np.float64).reshape(-1, width):
        pooled = pooled + w
    return pooled


def _solve_finite(M, rhs):
    """np.linalg.solve; None for a singular matrix or a solution that is not finite."""
    try:
        x = np.linalg.solve(M, rhs)
    except np.linalg.LinAlgError:
        return None
    return x if np.isfinite(x).all() else None


def _step(A, g, active, lam: float) -> np.ndarray:
    """(A + lam diag A) d = -g on the active unknowns whose diagonal entry is positive -> d; zero for every other unknown, and zero
    altogether when the system is singular or its solution not finite."""
    idx = [j for j in active if A[j, j] > 0]
    d = np.zeros(len(g))
    if idx:
        S = A[np.ix_(idx, idx)]
        sol = _solve_finite(S + lam * np.diag(np.diag(S)), -g[idx])
        if sol is not None:
            d[idx] = sol
    return d


def _sigma(A, inliers: float, r2: float, active) -> np.ndarray:
    """sqrt(s^2 diag(A^-1)) with s^2 = r2 / (inliers - p), p the active unknowns with a positive diagonal.  inf for an active unknown
    with a zero diagonal, for fewer inliers than p + 1 and for a singular A; nan for what is not active."""
    out = np.full(len(A), np.nan)
    out[list(active)] = np.inf
    idx = [j for j in active if A[j, j] > 0]
    p = len(idx)
    if p == 0 or inliers < p + 1:
        return out
    cov = _solve_finite(A[np.ix_(idx, idx)], np.eye(p))                 # LAPACK's gesv on the identity, as np.linalg.inv
    if cov is None:
        return out
    var = (r2 / (inliers - p)) * np.diag(cov)
    if np.isfinite(var).all() and (var >= 0).all():
        out[idx] = np.sqrt(var)
    return out


def unpack_normal_equations(words: np.ndarray):
    """One frame's 32 words -> (A (6, 6) = J^T J, g (6,) = J^T r)."""
    return _unpack(words, 6)


def levenberg_step(words: np.ndarray, active, lam: float) -> np.ndarray:
    """(A + lam diag A) d = -g on the active joints whose diagonal entry is positive -> d (6,); zero for every other joint, and
    zero altogether when the system is singular."""
    return _step(*unpack_normal_equations(words), active, lam)


def formal_sigma(words: np.ndarray, active) -> np.ndarray:
    """sqrt(s^2 diag(A^-1)) with s^2 = [3] / ([2] - p), p the active joints with a positive diagonal -> (6,) rad.  inf for an active
    joint with a zero diagonal (no inlier pixel moves with it), for fewer inliers than p + 1 and for a singular A; nan for joints
    that are not active.  This is a FORMAL sigma: it treats the pixels as independent measurements, and neighbouring pixels of a
    depth frame are not, so it is optimistic — good for telling an observable joint from a hidden one and for ranking, not an
    error bar to be taken at its face value."""
    return _sigma(unpack_normal_equations(words)[0], words[2], words[3], active)


def mean_cost(words: np.ndarray) -> np.ndarray:
    """(N, 32) -> (N,): [1] / [0], the mean of min(r^2, clip^2) over the pixels both rendered and measured; inf where there are none."""
    w = np.asarray(words, np.float64)
    return np.where(w[:, 0] > 0, w[:, 1] / np.where(w[:, 0] > 0, w[:, 0], 1.0), np.inf)


def joint_axes_camera(fk, Rwc, tc, angles: np.ndarray) -> np.ndarray:
    """(N, 6) angles -> (N, 6, 6): per joint its unit axis and a point on it at those angles, in the kernel's camera axes
    X_c = Rwc (X_w - tc)."""
    angles = np.asarray(angles, np.float64).reshape(-1, 6)
    N = len(angles)
    out = np.empty((N, 6, 6))
    R = np.broadcast_to(np.eye(3), (N, 3, 3))          # ForwardKinematics.calc's chain, all frames at once
    t = np.zeros((N, 3))
    eye = np.eye(3)
    for j in range(6):
        a = fk.axes[j]
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        s, c = np.sin(angles[:, j])[:, None, None], np.cos(angles[:, j])[:, None, None]
        rot = c * eye + s * K + (1 - c) * np.outer(a, a)
        t = t + R @ fk.fixed[j, :, 3]
        R = R @ (fk.fixed[j, :, :3] @ rot)
        out[:, j, :3] = (R @ a) @ Rwc.T
        out[:, j, 3:] = (t - tc) @ Rwc.T
    return out


class PoseRefiner(_DrawsEveryLink):
    """renderer_or_engine  a simulation.render.Renderer (its camera is moved to camera_pose here unless it stands there) — or an
                        Engine on which robot and camera are set already, all links rendered
    camera_pose         [x, y, z, a3, a4, a5] as the Predictor takes it
    intrinsics          projection.Intrinsics of the frames (the working resolution)
    do_angles           the joints to refine, letters of 'SLUBRT'
    clip                metres at which a residual is truncated (the Verifier's tol means the same)
    iterations          rounds at most: iterations + 1 renders and kernel calls a batch
    damping             the Levenberg factor a frame starts with; multiplied by 10 for a frame whenever its step is refused
    native              False (the default): the loop below, on the host, numpy's LAPACK for the solves.  True: refine is one
                        Engine.refine_poses call per chunk of frames (rope_refine_poses, csrc/rope_polish.hip) — the same loop with
                        the joint axes, the solves, accept / reject, damping and the variances on the device.  Same fields, same
                        meanings; the numbers differ by the rounding of another elimination order and of the device's sine"""

    NATIVE_WORK_BYTES = 512 << 20           # device scratch one native call may ask for: the frames are cut to fit

    def __init__(self, renderer_or_engine, camera_pose, intrinsics, do_angles: str = 'SLU', clip: float = 2 ** -5, iterations: int = 5,
                 damping: float = 1e-3, native: bool = False):
        _check_loop_args(clip, iterations, damping)
        self.renderer = renderer_or_engine if hasattr(renderer_or_engine, 'render_ids_batch_device') else None
        self.engine = self.renderer.engine if self.renderer is not None else renderer_or_engine
        self.intrinsics = intrinsics
        self.active = [int(j) for j in np.flatnonzero(str_to_arr(do_angles.upper()))]
        self.clip, self.iterations, self.damping = float(clip), int(iterations), float(damping)
        self.native = bool(native)
        self.fk = ForwardKinematics()
        self.limits = np.asarray(self.fk.reader.joint_limits, np.float64)
        self.setCameraPose(camera_pose)

    def setCameraPose(self, camera_pose):
        self.camera_pose = np.asarray(camera_pose, np.float64).copy()
        # a renderer that stands at this pose already is left alone: setting a camera anew drops what its engine built for it
        # (the Predictor's lookup table)
        if self.renderer is not None and not np.array_equal(getattr(self.renderer, '_camera_pose6', None), self.camera_pose):
            self.renderer.setCameraPose(self.camera_pose)
        self._Rwc, self._tc = _camera_axes(self.camera_pose)

    def joint_axes(self, angles: np.ndarray) -> np.ndarray:
        """(N, 6) angles -> (N, 6, 6): per joint its unit axis and a point on it, in camera axes, at those angles."""
        return joint_axes_camera(self.fk, self._Rwc, self._tc, angles)

    def _render(self, angles):
        return self.engine.render_batch_device(np.ascontiguousarray(angles, np.float64), self.n_links, None)

    def equations(self, angles: np.ndarray, depth_t) -> np.ndarray:
        """One render and one kernel call: the normal equations of the poses `angles` against the frames depth_t (a float32 tensor
        on the engine's device) -> (N, 32)."""
        rd, ri = self._render(angles)
        return self.engine.pose_normal_equations(rd, ri, depth_t, self.joint_axes(angles), self.n_links, self.clip, _intr4(self.intrinsics))

    def refine(self, angles, depth) -> RefineResult:
        """angles (N, 6); depth (N, H, W) metres at the refiner's resolution, a numpy array or a torch tensor on the host or the
        device, 0 / NaN where nothing was measured -> RefineResult."""
        q = np.array(angles, np.float64).reshape(-1, 6)
        N = len(q)
        if N == 0:
            e = np.zeros(0)
            return RefineResult(q, np.zeros((0, 6)), e, e.copy(), np.zeros(0, np.int64), e.copy())
        depth_t = _stage_depth(self.engine, depth, N)
        if self.native:
            return self._refine_native(q, depth_t)
        # _levenberg_loop's rule with a damping, a cost and a verdict PER FRAME, and all frames in one render: vectors, so its own loop
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

    def _refine_native(self, q: np.ndarray, depth_t) -> RefineResult:
        """refine through rope_refine_poses: one call per chunk of frames whose scratch fits NATIVE_WORK_BYTES."""
        N = len(q)
        mask = sum(1 << j for j in self.active)
        chunk = max(1, min(N, self.NATIVE_WORK_BYTES // max(1, self.engine.refine_workspace(1))))
        parts = []
        for lo in range(0, N, chunk):
            r = self.engine.refine_poses(q[lo:lo + chunk], depth_t[lo:lo + chunk], self.camera_pose, _intr4(self.intrinsics), mask,
                                         self.limits, self.clip, self.iterations, self.damping)
            parts.append(RefineResult(r['angles'], np.sqrt(r['var']), r['cost_before'], r['cost_after'], r['steps'].astype(np.int64), r['inliers']))
        return parts[0] if len(parts) == 1 else RefineResult.concatenate(parts)


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
    Rwc, _ = _camera_axes(p)
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
    """(N, 32) -> (32,): the frames' words added in frame order (_pool)."""
    return _pool(words, NEQ_WORDS)


def _render_under(engine, intr, pose, angles, n_links):
    """One render of the N frames' angles under the camera `pose`, which brings its own P V -> (depth, ids) on the device."""
    from ..projection import camera_matrix
    return engine.render_batch_device(angles, n_links, np.tile(camera_matrix(pose, intr)[None], (len(angles), 1, 1)))


class CameraPoseRefiner(_DrawsEveryLink):
    """A continuous last step for a CAMERA pose seen in N frames at known joint angles, and how sure it is: PoseRefiner's loop
    with the six pose parameters as columns (camera_twists, rope_camera_normal_equations) and ONE system pooled over the frames.

    renderer_or_engine  a simulation.render.Renderer or an Engine on which robot and camera are set (the camera's resolution is
                        what counts: every render here brings its own P V, projection.camera_matrix's, the renderer's own camera
                        is neither read nor moved)
    intrinsics          projection.Intrinsics of the frames (the working resolution)
    do_params           the parameters of [x, y, z, a3, a4, a5] to refine
    clip, iterations, damping   as PoseRefiner's; damping is multiplied by 10 whenever a step is refused"""

    def __init__(self, renderer_or_engine, intrinsics, do_params=(True,) * 6, clip: float = 2 ** -5, iterations: int = 5, damping: float = 1e-3):
        _check_loop_args(clip, iterations, damping)
        self.active = _active_params(do_params)
        self.engine = renderer_or_engine.engine if hasattr(renderer_or_engine, 'render_ids_batch_device') else renderer_or_engine
        self.intrinsics = intrinsics
        self.clip, self.iterations, self.damping = float(clip), int(iterations), float(damping)

    def equations(self, pose, angles: np.ndarray, depth_t) -> np.ndarray:
        """One render of the N frames' angles under the camera `pose` and one kernel call -> (N, 32), per frame."""
        rd, ri = _render_under(self.engine, self.intrinsics, pose, angles, self.n_links)
        twists = np.tile(camera_twists(pose)[None], (len(angles), 1, 1))
        return self.engine.camera_normal_equations(rd, ri, depth_t, twists, self.n_links, self.clip, _intr4(self.intrinsics))

    def refine(self, camera_pose, angles, depth) -> CameraRefineResult:
        """camera_pose (6,); angles (N, 6) the robot's joint angles in the frames; depth (N, H, W) metres at the refiner's
        resolution, a numpy array or a torch tensor on the host or the device, 0 / NaN where nothing was measured.

        sigma is formal_sigma's of the pooled system: it treats the pixels as independent measurements, and neighbouring pixels
        of a depth frame are not, so it is FORMAL and optimistic — good for telling a parameter the views pin down from one they
        do not (a camera seen head-on barely fixes its distance) and for ranking, not an error bar to be taken at face value."""
        pose = np.array(camera_pose, np.float64).reshape(6)
        q = np.ascontiguousarray(np.asarray(angles, np.float64).reshape(-1, 6))
        N = len(q)
        if N == 0:
            sig = np.full(6, np.nan)
            sig[self.active] = np.inf
            return CameraRefineResult(pose, sig, np.inf, np.inf, 0, 0.0, np.zeros(0))
        depth_t = _stage_depth(self.engine, depth, N)

        def evaluate(pose):
            words = self.equations(pose, q, depth_t)
            pooled = pool_frames(words)
            cost = float(mean_cost(pooled[None])[0])
            return (words, pooled, cost), cost

        pose, (words, pooled, cost), (_, _, cost_before), steps = _levenberg_loop(
            evaluate, lambda pose, held, lam: pose + levenberg_step(held[1], self.active, lam), pose, self.iterations, self.damping)
        return CameraRefineResult(pose, formal_sigma(pooled, self.active), cost_before, cost, steps, float(pooled[2]), mean_cost(words))


# ---------------------------------------------------------------------------------------------- angles and camera in one solve
BNEQ_WORDS = 96
BNEQ_SLOTS = 12
SIL_MAX_RADIUS = 16             # ROPE_SIL_MAX_RADIUS


@dataclass
class BundleRefineResult:
    """What BundleRefiner.refine returns: one camera and every frame's angles, from one system."""
    pose: np.ndarray            # (6,) the refined [x, y, z, a3, a4, a5]; parameters outside do_params as they came
    angles: np.ndarray          # (N, 6) the refined angles ('offset': the input angles plus the offsets); other joints as they came
    offsets: np.ndarray         # (6,) 'offset' mode: the joints' zero offsets, 0 outside do_angles; nan in 'frame' mode
    sigma_pose: np.ndarray      # (6,) formal standard deviation, m and rad, with the angles (or offsets) unknown as well
    sigma_angles: np.ndarray    # (N, 6) 'frame' mode, rad; None in 'offset' mode
    sigma_offsets: np.ndarray   # (6,) 'offset' mode, rad; None in 'frame' mode
    cost_before: float          # pooled mean truncated squared residual at the start, m^2 (inf: nothing to compare)
    cost_after: float           # the same at the end; never larger than cost_before
    steps_taken: int            # accepted steps, 0 .. iterations
    inliers: float              # pixels of all frames that carried the final system
    frame_cost: np.ndarray      # (N,) every frame's own mean truncated cost at the end
    # the silhouette term (BundleRefiner(silhouette > 0)); the fields above keep their depth meaning, nan / 0 without depth frames
    cost_silhouette_before: float = float('nan')    # pooled mean truncated squared outline distance at the start, pixels^2
    cost_silhouette_after: float = float('nan')     # the same at the end
    inliers_silhouette: float = 0.0                 # contour pixels of all frames that carried the final system
    # robust weights (BundleRefiner(robust=...)): the scale every round of the call was weighted at, metres; nan without them.  The
    # costs above are then means of the robust cost at that scale, and compare only with costs at the same kind and scale
    robust_scale: float = float('nan')
    # the outline's second direction (BundleRefiner(both_ways=True)): the MASK's contour pixels of all frames that carried the final
    # system.  The outline costs above are then means over both directions' contour pixels; inliers_silhouette stays the render's
    inliers_silhouette_reverse: float = 0.0


def unpack_bundle(words: np.ndarray):
    """One frame's (or the pooled) 96 words -> (A (12, 12) = J^T J, g (12,) = J^T r); slots 0 .. 5 the joints, 6 .. 11 the camera."""
    return _unpack(words, BNEQ_SLOTS)


def pool_bundle(words: np.ndarray) -> np.ndarray:
    """(N, 96) -> (96,): pool_frames for the bundle's words, added in frame order."""
    return _pool(words, BNEQ_WORDS)


def _arrow_blocks(words, active_j, active_c):
    """-> ([(idx_f, A_f, B_f, g_f)] per frame, kc, C, gc): idx_f the active joints of the frame with a positive diagonal, kc the
    active camera parameters with a positive diagonal in the pooled camera block C (the frames' added in frame order)."""
    Ap, gp = unpack_bundle(pool_bundle(words))
    kc = [k for k in active_c if Ap[6 + k, 6 + k] > 0]
    cc = [6 + k for k in kc]
    frames = []
    for w in words:
        A, g = unpack_bundle(w)
        idx = [j for j in active_j if A[j, j] > 0]
        frames.append((idx, A[np.ix_(idx, idx)], A[np.ix_(idx, cc)], g[idx]))
    return frames, kc, Ap[np.ix_(cc, cc)], gp[cc]


def schur_step(words: np.ndarray, active_j, active_c, lam: float):
    """The Levenberg step of the block-arrow system (every frame's joints, one camera) by its Schur complement, never assembled
    densely -> (dq (N, 6), dc (6,)).  D_f = A_f + lam diag A_f; S = C + lam diag C - sum B_f^T D_f^-1 B_f;
    dc = -S^-1 (gc - sum B_f^T D_f^-1 g_f); dq_f = -D_f^-1 (g_f + B_f dc).  A singular D_f: a zero step for that frame's joints (the
    frame leaves the sums); a singular S: a zero step for the camera."""
    words = np.asarray(words, np.float64).reshape(-1, BNEQ_WORDS)
    frames, kc, C, gc = _arrow_blocks(words, active_j, active_c)
    dq, dc = np.zeros((len(words), 6)), np.zeros(6)
    S = C + lam * np.diag(np.diag(C))
    rhs = gc.copy()
    solved = []
    for idx, A, B, g in frames:
        X = _solve_finite(A + lam * np.diag(np.diag(A)), np.column_stack([B, g])) if idx else None       # D_f^-1 [B_f, g_f]
        solved.append(X)
        if X is not None:
            S = S - B.T @ X[:, :-1]
            rhs = rhs - B.T @ X[:, -1]
    d = _solve_finite(S, -rhs) if kc else None
    if d is None:
        d = np.zeros(len(kc))
    dc[kc] = d
    for f, ((idx, A, B, g), X) in enumerate(zip(frames, solved)):
        if X is not None:
            dq[f, idx] = -(X[:, -1] + X[:, :-1] @ d)
    return dq, dc


def schur_sigma(words: np.ndarray, active_j, active_c):
    """formal_sigma for the arrow system at lam = 0 -> (sigma_angles (N, 6), sigma_pose (6,)): s^2 = sum [3] / (sum [2] - p) with p
    all live unknowns, cov_c = S0^-1 and cov_qf = A_f^-1 + A_f^-1 B_f S0^-1 B_f^T A_f^-1.  inf for an active unknown with a zero
    diagonal, for fewer inliers than p + 1 and for a singular block; nan for what is not refined.  FORMAL, as formal_sigma's: the
    pixels are taken as independent measurements, which neighbours in a depth frame are not."""
    words = np.asarray(words, np.float64).reshape(-1, BNEQ_WORDS)
    sq, sc = np.full((len(words), 6), np.nan), np.full(6, np.nan)
    sq[:, list(active_j)] = np.inf
    sc[list(active_c)] = np.inf
    frames, kc, C, _ = _arrow_blocks(words, active_j, active_c)
    pooled = pool_bundle(words)
    p = len(kc) + sum(len(fr[0]) for fr in frames)
    if p == 0 or pooled[2] < p + 1:
        return sq, sc
    s2 = pooled[3] / (pooled[2] - p)
    S0 = C.copy()
    solved = []
    for idx, A, B, g in frames:
        X = _solve_finite(A, np.column_stack([B, np.eye(len(idx))])) if idx else None                     # A_f^-1 [B_f, I]
        solved.append(X)
        if X is not None:
            S0 = S0 - B.T @ X[:, :len(kc)]
    covc = _solve_finite(S0, np.eye(len(kc))) if kc else np.zeros((0, 0))
    if covc is None:
        return sq, sc
    var = s2 * np.diag(covc)
    if np.isfinite(var).all() and (var >= 0).all():
        sc[kc] = np.sqrt(var)
    for f, ((idx, A, B, g), X) in enumerate(zip(frames, solved)):
        if X is None:
            continue
        Y, Ainv = X[:, :len(kc)], X[:, len(kc):]
        var = s2 * np.diag(Ainv + Y @ covc @ Y.T)
        if np.isfinite(var).all() and (var >= 0).all():
            sq[f, idx] = np.sqrt(var)
    return sq, sc


RESID_BINS = 256                # ROPE_RESID_WORDS - 2: the bins of |r| <= clip in a frame's residual histogram
ROBUST_TUNING = {'huber': 1.345, 'tukey': 4.685}       # the usual constants of 95 % efficiency on Gaussian residuals


def robust_scale_from_histogram(hist, clip: float, kind: str) -> float:
    """The scale of the robust weights, metres, from residual histograms (Engine.residual_histogram: (N, 258) or (258,)): the
    frames' counts pooled, n the sum of bins 0 .. 255 (the residuals within clip), m = (b + 1) clip / 256 with b the first bin at
    which the running count reaches ceil(n / 2) — the median of |r|, taken at its bin's upper edge — sigma = 1.4826 m (the median
    absolute deviation of a Gaussian), and the scale 1.345 sigma for 'huber', 4.685 sigma for 'tukey'.  Clamped to [clip / 128,
    clip]: above clip nothing is left to weigh, and the floor, two bin widths, is a DESIGN CONSTANT, not a measurement — below it
    the histogram cannot tell one scale from another, and a perfect fit would drive the scale, and with it every weight, to nothing.
    With no residual within clip (n == 0) the scale is clip.  Pure host arithmetic on integers and Python floats."""
    if kind not in ROBUST_TUNING:
        raise ValueError(f"kind: 'huber' or 'tukey', got {kind!r}")
    clip = float(clip)
    if not (np.isfinite(clip) and clip > 0):
        raise ValueError(f"clip must be finite and positive, got {clip}")
    h = np.asarray(hist)
    if h.ndim not in (1, 2) or h.shape[-1] != RESID_BINS + 2:
        raise ValueError(f"hist: (N, {RESID_BINS + 2}) or ({RESID_BINS + 2},) counts, got {h.shape}")
    bins = h.reshape(-1, RESID_BINS + 2)[:, :RESID_BINS].astype(np.int64).sum(axis=0)
    n = int(bins.sum())
    if n == 0:
        return clip
    b = int(np.searchsorted(np.cumsum(bins), (n + 1) // 2))            # the first bin whose running count is >= ceil(n / 2)
    m = (b + 1) * clip / RESID_BINS
    return float(min(max(ROBUST_TUNING[kind] * (1.4826 * m), clip / 128.0), clip))


def bundle_columns_step(pooled: np.ndarray, active, lam: float) -> np.ndarray:
    """levenberg_step's rule over the twelve slots of a pooled system -> (12,)."""
    return _step(*unpack_bundle(pooled), active, lam)


def bundle_columns_sigma(pooled: np.ndarray, active) -> np.ndarray:
    """formal_sigma's rule over the twelve slots of a pooled system -> (12,)."""
    return _sigma(unpack_bundle(pooled)[0], pooled[2], pooled[3], active)


class BundleRefiner(_DrawsEveryLink):
    """Joint angles AND camera pose of N frames of one fixed camera polished in ONE Gauss-Newton / Levenberg system
    (rope_bundle_normal_equations, csrc/rope_bundle.hip): PoseRefiner takes the camera as exact and CameraPoseRefiner the angles,
    and each absorbs the other's error; here neither half is assumed, and the formal sigmas say what the views pin down then.

    renderer_or_engine  as CameraPoseRefiner's: every render brings its own P V, the renderer's camera is neither read nor moved
    intrinsics          projection.Intrinsics of the frames (the working resolution)
    do_angles           the joints to refine, letters of 'SLUBRT'
    do_params           the parameters of [x, y, z, a3, a4, a5] to refine
    joints              'frame': every frame's active joints are unknowns of their own (a block-arrow system, solved by its Schur
                        complement); 'offset': ONE zero offset per active joint, added to every frame's input angles (kinematic
                        calibration: a pooled 12-column system)
    clip, iterations, damping   as PoseRefiner's; ONE damping for the whole system, multiplied by 10 whenever a step is refused.
                        A step is kept only if the pooled cost sum [1] / sum [0] over all frames is strictly smaller.
    silhouette          0 (the default): depth alone, exactly as before.  > 0: the weight of the outline term
                        (rope_silhouette_normal_equations, csrc/rope_silhouette.hip) — refine then takes the frames' robot masks,
                        and may go without depth frames altogether.  Both costs are normalised by their truncations, c_d = mean
                        cost / clip^2 and c_s = mean outline cost / R'^2 with R' = sqrt(radius^2 + 1) - 0.5; a step is kept if
                        c_d + silhouette c_s is strictly smaller, and the system solved is the sum of the two terms' words, each
                        divided by its pixel count and truncation at the iterate held.  One-directional unless both_ways: the
                        render's outline is measured against the mask
    radius              1 .. 16 pixels: the truncation of the mask's distance field
    native              False (the default): the loop below, on the host, numpy's LAPACK for the solves.  True: refine is one
                        Engine.refine_bundle call per batch (rope_refine_bundle, csrc/rope_bundle_polish.hip) — the same loop with the
                        joint axes, the pool, the Schur or twelve-column solves, accept / reject, damping and the variances on the
                        device.  Same fields, same meanings; the numbers differ by the rounding of another elimination order and of
                        the device's sine in the joint axes.  Depth term only: with silhouette > 0 it raises ValueError
    robust              None (the default): a residual counts fully up to clip and not at all beyond it, exactly as before, not a
                        launch more.  'huber' or 'tukey': every inlier is weighted (rope_bundle_normal_equations_robust,
                        csrc/rope_robust.hip) — Huber's weight falls as scale / |r| beyond the scale and its inliers end at clip,
                        Tukey's falls to zero AT the scale and its inliers end there — so that a cable, a payload or a fringe of
                        flying pixels a centimetre or two in front of a link, inside clip, does not pull the solve with full weight.
                        The step, the Schur complement, the sigmas and frame_cost are the code below on the weighted words; cost_before,
                        cost_after and frame_cost are means of the robust cost.  Not with native=True and not with silhouette > 0
                        (ValueError): the native loop and the normalisation of a mixed robust cost are not built
    robust_scale        'auto' (the default): the scale is robust_scale_from_histogram of the residuals at the START pose
                        (rope_residual_histogram), once per refine call; or the scale in metres, finite, 0 < scale <= clip.  It is
                        never re-estimated between the rounds of a call: a step is kept when the cost falls, and two costs compare
                        only under one weighting.  The result's robust_scale says what was used
    both_ways           False (the default): the outline term as above, not a launch more.  True, with silhouette > 0 (ValueError
                        without): the MASK's outline is measured against the render as well — every round one rope_render_nearest of
                        the round's own render and one rope_silhouette_normal_equations_reverse (csrc/rope_silhouette_reverse.hip),
                        whose words are ADDED to the forward ones, both in pixels^2 under the same truncation; c_s, the term's share
                        of the system and its s^2 are then the rules above on the summed words.  A part of the mask that no outline of
                        the render comes near then pulls: a link rotated out of its mask, a forearm hidden inside the mask's area"""

    def __init__(self, renderer_or_engine, intrinsics, do_angles: str = 'SLU', do_params=(True,) * 6, joints: str = 'frame',
                 clip: float = 2 ** -5, iterations: int = 5, damping: float = 1e-3, silhouette: float = 0.0, radius: int = 8,
                 native: bool = False, robust=None, robust_scale='auto', both_ways: bool = False):
        _check_loop_args(clip, iterations, damping)
        if robust is not None and robust not in ROBUST_TUNING:
            raise ValueError(f"robust: None, 'huber' or 'tukey', got {robust!r}")
        if robust is not None and native:
            raise ValueError("robust weights run in the host loop alone: native must be False (rope_refine_bundle has no weights)")
        if robust is not None and silhouette > 0:
            raise ValueError("robust weights are for the depth term alone: silhouette must be 0")
        if isinstance(robust_scale, str) or isinstance(robust_scale, bool):
            if robust_scale != 'auto':
                raise ValueError(f"robust_scale: 'auto' or metres, got {robust_scale!r}")
        elif not (np.isfinite(robust_scale) and 0 < robust_scale <= clip):
            raise ValueError(f"robust_scale: 'auto' or metres, finite and in (0, clip], got {robust_scale!r}")
        self.robust, self.robust_scale = robust, robust_scale if isinstance(robust_scale, str) else float(robust_scale)
        if not (np.isfinite(silhouette) and silhouette >= 0):
            raise ValueError(f"silhouette: a finite weight, 0 or more, got {silhouette}")
        if native and silhouette > 0:
            raise ValueError("native=True polishes on the depth term alone: silhouette must be 0 (rope_refine_bundle has no outline term)")
        self.native = bool(native)
        if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= SIL_MAX_RADIUS:
            raise ValueError(f"radius: a whole number of pixels in 1 .. {SIL_MAX_RADIUS}, got {radius}")
        self.silhouette, self.radius = float(silhouette), int(radius)
        if both_ways and not silhouette > 0:
            raise ValueError("both_ways is the outline term's second direction: silhouette must be > 0")
        self.both_ways = bool(both_ways)
        if joints not in ('frame', 'offset'):
            raise ValueError(f"joints: 'frame' or 'offset', got {joints!r}")
        self.active_c = _active_params(do_params)
        self.engine = renderer_or_engine.engine if hasattr(renderer_or_engine, 'render_ids_batch_device') else renderer_or_engine
        self.intrinsics = intrinsics
        self.active_j = [int(j) for j in np.flatnonzero(str_to_arr(do_angles.upper()))]
        if not self.active_j and not self.active_c:
            raise ValueError("nothing to refine: do_angles and do_params are both empty")
        self.mode = joints
        self.clip, self.iterations, self.damping = float(clip), int(iterations), float(damping)
        self.fk = ForwardKinematics()
        self.limits = np.asarray(self.fk.reader.joint_limits, np.float64)

    def joint_axes(self, pose, angles: np.ndarray) -> np.ndarray:
        """PoseRefiner.joint_axes under the camera `pose` -> (N, 6, 6)."""
        return joint_axes_camera(self.fk, *_camera_axes(pose), angles)

    def _equations(self, pose, angles: np.ndarray, depth_t, sd2_t, scale=None, mask_t=None):
        """One render of the N frames' angles under the camera `pose`, the joint axes and the twists there, and one kernel call per
        term that is given -> (depth words (N, 96) or None without depth_t, outline words (N, 96) or None without sd2_t, the
        words of the outline's second direction or None without mask_t: the masks against render_nearest's field of THIS render).
        With robust weights the depth words are the weighted ones at `scale` metres."""
        angles = np.ascontiguousarray(angles, np.float64)
        rd, ri = _render_under(self.engine, self.intrinsics, pose, angles, self.n_links)
        axes = self.joint_axes(pose, angles) if self.active_j else None
        twists = np.tile(camera_twists(pose)[None], (len(angles), 1, 1)) if self.active_c else None
        intr4 = _intr4(self.intrinsics)
        if depth_t is None:
            w_d = None
        elif self.robust is None:
            w_d = self.engine.bundle_normal_equations(rd, ri, depth_t, axes, twists, self.n_links, self.clip, intr4)
        else:
            w_d = self.engine.bundle_normal_equations_robust(rd, ri, depth_t, axes, twists, self.n_links, self.clip, intr4, self.robust, scale)
        w_s = None if sd2_t is None else self.engine.silhouette_normal_equations(rd, ri, sd2_t, axes, twists, self.n_links, self.radius, intr4)
        w_r = None
        if mask_t is not None:
            near_t = self.engine.render_nearest(ri, self.n_links, self.radius)
            w_r = self.engine.silhouette_normal_equations_reverse(mask_t, near_t, rd, ri, axes, twists, self.n_links, self.radius, intr4)
        return w_d, w_s, w_r

    def equations(self, pose, angles: np.ndarray, depth_t, scale=None) -> np.ndarray:
        """One render of the N frames' angles under the camera `pose`, the joint axes and the twists there and one kernel call ->
        (N, 96), per frame.  scale: the scale of the robust weights, metres; read only by a refiner with robust weights."""
        return self._equations(pose, angles, depth_t, None, scale)[0]

    def residual_scale(self, pose, angles: np.ndarray, depth_t) -> float:
        """The 'auto' scale of the robust weights at (pose, angles): one render, one rope_residual_histogram call,
        robust_scale_from_histogram of the frames' pooled counts -> metres."""
        angles = np.ascontiguousarray(angles, np.float64)
        rd, ri = _render_under(self.engine, self.intrinsics, pose, angles, self.n_links)
        return robust_scale_from_histogram(self.engine.residual_histogram(rd, ri, depth_t, self.n_links, self.clip), self.clip, self.robust)

    def equations_both(self, pose, angles: np.ndarray, depth_t, sd2_t):
        """equations' render, axes and twists, handed to both kernels -> (depth words (N, 96) or None without depth_t, outline
        words (N, 96))."""
        return self._equations(pose, angles, depth_t, sd2_t)[:2]

    def _result(self, pose, q, off, sigma_pose, sigma_joints, *fields, **named) -> BundleRefineResult:
        """The result in the refiner's mode: sigma_joints is sigma_angles (N, 6) in 'frame' mode and sigma_offsets (6,) in 'offset'
        mode; fields are cost_before and what follows it, named the fields given by name (robust_scale)."""
        if self.mode == 'frame':
            return BundleRefineResult(pose, q, np.full(6, np.nan), sigma_pose, sigma_joints, None, *fields, **named)
        return BundleRefineResult(pose, q, np.where(np.isin(np.arange(6), self.active_j), off, 0.0), sigma_pose, None, sigma_joints, *fields, **named)

    def _stage_masks(self, mask, depth, N):
        """refine's masks and, where given, depth of the same shape -> (depth_t or None, mask_distance's field of the masks, the
        masks as uint8 on the device)."""
        import torch
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask))
        if mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 3 or mask.shape[0] != N:
            raise ValueError(f"mask: ({N}, H, W) bool or uint8, got {tuple(mask.shape)} {mask.dtype}")
        mask_t = mask.to(device=torch.device('cuda', self.engine.device)).ne(0).to(torch.uint8).contiguous()
        depth_t = None if depth is None else _stage_depth(self.engine, depth, N)
        if depth_t is not None and depth_t.shape != mask_t.shape:
            raise ValueError(f"depth: {tuple(mask_t.shape)} as the masks, got {tuple(depth_t.shape)}")
        return depth_t, self.engine.mask_distance(mask_t, self.radius), mask_t          # once: the masks do not move

    def refine(self, camera_pose, angles, depth, mask=None) -> BundleRefineResult:
        """camera_pose (6,); angles (N, 6); depth (N, H, W) metres at the refiner's resolution, a numpy array or a torch tensor on
        the host or the device, 0 / NaN where nothing was measured.  mask (N, H, W) bool or uint8, non-zero = robot, likewise: read
        only with silhouette > 0, and required then; depth may then be None (the outline alone, for colour-only frames).  The
        sigmas are FORMAL (schur_sigma, formal_sigma): good for telling what the views pin down and for ranking, not error bars to
        be taken at face value."""
        outline = self.silhouette > 0
        if outline and mask is None:
            raise ValueError("silhouette > 0: refine needs the frames' robot masks (mask=)")
        pose = np.array(camera_pose, np.float64).reshape(6)
        q0 = np.ascontiguousarray(np.array(angles, np.float64).reshape(-1, 6))
        N = len(q0)
        frame_mode = self.mode == 'frame'
        slots = self.active_j + [6 + k for k in self.active_c]
        lo, hi = self.limits[:, 0], self.limits[:, 1]
        nan = float('nan')
        if N == 0:
            sp, so = np.full(6, np.nan), np.full(6, np.nan)
            sp[self.active_c], so[self.active_j] = np.inf, np.inf
            c_d = np.inf if depth is not None or not outline else nan
            return self._result(pose, q0, np.zeros(6), sp, np.zeros((0, 6)) if frame_mode else so, c_d, c_d, 0, 0.0, np.zeros(0),
                                *((np.inf, np.inf, 0.0) if outline else ()))
        depth_t, sd2_t, mask_t = self._stage_masks(mask, depth, N) if outline else (_stage_depth(self.engine, depth, N), None, None)
        if self.native:
            return self._refine_native(pose, q0, depth_t)
        # the scale of the robust weights: fixed here, at the start pose, for every round of this call
        scale = None if self.robust is None else self.residual_scale(pose, q0, depth_t) if self.robust_scale == 'auto' else self.robust_scale
        if scale is not None:
            scale = float(np.float32(scale))                                            # what the kernel is handed, and what the result reports
        far = np.sqrt(self.radius * self.radius + 1.0) - 0.5                            # R'
        norm_d, norm_s = self.clip * self.clip, far * far

        def evaluate(state):
            """-> ((the terms' words, their pools, their mean costs, the outline's inliers by direction), the cost a step is judged
            by): depth alone its mean cost, with the outline c_d / clip^2 + silhouette c_s / R'^2"""
            w_d, w_s, w_r = self._equations(state[0], state[2], depth_t, sd2_t, scale, mask_t if self.both_ways else None)
            n_sr = None
            if w_r is not None:                                         # both directions: ONE outline term, the sum of their words
                n_sr = (float(pool_bundle(w_s)[2]), float(pool_bundle(w_r)[2]))
                w_s = w_s + w_r
            p_d, p_s = (None if w is None else pool_bundle(w) for w in (w_d, w_s))
            c_d, c_s = (nan if p is None else float(p[1] / p[0]) if p[0] > 0 else np.inf for p in (p_d, p_s))
            if not outline:
                cost = c_d
            else:
                cost = float(self.silhouette * (c_s / norm_s)) if p_d is None else float(c_d / norm_d + self.silhouette * (c_s / norm_s))
            return (w_d, p_d, c_d, w_s, p_s, c_s, n_sr), cost

        def system(w_d, p_d, w_s, p_s):
            """a_d w_d + a_s w_s on the words of the system, [4 .. 93], each term divided by its pixel count and truncation; the rest 0"""
            a_d = 1.0 / (p_d[0] * norm_d) if p_d is not None and p_d[0] > 0 else 0.0
            a_s = self.silhouette / (p_s[0] * norm_s) if p_s[0] > 0 else 0.0
            out = np.zeros_like(w_s)
            out[..., 4:94] = a_s * w_s[..., 4:94] if w_d is None else a_d * w_d[..., 4:94] + a_s * w_s[..., 4:94]
            return out

        def propose(state, held, lam):
            pose, off, q = state
            w_d, p_d, _, w_s, p_s, _, _ = held
            words = system(w_d, p_d, w_s, p_s) if outline else w_d      # depth alone: the kernel's words as they came
            if frame_mode:
                dq, dc = schur_step(words, self.active_j, self.active_c, lam)
                return pose + dc, off, np.clip(q + dq, lo, hi)
            d = bundle_columns_step(pool_bundle(words) if outline else p_d, slots, lam)
            t_off = off + d[:6]
            return pose + d[6:], t_off, np.clip(q0 + t_off, lo, hi)

        (pose, off, q), (w_d, p_d, c_d, w_s, p_s, c_s, n_sr), first, steps = _levenberg_loop(evaluate, propose, (pose, np.zeros(6), q0.copy()),
                                                                                     self.iterations, self.damping)
        words, pooled = w_d, p_d
        if outline:
            # the sigmas: the information of the two terms added, each over its own s^2 = [3] / ([2] - p).  The sum goes through
            # schur_sigma / bundle_columns_sigma with [2] = p + 1 and [3] = 1, which makes their own factor s^2 exactly 1.
            terms = [(w, pl) for w, pl in ((w_d, p_d), (w_s, p_s)) if w is not None]
            if frame_mode:
                frames, kc, _, _ = _arrow_blocks(sum(w for w, _ in terms), self.active_j, self.active_c)
                p = len(kc) + sum(len(fr[0]) for fr in frames)
            else:
                A, _ = unpack_bundle(sum(pl for _, pl in terms))
                p = sum(1 for c in slots if A[c, c] > 0)
            words = np.zeros_like(w_s)
            for w, pl in terms:
                if p > 0 and pl[2] >= p + 1 and pl[3] > 0:
                    words[:, 4:94] += w[:, 4:94] / (pl[3] / (pl[2] - p))
            if words.any():
                words[0, 2], words[0, 3] = p + 1.0, 1.0
            pooled = None if frame_mode else pool_bundle(words)
        sj, sp = schur_sigma(words, self.active_j, self.active_c) if frame_mode else np.split(bundle_columns_sigma(pooled, slots), 2)
        return self._result(pose, q, off, sp, sj, first[2], c_d, steps, 0.0 if p_d is None else float(p_d[2]),
                            np.full(N, np.nan) if w_d is None else mean_cost(w_d[:, :NEQ_WORDS]),
                            *((first[5], c_s, float(p_s[2]) if n_sr is None else n_sr[0]) if outline else ()),
                            **({} if scale is None else {'robust_scale': float(scale)}),
                            **({} if n_sr is None else {'inliers_silhouette_reverse': n_sr[1]}))

    def _refine_native(self, pose: np.ndarray, q0: np.ndarray, depth_t) -> BundleRefineResult:
        """refine through rope_refine_bundle: ONE call, because one system spans all frames — a batch whose scratch one call does
        not take is refused (Engine.refine_bundle_workspace says what a batch needs)."""
        from ..constants import ZFAR, ZNEAR
        jm, cm = sum(1 << j for j in self.active_j), sum(1 << k for k in self.active_c)
        r = self.engine.refine_bundle(self.mode, pose, q0, depth_t, _intr4(self.intrinsics), ZNEAR, ZFAR, jm, cm, self.limits,
                                      self.clip, self.iterations, self.damping)
        return self._result(r['pose'], r['angles'], r['offsets'], np.sqrt(r['var_pose']), np.sqrt(r['var_joints']), r['cost_before'], r['cost_after'],
                            r['steps'], r['inliers'], r['frame_cost'])
