"""Renderer with the reference's surface, drawn by the HIP engine.

Reference: robotpose/simulation/render.py:25-163 (pyrender scene of the six link meshes, an
intrinsics camera, SEG-flag offscreen render returning a flat-colour image and metric
depth).  Here `render()` is one rope_render call; colours come from the link-id image
through the same DEFAULT_RENDER_COLORS table.  `render_batch` draws many poses (and cameras) in one
rope_render_batch call; DatasetRenderer (render.py:167-187) is built on it.
"""
from typing import List, Tuple, Union

import numpy as np

from ..constants import (BACKGROUND_ID, DEFAULT_RENDER_COLORS, NUM_RENDER_LINKS,
                         RENDERER_FALLBACK_CAMERA_POSE, ZFAR, ZNEAR)
from ..engine import Engine
from ..projection import Intrinsics, camera_matrix, camera_pose_matrix, view_matrix
from ..robot import RobotModel
from ..urdf import URDFReader

_robot_cache = {}


def active_robot() -> RobotModel:
    """RobotModel of the active URDF, parsed and partitioned once per process."""
    reader = URDFReader()
    key = reader.path
    if key not in _robot_cache:
        _robot_cache[key] = RobotModel.from_urdf(reader)
    return _robot_cache[key]


def shade_depth(depth: np.ndarray, ids: np.ndarray, intr: Intrinsics, ambient: float = 0.12) -> np.ndarray:
    """Mode 'real' (render.py:92-98 without the SEG flag: the untextured meshes lit by one directional light that sits at the
    camera and shines along its view axis, render.py:57-59).  The reference's picture comes out of pyrender's physically based
    shader; this is the same scene with the simplest model of it — grey Lambert surface, head-on light, normals from the
    rendered depth (differences taken inside one link only, so silhouettes stay sharp) — for the viewers that show it to a
    person.  Nothing on the prediction path reads this image.  -> (H, W, 3) uint8."""
    H, W = depth.shape
    z = depth.astype(np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    X, Y = (u - intr.cx) / intr.fx * z, (v - intr.cy) / intr.fy * z
    P = np.stack([X, Y, z], -1)

    def diff(axis):
        fwd = np.roll(P, -1, axis) - P
        bwd = P - np.roll(P, 1, axis)
        ok_f = (np.roll(ids, -1, axis) == ids)
        ok_b = (np.roll(ids, 1, axis) == ids)
        edge = np.zeros(ids.shape, bool)
        if axis == 0:
            edge[-1, :] = True
            ok_f &= ~edge
            edge[:] = False
            edge[0, :] = True
            ok_b &= ~edge
        else:
            edge[:, -1] = True
            ok_f &= ~edge
            edge[:] = False
            edge[:, 0] = True
            ok_b &= ~edge
        return np.where(ok_f[..., None], fwd, np.where(ok_b[..., None], bwd, 0.0))
    n = np.cross(diff(1), diff(0))
    norm = np.linalg.norm(n, axis=-1)
    facing = np.where(norm > 0, np.abs(n[..., 2]) / np.where(norm > 0, norm, 1.0), 1.0)      # light along the view axis: |n . z|
    shade = np.clip(ambient + (1.0 - ambient) * facing, 0.0, 1.0)
    grey = np.where(ids != BACKGROUND_ID, np.round(200.0 * shade), 0.0).astype(np.uint8)
    return np.repeat(grey[..., None], 3, -1)


class Renderer:

    def __init__(self, mode: str = 'seg', camera_pose: np.ndarray = None,
                 camera_intrin: Union[str, Intrinsics] = '1280_720_color', suppress_warnings: bool = False,
                 intrinsic_ds_factor: int = None, device: int = 0):
        self.suppress_warnings = suppress_warnings
        self.intrinsics = Intrinsics(camera_intrin)
        if intrinsic_ds_factor is not None:
            self.intrinsics.downscale(intrinsic_ds_factor)
        self.robot = active_robot()
        self.engine = Engine(device)
        self.engine.set_robot(self.robot)
        self.limit_parts, self.limit_number = False, None
        self._angles = np.zeros(6)
        self.joint_names = list(self.robot.link_names)
        self.setCameraPose(camera_pose if camera_pose is not None else RENDERER_FALLBACK_CAMERA_POSE)
        self.setMode(mode)

    # -- scene state ----------------------------------------------------------------------------
    def setJointAngles(self, angles: List[float]):
        self._angles = np.asarray(angles, dtype=np.float64).reshape(6).copy()

    def setCameraPose(self, pose_in: np.ndarray):
        """Camera pose with the reference's pitch convention (render.py:107-111)."""
        self._camera_pose6 = np.asarray(pose_in, dtype=np.float64).copy()
        PV = camera_matrix(self._camera_pose6, self.intrinsics, ZNEAR, ZFAR)
        self.engine.set_camera(PV, self.intrinsics.width, self.intrinsics.height, ZNEAR, ZFAR)

    def setMode(self, mode: str):
        valid_modes = ['seg', 'seg_full', 'real']
        assert mode in valid_modes, f"Mode invalid; must be one of: {valid_modes}"
        self.mode = mode
        self._updateMode()

    def setMaxParts(self, number_of_parts: int):
        """Limit how many links are drawn (render.py:121-129)."""
        if number_of_parts is not None:
            self.limit_parts, self.limit_number = True, int(number_of_parts)
        else:
            self.limit_parts = False
        self._updateMode()

    def _updateMode(self):
        n = min(self.limit_number, NUM_RENDER_LINKS) if self.limit_parts else NUM_RENDER_LINKS
        self._n_render = n
        if self.mode == 'seg':
            self._colors = [DEFAULT_RENDER_COLORS[i] for i in range(n)]
        else:                                       # 'seg_full'; 'real' shades the surface instead of looking colours up
            self._colors = [DEFAULT_RENDER_COLORS[0]] * n
        lut = np.zeros((256, 3), np.uint8)
        for i, c in enumerate(self._colors):
            lut[i] = c
        lut[BACKGROUND_ID] = 0
        self._lut = lut

    # -- output -----------------------------------------------------------------------------------
    @property
    def n_render(self) -> int:
        return self._n_render

    def render_ids(self):
        """-> (depth float32 HxW, link ids uint8 HxW with 255 = background)."""
        return self.engine.render(self._angles, self._n_render)

    def render(self):
        """-> (colour uint8 HxWx3, depth float32 HxW), as pyrender's SEG pass (render.py:92-98)."""
        depth, ids = self.render_ids()
        if self.mode == 'real':
            return shade_depth(depth, ids, self.intrinsics), depth
        return self._lut[ids], depth

    def _views(self, camera_poses, n: int):
        """P·V per pose from camera_matrix, the one setCameraPose uses; None = the renderer's own camera."""
        if camera_poses is None:
            return None
        poses = np.asarray(camera_poses, dtype=np.float64).reshape(-1, 6)
        if len(poses) != n:
            raise ValueError(f"{len(poses)} camera poses for {n} joint vectors")
        return np.stack([camera_matrix(p, self.intrinsics, ZNEAR, ZFAR) for p in poses]) if n else np.zeros((0, 4, 4))

    def render_ids_batch(self, angles, camera_poses=None, crop=None):
        """N poses, each under its own camera pose (the renderer's when None), in one rope_render_batch call: what N rounds of
        setJointAngles [+ setCameraPose] + render_ids give.  The renderer's own angles and camera stay as they were.
        -> (depths float32 (N, h, w), link ids uint8 (N, h, w)), h x w the crop (whole frame when None)."""
        angles = np.asarray(angles, dtype=np.float64).reshape(-1, 6)
        return self.engine.render_batch(angles, self._n_render, self._views(camera_poses, len(angles)), crop)

    def render_ids_batch_device(self, angles, camera_poses=None):
        """render_ids_batch of the whole frame with the planes left on the GPU (rope_render_batch_device), each pose under its own
        camera pose (the renderer's when None)
        -> (depths float32 (N, H, W), link ids uint8 (N, H, W)) as torch tensors on the engine's device."""
        angles = np.asarray(angles, dtype=np.float64).reshape(-1, 6)
        return self.engine.render_batch_device(angles, self._n_render, self._views(camera_poses, len(angles)))

    def render_photo_batch_device(self, angles, camera_poses=None, params=None, backgrounds=None, frame0: int = 0, seed: int = 0):
        """N poses as photographs, made on the GPU: render_ids_batch_device followed by rope_shade_frames (csrc/rope_shade.hip) —
        the surface lit by one directional light with normals from the rendered depth, a colour per link, a background picture or
        colour, sensor noise, and a depth map with a plane behind the robot.  params: N records (simulation/shading.py:
        default_params when None, which is shade_depth's scene); backgrounds: (n_bg, H, W, 3) uint8, a torch tensor on the engine's
        device or a numpy array (uploaded here), None when every record's bg_index is -1.  Plane m takes the noise of frame
        frame0 + m of `seed`.  Mode 'real', render and render_batch are not touched by this.
        -> (bgr uint8 (N, H, W, 3), depth float32 (N, H, W), ids uint8 (N, H, W)) torch tensors on the engine's device."""
        import torch
        from .shading import default_params
        depth, ids = self.render_ids_batch_device(angles, camera_poses)
        if params is None:
            params = default_params(len(depth), self._n_render)
        if backgrounds is not None and not isinstance(backgrounds, torch.Tensor):
            backgrounds = torch.from_numpy(np.ascontiguousarray(backgrounds, np.uint8)).to(depth.device)
        intr = self.intrinsics
        bgr, depth = self.engine.shade_frames(depth, ids, params, (intr.fx, intr.fy, intr.cx, intr.cy), self._n_render, backgrounds, frame0,
                                              seed, depth_out=depth)
        return bgr, depth, ids

    def render_photo_batch(self, angles, camera_poses=None, params=None, backgrounds=None, frame0: int = 0, seed: int = 0):
        """render_photo_batch_device with the three stacks copied down -> numpy (bgr, depth, ids)."""
        return tuple(t.cpu().numpy() for t in self.render_photo_batch_device(angles, camera_poses, params, backgrounds, frame0, seed))

    @property
    def blue_of_id(self) -> np.ndarray:
        """Channel 0 of the colour every link id is drawn in (256 bytes, the background's included): render()'s colour image has
        blue_of_id[ids] as its first channel."""
        return np.ascontiguousarray(self._lut[:, 0])

    def render_batch(self, angles, camera_poses=None):
        """-> (colours uint8 (N, H, W, 3), depths float32 (N, H, W)): render() for every pose (and camera pose) in one batch."""
        depth, ids = self.render_ids_batch(angles, camera_poses)
        if self.mode == 'real':
            color = np.empty(ids.shape + (3,), np.uint8)
            for k in range(len(ids)):
                color[k] = shade_depth(depth[k], ids[k], self.intrinsics)
            return color, depth
        return self._lut[ids], depth

    def render_masks_batch(self, angles, camera_poses=None, pad: int = 3):
        """Label bit planes of N poses (each under its own camera pose, the renderer's when None) in rope_render_masks calls:
        bit i is the i-th label of color_dict ('seg': link i; 'seg_full': every link is 'robot'), dilated by a pad x pad window
        as Annotator._mask_color does.  The renderer's own angles and camera stay as they were.
        -> (masks uint8 (N, H, W), boxes int32 (N, 8, 4) {r0, r1, c0, c1} per bit, -1 when empty)."""
        if self.mode == 'real':
            raise ValueError("render_masks_batch: mode 'real' has no labels")
        angles = np.asarray(angles, dtype=np.float64).reshape(-1, 6)
        labels = np.arange(self._n_render, dtype=np.uint8) if self.mode == 'seg' else np.zeros(self._n_render, np.uint8)
        return self.engine.render_masks(angles, self._n_render, labels, pad, self._views(camera_poses, len(angles)))

    @property
    def resolution(self) -> Tuple[int]:
        return (self.intrinsics.height, self.intrinsics.width)

    @property
    def camera_pose(self) -> np.ndarray:
        return camera_pose_matrix(self._camera_pose6)

    @property
    def color_dict(self) -> dict:
        if self.mode == 'seg':
            return {name: color for name, color in zip(self.joint_names[:self._n_render], self._colors)}
        return {'robot': DEFAULT_RENDER_COLORS[0]}


class DatasetRenderer(Renderer):
    """Renders a dataset's frames at their recorded joint angles and camera poses (render.py:167-187).  `dataset` is a name
    (open_dataset: 'synthetic:...' and 'photo:...' names too) or an opened Dataset / SyntheticDataset.  render_range / render_indices draw many
    frames in one batch, each under its own camera pose."""

    def __init__(self, dataset, mode: str = 'seg', camera_pose: np.ndarray = None):
        from ..data.dataset import open_dataset
        self.ds = open_dataset(dataset) if isinstance(dataset, str) else dataset
        self._ds_angles = np.asarray(self.ds.angles[:], dtype=np.float64).reshape(-1, 6)
        self._ds_poses = np.asarray(self.ds.camera_pose[:], dtype=np.float64).reshape(-1, 6)
        if camera_pose is None:
            camera_pose = self._ds_poses[0]
        super().__init__(mode, camera_pose, str(self.ds.attrs['color_intrinsics']))

    def render_at(self, idx: int):
        """Render one frame of the dataset at its own joint angles and camera pose."""
        self.setPosesFromDS(idx)
        return self.render()

    def setPosesFromDS(self, idx: int):
        """Set the robot and camera poses to those of frame idx."""
        self.setJointAngles(self._ds_angles[idx])
        self.setCameraPose(self._ds_poses[idx])

    def render_indices(self, idx):
        """-> (colours (N, H, W, 3), depths (N, H, W)) of the frames idx, each at its own angles and camera pose, in one batch;
        the renderer's own pose stays as it was."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        return self.render_batch(self._ds_angles[idx], self._ds_poses[idx])

    def render_range(self, start: int, stop: int):
        """render_indices(range(start, stop))."""
        return self.render_indices(np.arange(start, stop))

    def close(self):
        """Release the dataset and the engine context."""
        ds, self.ds = getattr(self, 'ds', None), None
        if ds is not None:
            ds.close()
        eng = getattr(self, 'engine', None)
        if eng is not None:
            eng.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
