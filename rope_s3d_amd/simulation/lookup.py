"""Lookup pose grids (reference: robotpose/simulation/lookup.py:30-106,184-316).

The reference pre-renders the grid into an HDF5 table of cropped depth images and scores a
frame against it with TensorFlow.  The engine renders and scores the grid on the fly
(ROPE_LOSS_LOOKUP), so the prediction path only needs the same grid, in the same order, with
the same size rule.  RobotLookupCreator still writes the reference's table file, rendered in
batches (rope_render_batch) with only the crop coming back from the device.
"""
from typing import Union

import numpy as np

from ..constants import GPU_MEMORY_ALLOWED_FOR_LOOKUP, LOOKUP_MAX_DIV_PER_LINK
from ..utils import str_to_arr
from .render import Renderer

# The reference sizes the table from the GPU's VRAM read through nvidia-smi (utils.py:21-37):
# bits = MiB * 8.389e6.  nvidia-smi does not exist here, so the budget is explicit; the default
# is the 8 GiB class of card the reference was configured on (crop.py:121 "GTX 1070").
DEFAULT_LOOKUP_VRAM_MIB = 8192


def lookup_grid(joint_limits: np.ndarray, varying: Union[str, np.ndarray], divisions) -> np.ndarray:
    """Grid of joint vectors, joint 0 varying fastest (lookup.py:39-66)."""
    varying = str_to_arr(varying) if isinstance(varying, str) else np.asarray(varying, bool)
    divisions = np.clip(np.array(divisions, dtype=int), 0, LOOKUP_MAX_DIV_PER_LINK)
    divisions[~varying] = 1
    num = int(np.prod(divisions))
    angles = np.zeros((num, 6))
    for idx in np.where(varying)[0]:
        rng = np.linspace(joint_limits[idx, 0], joint_limits[idx, 1], divisions[idx])
        repeat = int(np.prod(divisions[:idx]))
        tile = num // (repeat * divisions[idx])
        angles[:, idx] = np.tile(np.repeat(rng, repeat), tile)
    return angles


def default_divisions(crop_size: int, varying: Union[str, np.ndarray], vram_mib: float = DEFAULT_LOOKUP_VRAM_MIB,
                      element_bits: int = 32) -> np.ndarray:
    """Equal split of the pose budget over the varying joints (lookup.py:224-225,266-274)."""
    varying = str_to_arr(varying) if isinstance(varying, str) else np.asarray(varying, bool)
    max_elements = int(vram_mib * 8.389e6 * GPU_MEMORY_ALLOWED_FOR_LOOKUP)
    max_poses = max_elements / (crop_size * element_bits)
    divisions = np.zeros(6, int)
    divisions[varying] = int(max_poses ** (1 / sum(varying)))
    return divisions


class RobotLookupManager:
    """`get` keeps the reference's call shape but returns (angles, None): there is no table."""

    def __init__(self, joint_limits: np.ndarray, element_bits: int = 32):
        self.joint_limits = joint_limits
        self.element_bits = element_bits

    def get(self, crop_size: int, varying_angles: Union[str, np.ndarray], max_poses: int = None,
            divisions: np.ndarray = None, vram_mib: float = DEFAULT_LOOKUP_VRAM_MIB):
        assert not (max_poses is not None and divisions is not None), "give at most one of max_poses / divisions"
        varying = str_to_arr(varying_angles) if isinstance(varying_angles, str) else np.asarray(varying_angles, bool)
        if divisions is None:
            if max_poses is not None:
                divisions = np.zeros(6, int)
                divisions[varying] = int(max_poses ** (1 / sum(varying)))
            else:
                divisions = default_divisions(crop_size, varying, vram_mib, self.element_bits)
        return lookup_grid(self.joint_limits, varying, divisions), None


def write_lookup_file(file_name: str, angles: np.ndarray, depth: np.ndarray, pose, intrinsics: str, num_links_rendered: int,
                      angles_changed, divisions, urdf: str) -> str:
    """The reference's lookup file (lookup.py:88-106): attrs pose, intrinsics, num_links_rendered, angles_changed (a bool array,
    stored as integers), divisions, urdf; datasets `angles` and `depth` (float64, gzip level 1)."""
    from ..data import hdf5
    attrs = {'pose': np.asarray(pose, np.float64), 'intrinsics': str(intrinsics), 'num_links_rendered': int(num_links_rendered),
             'angles_changed': np.asarray(angles_changed, bool), 'divisions': np.asarray(divisions, np.int64), 'urdf': str(urdf)}
    return hdf5.write_arrays(file_name, {'angles': np.asarray(angles, np.float64), 'depth': np.asarray(depth, np.float64)},
                             attrs=attrs, gzip={'depth': 1})


class RobotLookupCreator(Renderer):
    """Renders a joint grid and writes its cropped depth table to HDF5 (lookup.py:30-106).  preview=True opens no window."""

    # poses per rope_render_batch call: bounds the host block of one call
    BATCH = 4096

    def __init__(self, camera_pose: np.ndarray, intrinsics):
        from ..crop import Crop
        from ..urdf import URDFReader
        self.inp_pose = camera_pose
        self.u_reader = URDFReader()
        super().__init__('seg', camera_pose=camera_pose, camera_intrin=intrinsics)
        self.croppper = Crop(camera_pose, self.intrinsics, renderer=self)

    def load_config(self, joints_to_render: int, angles_to_do: Union[str, np.ndarray], divisions: np.ndarray):
        """Load the specification of the table: links drawn, joints varied, divisions per joint."""
        self.num_rendered = joints_to_render
        self.setMaxParts(joints_to_render)
        self.crop = self.croppper[joints_to_render]
        self.angles_to_do = str_to_arr(angles_to_do) if isinstance(angles_to_do, str) else np.asarray(angles_to_do, bool)
        self.divisions = np.clip(np.array(divisions), 0, LOOKUP_MAX_DIV_PER_LINK)
        self.divisions[~self.angles_to_do] = 1
        self.num = int(np.prod(self.divisions))
        self.angles = lookup_grid(self.u_reader.joint_limits, self.angles_to_do, self.divisions)

    def _render_depth(self, crop=None) -> np.ndarray:
        H, W = self.resolution
        h, w = (H, W) if crop is None else (int(crop[1]) - int(crop[0]) + 1, int(crop[3]) - int(crop[2]) + 1)
        out = np.empty((self.num, h, w))
        for s in range(0, self.num, self.BATCH):
            depth, _ = self.engine.render_batch(self.angles[s:s + self.BATCH], self.n_render, crop=crop, ids=False)
            out[s:s + len(depth)] = depth
        return out

    def _generate_depth_array(self, preview: bool = False) -> np.ndarray:
        """Full-frame float64 depth, one image per grid pose (preview: no window here)."""
        return self._render_depth()

    def run(self, file_name: str, preview: bool = False):
        """Create a new lookup file: the crop of every grid pose's depth."""
        depth = self._render_depth(self.crop)
        return write_lookup_file(file_name, self.angles, depth, self.inp_pose, str(self.intrinsics), self.num_rendered,
                                 self.angles_to_do, self.divisions, self.u_reader.name)
