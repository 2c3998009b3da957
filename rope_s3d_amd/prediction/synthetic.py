"""Synthetic self-consistency harness (reference: robotpose/prediction/synthetic.py:11-75).

Render the robot at a known pose, feed colour+depth to the Predictor in synthetic mode
(link masks read from the colour image), compare predicted with actual.
"""
import numpy as np

from ..simulation.noise import NoiseMaker
from ..simulation.render import Renderer
from ..urdf import URDFReader
from ..utils import str_to_arr
from .predict import Predictor


class SyntheticPredictor:

    def __init__(self, camera_pose, base_intrin, ds_factor, do_angles, noise, *, device: int = 0, seed: int = None,
                 lookup_divisions=None, refine: bool = False):
        self.renderer = Renderer(camera_pose=camera_pose, camera_intrin=base_intrin, device=device)
        self.predictor = Predictor(camera_pose, ds_factor, do_angles=do_angles, base_intrin=base_intrin,
                                   color_dict=self.renderer.color_dict, device=device,
                                   lookup_divisions=lookup_divisions, refine=refine)
        self.urdf_reader = URDFReader()
        self.do_angles = do_angles
        self.rng = np.random.default_rng(seed)
        self.noise = NoiseMaker(self.rng)
        self.do_noise = noise

    def run(self, pose=None):
        if pose is None:
            pose = self._generatePose()
        self.renderer.setJointAngles(pose)
        color, depth = self.renderer.render()
        if self.do_noise:
            depth = self.noise.holes(depth)
        predicted = self.predictor.run(color, depth)
        return pose, predicted

    def _generatePose(self):
        lim = self.urdf_reader.joint_limits
        return self.rng.uniform(lim[:, 0], lim[:, 1]) * str_to_arr(self.do_angles)

    def run_batch(self, number: int, file: str = 'synth_test', batch: int = None):
        return self.run_batch_poses([None] * number, file, batch)

    SUB_BATCH = 16     # batched runs: frames per render / holes / staging call (full-size planes: 74 MB at 1280x720)

    def _batched_ok(self) -> bool:
        """The batched path takes this run: frames may walk the stages in lockstep, the down-sampling is the four-tap one, the
        colour image is the link colours of mode 'seg' (which the predictor knows all of), and both contexts are on one device."""
        p, r, f = self.predictor, self.renderer, int(self.predictor.ds_factor)
        return p._batch_ok() and p.synthetic and (f == 1 or (f > 1 and f % 2 == 0)) and r.mode == 'seg' and \
            all(k in p.color_dict for k in p.link_names) and r.engine.device == p.engine.device and \
            r.engine.H == p.engine.H * f and r.engine.W == p.engine.W * f

    def run_batch_poses(self, poses, file: str = 'synth_test', batch: int = None):
        """Without `batch`: run() pose after pose.  With it, groups of up to `batch` frames stay on the GPU from the render to the
        prediction: rendered on the renderer's context into device planes, holed there (do_noise: Engine.depth_holes, its own random
        stream and float32 planes, where run() hands the predictor NoiseMaker's float64), turned into the predictor context's staged
        targets (Engine.stage_targets_synthetic) and predicted in lockstep (rope_predict_batch).  Without noise the angles are those
        of the loop on the same poses."""
        if not file.endswith('.npy'):
            file += '.npy'
        if batch is not None and int(batch) >= 1 and len(poses) and self._batched_ok():
            return self._run_batched(poses, file, int(batch))
        results = np.zeros((2, len(poses), 6))            # [actual, predicted]
        for i in range(len(poses)):
            results[0, i], results[1, i] = self.run(poses[i])
            if i % 250 == 0:                               # periodic partial save (synthetic.py:57-58)
                np.save(file, results)
        np.save(file, results)
        return results

    def _run_batched(self, poses, file: str, batch: int):
        from ..constants import LOOKUP_NUM_RENDERED
        p, r = self.predictor, self.renderer
        n = len(poses)
        seed = int(self.rng.integers(0, 1 << 64, dtype=np.uint64)) if self.do_noise else 0     # before the poses: one seed per run
        actual = np.array([self._generatePose() if q is None else np.asarray(q, dtype=np.float64).reshape(6) for q in poses]).reshape(n, 6)
        results = np.zeros((2, n, 6))
        results[0] = actual
        p._setStages()
        want_ts = p._has_tsweep() or p.refine            # refine: the whole reduced depth stays beside the targets, for the polish
        f = int(p.ds_factor)
        polished = []
        blue_of_id, link_blue = r.blue_of_id, [int(p.color_dict[k][0]) for k in p.link_names]
        for lo in range(0, n, batch):
            hi = min(lo + batch, n)
            for j0 in range(lo, hi, self.SUB_BATCH):
                j1 = min(j0 + self.SUB_BATCH, hi)
                depth_t, ids_t = r.render_ids_batch_device(actual[j0:j1])
                if self.do_noise:
                    r.engine.depth_holes(depth_t, seed, frame0=j0)       # frame index = position in the run
                p.engine.stage_targets_synthetic(depth_t, ids_t, f, blue_of_id, link_blue, LOOKUP_NUM_RENDERED, hi - lo, j0 - lo, want_ts)
            p.engine.commit_targets()
            results[1, lo:hi] = p._run_resident(hi - lo)
            if p.refine:
                results[1, lo:hi] = p._polish(results[1, lo:hi], p.engine.resident_depth())
                polished.append(p.last_refinement)
            np.save(file, results)                          # one save per group
        if p.refine:
            from .refinement import RefineResult
            p.last_refinement = RefineResult.concatenate(polished)
        return results
