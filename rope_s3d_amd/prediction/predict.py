"""Joint-angle prediction by render-and-compare, driven from Python, evaluated on the GPU.

`Predictor` keeps the reference's constructor and `run` signature
(robotpose/prediction/predict.py:37-48,127,375) so predict_dataset.py / predict_live.py /
SyntheticPredictor call it unchanged.  The stage machine runs in the library (rope_predict,
csrc/rope_predict.cpp) and follows the reference's control flow decision for decision,
quirks included; what changes is how a candidate is evaluated: every `render_at_pos` +
`_error` pair of the reference (predict.py:159-161,475-509) becomes one row of a batch
handed to the HIP engine, which does FK, rasterisation and the error reduction on the device.
"""
import os
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from ..config import Paths
from ..constants import DEFAULT_CAMERA_POSE, DEFAULT_RENDER_COLORS, LOOKUP_JOINTS, LOOKUP_NUM_RENDERED
from ..crop import Crop
from ..engine import (STAGE_DESCENT, STAGE_ISWEEP, STAGE_LOOKUP, STAGE_SFLIP, STAGE_TSWEEP, StageDesc, pack_target, prepare_segmented,
                      prepare_synthetic)
from ..imgproc import dilate, erode, resize_linear
from ..projection import Intrinsics
from ..simulation.lookup import RobotLookupManager
from ..simulation.render import Renderer
from ..urdf import URDFReader
from .stages import Descent, InterpolativeSweep, Lookup, SFlip, TensorSweep, getStages

HISTORY_LENGTH = 5      # predict.py:30


def cubic_interp(x: np.ndarray, y: np.ndarray, xq: np.ndarray) -> np.ndarray:
    """interp1d(x, y, kind='cubic')(xq) — the not-a-knot cubic spline of predict.py:310.

    scipy (the reference's own dependency) is used when importable; otherwise the same spline
    is solved directly."""
    try:
        from scipy.interpolate import interp1d
        return interp1d(x, y, kind='cubic')(xq)
    except ImportError:
        return _not_a_knot(np.asarray(x, float), np.asarray(y, float), np.asarray(xq, float))


def _not_a_knot(x, y, xq):
    n = len(x)
    h = np.diff(x)
    A = np.zeros((n, n))
    r = np.zeros(n)
    for i in range(1, n - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2 * (h[i - 1] + h[i]), h[i]
        r[i] = 6 * ((y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1])
    A[0, 0], A[0, 1], A[0, 2] = h[1], -(h[0] + h[1]), h[0]
    A[-1, -3], A[-1, -2], A[-1, -1] = h[-1], -(h[-2] + h[-1]), h[-2]
    M = np.linalg.solve(A, r)
    i = np.clip(np.searchsorted(x, xq, side='right') - 1, 0, n - 2)
    t0, t1 = xq - x[i], x[i + 1] - xq
    return (M[i] * t1 ** 3 + M[i + 1] * t0 ** 3) / (6 * h[i]) + (y[i] / h[i] - M[i] * h[i] / 6) * t1 \
        + (y[i + 1] / h[i] - M[i + 1] * h[i] / 6) * t0


@dataclass
class PreparedTarget:
    """One frame as the engine takes it (Predictor.prepare): everything _load_target caches in the reference."""
    tgt_depth: np.ndarray          # (H, W) float64, body-masked on the segmentation path
    lookup_f32: np.ndarray         # (H, W) float32 depth under the lookup links
    target_masks: dict             # link name -> bool mask
    tq: np.ndarray                 # packed uint64 plane (engine.pack_target)
    flags: np.ndarray              # (8,) uint8 per-link flags
    links_image: Optional[np.ndarray] = None     # what the preview shows as "detected links"


def segment_targets(seg: dict, target_depth: np.ndarray, lookup_links) -> np.ndarray:
    """Depth masking of the segmentation path (predict.py:419-438).

    Zeroes `target_depth` IN PLACE outside erode7(dilate8(sum of all link masks)) and returns the lookup
    depth: a copy further restricted to the links the lookup table renders."""
    def body(keys):
        new = np.zeros(target_depth.shape)
        for k in keys:
            new += seg[k]['mask']
        return erode(dilate(new, 8), 7).astype(bool).astype(float)

    target_depth *= body(seg.keys())
    lookup_depth = target_depth.copy()
    lookup_depth *= body([k for k in seg if k in lookup_links])
    return lookup_depth


def preview_rows(sflip: bool, rows: np.ndarray, limits: np.ndarray) -> np.ndarray:
    """The poses the reference renders for one scored batch of a stage (rope_predict's on_eval), in its order: the rows
    themselves, and in an SFlip batch also the pose the reference renders at the lower limit only to overwrite its error
    (predict.py:270-277), which the library does not ask for.  The library's SFlip batch is [angles, flipped (in limits),
    upper endpoint (out of or within 0.15 of a limit)]: the last row's S angle is the upper limit exactly when the endpoint
    branch ran (a last row that is the flipped pose lies at least 0.15 inside it), and the lower endpoint goes before it."""
    if not sflip or rows[-1][0] != limits[0][1]:
        return rows
    lower = rows[-1].copy()
    lower[0] = limits[0][0]
    return np.vstack([rows[:-1], lower, rows[-1:]])


class _BatchTraces:
    """Per-stage traces of a lockstep batch, frame by frame, as run() keeps them for one frame: entry f is
    [(stage name, angles after the stage), ...].  Built when asked for — a batch of 512 frames is 4 600 small arrays."""

    def __init__(self, trace: np.ndarray, names):
        self._trace, self._names = trace, list(names)

    def __len__(self):
        return len(self._trace)

    def __getitem__(self, f):
        if isinstance(f, slice):
            return [self[i] for i in range(*f.indices(len(self)))]
        return [(name, self._trace[f, i].copy()) for i, name in enumerate(self._names)]

    def __iter__(self):
        return (self[f] for f in range(len(self)))


class Predictor:

    SPECULATE = 3      # joints of a Descent iteration evaluated as one batch (1 = the reference's two renders at a time)
    SPECULATE_BATCH = 1     # the same for a lockstep batch of SPECULATE_BATCH_FROM frames or more: with hundreds of frames in every device
    SPECULATE_BATCH_FROM = 16   # batch the GPU is full anyway, and the reference's own order — one joint's under/over pair at a time, 2 rows
                            # per frame instead of 26 — renders a third of the poses (5 550 against 3 220 frames/s at the defaults)
    NATIVE_PREPARE = True   # synthetic path: prepare() as one pass in the library (rope_prepare_synthetic); False: the numpy steps, same arrays
    BATCH = None       # run_many: frames that walk the stage list in lockstep, every step one device batch over all of them
                       # (rope_predict_batch).  None: as many as fit BATCH_BYTES of target planes, 16..1024 (1024 at 160x90,
                       # 582 at 640x480, 194 at 1280x720); 1: frame after frame (rope_predict).  Same angles either way.
    PREPARE_WORKERS = int(os.environ.get('ROPE_PREPARE_WORKERS', '8'))   # run_many: most threads that prepare the frames of the next batches
    BATCH_BYTES = 2 << 30   # two page-locked sets of this size on the host and two on the device (288 GB of HBM: a batch is small
                            # change).  The more frames per batch, the shorter its tail of stragglers weighs: at the defaults
                            # the stage machine alone does 8 540 frames/s with 512, 9 320 with 1 024, 10 340 with 2 048

    def __init__(self,
                 camera_pose: np.ndarray = DEFAULT_CAMERA_POSE,
                 ds_factor: int = 8,
                 preview: bool = False,
                 save_to: str = None,
                 do_angles: str = 'SLU',
                 min_angle_inc: np.ndarray = np.array([.005] * 6),
                 base_intrin: str = '1280_720_color',
                 model_ds: str = 'set10',
                 color_dict: dict = None,
                 *,
                 device: int = 0,
                 segmenter: Optional[Callable] = None,
                 lookup_divisions=None,
                 lookup_table_budget: int = 32 << 30,
                 reference_table_aliasing: bool = False,
                 device_targets: bool = False,
                 refine: bool = False):
        """Reference parameters as in predict.py:38-70.  Extra keyword-only arguments:

        device            HIP device ordinal of the engine context
        segmenter         callable(colour uint8 HxWx3) -> {'class_ids', 'scores', 'masks' (H,W,K) bool};
                          stands in for pixellib's segmentImage (predict.py:416) when color_dict is None
        lookup_divisions  explicit lookup grid divisions (six ints or one int for every lookup joint);
                          default: the reference's size rule with an 8 GiB budget (simulation/lookup.py)
        lookup_table_budget  bytes of HBM the stored lookup table may take (default 32 GiB); larger grids are
                          rendered and scored on the fly every frame instead
        reference_table_aliasing  the reference's own behaviour over a SEQUENCE of frames, opt-in: its Lookup stage returns a
                          numpy view of a row of the angle table (predict.py:171) and Descent then steps that row in place
                          (predict.py:212-215), so the table drifts and a frame's answer depends on the frames before it
                          (until the camera pose changes: _loadLookup reloads the table).  Default False: every frame starts
                          from the grid itself, frames are independent — which is what sharding over GPUs needs.  With True,
                          use ONE Predictor and feed it the frames in the reference's order.
        device_targets    run_many on the segmentation path with a segmenter that offers `batch_device(frames)` (MaskRCNNSegmenter:
                          the instance masks stay on the GPU): the targets are built there as well (rope_stage_targets_segmented)
                          instead of on the host from a copy of the masks.  Same planes, bit for bit, hence the same angles.
                          Without such a segmenter, and in run() / prepare(), the flag changes nothing.
        refine            polish the stages' answer with a few Gauss-Newton steps on the depth residual against the frame's depth at
                          the working resolution (prediction/refinement.py: PoseRefiner over do_angles), in run, run_batch and
                          run_many; the RefineResult of the last call — one row per frame, with the formal sigma of every angle — is
                          left in `last_refinement`.  Off by default: the stages, their trace and their angles are untouched.
                          On the segmentation path the polish sees the body-masked depth (PreparedTarget.tgt_depth); with
                          device_targets it sees the reduced depth before masking, since the mask never leaves the device — so
                          there the two run_many paths give the same stage angles but may polish them differently.
                          'native': the same polish through rope_refine_poses (PoseRefiner(native=True)): the loop, the solves and
                          the sigmas inside the library instead of on the host.  True keeps the host loop.
        """
        self.device_targets = bool(device_targets)
        self.refine, self.last_refinement, self._refiner = bool(refine), None, None
        self.refine_native = isinstance(refine, str) and refine == 'native'
        if isinstance(refine, str) and not self.refine_native:
            raise ValueError(f"refine: False, True or 'native', got {refine!r}")
        self.ds_factor, self.preview = ds_factor, preview
        if preview:                       # headless: frames go to .viz.frame and, with save_to, an uncompressed AVI
            from .viz import ProjectionViz
            self.viz = ProjectionViz(save_to)
            self.SPECULATE = 1            # show exactly the renders the reference's serial descent would look at
        self.do_angles = do_angles.upper()
        self.min_ang_inc, self.history_length = np.asarray(min_angle_inc, dtype=float), HISTORY_LENGTH

        self.intrinsics = Intrinsics(base_intrin)
        self.intrinsics.downscale(ds_factor)
        self.u_reader = URDFReader()
        self.renderer = Renderer('seg', camera_pose, self.intrinsics, device=device)
        self.engine = self.renderer.engine

        self.synthetic = color_dict is not None
        self.classes = ["BG"]
        self.classes.extend(self.u_reader.mesh_names[:6])
        self.link_names = self.classes[1:]

        if self.synthetic:
            self.color_dict = color_dict
        else:
            self.model_ds = model_ds
            self.seg = segmenter if segmenter is not None else self._load_segmenter(model_ds, device)
        self._lookup_divisions = lookup_divisions
        self.lookup_table_budget = int(lookup_table_budget)
        self.reference_table_aliasing = bool(reference_table_aliasing)
        self.camera_pose = None
        self.changeCameraPose(camera_pose)
        self.evaluations = 0          # candidates rendered+scored, for throughput accounting

    def _load_segmenter(self, model_ds: str, device: int):
        """The reference's default: the newest model trained on `model_ds` (ModelManager().dynamicLoad(dataset=model_ds),
        predict.py:94-98), as the torch Mask R-CNN with those weights.  None when no trained model is on disk — run()
        then asks for a segmenter instead of guessing."""
        from ..models import ModelManager
        path = ModelManager().dynamicLoad(dataset=model_ds)
        if path is None:
            return None
        from ..maskrcnn import MaskRCNNSegmenter, load_matterport_weights
        return MaskRCNNSegmenter(len(self.classes), device=f'cuda:{device}', state_dict=load_matterport_weights(path, len(self.classes)))

    # ------------------------------------------------------------------ camera / lookup grid
    def changeCameraPose(self, camera_pose):
        self.camera_pose = np.asarray(camera_pose, dtype=float).copy()
        self.renderer.setCameraPose(self.camera_pose)
        self.crops = Crop(self.camera_pose, self.intrinsics, renderer=self.renderer)
        self._loadLookup()

    def _loadLookup(self):
        lm = RobotLookupManager(self.u_reader.joint_limits)
        div = self._lookup_divisions
        if div is not None and np.ndim(div) == 0:
            from ..utils import str_to_arr
            d = np.zeros(6, int)
            d[str_to_arr(LOOKUP_JOINTS)] = int(div)
            div = d
        self.lookup_angles, _ = lm.get(self.crops.size(LOOKUP_NUM_RENDERED), LOOKUP_JOINTS, divisions=div)
        self.lookup_crop = np.asarray(self.crops[LOOKUP_NUM_RENDERED], dtype=np.int32)
        # reference_table_aliasing: the table the reference's run() edits; the grid itself stays what the depth table
        # was rendered from (the reference's .h5 depths never change either)
        self._lookup_live = np.ascontiguousarray(self.lookup_angles, np.float64).copy() if self.reference_table_aliasing else None
        # The reference keeps the grid as a table of cropped depth images (lookup.py:92-106) and takes its square
        # root once (predict.py:117).  Same here, in HBM, when it fits the budget; otherwise every frame renders
        # and scores the grid on the fly (identical scores either way).
        c = self.lookup_crop
        table_bytes = len(self.lookup_angles) * int(c[1] - c[0] + 1) * int(c[3] - c[2] + 1) * 4
        self._lookup_table = table_bytes <= self.lookup_table_budget
        if self._lookup_table:
            self.engine.lookup_build(self.lookup_angles, LOOKUP_NUM_RENDERED, self.lookup_crop)

    def _setStages(self):
        self.stages = getStages(self.do_angles)
        if self.stages is None:
            raise ValueError(f"Stages not defined for joint set {self.do_angles}. "
                             "Please define in rope_s3d_amd/prediction/stages.py.")

    def _native_stages(self):
        """self.stages as rope_stage descriptors (include/rope_s3d.h).  ValueError for a stage the reference could not run
        either (a cubic through fewer than 4 sweep samples, predict.py:310; a TensorSweep without samples)."""
        nan = float('nan')
        out = (StageDesc * len(self.stages))()
        for d, stage in zip(out, self.stages):
            d.init_rate[:] = [nan] * 6
            d.range = nan
            if type(stage) is Lookup:
                d.kind, d.to_render = STAGE_LOOKUP, LOOKUP_NUM_RENDERED
                continue
            if type(stage) is SFlip:
                d.kind, d.to_render = STAGE_SFLIP, stage.to_render
                continue
            d.joints = sum(1 << j for j in range(6) if stage.joints[j])
            if type(stage) is Descent:
                d.kind, d.to_render, d.count = STAGE_DESCENT, stage.to_render, stage.its
                d.init_rate[:] = [nan if r is None else float(r) for r in stage.init_rate]
                d.rate_reduction, d.early_stop = stage.rate_redux, stage.early_stop
            elif type(stage) is InterpolativeSweep:
                if stage.divs < 4:
                    raise ValueError(f"InterpolativeSweep needs at least 4 divisions, got {stage.divs}")
                d.kind, d.to_render, d.count = STAGE_ISWEEP, stage.to_render, stage.divs
                d.range = nan if stage.range is None else float(stage.range)
            elif type(stage) is TensorSweep:
                if stage.divs < 1:
                    raise ValueError(f"TensorSweep needs at least 1 division, got {stage.divs}")
                d.kind, d.to_render, d.count = STAGE_TSWEEP, stage.to_render, stage.divs
                d.range = nan if stage.range is None else float(stage.range)
            else:
                raise ValueError(f"no stage kind of the library for {type(stage).__name__}")
        return out

    def _has_tsweep(self) -> bool:
        return any(type(stage) is TensorSweep for stage in self.stages)

    # ------------------------------------------------------------------ target preparation
    def _downsample(self, base: np.ndarray, factor: int) -> np.ndarray:
        h, w = base.shape[0] // factor, base.shape[1] // factor
        return resize_linear(base, w, h)                # cv2.resize(base, (w, h)), predict.py:378-381

    def _reorganize_by_link(self, data: dict) -> dict:
        """Merge instances of one class: OR the masks, keep the best score (predict.py:383-395)."""
        out = {}
        ids = list(data['class_ids'])
        for idx, cid in enumerate(ids):
            name = self.classes[cid]
            if cid not in ids[:idx]:
                out[name] = {'confidence': data['scores'][idx], 'mask': np.array(data['masks'][..., idx], dtype=bool)}
            else:
                out[name]['mask'] = out[name]['mask'] | np.asarray(data['masks'][..., idx], dtype=bool)
                out[name]['confidence'] = max(out[name]['confidence'], data['scores'][idx])
        return out

    def _pack_target(self, tgt_depth: np.ndarray, lookup_depth: np.ndarray, masks: dict, links_image=None) -> PreparedTarget:
        """What _load_target caches in the reference (predict.py:397-413), as one packed plane + per-link flags.
        Host work only: nothing of the Predictor or the engine changes here."""
        lookup_f32 = np.ascontiguousarray(lookup_depth, dtype=np.float32)
        target_masks = {}
        bits = np.zeros(tgt_depth.shape, np.uint8)
        flags = np.zeros(8, np.uint8)
        has_depth = tgt_depth != 0
        for l, link in enumerate(self.link_names):
            if link in masks:
                m = np.asarray(masks[link], dtype=bool)
                target_masks[link] = m
                bits |= m.view(np.uint8) << np.uint8(l)
                flags[l] |= 1
                # predict.py:495: np.sum(mask * depth != 0) > .05 * np.sum(mask), a target-only fact (counted, not multiplied)
                if np.count_nonzero(m & has_depth) > (.05 * np.count_nonzero(m)):
                    flags[l] |= 2
        return PreparedTarget(tgt_depth, lookup_f32, target_masks, pack_target(tgt_depth, bits), flags, links_image)

    def _install(self, prep: PreparedTarget):
        """The frame's target into HBM; from here on the stages score against it."""
        self._target = prep
        self.engine.set_target(prep.tq, prep.lookup_f32, prep.flags)
        if self._has_tsweep():          # TensorSweep compares against the whole target depth, not the lookup plane (predict.py:363)
            self.engine.set_target_tsweep(np.ascontiguousarray(prep.tgt_depth, dtype=np.float32))

    def _segmentLoad(self, target_color, target_depth):
        """Segmentation path (predict.py:415-442).  NB: like the reference, zeroes target_depth in place."""
        if self.seg is None:
            raise NotImplementedError(
                f"no trained segmentation model for '{self.model_ds}' under {Paths().MODELS} and no segmenter given: pass "
                "segmenter=callable(colour)->{'class_ids','scores','masks'} (e.g. rope_s3d_amd.maskrcnn.MaskRCNNSegmenter), "
                "or color_dict for synthetic input")
        small = self._downsample(target_color, self.ds_factor)
        r = self.seg(small)
        seg = self._reorganize_by_link(r)
        # pixellib hands back the frame with its masks painted on (predict.py:416): only the preview looks at it
        links_image = self._paint_links(small, seg) if self.preview else None
        lookup_depth = segment_targets(seg, target_depth, self.u_reader.mesh_names[:LOOKUP_NUM_RENDERED])
        return self._pack_target(target_depth, lookup_depth, {k: v['mask'] for k, v in seg.items()}, links_image)

    def _loadSynthetic(self, target_color, target_depth):
        """Synthetic path: link masks are read off channel 0 of the colour render (predict.py:445-469)."""
        target_color = self._downsample(target_color, self.ds_factor)
        blue = np.ascontiguousarray(target_color[..., 0])          # contiguous: the comparisons below run over it a dozen times
        hit = np.zeros(target_depth.shape, bool)            # the reference sums the comparisons and casts to bool (predict.py:449-454)
        for k in self.color_dict:
            if k in self.u_reader.mesh_names[:LOOKUP_NUM_RENDERED]:
                hit |= blue == self.color_dict[k][0]
        lookup_depth = target_depth * hit
        masks = {}
        for link in self.link_names:
            m = blue == self.color_dict[link][0]
            if m.any():                                        # np.sum(mask) > 0 (predict.py:465)
                masks[link] = m
        return self._pack_target(target_depth, lookup_depth, masks, target_color)       # target_color: `output` of predict.py:469

    def _prepare_synthetic_native(self, target_color, target_depth, tq=None, lookup_f32=None, flags=None, tgt_depth=None, want_depth=True):
        """The synthetic path's prepare() as ONE pass in the library (rope_prepare_synthetic: the same taps, comparisons, counts and
        roundings as _downsample + _loadSynthetic + _pack_target), into the given arrays (slots of a batch) or fresh ones.  None when
        the frame's layout or the colour dictionary is not what that pass takes — the numpy steps do it then."""
        if not self.synthetic or self.preview or any(k not in self.color_dict for k in self.link_names):
            return None
        color, depth = np.asarray(target_color), np.asarray(target_depth)
        if color.ndim != 3 or depth.ndim != 2 or depth.dtype not in (np.float32, np.float64):
            return None
        f = int(self.ds_factor)
        if f < 1 or (f > 1 and f % 2) or depth.shape[0] % f or depth.shape[1] % f:
            return None
        shape = (depth.shape[0] // f, depth.shape[1] // f)
        tq = np.empty(shape, np.uint64) if tq is None else tq
        lookup_f32 = np.empty(shape, np.float32) if lookup_f32 is None else lookup_f32
        flags = np.zeros(8, np.uint8) if flags is None else flags
        tgt_depth = np.empty(shape, np.float64) if (tgt_depth is None and want_depth) else tgt_depth
        blue = [int(self.color_dict[k][0]) for k in self.link_names]
        if not prepare_synthetic(color, depth, f, blue, LOOKUP_NUM_RENDERED, tq, lookup_f32, flags, tgt_depth):
            return None
        return PreparedTarget(tgt_depth, lookup_f32, None, tq, flags, None)

    def _prepare_segmented_native(self, target_color, target_depth, tq=None, lookup_f32=None, flags=None, tgt_depth=None, want_depth=True):
        """The segmentation path's prepare() with everything after the segmenter as ONE pass in the library (rope_prepare_segmented: the
        instance merge, both body masks, the depth's down-sampling, flags and packing of _segmentLoad + _pack_target — same arrays).
        None when it does not apply."""
        if self.synthetic or self.preview or self.seg is None:
            return None
        depth = np.asarray(target_depth)
        f = int(self.ds_factor)
        if depth.ndim != 2 or depth.dtype not in (np.float32, np.float64) or f < 1 or (f > 1 and f % 2) or depth.shape[0] % f or depth.shape[1] % f:
            return None
        r = self.seg(self._downsample(target_color, self.ds_factor))
        shape = (depth.shape[0] // f, depth.shape[1] // f)
        tq = np.empty(shape, np.uint64) if tq is None else tq
        lookup_f32 = np.empty(shape, np.float32) if lookup_f32 is None else lookup_f32
        flags = np.zeros(8, np.uint8) if flags is None else flags
        tgt_depth = np.empty(shape, np.float64) if (tgt_depth is None and want_depth) else tgt_depth
        link_of = [self.link_names.index(self.classes[c]) if self.classes[c] in self.link_names else -1 for c in r['class_ids']]
        if not prepare_segmented(depth, f, np.asarray(r['masks']), link_of, len(self.link_names), LOOKUP_NUM_RENDERED, tq, lookup_f32, flags, tgt_depth):
            # the segmenter has been asked already (and may keep per-frame state): finish this frame the numpy way from its answer
            d = self._downsample(depth, self.ds_factor).astype(np.float64)
            seg = self._reorganize_by_link(r)
            lookup_depth = segment_targets(seg, d, self.u_reader.mesh_names[:LOOKUP_NUM_RENDERED])
            return self._pack_target(d, lookup_depth, {k: v['mask'] for k, v in seg.items()})
        return PreparedTarget(tgt_depth, lookup_f32, None, tq, flags, None)

    def prepare(self, target_color, target_depth) -> PreparedTarget:
        """The host half of run(): down-sampling, link masks (colour read-off or the segmenter), body masking and
        packing (predict.py:132-137).  Touches neither the engine nor the Predictor's state, so the next frame can
        be prepared while this one is on the GPU (run_many)."""
        if self.NATIVE_PREPARE:
            prep = self._prepare_synthetic_native(target_color, target_depth) if self.synthetic else \
                self._prepare_segmented_native(target_color, target_depth)
            if prep is not None:
                return prep
        target_depth = self._downsample(np.asarray(target_depth), self.ds_factor)
        if target_depth.dtype != np.float64:
            target_depth = target_depth.astype(np.float64)
        if self.synthetic:
            return self._loadSynthetic(target_color, target_depth)
        return self._segmentLoad(target_color, target_depth)

    def _polish(self, angles: np.ndarray, depths) -> np.ndarray:
        """refine=True: the stages' angles (N, 6) polished against the frames' depth (N, H, W) at the working resolution ->
        (N, 6); the RefineResult goes to last_refinement."""
        from .refinement import PoseRefiner
        if self._refiner is None:
            self._refiner = PoseRefiner(self.renderer, self.camera_pose, self.intrinsics, self.do_angles, native=self.refine_native)
        elif np.any(self._refiner.camera_pose != self.camera_pose):
            self._refiner.setCameraPose(self.camera_pose)
        self.last_refinement = self._refiner.refine(np.asarray(angles, np.float64).reshape(-1, 6), depths)
        return self.last_refinement.angles

    def run_batch(self, prepared: list, camera_pose=None) -> np.ndarray:
        """B prepared frames (Predictor.prepare) under ONE camera pose through the stage list in lockstep -> (B, 6): every step of a
        stage is one device batch holding the rows of all frames, each row scored against its own frame's target
        (rope_predict_batch).  The frames do not see each other — every state starts fresh (predict.py:144-148) — so the angles are
        those of run() frame by frame; `self.traces[i]` is frame i's per-stage trace."""
        if camera_pose is not None and np.any(np.asarray(camera_pose) != self.camera_pose):
            self.changeCameraPose(camera_pose)
        self._setStages()
        if not self._batch_ok() or len(prepared) == 0:
            out = np.zeros((len(prepared), 6))
            self.traces, polished = [], []
            for i, prep in enumerate(prepared):
                out[i] = self.run(None, None, prepared=prep)
                self.traces.append(self.trace)
                polished.append(self.last_refinement)
            if self.refine and polished:
                from .refinement import RefineResult
                self.last_refinement = RefineResult.concatenate(polished)
            return out
        ts = np.stack([np.asarray(p.tgt_depth, np.float32) for p in prepared]) if self._has_tsweep() or self.refine else None
        angles = self._run_planes(np.stack([p.tq for p in prepared]), np.stack([p.lookup_f32 for p in prepared]),
                                  np.stack([p.flags for p in prepared]), ts if self._has_tsweep() else None)
        return self._polish(angles, ts) if self.refine else angles

    def _plane_set(self, which: int, b: int, H: int, W: int, want_ts: bool):
        """One of the two sets of stacked target planes for `b` frames (page-locked host memory, kept between calls)."""
        from ..engine import pinned_empty
        pool = self.__dict__.setdefault('_planes', {})
        key = (which, b, H, W, want_ts)
        if key not in pool:
            for old in [k for k in pool if k[0] == which]:
                del pool[old]
            pool[key] = (pinned_empty((b, H, W), np.uint64), pinned_empty((b, H, W), np.float32), np.zeros((b, 8), np.uint8),
                         pinned_empty((b, H, W), np.float32) if want_ts else None)
        return pool[key]

    def _batch_ok(self) -> bool:
        """Frames may walk the stage list in lockstep (rope_predict_batch): one preview frame per pose, and the table aliasing,
        need them one at a time."""
        return not self.preview and not self.reference_table_aliasing

    def _run_planes(self, tq, lookup_f32, flags, tsweep=None) -> np.ndarray:
        """run_batch on the frames' stacked target planes: (B,H,W) uint64, (B,H,W) float32, (B,8) uint8 [, (B,H,W) float32]."""
        self.engine.set_targets(tq, lookup_f32, flags, tsweep)
        return self._run_resident(len(tq))

    def _run_resident(self, n: int) -> np.ndarray:
        """The stage list over the engine's n resident targets in lockstep."""
        speculate = self.SPECULATE_BATCH if n >= self.SPECULATE_BATCH_FROM else self.SPECULATE
        angles, trace, n_eval = self.engine.predict_batch(self._native_stages(), self.u_reader.joint_limits, self.camera_pose, self.min_ang_inc,
                                                          self.lookup_angles, self.lookup_crop, self._lookup_table, speculate)
        self.evaluations += n_eval
        self.traces = _BatchTraces(trace, [type(stage).__name__ for stage in self.stages])
        self.trace = self.traces[-1]
        return angles

    @staticmethod
    def _groups(n: int, camera_poses, batch: int) -> list:
        """[lo, hi) runs of consecutive frames with the same camera pose, at most `batch` of them each."""
        groups, lo = [], 0
        while lo < n:
            hi = lo + 1
            while hi < n and hi - lo < batch and (camera_poses is None or np.array_equal(camera_poses[hi], camera_poses[lo])):
                hi += 1
            groups.append((lo, hi))
            lo = hi
        return groups

    SEG_BATCH = 8      # device_targets: frames per pass of the segmenter (batch_device) and per rope_stage_targets_segmented call

    @staticmethod
    def _stacked(results):
        """The (K_i, H, W) mask tensors of a sub-batch's frames as one (sum K_i, H, W) tensor: the segmenter's own, when it says
        that the frames' planes lie in one in frame order ('masks_stacked', MaskRCNNSegmenter.batch_device), a copy otherwise;
        None when no frame has an instance."""
        import torch
        where = [r.get('masks_stacked') for r in results]
        if all(w is not None and w[0] is where[0][0] for w in where):
            at = where[0][1]
            for r, w in zip(results, where):
                if w[1] != at:
                    break
                at += r['masks_device'].shape[0]
            else:
                return where[0][0][where[0][1]:at] if at > where[0][1] else None
        planes = [r['masks_device'] for r in results if r['masks_device'].shape[0]]
        return torch.cat(planes).contiguous() if planes else None

    def _device_targets_apply(self, target_depths) -> bool:
        """device_targets is on, the segmenter leaves its masks on the GPU, and the frames are what that path takes."""
        if not self.device_targets or self.synthetic or self.seg is None or not hasattr(self.seg, 'batch_device'):
            return False
        f = int(self.ds_factor)
        if f < 1 or (f > 1 and f % 2):
            return False
        H, W = self.intrinsics.height, self.intrinsics.width
        d0 = np.asarray(target_depths[0])
        return d0.dtype in (np.float32, np.float64) and \
            all(np.asarray(d).dtype == d0.dtype and np.asarray(d).shape == (H * f, W * f) for d in target_depths)

    def _run_many_device(self, target_colors, target_depths, camera_poses, batch: int) -> np.ndarray:
        """_run_many_batched with the targets built on the GPU.  Worker threads down-sample a group's colour and depth on the host
        (the reduced depth is what travels, in page-locked memory); the staging thread runs the segmenter over the group in
        sub-batches of SEG_BATCH frames, in order, and hands each sub-batch's masks — still on the device — with its depth planes
        to rope_stage_targets_segmented, which fills the sub-batch's slots of the engine's second set of planes on the same
        stream; all of it while the group before is on the GPU."""
        import torch
        from concurrent.futures import ThreadPoolExecutor
        from ..engine import pinned_empty
        from ..utils import cpu_budget
        from .refinement import RefineResult
        n = len(target_colors)
        out = np.zeros((n, 6))
        groups = self._groups(n, camera_poses, batch)
        self._setStages()
        want_ts = self._has_tsweep()
        H, W, f = self.intrinsics.height, self.intrinsics.width, int(self.ds_factor)
        dtype = np.asarray(target_depths[0]).dtype
        device = torch.device('cuda', self.engine.device)
        link_of_class = [self.link_names.index(c) if c in self.link_names else -1 for c in self.classes]
        cap = min(batch, n)
        depth_sets = [pinned_empty((cap, H, W), dtype) for _ in range(min(2, len(groups)))]   # two, taken in turn
        polished = []

        def shrink(depths, colors, j0, j1, lo_):
            for j in range(j0, j1):
                colors[j] = self._downsample(target_colors[lo_ + j], f)
                depths[j] = self._downsample(np.asarray(target_depths[lo_ + j]), f)

        workers = max(1, min(self.PREPARE_WORKERS, cpu_budget() - 1))
        with ThreadPoolExecutor(max_workers=workers) as pool, ThreadPoolExecutor(max_workers=1) as stager:
            def submit(k):
                lo_, hi_ = groups[k]
                b = hi_ - lo_
                depths, colors = depth_sets[k & 1][:b], [None] * b
                step = max(1, -(-b // (4 * workers)))
                return depths, colors, [pool.submit(shrink, depths, colors, j0, min(j0 + step, b), lo_) for j0 in range(0, b, step)]

            def stage(filled):
                depths, colors, jobs = filled
                for j in jobs:
                    j.result()
                b = len(colors)
                subs = [(j0, min(j0 + self.SEG_BATCH, b)) for j0 in range(0, b, self.SEG_BATCH)]
                with torch.cuda.device(device):
                    # a segmenter that can work ahead (batches_device: the next sub-batch's trunk beside this one's box steps) does
                    several = getattr(self.seg, 'batches_device', None) or (lambda gs: (self.seg.batch_device(g) for g in gs))
                    for (j0, j1), results in zip(subs, several(colors[j0:j1] for j0, j1 in subs)):
                        first, link_of = [0], []
                        for r in results:
                            link_of += [link_of_class[c] for c in r['class_ids']]
                            first.append(len(link_of))
                        masks_t = self._stacked(results)
                        depth_t = torch.from_numpy(depths[j0:j1]).to(device, non_blocking=True)
                        self.engine.stage_targets_segmented(depth_t, masks_t, first, link_of, LOOKUP_NUM_RENDERED, b, j0, want_ts)

            filled = {0: submit(0)}
            staging = stager.submit(stage, filled[0])
            if len(groups) > 1:
                filled[1] = submit(1)
            for k, (lo, hi) in enumerate(groups):
                staging.result()
                self.engine.commit_targets()            # waits for the staging kernels: group k resident, its host depth planes free again
                kept = np.array(filled[k][0], np.float32) if self.refine else None      # the reduced depth, before its planes are written again
                del filled[k]
                if k + 2 < len(groups):
                    filled[k + 2] = submit(k + 2)
                if camera_poses is not None and np.any(np.asarray(camera_poses[lo]) != self.camera_pose):
                    self.changeCameraPose(camera_poses[lo])     # before the staging thread touches the context again
                if k + 1 < len(groups):
                    staging = stager.submit(stage, filled[k + 1])
                out[lo:hi] = self._run_resident(hi - lo)
                if self.refine:
                    out[lo:hi] = self._polish(out[lo:hi], kept)
                    polished.append(self.last_refinement)
        if self.refine:
            self.last_refinement = RefineResult.concatenate(polished)
        return out

    def _run_many_batched(self, target_colors, target_depths, camera_poses, batch: int) -> np.ndarray:
        """run_many in groups of up to `batch` consecutive frames under one camera pose.  Worker threads prepare a group's frames
        straight into the slots of its stacked planes (host work only: down-sampling, masks, packing — the library's one-pass form
        where it applies) and an uploader thread sends them to the engine's second set of planes (rope_stage_targets), both
        while the group before it is on the GPU."""
        from concurrent.futures import ThreadPoolExecutor
        from ..utils import cpu_budget
        if self._device_targets_apply(target_depths):
            return self._run_many_device(target_colors, target_depths, camera_poses, batch)
        n = len(target_colors)
        out = np.zeros((n, 6))
        groups = self._groups(n, camera_poses, batch)
        self._setStages()
        want_ts = self._has_tsweep() or self.refine      # refine: the frame's depth at the working resolution, kept beside the planes
        H, W = self.intrinsics.height, self.intrinsics.width
        polished = []

        def fill(planes, k, i):
            tq, t32, fl, ts = planes
            prep = None
            if self.NATIVE_PREPARE:
                native = self._prepare_synthetic_native if self.synthetic else self._prepare_segmented_native
                prep = native(target_colors[i], target_depths[i], tq[k], t32[k], fl[k], want_depth=want_ts)
                if prep is not None and not np.shares_memory(prep.tq, tq[k]):      # finished the numpy way
                    tq[k], t32[k], fl[k] = prep.tq, prep.lookup_f32, prep.flags
            if prep is None:
                prep = self.prepare(target_colors[i], target_depths[i])
                tq[k], t32[k], fl[k] = prep.tq, prep.lookup_f32, prep.flags
            if ts is not None:
                ts[k] = prep.tgt_depth

        def fill_run(planes, j0, j1, lo_):
            for j in range(j0, j1):
                fill(planes, j, lo_ + j)

        # a segmenter (a network on the GPU, or one that keeps per-chunk state) sees the frames one at a time and in order,
        # unless it says it keeps no state (`stateless`)
        workers = max(1, min(self.PREPARE_WORKERS, cpu_budget() - 1)) if (self.synthetic or getattr(self.seg, 'stateless', False)) else 1
        with ThreadPoolExecutor(max_workers=workers) as pool, ThreadPoolExecutor(max_workers=1) as uploader:
            def submit(k):
                lo_, hi_ = groups[k]
                b = hi_ - lo_
                # two sets of planes in page-locked memory, taken in turn
                tq, t32, fl, ts = self._plane_set(k & 1, min(batch, n), H, W, want_ts)
                planes = (tq[:b], t32[:b], fl[:b], None if ts is None else ts[:b])
                # a few jobs per worker, each a run of consecutive frames (a job per frame costs the submitting thread 20 us each)
                step = max(1, -(-b // (4 * workers)))
                return planes, [pool.submit(fill_run, planes, j0, min(j0 + step, b), lo_) for j0 in range(0, b, step)]

            def stage(filled):
                planes, jobs = filled
                for j in jobs:
                    j.result()
                self.engine.stage_targets(*planes[:3], planes[3] if self._has_tsweep() else None)

            # Group k's stages run on the GPU while group k+1's planes go up on the engine's upload stream (as soon as its frames are
            # prepared: the uploader thread waits for them) and the workers write group k+2 into the host planes group k has left.
            filled = {0: submit(0)}
            staging = uploader.submit(stage, filled[0])
            if len(groups) > 1:
                filled[1] = submit(1)
            for k, (lo, hi) in enumerate(groups):
                staging.result()
                self.engine.commit_targets()            # group k resident; its host planes are free again
                kept = np.array(filled[k][0][3]) if self.refine else None
                del filled[k]
                if k + 2 < len(groups):
                    filled[k + 2] = submit(k + 2)
                if camera_poses is not None and np.any(np.asarray(camera_poses[lo]) != self.camera_pose):
                    self.changeCameraPose(camera_poses[lo])     # before the uploader touches the context again
                if k + 1 < len(groups):
                    staging = uploader.submit(stage, filled[k + 1])
                out[lo:hi] = self._run_resident(hi - lo)
                if self.refine:
                    out[lo:hi] = self._polish(out[lo:hi], kept)
                    polished.append(self.last_refinement)
        if self.refine:
            from .refinement import RefineResult
            self.last_refinement = RefineResult.concatenate(polished)
        return out

    def default_batch(self) -> int:
        """Frames per lockstep batch when run_many is not told: BATCH, or what fits BATCH_BYTES of target planes (12 bytes per
        pixel and frame: uint64 + float32)."""
        if self.BATCH is not None:
            return int(self.BATCH)
        return int(min(1024, max(16, self.BATCH_BYTES // (12 * self.intrinsics.width * self.intrinsics.height))))

    def run_many(self, target_colors, target_depths, camera_poses=None, prefetch: bool = True, batch: int = None) -> np.ndarray:
        """run() over a sequence of frames -> (N, 6).  By default BATCH frames at a time walk the stage list in lockstep
        (run_batch).  With batch = 1: frame after frame, and with prefetch frame i+1 is prepared on a worker thread while
        frame i's stages run on the GPU (numpy and the library both release the interpreter lock).  Every frame starts from a
        fresh state either way — same angles as a loop of run()."""
        n = len(target_colors)
        out = np.zeros((n, 6))
        if n == 0:
            return out
        batch = self.default_batch() if batch is None else int(batch)
        self._setStages()
        if batch > 1 and n > 1 and self._batch_ok():
            return self._run_many_batched(target_colors, target_depths, camera_poses, batch)
        pose = (lambda i: None) if camera_poses is None else (lambda i: camera_poses[i])
        polished = []
        if not prefetch or self.preview or n == 1:
            for i in range(n):
                out[i] = self.run(target_colors[i], target_depths[i], pose(i))
                polished.append(self.last_refinement)
        else:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=1) as pool:
                nxt = pool.submit(self.prepare, target_colors[0], target_depths[0])
                for i in range(n):
                    prep = nxt.result()
                    if i + 1 < n:
                        nxt = pool.submit(self.prepare, target_colors[i + 1], target_depths[i + 1])
                    out[i] = self.run(None, None, pose(i), prepared=prep)
                    polished.append(self.last_refinement)
        if self.refine:
            from .refinement import RefineResult
            self.last_refinement = RefineResult.concatenate(polished)
        return out

    # ------------------------------------------------------------------ preview
    def _show(self, stage: int, n_render: int, rows: np.ndarray):
        """preview_if_applicable (predict.py:153-157): one preview frame per pose a stage evaluated, in the reference's order."""
        self.renderer.setMaxParts(n_render)
        for q in preview_rows(type(self.stages[stage]) is SFlip, rows, self.u_reader.joint_limits):
            self.renderer.setJointAngles(q)
            color, depth = self.renderer.render()
            self.viz.loadRenderedColor(color)
            self.viz.loadRenderedDepth(depth)
            self.viz.show()

    def _paint_links(self, color: np.ndarray, seg: dict) -> np.ndarray:
        out = color.astype(np.float64)
        for name, d in seg.items():
            if name in self.link_names:
                c = np.array(DEFAULT_RENDER_COLORS[self.link_names.index(name)], np.float64)
                out[d['mask']] = out[d['mask']] * .5 + c * .5
        return np.rint(out).astype(np.uint8)

    # ------------------------------------------------------------------ the state machine
    def run(self, target_color, target_depth, camera_pose=None, *, prepared: PreparedTarget = None):
        """One frame through the stage list (rope_predict).  With preview, every pose the stages evaluated is shown afterwards,
        in the order they were scored: rendering inside the library's callback would re-enter the engine it holds."""
        if camera_pose is not None and np.any(np.asarray(camera_pose) != self.camera_pose):
            self.changeCameraPose(camera_pose)
        self._setStages()
        stages = self._native_stages()
        self._install(prepared if prepared is not None else self.prepare(target_color, target_depth))
        if self.preview:
            self.viz.loadTargetColor(target_color)
            self.viz.loadTargetDepth(self._target.tgt_depth)
            self.viz.loadSegmentedLinks(self._target.links_image)
        evaluated = []
        angles, trace, n = self.engine.predict(stages, self.u_reader.joint_limits, self.camera_pose, self.min_ang_inc, self.lookup_angles,
                                               self.lookup_crop, self._lookup_table, self.SPECULATE, self._lookup_live,
                                               on_eval=(lambda *batch: evaluated.append(batch)) if self.preview else None)
        self.evaluations += n
        self.trace = [(type(stage).__name__, trace[i].copy()) for i, stage in enumerate(self.stages)]
        for batch in evaluated:
            self._show(*batch)
        if self.refine:
            angles = self._polish(angles, np.asarray(self._target.tgt_depth, np.float32)[None])[0]
        return angles
