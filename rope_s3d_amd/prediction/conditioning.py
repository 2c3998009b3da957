"""Conditioning of raw depth frames on the GPU: what the reference's LiveCamera has pyrealsense2 do to every depth frame before
the Predictor sees it (robotpose/prediction/feed.py:32-99) — decimation by 2, the edge-preserving spatial filter (2 iterations,
alpha 0.5, delta 20, no hole filling), the temporal filter (alpha 0.5) with its persistence rule, alignment of the depth image to
the colour sensor, scaling to metres, and get_average's mean of 20 frames.  A raw frame is a z16 depth image at the depth sensor's
intrinsics.  The arithmetic is the one include/rope_s3d.h writes down for the rope_depth_* calls (csrc/rope_feed.hip): this
project's definition, restated from memory of librealsense's filters and not checked against them.

There is no CPU path: without the library or a device, processing raises engine.EngineUnavailable."""
import ctypes as C

import numpy as np

from .. import engine as eng

_TERMS = ('fx', 'fy', 'cx', 'cy')


def sensor_terms(desc):
    """A sensor description -> (width, height, [fx, fy, cx, cy]).  `desc` is a dict with width, height, fx, fy, cx, cy and
    optionally coeffs (sensor.json's form), a projection.Intrinsics, or the string form of one.  Distortion coefficients other
    than zero are refused: the alignment has no lens model."""
    if isinstance(desc, str):
        from ..projection import Intrinsics
        desc = Intrinsics(desc)
    get = (lambda k, d=None: desc.get(k, d)) if isinstance(desc, dict) else (lambda k, d=None: getattr(desc, k, d))
    missing = [k for k in ('width', 'height') + _TERMS if get(k) is None]
    if missing:
        raise ValueError(f"sensor description lacks {missing}")
    coeffs = get('coeffs')
    if coeffs is not None and any(float(c) != 0.0 for c in np.ravel(coeffs)):
        raise ValueError(f"distortion coefficients {list(np.ravel(coeffs))}: the alignment takes sensors without a lens model only")
    width, height = int(get('width')), int(get('height'))
    terms = [float(get(k)) for k in _TERMS]
    if width < 1 or height < 1 or not all(np.isfinite(terms)) or terms[0] == 0.0 or terms[1] == 0.0:
        raise ValueError(f"sensor description {width} x {height}, {dict(zip(_TERMS, terms))}: sizes of at least 1, finite terms, fx and fy not 0")
    return width, height, terms


def _extrinsics(ext):
    """Depth-to-colour extrinsics -> 12 doubles, row-major R then t (metres).  Takes {'rotation': 3x3 or 9, 'translation': 3},
    a 3x4 or 4x4 matrix [R | t], or the 12 numbers themselves."""
    if isinstance(ext, dict):
        out = np.concatenate([np.asarray(ext['rotation'], np.float64).reshape(9), np.asarray(ext['translation'], np.float64).reshape(3)])
    else:
        a = np.asarray(ext, np.float64)
        if a.shape in ((3, 4), (4, 4)):
            out = np.concatenate([a[:3, :3].reshape(9), a[:3, 3]])
        elif a.size == 12:
            out = a.reshape(12).copy()
        else:
            raise ValueError(f"extrinsics of shape {a.shape}: a rotation and a translation, [R | t], or 12 numbers")
    if not np.all(np.isfinite(out)):
        raise ValueError("extrinsics must be finite")
    return np.ascontiguousarray(out)


class DepthConditioner:
    """decimate -> spatial -> temporal -> align on one device, with the state planes and the scratch it needs.  The defaults are
    the reference's LiveCamera settings.  `spatial` is (iterations, alpha, delta), `temporal` (alpha, delta, persistence); any of
    the three filters is switched off with None.  Nothing touches the device before the first frame arrives."""

    def __init__(self, depth_intrin, color_intrin, extrinsics, depth_scale, decimation=2, spatial=(2, 0.5, 20), temporal=(0.5, 20, 3),
                 device: int = 0):
        *self.depth_size, self.depth_terms = sensor_terms(depth_intrin)       # depth_size: [width, height]
        self.Wc, self.Hc, self.color_terms = sensor_terms(color_intrin)
        self.extrin = _extrinsics(extrinsics)
        self.depth_scale = float(depth_scale)
        if not np.isfinite(self.depth_scale) or self.depth_scale <= 0:
            raise ValueError(f"depth_scale {depth_scale}: metres per sensor unit, finite and above 0")
        if decimation is not None and (int(decimation) != decimation or not 2 <= decimation <= 8):
            raise ValueError(f"decimation {decimation}: 2 .. 8, or None")
        if spatial is not None:
            it, alpha, delta = spatial
            if int(it) != it or not 1 <= it <= 5 or not 0 < alpha <= 1 or int(delta) != delta or not 1 <= delta <= 65535:
                raise ValueError(f"spatial {spatial}: (iterations 1 .. 5, alpha in (0, 1], delta 1 .. 65535), or None")
        if temporal is not None:
            alpha, delta, pers = temporal
            if not 0 < alpha <= 1 or int(delta) != delta or not 1 <= delta <= 65535 or int(pers) != pers or not 0 <= pers <= 8:
                raise ValueError(f"temporal {temporal}: (alpha in (0, 1], delta 1 .. 65535, persistence 0 .. 8), or None")
        self.decimation = None if decimation is None else int(decimation)
        self.spatial = None if spatial is None else (int(spatial[0]), float(spatial[1]), int(spatial[2]))
        self.temporal = None if temporal is None else (float(temporal[0]), int(temporal[1]), int(temporal[2]))
        k = self.decimation or 1
        self.align_terms = [v / k for v in self.depth_terms] if self.decimation else list(self.depth_terms)
        self.device = int(device)
        self._lib = None
        self._last = self._history = self._scratch = None

    # ------------------------------------------------------------------------------------------------------------------ device
    def _ready(self):
        import torch
        if self._lib is None:
            lib = eng.load_library()
            if not torch.cuda.is_available() or self.device >= torch.cuda.device_count():
                raise eng.EngineUnavailable(f"DepthConditioner needs HIP device {self.device}; the conditioning has no CPU path")
            self._lib = lib
        return torch, torch.device('cuda', self.device)

    def conditioned_shape(self, H: int, W: int):
        """The shape of the planes between decimation and alignment for H x W raw frames."""
        if not self.decimation:
            return int(H), int(W)
        h, w = C.c_int(0), C.c_int(0)
        if eng.load_library().rope_depth_decimated_shape(int(H), int(W), self.decimation, C.byref(h), C.byref(w)):
            raise ValueError(f"{H} x {W} frames are too small to decimate by {self.decimation}")
        return h.value, w.value

    def reset(self):
        """Forget the frames seen so far: the temporal filter starts anew."""
        if self._last is not None:
            self._last.zero_()
            self._history.zero_()

    def process_many_device(self, raw_t):
        """(N, H, W) raw frames, consecutive in time, as a contiguous 16-bit integer tensor on this conditioner's device ->
        (N, Hc, Wc) aligned planes as a torch.uint16 tensor on the device.  The kernels go to torch's current stream; nothing is
        waited for."""
        torch, dev = self._ready()
        if not isinstance(raw_t, torch.Tensor) or raw_t.dim() != 3 or raw_t.element_size() != 2 or raw_t.is_floating_point() or not raw_t.is_contiguous():
            raise ValueError("raw frames: a contiguous (N, H, W) tensor of 16-bit integers")
        if raw_t.device != dev:
            raise ValueError(f"raw frames must be on {dev}, got {raw_t.device}")
        N, H, W = raw_t.shape
        if (H, W) != (self.depth_size[1], self.depth_size[0]):
            raise ValueError(f"raw frames are {H} x {W}, the depth sensor is {self.depth_size[1]} x {self.depth_size[0]}")
        h, w = self.conditioned_shape(H, W)
        if N == 0:
            return torch.empty((0, self.Hc, self.Wc), dtype=torch.int16, device=dev).view(torch.uint16)
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if self.decimation:
                planes = torch.empty((N, h, w), dtype=torch.int16, device=dev)
                self._check(self._lib.rope_depth_decimate(p(raw_t), N, H, W, self.decimation, p(planes), st), 'rope_depth_decimate')
            else:
                planes = raw_t.clone()              # the filters work in place: the caller's frames stay as they are
            if self.spatial:
                it, alpha, delta = self.spatial
                self._check(self._lib.rope_depth_spatial(p(planes), N, h, w, alpha, delta, it, st), 'rope_depth_spatial')
            if self.temporal:
                if self._last is None or tuple(self._last.shape) != (h, w):
                    self._last = torch.zeros((h, w), dtype=torch.int16, device=dev)
                    self._history = torch.zeros((h, w), dtype=torch.uint8, device=dev)
                alpha, delta, pers = self.temporal
                self._check(self._lib.rope_depth_temporal(p(planes), N, h, w, alpha, delta, pers, p(self._last), p(self._history), st),
                            'rope_depth_temporal')
            if self._scratch is None or self._scratch.shape[0] < N:
                self._scratch = torch.empty((N, self.Hc, self.Wc), dtype=torch.int32, device=dev)
            out = torch.empty((N, self.Hc, self.Wc), dtype=torch.int16, device=dev)
            d, c = (C.c_double * 4)(*self.align_terms), (C.c_double * 4)(*self.color_terms)
            e = (C.c_double * 12)(*self.extrin)
            self._check(self._lib.rope_depth_align(p(planes), N, h, w, d, c, e, self.depth_scale, self.Hc, self.Wc, p(self._scratch), p(out), st),
                        'rope_depth_align')
        return out.view(torch.uint16)

    @staticmethod
    def _check(rc, name):
        if rc == -1:
            raise ValueError(f"{name} refused its arguments")
        if rc:
            raise eng.EngineError(f"{name} failed ({rc})")

    def _upload(self, raw):
        torch, dev = self._ready()
        a = np.ascontiguousarray(raw)
        if a.dtype != np.uint16:
            raise ValueError(f"raw frames are z16: uint16, not {a.dtype}")
        return torch.from_numpy(a.view(np.int16)).to(dev)

    # -------------------------------------------------------------------------------------------------------------------- host
    def process_many(self, raw) -> np.ndarray:
        """(N, H, W) uint16 raw frames, consecutive in time, in one chain of calls -> (N, Hc, Wc) uint16 aligned planes."""
        raw = np.asarray(raw)
        if raw.ndim != 3:
            raise ValueError(f"raw frames of shape {raw.shape}: (N, H, W)")
        return self.process_many_device(self._upload(raw)).view(self._ready()[0].int16).cpu().numpy().view(np.uint16)

    def process(self, raw) -> np.ndarray:
        """One (H, W) uint16 raw frame, the next in time -> the (Hc, Wc) uint16 aligned plane."""
        raw = np.asarray(raw)
        if raw.ndim != 2:
            raise ValueError(f"a raw frame of shape {raw.shape}: (H, W)")
        return self.process_many(raw[None])[0]

    def metres(self, plane) -> np.ndarray:
        """Sensor units -> float64 metres, the reference's np.array(..., dtype=float) * depth_scale (feed.py:69)."""
        return np.array(plane, dtype=float) * self.depth_scale

    def average(self, raws) -> np.ndarray:
        """The mean over the frames of the conditioned planes, in metres (feed.py:71-99).  The planes are summed in 32 bits on
        the device — the reference sums in the frames' own uint16 and can wrap — and scaled on the host:
        sum * depth_scale / N."""
        raws = np.asarray(raws)
        if raws.ndim != 3 or len(raws) == 0:
            raise ValueError(f"raw frames of shape {raws.shape}: (N, H, W), N at least 1")
        torch, _ = self._ready()
        planes = self.process_many_device(self._upload(raws))
        total = (planes.view(torch.int16).to(torch.int32) & 0xFFFF).sum(dim=0, dtype=torch.int32)
        return total.cpu().numpy().astype(np.float64) * self.depth_scale / len(raws)
