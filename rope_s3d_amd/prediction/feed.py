"""Sources of the live loop (predict_live.py): where frames and the controller's claimed joint angles come from.

The reference reads an Intel RealSense through pyrealsense2 (robotpose/prediction/feed.py:14-86) and the robot
controller's joint state from a JSON file the controller rewrites (robotpose/textfile_integration.py:19-69).  The
JSON link is plain file traffic and is kept as is; the camera needs pyrealsense2 and the device, neither of which
exists here, so `LiveCamera` says so loudly and `DatasetCamera` replays a recorded Dataset through the same
`start / get / stop` surface (its `claims()` pairs every frame with the recorded joint angles).  `RawRecordingCamera` replays a
capture of RAW sensor frames — z16 depth at the depth sensor's intrinsics plus a BGR image — and conditions every depth frame
on the GPU as LiveCamera.get has pyrealsense2 do it (prediction/conditioning.py)."""
import json
import os
import time

import numpy as np

from ..constants import JSON_LINK_FILE


class JSONCoupling:
    """The controller writes {"position": [six joint angles]} to a file; get_pose polls for it, reset removes it so
    that the next pose read is a fresh one (textfile_integration.py:23-69)."""

    def __init__(self, path: str = JSON_LINK_FILE, poll: float = 0.0001):
        self.path, self.poll, self.data = path, poll, None

    def get_pose(self, timeout: float = None):
        start = time.time()
        while True:
            if os.path.isfile(self.path):
                try:
                    with open(self.path, 'r') as f:
                        self.data = json.load(f)
                    break
                except (OSError, ValueError):       # the controller is mid-write: try again
                    pass
            if timeout is not None and time.time() - start > timeout:
                return None
            time.sleep(self.poll)
        return np.array(self.data['position'])

    def reset(self, timeout: float = None):
        start = time.time()                      # the reference's `start = time.time` (no call) makes its timeout a TypeError
        while os.path.isfile(self.path):
            try:
                os.remove(self.path)
                break
            except OSError:
                pass
            if timeout is not None and time.time() - start > timeout:
                break
            time.sleep(self.poll)


class LiveCamera:
    """RealSense colour + aligned depth (feed.py:14-86).  Needs pyrealsense2 and the camera."""

    def __init__(self, width: int = 1280, height: int = 720, fps: int = 30):
        try:
            import pyrealsense2  # noqa: F401
        except ImportError as e:
            raise RuntimeError("LiveCamera needs pyrealsense2 and an Intel RealSense device; replay a recorded set "
                               "with DatasetCamera instead (predict_live.py -replay <dataset>)") from e
        raise NotImplementedError("RealSense capture is outside the prediction path (DESIGN.md §9)")


class DatasetCamera:
    """A recorded Dataset played back as a camera: get() returns (colour uint8 BGR, depth metres) of the next frame,
    None when the recording is over."""

    def __init__(self, dataset, start: int = 0, stop: int = None):
        self.ds, self.i, self.end = dataset, start, dataset.length if stop is None else min(stop, dataset.length)

    def start(self):
        pass

    def stop(self):
        pass

    def get(self):
        if self.i >= self.end:
            return None
        i, self.i = self.i, self.i + 1
        return np.copy(self.ds.og_img[i]), np.copy(self.ds.depthmaps[i])

    def claims(self):
        """The controller side of a replay: the recorded joint angles of the frame get() hands out next."""
        ds, cam = self.ds, self

        class _Recorded:
            def get_pose(self, timeout=None):
                return None if cam.i >= cam.end else np.array(ds.angles[cam.i], dtype=float)

            def reset(self, timeout=None):
                pass
        return _Recorded()


class RawRecordingCamera:
    """A folder of raw sensor frames played back as a camera.  The folder holds depth_%06d.npy (uint16 z16, at the depth sensor's
    intrinsics), color_%06d.npy or color_%06d.png (BGR; a PNG stores R, G, B and is turned round as cv2.imread would) and
    sensor.json: {"depth": {width, height, fx, fy, cx, cy[, coeffs]}, "color": {the same}, "extrinsics": {"rotation": 9 numbers
    row-major, "translation": 3, metres, depth to colour}, "depth_scale": metres per unit[, "angles": one row of six per frame]}.
    get() returns (colour uint8 BGR, depth in metres float64 aligned to the colour image) of the next frame, as LiveCamera.get
    does (feed.py:56-69), None when the recording is over; get_average(num) what LiveCamera.get_average does with the next `num`
    frames.  The depth goes through a conditioning.DepthConditioner (the reference's filter settings unless one is handed in:
    anything with process / average / metres / reset serves)."""

    def __init__(self, folder: str, conditioner=None):
        with open(os.path.join(folder, 'sensor.json')) as f:
            self.sensor = json.load(f)
        self.folder, self.files = folder, []
        while True:
            i = len(self.files)
            depth = os.path.join(folder, f'depth_{i:06d}.npy')
            color = [c for c in (os.path.join(folder, f'color_{i:06d}{ext}') for ext in ('.npy', '.png')) if os.path.isfile(c)]
            if not os.path.isfile(depth) or not color:
                break
            self.files.append((depth, color[0]))
        if not self.files:
            raise ValueError(f"{folder} holds no depth_000000.npy with a color_000000.npy or .png beside it")
        self.angles = None
        if self.sensor.get('angles') is not None:
            self.angles = np.asarray(self.sensor['angles'], dtype=float).reshape(-1, 6)
            if len(self.angles) != len(self.files):
                raise ValueError(f"{folder}: {len(self.angles)} rows of angles for {len(self.files)} frames")
        if conditioner is None:
            from .conditioning import DepthConditioner
            conditioner = DepthConditioner(self.sensor['depth'], self.sensor['color'], self.sensor['extrinsics'], self.sensor['depth_scale'])
        self.conditioner, self.i = conditioner, 0

    def __len__(self):
        return len(self.files)

    def start(self):
        self.i = 0
        self.conditioner.reset()

    def stop(self):
        pass

    def raw(self, i: int):
        """Frame i as it was captured: (colour uint8 BGR, depth uint16 sensor units at the depth sensor's size)."""
        depth_path, color_path = self.files[i]
        if color_path.endswith('.png'):
            from ..data.labelme import decode_png
            with open(color_path, 'rb') as f:
                img = decode_png(f.read())
            img = img[..., 2::-1] if img.shape[2] >= 3 else np.repeat(img[..., :1], 3, axis=2)
            color = np.ascontiguousarray(img)
        else:
            color = np.load(color_path)
        return color, np.load(depth_path)

    def get(self):
        if self.i >= len(self.files):
            return None
        color, depth = self.raw(self.i)
        self.i += 1
        return color, self.conditioner.metres(self.conditioner.process(depth))

    def get_average(self, num: int = 20):
        """The colour image of the first and the mean conditioned depth, in metres, of the next `num` frames (fewer when the
        recording ends first); None when none is left."""
        stop = min(self.i + num, len(self.files))
        if self.i >= stop:
            return None
        frames = [self.raw(i) for i in range(self.i, stop)]
        self.i = stop
        return frames[0][0], self.conditioner.average(np.stack([d for _, d in frames]))

    def claims(self):
        """The controller side of a replay: the recorded joint angles of the frame get() hands out next (sensor.json's "angles")."""
        if self.angles is None:
            raise ValueError(f"{self.folder}/sensor.json records no angles")
        cam = self

        class _Recorded:
            def get_pose(self, timeout=None):
                return None if cam.i >= len(cam.files) else np.array(cam.angles[cam.i], dtype=float)

            def reset(self, timeout=None):
                pass
        return _Recorded()
