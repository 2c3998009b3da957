"""CPU: the host side of the depth conditioning — the ABI of the rope_depth_* calls, the host-only shape call, what DepthConditioner
refuses before it touches a device, and RawRecordingCamera on a folder written here."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import feed_ref
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(helpers.__file__)))
SYMBOLS = {'rope_depth_decimated_shape': 5, 'rope_depth_decimate': 7, 'rope_depth_spatial': 8, 'rope_depth_temporal': 10, 'rope_depth_align': 13}
SENSOR = {'width': 16, 'height': 8, 'fx': 8.0, 'fy': 8.0, 'cx': 8.0, 'cy': 4.0, 'coeffs': [0, 0, 0, 0, 0]}
IDENTITY = {'rotation': [1, 0, 0, 0, 1, 0, 0, 0, 1], 'translation': [0, 0, 0]}


def test_symbols_are_declared_exported_and_built_from_rope_feed():
    from rope_s3d_amd import build, engine as eng
    hdr = open(os.path.join(ROOT, 'include', 'rope_s3d.h')).read()
    lib = eng.load_library()
    for name, n_args in SYMBOLS.items():
        assert re.search(r'\bint ' + name + r'\(', hdr), name
        assert name in eng.ABI_SYMBOLS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args, name
    assert lib.rope_depth_spatial.argtypes[4] is C.c_float and lib.rope_depth_temporal.argtypes[4] is C.c_float
    assert lib.rope_depth_align.argtypes[7] is C.c_double
    assert 'rope_feed.hip' in build._SOURCES and 'rope_feed.hip' in build._DEPS
    assert os.path.isfile(os.path.join(os.path.dirname(build.LIB_PATH), 'rope_feed.hip'))


@pytest.mark.parametrize('H,W,k,want', [(8, 8, 2, (4, 4)), (10, 22, 2, (4, 8)), (13, 29, 3, (4, 8)), (33, 67, 4, (8, 16)), (7, 64, 2, None),
                                        (720, 1280, 2, (360, 640)), (64, 3, 2, None), (64, 64, 1, None), (64, 64, 9, None), (64, 64, 8, (8, 8)),
                                        (0, 64, 2, None), (64, -1, 2, None)])
def test_decimated_shape(H, W, k, want):
    from rope_s3d_amd import engine as eng
    lib = eng.load_library()
    h, w = C.c_int(-7), C.c_int(-7)
    rc = lib.rope_depth_decimated_shape(H, W, k, C.byref(h), C.byref(w))
    if want is None:
        assert rc == -1 and (h.value, w.value) == (-7, -7)
    else:
        assert rc == 0 and (h.value, w.value) == want == feed_ref.decimated_shape(H, W, k)
    assert lib.rope_depth_decimated_shape(H, W, k, None, C.byref(w)) == -1


def test_conditioner_refuses_what_it_cannot_do_before_any_device():
    from rope_s3d_amd.prediction.conditioning import DepthConditioner, sensor_terms
    from rope_s3d_amd.projection import Intrinsics
    c = DepthConditioner(SENSOR, dict(SENSOR, width=8, height=4, fx=4.0, fy=4.0, cx=4.0, cy=2.0), IDENTITY, 0.001)
    assert c.decimation == 2 and c.spatial == (2, 0.5, 20) and c.temporal == (0.5, 20, 3)       # the reference's LiveCamera settings
    assert c.align_terms == [4.0, 4.0, 4.0, 2.0] and (c.Hc, c.Wc) == (4, 8) and c.extrin.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert c.conditioned_shape(8, 16) == (4, 8) and c._lib is None and c._last is None
    assert c.metres(np.array([[0, 1000]], np.uint16)).dtype == np.float64 and c.metres(np.array([1000], np.uint16))[0] == 1000 * 0.001
    off = DepthConditioner(SENSOR, SENSOR, np.eye(4), 0.001, decimation=None, spatial=None, temporal=None)
    assert off.align_terms == [8.0, 8.0, 8.0, 4.0] and off.conditioned_shape(8, 16) == (8, 16)
    intr = Intrinsics('640_480_color')
    assert sensor_terms(intr) == (640, 480, [intr.fx, intr.fy, intr.cx, intr.cy]) == sensor_terms(str(intr))
    with pytest.raises(ValueError, match='distortion'):
        DepthConditioner(dict(SENSOR, coeffs=[0, 0, 1e-3, 0, 0]), SENSOR, IDENTITY, 0.001)
    with pytest.raises(ValueError, match='distortion'):
        DepthConditioner(SENSOR, dict(SENSOR, coeffs=[0.1, 0, 0, 0, 0]), IDENTITY, 0.001)
    with pytest.raises(ValueError, match='lacks'):
        DepthConditioner({'width': 16, 'height': 8, 'fx': 8.0}, SENSOR, IDENTITY, 0.001)
    for kw in (dict(decimation=1), dict(decimation=9), dict(decimation=2.5), dict(spatial=(0, 0.5, 20)), dict(spatial=(6, 0.5, 20)),
               dict(spatial=(2, 0.0, 20)), dict(spatial=(2, 1.5, 20)), dict(spatial=(2, 0.5, 0)), dict(spatial=(2, 0.5, 65536)),
               dict(temporal=(0.0, 20, 3)), dict(temporal=(0.5, 0, 3)), dict(temporal=(0.5, 20, 9)), dict(temporal=(0.5, 20, -1))):
        with pytest.raises(ValueError):
            DepthConditioner(SENSOR, SENSOR, IDENTITY, 0.001, **kw)
    for scale in (0.0, -0.001, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='depth_scale'):
            DepthConditioner(SENSOR, SENSOR, IDENTITY, scale)
    with pytest.raises(ValueError, match='extrinsics'):
        DepthConditioner(SENSOR, SENSOR, np.eye(3), 0.001)
    with pytest.raises(ValueError, match='too small'):
        c.conditioned_shape(7, 64)


class _HostConditioner:
    """The reference chain behind the conditioner's surface: what RawRecordingCamera needs of one."""

    def __init__(self, sensor):
        terms = lambda s: [s['fx'], s['fy'], s['cx'], s['cy']]     # noqa: E731
        ext = sensor['extrinsics']['rotation'] + sensor['extrinsics']['translation']
        self.chain = feed_ref.Chain(terms(sensor['depth']), terms(sensor['color']), ext, sensor['depth_scale'],
                                    (sensor['color']['height'], sensor['color']['width']))
        self.resets = 0

    def reset(self):
        self.resets += 1
        self.chain.reset()

    def process(self, raw):
        return self.chain.process(raw)

    def metres(self, plane):
        return self.chain.metres(plane)

    def average(self, raws):
        return self.chain.average(raws)


def _write_folder(folder, n=3, angles=True, png_at=()):
    from rope_s3d_amd.data.annotation import encode_png
    rng = np.random.default_rng(17)
    os.makedirs(folder, exist_ok=True)
    sensor = {'depth': SENSOR, 'color': dict(SENSOR, width=8, height=4, fx=4.0, fy=4.0, cx=4.0, cy=2.0), 'extrinsics': IDENTITY,
              'depth_scale': 0.001}
    if angles:
        sensor['angles'] = [[float(i), 0.5, 0, 0, 0, 0] for i in range(n)]
    with open(os.path.join(folder, 'sensor.json'), 'w') as f:
        json.dump(sensor, f)
    depths = rng.integers(900, 940, (n, 8, 16)).astype(np.uint16)
    depths[rng.random(depths.shape) < 0.1] = 0
    colors = rng.integers(0, 255, (n, 4, 8, 3), dtype=np.uint8)
    for i in range(n):
        np.save(os.path.join(folder, f'depth_{i:06d}.npy'), depths[i])
        if i in png_at:
            with open(os.path.join(folder, f'color_{i:06d}.png'), 'wb') as f:
                f.write(encode_png(colors[i]))                            # BGR in, R, G, B in the file, as cv2.imwrite stores it
        else:
            np.save(os.path.join(folder, f'color_{i:06d}.npy'), colors[i])
    return sensor, depths, colors


def test_raw_recording_camera_replays_a_folder_in_order(tmp_path):
    from rope_s3d_amd.prediction.feed import RawRecordingCamera
    folder = str(tmp_path / 'raw3')
    sensor, depths, colors = _write_folder(folder, 3, png_at=(1,))
    cam = RawRecordingCamera(folder, conditioner=_HostConditioner(sensor))
    assert len(cam) == 3 and [os.path.basename(c) for _, c in cam.files] == ['color_000000.npy', 'color_000001.png', 'color_000002.npy']
    for i in range(3):
        c, d = cam.raw(i)
        assert np.array_equal(c, colors[i]) and np.array_equal(d, depths[i]) and d.dtype == np.uint16
    want = _HostConditioner(sensor)
    claims = cam.claims()
    cam.start()
    assert cam.conditioner.resets == 1
    for i in range(3):
        assert claims.get_pose().tolist() == [float(i), 0.5, 0, 0, 0, 0]
        color, depth = cam.get()
        assert np.array_equal(color, colors[i]) and depth.dtype == np.float64 and depth.shape == (4, 8)
        assert np.array_equal(depth, want.metres(want.process(depths[i])))
    assert cam.get() is None and claims.get_pose() is None and cam.get_average() is None
    cam.stop()
    cam.start()                                                           # from the top, the state forgotten
    color, mean = cam.get_average(num=2)
    want.reset()
    assert np.array_equal(color, colors[0]) and np.array_equal(mean, want.average(depths[:2])) and cam.i == 2
    color, mean = cam.get_average()                                       # one frame left of the 20 asked for
    assert np.array_equal(color, colors[2]) and cam.get() is None


def test_raw_recording_camera_refuses_a_folder_it_cannot_play(tmp_path):
    from rope_s3d_amd.prediction.feed import RawRecordingCamera
    sensor, _, _ = _write_folder(str(tmp_path / 'no_angles'), 2, angles=False)
    cam = RawRecordingCamera(str(tmp_path / 'no_angles'), conditioner=_HostConditioner(sensor))
    assert cam.angles is None
    with pytest.raises(ValueError, match='angles'):
        cam.claims()
    # the default conditioner is built from sensor.json without touching a device
    plain = RawRecordingCamera(str(tmp_path / 'no_angles'))
    assert plain.conditioner.decimation == 2 and plain.conditioner._lib is None and (plain.conditioner.Hc, plain.conditioner.Wc) == (4, 8)
    os.makedirs(tmp_path / 'empty')
    (tmp_path / 'empty' / 'sensor.json').write_text(json.dumps(sensor))
    with pytest.raises(ValueError, match='holds no'):
        RawRecordingCamera(str(tmp_path / 'empty'))
    sensor['angles'] = [[0] * 6]
    (tmp_path / 'no_angles' / 'sensor.json').write_text(json.dumps(sensor))
    with pytest.raises(ValueError, match='rows of angles'):
        RawRecordingCamera(str(tmp_path / 'no_angles'))
    with pytest.raises(OSError):
        RawRecordingCamera(str(tmp_path / 'missing'))
