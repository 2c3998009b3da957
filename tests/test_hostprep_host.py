"""The library's plain-CPU entry points (csrc/rope_hostprep.cpp) without a GPU: tests/hostprep_main.cpp calls each of them at its
edges with heap buffers of exactly the promised size and is built, together with rope_hostprep.cpp, as a program of its own under
AddressSanitizer and UBSan.  It prints one line per call — return code and FNV-1a hash of the output bytes — and the same calls made
here through ctypes on the shipped library, from the same inputs (val() below is hostprep_main.cpp's), must give the same lines."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rope_s3d_amd import build

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
CSRC = os.path.join(ROOT, 'rope_s3d_amd', 'csrc')


def test_hostprep_is_a_source_of_the_library_and_plain_cxx():
    assert 'rope_hostprep.cpp' in build._SOURCES and 'rope_ctx.h' in build._DEPS and 'rope_ctx.h' not in build._SOURCES
    with open(os.path.join(CSRC, 'rope_hostprep.cpp')) as f:
        src = f.read()
    includes = re.findall(r'#include\s+([<"][^>"]+[>"])', src)
    assert includes and all(i.startswith('<') or i == '"../../include/rope_s3d.h"' for i in includes), includes
    assert not [i for i in includes if 'hip' in i]
    # the limits of rope_depth_holes, which rope_hole_thresholds restates because their header is a HIP one
    with open(os.path.join(CSRC, 'rope_kernels.h')) as f:
        hdr = f.read()
    limits = {k: int(v) for k, v in re.findall(r'#define ROPE_(HOLE_MAX_\w+) (\d+)', hdr)}
    assert limits.keys() == {'HOLE_MAX_DILATIONS', 'HOLE_MAX_WINDOW'}
    assert {k: int(v) for k, v in re.findall(r'\b(HOLE_MAX_\w+) = (\d+)', src)} == limits


def val(seed, i):
    return (((i + seed) * 2654435761) & 0xFFFFFFFF) >> 16


def depth_of(seed, i):
    v = val(seed, i)
    return 0.0 if v % 5 == 0 else (v % 37) * 0.125


def image(H, W, ch, stride, dtype, f):
    """hostprep_main.cpp's image(): rows `stride` bytes apart in a block that ends with the last row's values."""
    item = np.dtype(dtype).itemsize
    b = np.full((H - 1) * stride + W * ch * item, 0xAA, np.uint8)
    for y in range(H):
        row = np.array([f(y * W * ch + i) for i in range(W * ch)], dtype)
        b[y * stride:y * stride + W * ch * item] = row.view(np.uint8)
    return b


def line(name, rc, *outs):
    h = 1469598103934665603
    for a in outs:
        for byte in (a.tobytes() if a is not None else b''):
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f'{name} rc={rc} fnv={h:016x}'


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def library_lines():
    from rope_s3d_amd import engine
    lib = engine.load_library()
    out = []
    for kind in range(3):
        for f in (1, 2):
            H, W, ch = 4, 6, (3 if kind == 0 else 1)
            dt = (np.uint8, np.float32, np.float64)[kind]
            stride = W * ch * np.dtype(dt).itemsize + 16
            gen = (lambda i: val(1, i) & 0xFF, lambda i: depth_of(2, i), lambda i: depth_of(3, i))[kind]
            src, dst = image(H, W, ch, stride, dt, gen), np.zeros((H // f) * (W // f) * ch, dt)
            out.append(line(f'downsample_even kind={kind} f={f}', lib.rope_downsample_even(_p(src), H, W, ch, stride, f, kind, _p(dst)), dst))
    H0, W0, f, H, W = 4, 6, 2, 2, 3
    blue, link_blue = [10, 10, 20, 20, 30, 30], np.array([10, 20, 30, 40, -1, 300], np.int32)

    def colour(i):
        c, x, y = i % 3, (i // 3) % W0, i // (3 * W0)
        return blue[(y // 2) * W + x // 2] if c == 0 else val(4, i) & 0xFF

    def depth(i):
        return 0.0 if blue[((i // W0) // 2) * W + (i % W0) // 2] == 30 else 0.5 + 0.125 * (i % 7)

    color = image(H0, W0, 3, 3 * W0 + 7, np.uint8, colour)
    for kind in (1, 2):
        for want_depth in (0, 1):
            dt = np.float32 if kind == 1 else np.float64
            stride = W0 * np.dtype(dt).itemsize + 8
            d = image(H0, W0, 1, stride, dt, depth)
            tq, look, flags = np.zeros(H * W, np.uint64), np.zeros(H * W, np.float32), np.full(8, 0xFF, np.uint8)
            tgt = np.zeros(H * W, np.float64) if want_depth else None
            rc = lib.rope_prepare_synthetic(_p(color), 3 * W0 + 7, _p(d), kind, stride, H0, W0, f, _p(link_blue), 6, 3, _p(tq), _p(look), _p(tgt), _p(flags))
            out.append(line(f'prepare_synthetic kind={kind} tgt={want_depth}', rc, tq, look, tgt, flags))
    for H, W in ((6, 8), (3, 4)):
        for f in (1, 2):
            for K in (0, 3):
                H0, W0, kind = H * f, W * f, f
                dt = np.float32 if kind == 1 else np.float64
                stride = W0 * np.dtype(dt).itemsize + 24
                d = image(H0, W0, 1, stride, dt, (lambda i: depth_of(5, i)) if kind == 1 else (lambda i: depth_of(6, i)))
                masks = np.array([val(7, i) % 3 == 0 for i in range(H * W * K)], np.uint8)
                link_of = np.array([0, -1, 2], np.int32)
                tq, look, tgt, flags = np.zeros(H * W, np.uint64), np.zeros(H * W, np.float32), np.zeros(H * W, np.float64), np.full(8, 0xFF, np.uint8)
                rc = lib.rope_prepare_segmented(_p(d), kind, stride, H0, W0, f, _p(masks) if K else None, K, _p(link_of) if K else None, 6, 3,
                                                _p(tq), _p(look), _p(tgt), _p(flags))
                out.append(line(f'prepare_segmented {H}x{W} f={f} K={K}', rc, tq, look, tgt, flags))
    limits = np.array([(1.0 if j % 2 else -1.0) * 0.25 * (1 + val(8, j) % 9) for j in range(12)])
    div = np.array([3, 2, 1, 0, 2, -1], np.int32)
    out.append(line('lookup_grid count', lib.rope_lookup_grid(_p(limits), _p(div), None, 0)))
    for capacity in (12, 11):
        rows = np.zeros(capacity * 6)
        out.append(line(f'lookup_grid capacity={capacity}', lib.rope_lookup_grid(_p(limits), _p(div), _p(rows), capacity), rows))
    for links in range(2, 7):
        d = np.full(6, -1, np.int32)
        out.append(line(f'crop_divisions n_pixels=1 links={links}', lib.rope_crop_divisions(1, links, _p(d)), d))
    for max_size in (3, 4, 25):
        n = C.c_int(-1)
        rc0 = lib.rope_hole_thresholds(0.22, 1.0, max_size, None, C.byref(n))
        T = np.zeros(max(n.value, 0), np.uint32)
        rc = lib.rope_hole_thresholds(0.22, 1.0, max_size, _p(T), C.byref(n))
        out.append(line(f'hole_thresholds max_size={max_size} n={n.value}', rc0 * 100 + rc, T))
    pose, PV = np.array([0.125 * (val(9, j) % 17) - 1.0 for j in range(6)]), np.zeros(16)
    out.append(line('camera_matrix', lib.rope_camera_matrix(_p(pose), 600.0, 601.5, 320.25, 239.75, 640, 480, 0.05, 100.0, _p(PV)), PV))
    depth8 = np.array([np.nan, -1.5, 0.0, 1.5, 127.99999999999, 128.0, 1.0e300, np.inf])
    mask = np.array([val(10, i) & 0xFF for i in range(8)], np.uint8)
    for with_mask in (0, 1):
        packed = np.full(8, 0xFFFFFFFFFFFFFFFF, np.uint64)
        out.append(line(f'pack_target mask={with_mask}', lib.rope_pack_target(_p(depth8), _p(mask) if with_mask else None, 8, _p(packed)), packed))
    return out


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_hostprep_under_asan_and_ubsan_matches_the_library(tmp_path):
    exe = str(tmp_path / 'hostprep_main')
    subprocess.check_call(['g++', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                           '-fno-sanitize-recover=undefined', '-g', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'hostprep_main.cpp'),
                           os.path.join(CSRC, 'rope_hostprep.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and r.stderr == ''
    got, want = r.stdout.splitlines(), library_lines()
    assert len(got) == 32 and got == want
    by_name = {ln.split(' rc=')[0]: int(ln.split(' rc=')[1].split()[0]) for ln in got}
    refused = {k for k, rc in by_name.items() if rc != 0 and not k.startswith('lookup_grid')}
    assert refused == {f'downsample_even kind={k} f=1' for k in range(3)}                      # f must be even there
    assert by_name['lookup_grid count'] == 12 and by_name['lookup_grid capacity=12'] == 12 and by_name['lookup_grid capacity=11'] == -1
