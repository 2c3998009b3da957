"""The geometry cache's plain C++ (csrc/rope_geomcache.h: the candidate shadow and the record's key) without a GPU:
tests/geomcache_main.cpp exercises both at their edges and is built as a program of its own under AddressSanitizer and UBSan."""
import os
import re
import subprocess

from rope_s3d_amd import build, engine

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
CSRC = os.path.join(ROOT, 'rope_s3d_amd', 'csrc')


def test_header_is_plain_cxx_and_part_of_the_build_id():
    assert 'rope_geomcache.h' in build._DEPS
    with open(os.path.join(CSRC, 'rope_geomcache.h')) as f:
        src = f.read()
    assert not re.search(r'#include\s*[<"](hip/|rope_)', src), "rope_geomcache.h must build without HIP and without the context"


def test_flag_and_entry_are_declared_everywhere():
    with open(os.path.join(ROOT, 'include', 'rope_s3d.h')) as f:
        pub = f.read()
    with open(os.path.join(CSRC, 'rope_kernels.h')) as f:
        priv = f.read()
    assert re.search(r'ROPE_STRATEGY_NO_GEOMETRY_CACHE\s*=\s*64\b', pub) and re.search(r'\bSTRATEGY_NO_GEOMETRY_CACHE\s*=\s*64\b', priv)
    assert engine.Engine.NO_GEOMETRY_CACHE == 64
    assert 'rope_geometry_cache_stats' in engine.ABI_SYMBOLS and 'int rope_geometry_cache_stats(' in pub


def test_shadow_and_key_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'geomcache_main')
    subprocess.check_call(['g++', '-std=c++17', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-fno-sanitize-recover=undefined',
                           '-g', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'geomcache_main.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and re.fullmatch(r'ok \d+\n', r.stdout), r.stdout + r.stderr
