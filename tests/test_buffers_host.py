"""The context's owning buffer types (csrc/rope_buffers.h) without a GPU: tests/buffers_main.cpp gives them malloc for an allocator
and is built and run as a program of its own under AddressSanitizer and UBSan — growth, the no-op, the failing allocator, swap,
move, release and the destructors."""
import os
import shutil
import subprocess

import pytest

from rope_s3d_amd import build

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))


def test_header_is_part_of_the_build_id_but_no_translation_unit():
    assert 'rope_buffers.h' in build._DEPS and 'rope_buffers.h' not in build._SOURCES


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_buffers_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'buffers_main')
    subprocess.check_call(['g++', '-std=c++17', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-fno-sanitize-recover=undefined', '-g',
                           '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'buffers_main.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout + r.stderr)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and r.stderr == ''
    assert lines[-1] == 'ok: nothing live at exit' and not [ln for ln in lines if ln.startswith('FAILED')]
    assert sum(ln.startswith('ok: ') for ln in lines) >= 2 * 15
