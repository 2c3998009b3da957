"""The kept fragments' plain C++ (csrc/rope_fragstore.h: the store's record, budget decision, scan and chunk plan) without a GPU:
tests/fragstore_main.cpp exercises them at their edges and is built as a program of its own under AddressSanitizer and UBSan."""
import os
import re
import subprocess

from rope_s3d_amd import build, engine

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), os.pardir))
CSRC = os.path.join(ROOT, 'rope_s3d_amd', 'csrc')


def test_header_is_plain_cxx_and_part_of_the_build_id():
    assert 'rope_fragstore.h' in build._DEPS
    with open(os.path.join(CSRC, 'rope_fragstore.h')) as f:
        src = f.read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', src)
    assert not [i for i in includes if i.startswith('hip/') or (i.startswith('rope_') and i != 'rope_geomcache.h')], \
        "rope_fragstore.h must build without HIP and without the context"


def test_flag_and_entries_are_declared_everywhere():
    with open(os.path.join(ROOT, 'include', 'rope_s3d.h')) as f:
        pub = f.read()
    with open(os.path.join(CSRC, 'rope_kernels.h')) as f:
        priv = f.read()
    assert re.search(r'ROPE_STRATEGY_NO_KEPT_FRAGMENTS\s*=\s*128\b', pub) and re.search(r'\bSTRATEGY_NO_KEPT_FRAGMENTS\s*=\s*128\b', priv)
    assert engine.Engine.NO_KEPT_FRAGMENTS == 128
    for name in ('rope_fragment_store_stats', 'rope_fragment_store_pairs', 'rope_set_fragment_budget'):
        assert name in engine.ABI_SYMBOLS and f'int {name}(' in pub


def test_default_budget_is_the_lookup_tables():
    from rope_s3d_amd.constants import GPU_MEMORY_ALLOWED_FOR_LOOKUP
    from rope_s3d_amd.simulation.lookup import DEFAULT_LOOKUP_VRAM_MIB
    with open(os.path.join(CSRC, 'rope_fragstore.h')) as f:
        m = re.search(r'FRAGMENT_DEFAULT_BUDGET\s*=\s*\(\(uint64_t\)(\d+)\s*<<\s*20\)\s*/\s*(\d+)\s*;', f.read())
    assert m and int(m.group(1)) == DEFAULT_LOOKUP_VRAM_MIB and 1.0 / int(m.group(2)) == GPU_MEMORY_ALLOWED_FOR_LOOKUP


def test_record_scan_and_chunks_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'fragstore_main')
    subprocess.check_call(['g++', '-std=c++17', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-fno-sanitize-recover=undefined',
                           '-g', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'fragstore_main.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and re.fullmatch(r'ok \d+\n', r.stdout), r.stdout + r.stderr
