#!/usr/bin/env python3
"""Records what the compiler says the raster kernels of the shipped build need: rope_s3d_amd.build.resource_usage() compiles
csrc/rope_kernels.hip device-only with the product's flags and the kernel-resource-usage remarks, and this script writes

  * tests/golden/kernel_resources_gfx950.json — per instantiation of raster_score_kernel / raster_queue_kernel<LOSS, MODE, CLIP>
    the VGPR spills and the scratch bytes per lane, which tests/test_kernel_resources.py pins (the one unexplained
    wrong result of this project came from a kernel that had begun to spill, so a change in spilling must be seen);
  * profiles/kernel_resources_gfx950.txt — the same table with registers and occupancy, to read.

Before re-recording after a compiler update or an edit that moved the numbers, run tests/test_gpu_instantiations.py on a GPU
once: it holds every instantiation to its scratch-free twin and to the oracle.

    python tests/golden/make_kernel_resources.py        # one device-only compile, one to two minutes
"""
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, os.pardir, os.pardir))
sys.path.insert(0, ROOT)

from rope_s3d_amd import build  # noqa: E402

JSON_PATH = os.path.join(HERE, 'kernel_resources_gfx950.json')
TEXT_PATH = os.path.join(ROOT, 'profiles', 'kernel_resources_gfx950.txt')


def key(r) -> str:
    return f"{r['kernel']}<{r['loss']}, {r['mode']}, {'CLIP' if r['clip'] else 'plain'}>"


def compiler_version() -> str:
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    out = subprocess.run([hipcc, '--version'], capture_output=True, text=True).stdout
    return ' / '.join(l.strip() for l in out.splitlines() if 'version' in l.lower())


def main():
    if os.environ.get('ROPE_HIPCC_EXTRA'):
        sys.exit("ROPE_HIPCC_EXTRA is set: the committed table is the shipped build's")
    records = [r for r in build.resource_usage() if r['loss'] is not None]
    version = compiler_version()
    table = {key(r): {'vgpr_spills': r['vgpr_spills'], 'scratch_bytes': r['scratch_bytes']} for r in records}
    with open(JSON_PATH, 'w') as f:
        json.dump({'flags': build.HIPCC_FLAGS, 'compiler': version, 'kernels': table}, f, indent=1, sort_keys=True)
        f.write('\n')
    lines = ["Registers, spills and scratch of every raster kernel instantiation in the shipped build, as the compiler reports them",
             f"(hipcc {' '.join(build.HIPCC_FLAGS)} -Rpass-analysis=kernel-resource-usage, device-only; no GPU run).",
             f"compiler: {version}",
             "written by tests/golden/make_kernel_resources.py; tests/test_kernel_resources.py pins the two spill columns.", "",
             f"{'kernel':<52}{'VGPRs':>6}{'SGPRs':>6}{'VGPR spills':>12}{'SGPR spills':>12}{'scratch B/lane':>15}{'waves/SIMD':>11}"]
    for r in sorted(records, key=lambda r: (r['kernel'], r['clip'], build.MODE_NAMES.index(r['mode']), build.LOSS_NAMES.index(r['loss']))):
        lines.append(f"{key(r):<52}{r['vgprs']:>6}{r['sgprs']:>6}{r['vgpr_spills']:>12}{r['sgpr_spills']:>12}{r['scratch_bytes']:>15}{r['occupancy']:>11}")
    lines += ["", "SGPR spills go to lanes of a VGPR, not to memory: a kernel with SGPR spills and 0 scratch bytes touches no scratch.",
              "CLIP kernels are compiled for 3 waves/SIMD (ROPE_MIN_WAVES_CLIP, up to 168 VGPRs) so that they need none (DESIGN.md §6a)."]
    with open(TEXT_PATH, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(f"{len(records)} kernels -> {JSON_PATH}, {TEXT_PATH}")


if __name__ == '__main__':
    main()
