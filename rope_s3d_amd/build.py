"""Builds librope_hip.so (gfx950) in-tree with hipcc.  Cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess
import tempfile

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
LIB_PATH = os.path.join(_CSRC, 'librope_hip.so')
_SOURCES = ['rope_kernels.hip', 'rope_fragments.hip', 'rope_table.hip', 'rope_abi.hip', 'rope_abi_targets.hip',
            'rope_hostprep.cpp', 'rope_seg.hip', 'rope_masks.hip',
            'rope_predict.cpp', 'rope_meshlets.cpp', 'rope_contours.cpp', 'rope_train.hip', 'rope_targets.hip', 'rope_synth.hip',
            'rope_eval.hip', 'rope_verify.hip', 'rope_feed.hip', 'rope_shade.hip', 'rope_refine.hip', 'rope_bundle.hip', 'rope_silhouette.hip',
            'rope_silhouette_reverse.hip', 'rope_polish.hip', 'rope_bundle_polish.hip', 'rope_robust.hip']
_DEPS = _SOURCES + ['rope_kernels.h', 'rope_lossmath.h', 'rope_launch.h', 'rope_buffers.h', 'rope_ctx.h', 'rope_geomcache.h', 'rope_fragstore.h', 'rope_passplan.h', 'rope_fk.h', 'rope_neq.h', 'rope_solve.h', os.path.join('..', '..', 'include', 'rope_s3d.h')]

# -ffp-contract=off: the arithmetic contract with the CPU oracle is "one IEEE operation per
# written step"; fused operations appear only where the source says fmaf.
HIPCC_FLAGS = ['-O3', '--offload-arch=gfx950', '-ffp-contract=off', '-fPIC', '-shared', '-std=c++17']


def source_hash() -> str:
    """Identity of what the library is built from: SHA-256 over the sources and headers (first 16 hex digits).  Compiled into the
    library (rope_build_id) and written into the profiles (tools/summarize_prof.py), so that bench.py can tell whether the
    committed counters belong to the build it is timing."""
    import hashlib
    h = hashlib.sha256()
    for d in sorted(_DEPS):
        h.update(d.encode())
        with open(os.path.join(_CSRC, d), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _built_id(path: str) -> str:
    try:
        with open(path + '.id') as f:
            return f.read().strip()
    except OSError:
        return ''


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    built = _built_id(LIB_PATH)
    if built:                                           # the library says what it was built from: time stamps do not survive a copy
        return built != source_hash()
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(os.path.join(_CSRC, d)) > t for d in _DEPS)


def build(force: bool = False, verbose: bool = False, out_name: str = 'librope_hip.so') -> str:
    if not force and not needs_build() and out_name == 'librope_hip.so':
        return LIB_PATH
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    extra = os.environ.get('ROPE_HIPCC_EXTRA', '').split()      # experiments only, e.g. -DROPE_SMALL_TRI_PIXELS=8
    build_id = source_hash()
    cmd = [hipcc] + HIPCC_FLAGS + [f'-DROPE_BUILD_ID="{build_id}"'] + extra + _SOURCES + ['-o', out_name]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd, cwd=_CSRC)
    with open(os.path.join(_CSRC, out_name) + '.id', 'w') as f:         # beside the library (git-ignored like it): needs_build reads it
        f.write(build_id + '\n')
    return os.path.join(_CSRC, out_name)


# Template arguments of raster_score_kernel / raster_queue_kernel<LOSS, MODE, CLIP> by value (include/rope_s3d.h, rope_kernels.h)
LOSS_NAMES = ('DEPTH', 'FULL', 'LOOKUP', 'TSWEEP', 'CAMFULL')
MODE_NAMES = ('SCORE', 'DUMP', 'COVER', 'LAYER', 'TABLE', 'SPLIT', 'SPLIT_GEO')
_REMARK = '-Rpass-analysis=kernel-resource-usage'
_FIELDS = {'VGPRs': 'vgprs', 'AGPRs': 'agprs', 'TotalSGPRs': 'sgprs', 'VGPRs Spill': 'vgpr_spills', 'SGPRs Spill': 'sgpr_spills',
           'ScratchSize [bytes/lane]': 'scratch_bytes', 'Occupancy [waves/SIMD]': 'occupancy', 'LDS Size [bytes/block]': 'lds_bytes'}


def parse_resource_remarks(text: str) -> list:
    """The compiler's kernel-resource-usage remarks -> one record per kernel, in the order reported.  The template arguments are
    read off the Itanium-mangled name, where they stand as literals (raster_queue_kernelILi4ELi0ELb1EE = <4, 0, true>): that
    needs no demangler, which not every ROCm tree ships."""
    records, cur = [], None
    for line in text.splitlines():
        m = re.search(r'remark:\s+(.*?)\s*\[' + re.escape(_REMARK) + r'\]', line)
        if not m:
            continue
        key, _, value = m.group(1).partition(': ')
        if key == 'Function Name':
            t = re.match(r'_ZN4rope\d+(\w+?)ILi(\d+)ELi(\d+)ELb([01])EE', value)
            n = re.match(r'_ZN4rope\d+([A-Za-z_]\w*?kernel)', value)
            cur = {'symbol': value, 'kernel': t.group(1) if t else (n.group(1) if n else value), 'loss': None, 'mode': None, 'clip': None}
            if t:
                cur.update(loss=LOSS_NAMES[int(t.group(2))], mode=MODE_NAMES[int(t.group(3))], clip=t.group(4) == '1')
            records.append(cur)
        elif cur is not None and key in _FIELDS:
            cur[_FIELDS[key]] = int(value)
    return records


def resource_usage(source: str = 'rope_kernels.hip') -> list:
    """What the compiler says every kernel of `source` (a file of _SOURCES; rope_kernels.hip unless asked) needs in the shipped build: a device-only compile with HIPCC_FLAGS
    (and ROPE_HIPCC_EXTRA, so that a variant is judged by the same rule) plus the resource-usage remarks, into a temporary
    directory — librope_hip.so is neither read nor written.  -> records {symbol, kernel, loss, mode, clip (None outside the raster
    templates), vgprs, agprs, sgprs, vgpr_spills, sgpr_spills, scratch_bytes (per lane), occupancy (waves/SIMD), lds_bytes}."""
    if source not in _SOURCES:
        raise ValueError(f"{source}: not a source of the library ({', '.join(_SOURCES)})")
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    extra = os.environ.get('ROPE_HIPCC_EXTRA', '').split()
    flags = [f for f in HIPCC_FLAGS if f != '-shared']
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc] + flags + [f'-DROPE_BUILD_ID="{source_hash()}"'] + extra + ['--cuda-device-only', '-c', _REMARK, source,
                                                                                 '-o', os.path.join(tmp, os.path.splitext(source)[0] + '.device.o')]
        r = subprocess.run(cmd, cwd=_CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-4000:]}")
    records = parse_resource_remarks(r.stderr)
    if not records:
        raise RuntimeError(f"{hipcc} printed no {_REMARK} remarks")
    return records


if __name__ == '__main__':
    print(build(force=True, verbose=True))
