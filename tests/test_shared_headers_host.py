"""CPU: the text the normal-equation files and the polish files share exists once.  csrc/rope_neq.h and csrc/rope_solve.h are
headers: part of the build id, no translation units; and no source file of the library defines a copy of what they hold.
csrc/rope_lossmath.h and csrc/rope_launch.h, which the kernel files share, are held to the first half of that."""
import os
import re

from rope_s3d_amd import build

HEADERS = ('rope_neq.h', 'rope_solve.h', 'rope_lossmath.h', 'rope_launch.h')


def _text(name):
    with open(os.path.join(build._CSRC, name)) as f:
        return f.read()


def test_headers_are_part_of_the_build_id_but_no_translation_units():
    for h in HEADERS:
        assert h in build._DEPS and h not in build._SOURCES, h


def test_no_source_file_keeps_a_copy_of_the_shared_text():
    own = {s: [m for m in (re.search(r'\bstruct\s+Vec3\b', _text(s)), re.search(r'\bsolve_block\b', _text(s)),
                            re.search(r'^(?:static\s+|inline\s+)*(?:long long|int|size_t|unsigned)\s+\w*neq_chunks\s*\(', _text(s), re.M)) if m]      # the chunk rule (rope_abi.hip's render_chunks is another thing)
           for s in build._SOURCES}
    assert not any(own.values()), {s: [m.group(0) for m in ms] for s, ms in own.items() if ms}
    # and the headers do hold them: a check that finds nothing anywhere would pass as well
    assert re.search(r'\bstruct\s+Vec3\b', _text('rope_neq.h')) and re.search(r'^inline long long neq_chunks\s*\(', _text('rope_neq.h'), re.M)
    assert re.search(r'\bbool eliminate\s*\(', _text('rope_solve.h'))
    for s in ('rope_refine.hip', 'rope_bundle.hip', 'rope_silhouette.hip'):
        assert '#include "rope_neq.h"' in _text(s), s
    for s in ('rope_polish.hip', 'rope_bundle_polish.hip'):
        assert '#include "rope_solve.h"' in _text(s), s
