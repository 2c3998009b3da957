"""CPU: the host side of the photographs — the ABI of rope_shade_frames and what it refuses before anything touches a device, and
the 'photo:' dataset names as far as they go without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(helpers.__file__)))
FAKE = 0x10000                       # a pointer that is not null and never followed: every call below is refused or has N == 0


def _call(lib, depth=FAKE, ids=FAKE, N=1, H=4, W=4, n_links=6, params='default', bg=None, n_bg=0, bgr=FAKE, depth_out=None, edit=None):
    from rope_s3d_amd.simulation.shading import default_params
    if isinstance(params, str):
        params = default_params(max(N, 1))
        if edit:
            for k, v in edit.items():
                params[k][-1] = v
    ptr = params.ctypes.data_as(C.c_void_p) if params is not None else None
    return lib.rope_shade_frames(depth, ids, N, H, W, n_links, 500.0, 500.0, 2.0, 2.0, ptr, bg, n_bg, 0, 0, bgr, depth_out, None)


def test_symbol_is_declared_exported_and_built_from_rope_shade():
    from rope_s3d_amd import build, engine as eng
    hdr = open(os.path.join(ROOT, 'include', 'rope_s3d.h')).read()
    lib = eng.load_library()
    assert re.search(r'\bint rope_shade_frames\(', hdr) and 'typedef struct rope_shade_params' in hdr
    assert 'rope_shade_frames' in eng.ABI_SYMBOLS and len(lib.rope_shade_frames.argtypes) == 18
    assert all(lib.rope_shade_frames.argtypes[i] is C.c_float for i in (6, 7, 8, 9)) and lib.rope_shade_frames.argtypes[14] is C.c_uint64
    assert 'rope_shade.hip' in build._SOURCES and 'rope_shade.hip' in build._DEPS
    assert eng.SHADE_DTYPE.itemsize == 64 and eng.SHADE_DTYPE.fields['albedo'][1] == 40 and eng.SHADE_DTYPE.fields['bg_colour'][1] == 58
    assert int(re.search(r'#define ROPE_SHADE_MAX_NOISE_Q (\d+)', hdr).group(1)) == eng.SHADE_MAX_NOISE_Q == 1023


@pytest.mark.parametrize('kw', [
    dict(depth=None), dict(ids=None), dict(bgr=None), dict(params=None), dict(N=-1),
    dict(H=0), dict(W=0), dict(H=-3), dict(H=1 << 16, W=1 << 15), dict(H=46341, W=46341),
    dict(n_links=0), dict(n_links=7), dict(n_bg=-1),
    dict(edit={'bg_index': 0}), dict(edit={'bg_index': -2}), dict(edit={'bg_index': 2}, bg=FAKE, n_bg=2), dict(edit={'bg_index': 0}, n_bg=1),
    dict(N=3, edit={'bg_index': 1}, bg=FAKE, n_bg=1),
    dict(edit={'noise_q': -1}), dict(edit={'noise_q': 1024}), dict(N=2, edit={'noise_q': 5000}),
    dict(depth=FAKE + 2), dict(depth=FAKE + 1), dict(depth_out=FAKE + 3)])
def test_refusals_come_before_any_device(kw):
    from rope_s3d_amd import engine as eng
    assert _call(eng.load_library(), **kw) == -1          # ROPE_E_ARG; no GPU is here to launch on, and none was asked


def test_no_frames_succeed():
    from rope_s3d_amd import engine as eng
    lib = eng.load_library()
    assert _call(lib, N=0) == 0 and _call(lib, N=0, depth=None, ids=None, bgr=None, params=None) == 0
    assert _call(lib, N=0, H=0) == -1                     # the shape is checked all the same


def test_photo_names(tmp_path, monkeypatch):
    from rope_s3d_amd.data import dataset as D
    assert D.PhotoDataset.PREFIX == 'photo:' and issubclass(D.PhotoDataset, D.SyntheticDataset)
    assert D.PhotoDataset.parse_name('photo:64') == (64, 7919, '640_480_color')
    assert D.PhotoDataset.parse_name('photo:6:11:1280_720_color') == (6, 11, '1280_720_color')
    a, s = D.PhotoDataset.link_anno_path_of('photo:6:11'), D.SyntheticDataset.link_anno_path_of('synthetic:6:11')
    assert a != s and a.endswith(os.path.join('photo_6_11_640_480_color', 'link_annotations'))
    assert D.rendered_set_of('photo:4') is D.PhotoDataset and D.rendered_set_of('synthetic:4') is D.SyntheticDataset
    assert D.rendered_set_of('set10') is None and D.rendered_set_of(None) is None
    opened = []
    monkeypatch.setattr(D.PhotoDataset, 'from_name', classmethod(lambda cls, name, device=0: opened.append((cls, name, device)) or 'P'))
    monkeypatch.setattr(D.SyntheticDataset, 'from_name', classmethod(lambda cls, name, device=0: opened.append((cls, name, device)) or 'S'))
    assert D.open_dataset('photo:5:3', 1) == 'P' and D.open_dataset('synthetic:5') == 'S'
    assert opened == [(D.PhotoDataset, 'photo:5:3', 1), (D.SyntheticDataset, 'synthetic:5', 0)]
    with pytest.raises(ValueError):
        D.open_dataset(str(tmp_path / 'photo'))            # a stored set's name still goes to Dataset


def test_model_folder_for_a_photo_set_needs_no_render(tmp_path, monkeypatch):
    from rope_s3d_amd import models
    from rope_s3d_amd.data import dataset as D
    anno = tmp_path / 'anno'
    for sub, n in (('train', 3), ('test', 1)):
        (anno / sub).mkdir(parents=True)
        for i in range(n):
            (anno / sub / f'{i}.json').write_text('{}')
            (anno / sub / f'{i}.png').write_bytes(b'')
    monkeypatch.setattr(D.PhotoDataset, 'link_anno_path_of', classmethod(lambda cls, name: str(anno)))
    mm = models.ModelManager.__new__(models.ModelManager)
    mm.dir, mm.info = str(tmp_path / 'models'), {}
    os.makedirs(mm.dir)
    monkeypatch.setattr(models.ModelManager, 'update', lambda self: None)
    folder = mm.allocateNew('photo:8:5', ['a', 'b'], name='PHOTO')
    import json
    md = json.load(open(os.path.join(folder, models.MODELDATA_FILE_NAME)))
    assert md['dataset'] == 'photo:8:5' and md['dataset_size'] == 8 and md['train_size'] == 3 and md['valid_size'] == 1
