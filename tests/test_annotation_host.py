"""Annotation on the host (no GPU): the numpy dilation against scipy, the library's border follower (rope_trace_contours) on
hand-derived cases, against the paper-form restatement in tests/contour_ref.py and against topological counts, the labelme
JSON + PNG files, and the Splitter."""
import base64
import json
import os
import random
import struct
import zlib

import numpy as np
import pytest
from scipy import ndimage

from rope_s3d_amd import engine as eng
from rope_s3d_amd.data import annotation as ann

import contour_ref


def trace(mask, bit=0, box=None, min_points=0):
    return [c.tolist() for c in eng.trace_contours(np.asarray(mask, np.uint8) << bit, bit, box, min_points)]


# ---------------------------------------------------------------------------------------------------------- dilation --

def cv2_dilate_by_scipy(mask, size):
    """cv2.dilate with ones((size, size)) and anchor size // 2: out(y, x) = OR over y - a .. y - a + size - 1.  scipy centres the
    structure at size // 2 too but mirrors it: origin shifted by -1 for even sizes gives the same window."""
    origin = -1 if size % 2 == 0 else 0
    return ndimage.binary_dilation(mask, np.ones((size, size), bool), origin=origin)


@pytest.mark.parametrize('size', range(1, 10))
def test_dilate_matches_scipy(size):
    rng = np.random.default_rng(size)
    for _ in range(20):
        h, w = rng.integers(1, 25, 2)
        m = rng.random((h, w)) < 0.08
        m[0, rng.integers(w)] = m[-1, rng.integers(w)] = m[rng.integers(h), 0] = m[rng.integers(h), -1] = True   # every edge
        got = ann.dilate(m.astype(np.uint8), size)
        assert np.array_equal(got.astype(bool), cv2_dilate_by_scipy(m, size)), (size, h, w)


def test_dilate_anchor_even_size():
    # one pixel at (2, 2), size 4, anchor 2: out(y, x) is set when 2 in y - 2 .. y + 1, i.e. y in 1 .. 4 (likewise x)
    m = np.zeros((6, 6), np.uint8)
    m[2, 2] = 1
    out = ann.dilate(m, 4)
    assert np.argwhere(out).min(0).tolist() == [1, 1] and np.argwhere(out).max(0).tolist() == [4, 4]


def test_dilate_bits_independent():
    rng = np.random.default_rng(3)
    planes = rng.integers(0, 256, (30, 40), dtype=np.uint8) & (rng.random((30, 40)) < 0.05) * 255
    out = ann.dilate(planes.astype(np.uint8), 5)
    for b in range(8):
        assert np.array_equal((out >> b) & 1, ann.dilate(((planes >> b) & 1).astype(np.uint8), 5))


# ------------------------------------------------------------------------------------------------- tracer, by hand --

def test_single_pixel():
    # an outer start whose clockwise search finds no neighbour: the isolated-pixel branch writes the start point only
    m = np.zeros((5, 5), np.uint8)
    m[2, 3] = 1
    assert trace(m) == [[[3, 2]]]


def test_filled_rectangle():
    # outer start at the top-left (x0, y0).  The first step is the first set neighbour counter-clockwise after east: south.
    # The chain runs down the left side to (x0, y1), turns east to (x1, y1), north to (x1, y0), west back to the start:
    # the four corners are the points where the direction changes.
    x0, y0, x1, y1 = 2, 1, 6, 4
    m = np.zeros((7, 9), np.uint8)
    m[y0:y1 + 1, x0:x1 + 1] = 1
    assert trace(m) == [[[x0, y0], [x0, y1], [x1, y1], [x1, y0]]]


def test_rectangle_flush_with_the_edges():
    # the frame of zeros that findContours adds makes the edge pixels border pixels: the same four corners, on the edges
    m = np.ones((5, 7), np.uint8)
    assert trace(m) == [[[0, 0], [0, 4], [6, 4], [6, 0]]]


def test_one_pixel_line():
    # a horizontal line: out east to the far end, then back west along the same pixels; the start and the far end are
    # the only direction changes
    m = np.zeros((3, 8), np.uint8)
    m[1, 2:7] = 1
    assert trace(m) == [[[2, 1], [6, 1]]]


def test_diagonal_pair_is_one_contour():
    # (1, 1) and (2, 2) touch by a corner: 8-connected, one component, one outer border there and back
    m = np.zeros((4, 4), np.uint8)
    m[1, 1] = m[2, 2] = 1
    assert trace(m) == [[[1, 1], [2, 2]]]


def test_square_ring_outer_and_hole():
    # 5 x 5 ring, 3 x 3 hole.  Outer: the four corners as for the rectangle.  The hole border starts at the scan's first
    # 1 -> 0 step into the hole, (0, 1); following it with the hole on the walker's side visits the inner ring, whose
    # direction changes are at the pixels diagonal to the hole's corners.
    m = np.ones((5, 5), np.uint8)
    m[1:4, 1:4] = 0
    outer, hole = trace(m)
    assert outer == [[0, 0], [0, 4], [4, 4], [4, 0]]
    assert hole == [[0, 1], [1, 0], [3, 0], [4, 1], [4, 3], [3, 4], [1, 4], [0, 3]]
    assert contour_ref.find_contours(m)[1][1] is True


def test_bit_and_box_select():
    m = np.zeros((10, 12), np.uint8)
    m[2:5, 3:8] |= 4                       # bit 2
    m[6:9, 1:3] |= 1                       # bit 0
    whole = eng.trace_contours(m, 2)
    boxed = eng.trace_contours(m, 2, (2, 4, 3, 7))
    assert [c.tolist() for c in whole] == [c.tolist() for c in boxed] == [[[3, 2], [3, 4], [7, 4], [7, 2]]]
    assert eng.trace_contours(m, 5) == [] and eng.trace_contours(m, 5, (-1, -1, -1, -1)) == []


def test_min_points_filter():
    m = np.zeros((8, 8), np.uint8)
    m[1:6, 1:6] = 1                        # 4 points
    assert len(eng.trace_contours(m, 0, None, 4)) == 1 and eng.trace_contours(m, 0, None, 5) == []


def test_large_output_grows_buffers():
    m = (np.indices((64, 64)).sum(0) % 2).astype(np.uint8)      # a checkerboard: one 8-connected component, hundreds of holes
    got = eng.trace_contours(m, 0)
    ref = contour_ref.find_contours(m)
    assert len(got) == len(ref) > 65 and all(np.array_equal(a, b) for a, (b, _) in zip(got, ref))


# ---------------------------------------------------------------------------------------- tracer, second implementation --

def random_mask(rng):
    h, w = rng.integers(1, 48, 2)
    kind = rng.integers(3)
    if kind == 0:                          # salt: many holes and thin parts
        m = rng.random((h, w)) < rng.uniform(0.2, 0.8)
    elif kind == 1:                        # blobs with holes
        m = ndimage.binary_dilation(rng.random((h, w)) < 0.05, np.ones((3, 3), bool)) & ~(rng.random((h, w)) < 0.1)
    else:                                  # rings touching the edges
        yy, xx = np.indices((h, w))
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, 20)
        d = np.hypot(yy - cy, xx - cx)
        m = (d < r) & (d > r * rng.uniform(0.2, 0.8))
    return m.astype(np.uint8)


def test_tracer_matches_second_implementation():
    rng = np.random.default_rng(20211)
    for n in range(300):
        m = random_mask(rng)
        bit = int(rng.integers(8))
        got = eng.trace_contours(m << bit, bit)
        ref = contour_ref.find_contours(m)
        assert len(got) == len(ref), n
        for a, (b, _) in zip(got, ref):
            assert np.array_equal(a, b), n


# ----------------------------------------------------------------------------------------------- tracer, properties --

def test_tracer_properties():
    rng = np.random.default_rng(77)
    st8 = np.ones((3, 3), int)
    for n in range(200):
        m = random_mask(rng)
        h, w = m.shape
        conts = eng.trace_contours(m, 0)
        holes = [is_hole for _, is_hole in contour_ref.find_contours(m)]
        assert len(holes) == len(conts)
        _, n8 = ndimage.label(m, st8)
        assert holes.count(False) == n8, n                          # one outer border per 8-connected component
        bg, nb = ndimage.label(np.pad(1 - m, 1, constant_values=1))  # 4-connected background, frame included
        assert holes.count(True) == nb - 1, n                       # one hole border per enclosed background component
        for c in conts:
            for x, y in c:
                assert m[y, x] == 1
                edge = x in (0, w - 1) or y in (0, h - 1)
                assert edge or min(m[y - 1, x], m[y + 1, x], m[y, x - 1], m[y, x + 1]) == 0
            for (xa, ya), (xb, yb) in zip(c, np.roll(c, -1, 0)):
                dx, dy = xb - xa, yb - ya
                k = max(abs(dx), abs(dy))
                assert dx in (0, k, -k) and dy in (0, k, -k)         # a straight 8-direction run ...
                for s in range(k + 1):                              # ... of set pixels
                    assert m[ya + (dy // k if k else 0) * s, xa + (dx // k if k else 0) * s] == 1


# -------------------------------------------------------------------------------------------------------------- files --

def decode_png(data: bytes) -> np.ndarray:
    """Standard-library PNG reader for 8-bit RGB, any of the five row filters."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, hdr = 8, b'', None
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat += body
        pos += 12 + n
    w, h, depth, ctype = hdr[:4]
    assert depth == 8 and ctype == 2
    raw = zlib.decompress(idat)
    stride, bpp = 3 * w, 3
    out = np.zeros((h, stride), np.int64)
    prev = np.zeros(stride, np.int64)
    for y in range(h):
        f = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        cur = np.zeros(stride, np.int64)
        for i in range(stride):
            a = cur[i - bpp] if i >= bpp else 0
            b, c = prev[i], (prev[i - bpp] if i >= bpp else 0)
            p = a + b - c
            paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
            pred = (0, a, b, (a + b) // 2, paeth)[f]
            cur[i] = (line[i] + pred) & 0xFF
        out[y], prev = cur, cur
    return out.reshape(h, w, 3).astype(np.uint8)


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    og = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    data = ann.encode_png(og)
    assert np.array_equal(decode_png(data), og[..., ::-1])


def test_annotation_files(tmp_path):
    rng = np.random.default_rng(9)
    H, W = 48, 64
    og = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    render = np.zeros((H, W, 3), np.uint8)
    colours = {'base': [0, 0, 85], 'arm': [0, 0, 170]}
    yy, xx = np.indices((H, W))
    render[np.hypot(yy - 14, xx - 16) < 11] = colours['base']           # a disc: many direction changes, kept
    render[2:5, 52:55] = colours['arm']                                 # a square: 4 points after dilation, dropped
    ring = np.hypot(yy - 34, xx - 44) < 14
    ring &= ((yy - 34) / 11) ** 2 + ((xx - 44) / 7) ** 2 > 1            # its hole border is a polygon of the same label
    render[ring] = colours['arm']
    a = ann.Annotator(pad_size=3, color_dict=colours)
    path = str(tmp_path / '00000')
    a.annotate(og, render, path)
    data = json.load(open(path + '.json'))
    assert list(data) == ['version', 'flags', 'shapes', 'imagePath', 'imageData', 'imageHeight', 'imageWidth']
    assert data['version'] == ann.LABELME_VERSION and data['flags'] == {}
    assert data['imagePath'] == path + '.png' and data['imageHeight'] == H and data['imageWidth'] == W
    png = open(path + '.png', 'rb').read()
    assert base64.b64decode(data['imageData']) == png
    assert np.array_equal(decode_png(png), og[..., ::-1])
    for s in data['shapes']:
        assert list(s) == ['label', 'points', 'group_id', 'shape_type', 'flags']
        assert s['group_id'] is None and s['shape_type'] == 'polygon' and s['flags'] == {} and len(s['points']) >= 20
    # expected shapes: the traced contours of the dilated masks, label order, contours of at least 20 points
    planes = a.label_planes(render)
    want = []
    for b, label in enumerate(colours):
        for c in eng.trace_contours(planes, b):
            if len(c) >= 20:
                want.append((label, c.tolist()))
    assert [(s['label'], s['points']) for s in data['shapes']] == want
    labels = [s['label'] for s in data['shapes']]
    assert labels == sorted(labels, key=list(colours).index) and labels.count('arm') >= 2       # the hole is kept
    all_arm = [len(c) for c in eng.trace_contours(planes, 1)]
    assert min(all_arm) < 20                                   # the filter dropped the small square
    text = open(path + '.json').read()
    assert text == json.dumps(data, ensure_ascii=False, indent=2)


# ----------------------------------------------------------------------------------------------------------- splitter --

def make_files(folder, n):
    os.makedirs(folder, exist_ok=True)
    for i in range(n):
        for e in ('.json', '.png'):
            open(os.path.join(folder, f'{i:05d}{e}'), 'w').write('x')


def test_splitter_counts_and_conservation(tmp_path):
    folder = str(tmp_path / 'anno')
    make_files(folder, 23)
    s = ann.Splitter(folder, rng=random.Random(1))
    assert not s.past_split and len(s.ignore) == 23
    s.split(.4, .1)
    assert (len(s.train), len(s.test), len(s.ignore)) == (int(23 * .4), int(23 * .1), 23 - 9 - 2)
    for name, lst in (('train', s.train), ('test', s.test), ('ignore', s.ignore)):
        assert sorted(x[:-5] for x in os.listdir(os.path.join(folder, name)) if x.endswith('.json')) == sorted(lst)
    d = json.load(open(os.path.join(folder, 'split.json')))
    assert d == {'train': s.train, 'test': s.test, 'ignore': s.ignore}
    before_train = set(s.train)
    s.split(.5, .1)                                            # growing train keeps the files already there
    assert before_train <= set(s.train) and len(s.train) == int(23 * .5)
    # load path: an existing split is read back as it is
    s2 = ann.Splitter(folder, rng=random.Random(2))
    assert s2.past_split and sorted(s2.train) == sorted(s.train) and sorted(s2.ignore) == sorted(s.ignore)
    assert s2.ratios_equal(.5, .1) and not s2.ratios_equal(.4, .1)
    s2.resplit(.4, .1)
    assert len(s2.train) == int(23 * .4) and set(s2.train) <= set(s.train)
    assert abs(sum(s2.ratios) - 1) < 1e-12


def test_split_json_format(tmp_path):
    # the reference's CompactJSONEncoder(indent=4): a short list on one line, a long one a name per line
    short = ann._split_json({'train': ['00001', '00002'], 'test': [], 'ignore': [f'{i:05d}' for i in range(7)]})
    assert short == ('{\n    "train": ["00001", "00002"],\n    "test": [],\n    "ignore": [\n'
                     + ',\n'.join(f'        "{i:05d}"' for i in range(7)) + '\n    ]\n}')


def test_dataset_link_anno_path(tmp_path):
    from rope_s3d_amd.data.dataset import Dataset, write_dataset
    d = write_dataset(str(tmp_path / 'set'), np.zeros((2, 4, 6, 3), np.uint8), np.zeros((2, 4, 6)), np.zeros((2, 6)),
                      np.zeros((2, 6)), '640_480_color')
    assert Dataset(d).link_anno_path == os.path.join(d, 'link_annotations')           # the reference's dataset.py:191
