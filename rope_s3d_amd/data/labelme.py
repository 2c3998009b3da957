"""Reads the annotation folders `Splitter` makes (`train/`, `test/`: labelme JSON + PNG per frame) into training samples for
Mask R-CNN (reference: PixelLib 0.5.6 custom_train.load_dataset, which reads the same layout for train.py:51).

Every polygon shape is one ground-truth instance (PixelLib fills each one with skimage.draw.polygon).  The PNG decoder is
the standard library's zlib plus the five PNG row filters: this package's encoder writes filter 0 only, labelme and other
tools write the others."""
import base64
import glob
import json
import os
import struct
import zlib
from typing import List, Tuple

import numpy as np

_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}                  # colour type -> samples per pixel (8-bit, non-palette)


def _unfilter(raw: np.ndarray, h: int, stride: int, bpp: int) -> np.ndarray:
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    rows = raw.reshape(h, stride + 1)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 1:                                    # Sub: running sum per sample position
            cur = np.cumsum(line.reshape(-1, bpp), axis=0).reshape(-1) & 0xFF
        elif ft == 2:                                    # Up
            cur = (line + prev) & 0xFF
        elif ft in (3, 4):                               # Average, Paeth: pixel by pixel (bpp samples at once)
            cur = line.copy()
            for x in range(0, stride, bpp):
                a = cur[x - bpp:x] if x else np.zeros(bpp, np.int32)
                b = prev[x:x + bpp]
                if ft == 3:
                    cur[x:x + bpp] = (line[x:x + bpp] + ((a + b) >> 1)) & 0xFF
                else:
                    c = prev[x - bpp:x] if x else np.zeros(bpp, np.int32)
                    p = a + b - c
                    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
                    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
                    cur[x:x + bpp] = (line[x:x + bpp] + pred) & 0xFF
        else:
            raise ValueError(f"PNG row {y}: unknown filter type {ft}")
        out[y] = cur
        prev = cur
    return out


def decode_png(data: bytes) -> np.ndarray:
    """8-bit greyscale / grey+alpha / RGB / RGBA non-interlaced PNG -> (H, W, channels) uint8 (channels as stored)."""
    if data[:8] != _PNG_MAGIC:
        raise ValueError("not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError("PNG without IHDR")
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or ctype not in _CHANNELS or interlace:
        raise ValueError(f"unsupported PNG (bit depth {depth}, colour type {ctype}, interlace {interlace})")
    ch = _CHANNELS[ctype]
    raw = np.frombuffer(zlib.decompress(b''.join(idat)), np.uint8)
    return _unfilter(raw, h, w * ch, ch).reshape(h, w, ch)


def fill_polygon(points, shape) -> np.ndarray:
    """skimage.draw.polygon's mask (skimage 0.16 and later, the versions PixelLib 0.5.6 runs on): pixel (r, c) is set when
    point_in_polygon(centre (r, c)) is not OUTSIDE.  That test is O'Rourke's (Computational Geometry in C, 2nd ed., ch. 7),
    restated here: with the centre as origin, edge (i - 1, i) crosses the +x ray when (y_i > 0) != (y_{i-1} > 0) and the -x ray
    when (y_i < 0) != (y_{i-1} < 0), at x = (x_i y_{i-1} - x_{i-1} y_i) / (y_{i-1} - y_i); an odd count on one side and an even one
    on the other puts the centre on an edge, odd on both inside, and a centre equal to a vertex is a vertex.  So the rule is
    closed: centres on an edge or a vertex are inside.  skimage itself is not a dependency; the restatement could not be run
    against it.  points: (x, y) pairs as labelme stores them."""
    h, w = shape
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    mask = np.zeros((h, w), bool)
    if len(pts) < 3:
        return mask
    vx, vy = pts[:, 0], pts[:, 1]
    r0, r1 = max(0, int(np.floor(vy.min()))), min(h - 1, int(np.ceil(vy.max())))
    c0, c1 = max(0, int(np.floor(vx.min()))), min(w - 1, int(np.ceil(vx.max())))
    if r0 > r1 or c0 > c1:
        return mask
    R, Cc = np.meshgrid(np.arange(r0, r1 + 1, dtype=np.float64), np.arange(c0, c1 + 1, dtype=np.float64), indexing='ij')
    r_odd = np.zeros(R.shape, bool)
    l_odd = np.zeros(R.shape, bool)
    vertex = np.zeros(R.shape, bool)
    for i in range(len(pts)):
        x0, y0 = vx[i] - Cc, vy[i] - R
        x1, y1 = vx[i - 1] - Cc, vy[i - 1] - R
        vertex |= (x0 == 0) & (y0 == 0)
        r_cross = (y0 > 0) != (y1 > 0)
        l_cross = (y0 < 0) != (y1 < 0)
        cross = r_cross | l_cross                           # then y0 != y1
        with np.errstate(divide='ignore', invalid='ignore'):
            xi = np.where(cross, (x0 * y1 - x1 * y0) / np.where(cross, y1 - y0, 1.0), 0.0)
        r_odd ^= r_cross & (xi > 0)
        l_odd ^= l_cross & (xi < 0)
    mask[r0:r1 + 1, c0:c1 + 1] = vertex | r_odd | l_odd    # VERTEX, INSIDE (both odd) or EDGE (one odd)
    return mask


def read_annotation(json_path: str, classes: List[str]):
    """One labelme file -> (RGB image (H, W, 3) uint8, masks (G, H, W) bool, class ids (G,) int32, 1-based in `classes`).
    The image is the PNG beside the JSON, else the embedded imageData.  Shapes of other labels are skipped."""
    with open(json_path) as f:
        d = json.load(f)
    png = os.path.splitext(json_path)[0] + '.png'
    if os.path.isfile(png):
        with open(png, 'rb') as f:
            img = decode_png(f.read())
    else:
        img = decode_png(base64.b64decode(d['imageData']))
    img = img[..., :3] if img.shape[2] >= 3 else np.repeat(img[..., :1], 3, axis=2)
    h, w = img.shape[:2]
    masks, ids = [], []
    for s in d.get('shapes', []):
        if s.get('shape_type', 'polygon') != 'polygon' or s['label'] not in classes:
            continue
        masks.append(fill_polygon(s['points'], (h, w)))
        ids.append(classes.index(s['label']) + 1)
    m = np.stack(masks) if masks else np.zeros((0, h, w), bool)
    return np.ascontiguousarray(img), m, np.asarray(ids, np.int32)


def split_files(folder: str) -> Tuple[List[str], List[str]]:
    """The labelme JSON files of `folder/train` and `folder/test` (sorted).  Raises when the split does not exist."""
    out = []
    for sub in ('train', 'test'):
        d = os.path.join(folder, sub)
        files = sorted(glob.glob(os.path.join(d, '*.json')))
        if not files:
            raise FileNotFoundError(f"no annotated split in {d}: run annotate.py on the dataset first (it annotates and splits)")
        out.append(files)
    return out[0], out[1]
