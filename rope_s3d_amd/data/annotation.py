"""Mask R-CNN training data from renders: labelme JSON + PNG per frame, then a train / test / ignore split
(reference: robotpose/data/annotation.py:30-344, run by annotate.py).

Annotator is the host path, for callers that hold a colour render: colour masks, a dilation, the library's border follower
(rope_trace_contours, which restates cv2.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE)).  AutomaticAnnotator is the device
path: every frame of a dataset is rendered at its own joint angles and camera pose and turned into dilated label planes on the
device (rope_render_masks, one byte per pixel); host threads trace and write one chunk while the device works on the next.
Both write the same bytes for the same frame.  Deviations from the reference: the contours of one label come in
raster-scan order, and the PNG is this module's own encoding (labelme re-encodes the file it is given), with the same pixels.
"""
import base64
import json
import os
import random
import shutil
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import List

import numpy as np

from ..engine import trace_contours
from ..utils import cpu_budget

# labelme's __version__ stamped into every file (LabelFile.save); the reference's requirements do not pin labelme
LABELME_VERSION = '4.5.7'
# contours of fewer points are left out (annotation.py:84-86)
MIN_CONTOUR_POINTS = 20
# zlib level of the PNG: cv2.imwrite's default IMWRITE_PNG_COMPRESSION
PNG_LEVEL = 1


def dilate(mask: np.ndarray, size: int) -> np.ndarray:
    """cv2.dilate(mask, ones((size, size))) (expandRegion, utils.py:46-48): out(y, x) = max of mask over rows y - size//2 ..
    y - size//2 + size - 1 and the same columns; pixels outside the image add nothing.  Any integer dtype (bit planes too)."""
    a = size // 2
    h, w = mask.shape
    pad = np.zeros((h + size - 1, w + size - 1), mask.dtype)
    pad[a:a + h, a:a + w] = mask
    rows = pad[:, 0:w].copy()
    for j in range(1, size):
        rows |= pad[:, j:j + w]
    out = rows[0:h].copy()
    for j in range(1, size):
        out |= rows[j:j + h]
    return out


def encode_png(bgr: np.ndarray, level: int = PNG_LEVEL) -> bytes:
    """8-bit RGB PNG of a BGR image, as cv2.imwrite stores it (every row filter 0), with the standard library only."""
    img = np.ascontiguousarray(np.asarray(bgr, np.uint8)[..., ::-1])
    h, w = img.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), np.uint8)
    raw[:, 1:] = img.reshape(h, 3 * w)

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
            + chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + chunk(b'IEND', b''))


def label_shapes(planes: np.ndarray, labels: List[str], boxes=None) -> list:
    """labelme shapes of a label bit plane: label i is bit i; in label order, then in contour order."""
    shapes = []
    for b, label in enumerate(labels):
        for c in trace_contours(planes, b, None if boxes is None else boxes[b], MIN_CONTOUR_POINTS):
            shapes.append({'label': label, 'points': c.tolist(), 'group_id': None, 'shape_type': 'polygon', 'flags': {}})
    return shapes


def write_annotation(image: np.ndarray, shapes: list, path: str):
    """path.json (labelme LabelFile.save: keys in its order, indent 2) and path.png, the BGR image's pixels as RGB.
    imagePath is path + '.png', as the reference passes it (annotation.py:72,105-112)."""
    png = encode_png(image)
    data = {'version': LABELME_VERSION, 'flags': {}, 'shapes': shapes, 'imagePath': path + '.png',
            'imageData': base64.b64encode(png).decode('utf-8'), 'imageHeight': int(image.shape[0]),
            'imageWidth': int(image.shape[1])}
    json_path = path if path.endswith('.json') else path + '.json'
    with open(json_path, 'w') as f:
        json.dump(data, f, ensure_ascii=False, indent=2)
    with open(path + '.png', 'wb') as f:
        f.write(png)


class Annotator:
    """labelme-compatible annotation JSONs and PNGs from colour renders (annotation.py:30-127)."""

    def __init__(self, pad_size: int = 5, color_dict: dict = None):
        self.pad_size = pad_size
        if color_dict is not None:
            self.color_dict = color_dict

    def setDict(self, color_dict: dict):
        """Set the colour dict if it was not given to __init__."""
        self.color_dict = color_dict

    def label_planes(self, render: np.ndarray) -> np.ndarray:
        """Bit i of each pixel: the dilated mask of the i-th colour of color_dict (_mask_color, annotation.py:117-122)."""
        if len(self.color_dict) > 8:
            raise ValueError(f"at most 8 labels, got {len(self.color_dict)}")
        planes = np.zeros(render.shape[:2], np.uint8)
        for b, color in enumerate(self.color_dict.values()):
            planes |= np.all(render == np.asarray(color, render.dtype), axis=-1).astype(np.uint8) << b
        return dilate(planes, self.pad_size)

    def annotate(self, image: np.ndarray, render: np.ndarray, path: str):
        """Annotate `image` (BGR) from its colour `render`; writes path.json and path.png (no extension in `path`)."""
        write_annotation(image, label_shapes(self.label_planes(render), list(self.color_dict)), path)


class AutomaticAnnotator:
    """Per-link segmentation annotations of a whole dataset from renders at its recorded poses (annotation.py:130-214).
    preview=True opens no window here.  dest_path overrides the dataset's link_anno_path."""

    PAD_SIZE = 3                                    # annotation.py:156
    CHUNK = 64                                      # frames per rope_render_masks call

    def __init__(self, dataset, ds_renderer=None, preview: bool = True, dest_path: str = None):
        from ..simulation.render import DatasetRenderer
        self.preview = preview
        if ds_renderer is None:
            self.rend = DatasetRenderer(dataset, 'seg')
        else:
            self.rend = ds_renderer
            self.rend.setMode('seg')
        self.anno = Annotator(color_dict=self.rend.color_dict, pad_size=self.PAD_SIZE)
        self.ds = self.rend.ds
        self.dest_path = dest_path if dest_path is not None else self.ds.link_anno_path
        os.makedirs(self.dest_path, exist_ok=True)

    def _write_chunk(self, start: int, og: np.ndarray, masks: np.ndarray, boxes: np.ndarray, labels: list):
        for k in range(len(masks)):
            write_annotation(og[k], label_shapes(masks[k], labels, boxes[k]), os.path.join(self.dest_path, f"{start + k:05d}"))

    def run(self):
        """Clear the destination, annotate every frame, then split .4 / .1 (annotation.py:163-214)."""
        shutil.rmtree(self.dest_path, ignore_errors=True)
        os.makedirs(self.dest_path)
        labels = list(self.anno.color_dict)
        n = self.ds.length
        angles, poses = self.rend._ds_angles, self.rend._ds_poses
        threads = max(1, cpu_budget() - 1)
        with ThreadPoolExecutor(threads) as pool:
            pending = []
            for a in range(0, n, self.CHUNK):
                b = min(n, a + self.CHUNK)
                masks, boxes = self.rend.render_masks_batch(angles[a:b], poses[a:b], self.PAD_SIZE)
                og = np.asarray(self.ds.og_img[a:b])
                while len(pending) > 2 * threads:   # the threads write this chunk while the next one is drawn
                    pending.pop(0).result()
                for lo in range(0, b - a, 4):
                    hi = min(b - a, lo + 4)
                    pending.append(pool.submit(self._write_chunk, a + lo, og[lo:hi], masks[lo:hi], boxes[lo:hi], labels))
            for p in pending:
                p.result()
        Splitter(self.dest_path).split(.4, .1)


def _split_json(d: dict) -> str:
    """split.json as the reference's CompactJSONEncoder(indent=4) writes a dict of lists of names: the dict over lines, a list on
    one line when it has at most 6 names and its repr is at most 82 characters, else one name per line."""
    def lst(v):
        if len(v) <= 6 and len(str(v)) - 2 <= 80:
            return '[' + ', '.join(f'"{x}"' for x in v) + ']'
        return '[\n' + ',\n'.join(' ' * 8 + f'"{x}"' for x in v) + '\n' + ' ' * 4 + ']'
    return '{\n' + ',\n'.join(' ' * 4 + f'{json.dumps(k)}: {lst(v)}' for k, v in d.items()) + '\n}'


class Splitter:
    """Splits an annotation folder into train / test / ignore subfolders and keeps split.json (annotation.py:217-344).
    rng: a random.Random for the shuffles (the module's generator when None)."""

    def __init__(self, folder: str, rng: random.Random = None):
        self.folder = folder
        self.rng = rng if rng is not None else random
        self.all, self.train, self.test, self.ignore = [[] for _ in range(4)]
        self.past_split = True
        for fold in ['test', 'train', 'ignore']:
            os.makedirs(os.path.join(self.folder, fold), exist_ok=True)
        self.load()

    def load(self):
        """Read in the annotations in the folder: those of an earlier split, or new ones, which go to ignore/."""
        if os.path.isfile(os.path.join(self.folder, 'split.json')):
            self.past_split = True
            with open(os.path.join(self.folder, 'split.json')) as f:
                split_data = json.load(f)

            def read_in(subfolder, validation):
                names = os.listdir(os.path.join(self.folder, subfolder))
                js = [x.replace('.json', '') for x in names if x.endswith('.json')]
                png = [x.replace('.png', '') for x in names if x.endswith('.png')]
                lst = [x for x in js if x in png]
                assert all(x in validation for x in lst), \
                    f"Data error found for {subfolder} when loading data to split. Please re-annotate data."
                return lst
            self.train = read_in('train', split_data['train'])
            self.test = read_in('test', split_data['test'])
            self.ignore = read_in('ignore', split_data['ignore'])
        else:
            self.past_split = False
            jsons_p = [os.path.join(r, x) for r, _, y in os.walk(self.folder) for x in y
                       if x.endswith('.json') and x not in ['test.json', 'train.json']]
            png_p = [os.path.join(r, x) for r, _, y in os.walk(self.folder) for x in y if x.endswith('.png')]
            assert len(jsons_p) == len(png_p), "Error encountered in data split: unequal number of png's and json's"
            for file in [*jsons_p, *png_p]:
                dst = os.path.join(self.folder, 'ignore', os.path.basename(file))
                if os.path.abspath(file) != os.path.abspath(dst):
                    shutil.move(file, dst)
            self.train = []
            self.test = []
            self.ignore = [x.replace('.json', '') for x in os.listdir(os.path.join(self.folder, 'ignore')) if x.endswith('.json')]

    def _move(self, name: str, src: str, dst: str):
        for e in ['.json', '.png']:
            shutil.move(os.path.join(self.folder, src, f"{name}{e}"), os.path.join(self.folder, dst, f"{name}{e}"))

    def split(self, train_prop: float, valid_prop: float):
        """int(total * prop) files in train and test; files already placed stay where they are as far as the counts allow."""
        tot = len(self.train) + len(self.test) + len(self.ignore)
        num_train, num_test = int(tot * train_prop), int(tot * valid_prop)
        for num, lst, name in zip((num_train, num_test), (self.train, self.test), ('train', 'test')):
            if len(lst) > num:                      # too many: the surplus goes back to ignore
                self.rng.shuffle(lst)
                num_transfer = len(lst) - num
                for f in lst[:num_transfer]:
                    self.ignore.append(f)
                    self._move(f, name, 'ignore')
                del lst[:num_transfer]
        for num, lst, name in zip((num_train, num_test), (self.train, self.test), ('train', 'test')):
            if len(lst) < num:                      # too few: taken at random from ignore
                self.rng.shuffle(self.ignore)
                num_transfer = num - len(lst)
                for f in self.ignore[:num_transfer]:
                    lst.append(f)
                    self._move(f, 'ignore', name)
                del self.ignore[:num_transfer]
        self.write()

    def write(self):
        """Write split.json."""
        with open(os.path.join(self.folder, 'split.json'), 'w') as f:
            f.write(_split_json({'train': self.train, 'test': self.test, 'ignore': self.ignore}))

    @property
    def ratios(self):
        """The folder's proportions of train, test and ignore."""
        tot = len(self.train) + len(self.test) + len(self.ignore)
        return len(self.train) / tot, len(self.test) / tot, len(self.ignore) / tot

    def ratios_equal(self, train_prop: float, valid_prop: float) -> bool:
        """Whether the current split has the counts split(train_prop, valid_prop) would give."""
        tot = len(self.train) + len(self.test) + len(self.ignore)
        return int(tot * train_prop) == len(self.train) and int(tot * valid_prop) == len(self.test)

    def resplit(self, train_prop: float, valid_prop: float):
        """split() unless the proportions are already there."""
        if not self.ratios_equal(train_prop, valid_prop):
            self.split(train_prop, valid_prop)
