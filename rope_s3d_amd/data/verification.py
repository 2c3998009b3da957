"""Does every frame of a dataset show the robot where its recorded joint angles put it?  (reference: robotpose/data/verification.py)

Annotation, training and the accuracy tables take angles[i] as the truth about frame i; a pose logged late or a stale image makes
it a lie.  The reference's Verifier renders every frame at its recorded pose, blends the render over the photograph
(verification.py:58-67, :222) and has a person click the bad frames away.  Here the frame's depth map is compared with the
render's depth pixel by pixel on the device (rope_frame_agreement, csrc/rope_verify.hip): exact integer sums per frame come back,
28 numbers each, and the table, the outlier rule and the removal are host arithmetic on them.

  Verifier(dataset).run()       the table: per frame the mean absolute depth difference over the pixels both rendered and
                                measured, and how many of them agree, are occluded, or lie behind the render
  .flagged()                    the frames to question: nothing measured under the render, or a mean difference above the upper
                                fence Q3 + 1.5 IQR of the set (the reference's own outlier rule, utils.py:68-80)
  .sheets(folder, idxs)         the reference's overlays of those frames as PNG contact sheets, for the person who decides
  .remove(idxs)                 the set without them (Builder.remove_idxs, building.py:77-91)

The GUI's click-through and its VERIFIER_SELECTED_GAMMA are not here."""
import os
import shutil

import numpy as np

from ..constants import THUMBNAIL_DS_FACTOR, VERIFIER_ALPHA, VERIFIER_COLUMNS, VERIFIER_ROWS, VERIFIER_SCALER
from ..engine import AGREE_WORDS, Q32

IQR_MULT = 1.5                                   # utils.py:68: outlier_min_max / reject_outliers_iqr's default


def agreement_table(sums, n_links: int) -> dict:
    """The (N, 28) sums of rope_frame_agreement as a table of float64 / int64 columns, one row per frame:
      valid, rendered, both, bad_ids   pixel counts (both: rendered and measured; bad_ids: ids of no link, should be 0)
      mean_abs_diff                    [2] / both / 2^32 in metres; NaN where both == 0
      coverage                         both / rendered; NaN where nothing is rendered
      close, front, behind             shares of both: within the tolerance, the recording nearer than the render (something
                                       stands before the robot), the recording farther (behind = both - close - front); NaN
                                       where both == 0
      links                            {'rendered', 'both', 'coverage', 'close', 'front', 'behind'}: the same per link, (N, n_links)"""
    s = np.asarray(sums).astype(np.uint64, copy=False).reshape(-1, AGREE_WORDS)
    per = s[:, 4:4 + 4 * n_links].astype(np.int64).reshape(len(s), n_links, 4)
    rendered_l, both_l, close_l, front_l = (per[:, :, k] for k in range(4))

    def share(a, b):
        out = np.full(np.shape(b), np.nan)
        np.divide(a, b, out=out, where=np.asarray(b) > 0)
        return out
    both, close, front = both_l.sum(axis=1), close_l.sum(axis=1), front_l.sum(axis=1)
    rendered = s[:, 1].astype(np.int64)
    return {'valid': s[:, 0].astype(np.int64), 'rendered': rendered, 'both': both, 'bad_ids': s[:, 3].astype(np.int64),
            'mean_abs_diff': share(s[:, 2].astype(np.float64), both) / Q32,
            'coverage': share(both, rendered), 'close': share(close, both), 'front': share(front, both),
            'behind': share(both - close - front, both),
            'links': {'rendered': rendered_l, 'both': both_l, 'coverage': share(both_l, rendered_l), 'close': share(close_l, both_l),
                      'front': share(front_l, both_l), 'behind': share(both_l - close_l - front_l, both_l)}}


def upper_fence(data, iqr_mult: float = IQR_MULT) -> float:
    """Q3 + iqr_mult IQR as reject_outliers_iqr computes it (utils.py:72-75): np.percentile(data, [75, 25])."""
    percentiles = np.percentile(np.asarray(data, np.float64), [75, 25])
    return float(percentiles[0] + iqr_mult * np.subtract(*percentiles))


def flag_frames(table: dict):
    """-> (flagged, unrendered) frame indices, ascending.  Flagged: nothing measured under a render that is there, or a mean
    difference above the upper fence of the frames that have one.  Frames with nothing rendered say nothing either way."""
    both, rendered, m = table['both'], table['rendered'], table['mean_abs_diff']
    scored = both > 0
    bad = (rendered > 0) & ~scored
    if scored.any():
        bad |= scored & (np.where(scored, m, 0.0) > upper_fence(m[scored]))
    return np.nonzero(bad)[0], np.nonzero(rendered == 0)[0]


def blend(a, alpha: float, b, beta: float, gamma: float = 0.0) -> np.ndarray:
    """cv2.addWeighted(a, alpha, b, beta, gamma) on uint8 images: a alpha + b beta + gamma in float32 (OpenCV takes the weights as
    floats for 8-bit images), rounded half to even, saturated to 0..255."""
    x = np.asarray(a, np.uint8).astype(np.float32) * np.float32(alpha) + np.asarray(b, np.uint8).astype(np.float32) * np.float32(beta)
    return np.clip(np.rint(x + np.float32(gamma)), 0, 255).astype(np.uint8)


def contact_sheets(overlays, rows: int = VERIFIER_ROWS, columns: int = VERIFIER_COLUMNS) -> list:
    """(K, h, w, 3) overlays -> sheets (rows h, columns w, 3), filled row by row as the reference's window is; black where a
    sheet has fewer."""
    overlays = np.asarray(overlays, np.uint8)
    k, h, w = overlays.shape[:3]
    sheets = []
    for a in range(0, k, rows * columns):
        sheet = np.zeros((rows * h, columns * w, 3), np.uint8)
        for j, img in enumerate(overlays[a:a + rows * columns]):
            r, c = divmod(j, columns)
            sheet[r * h:(r + 1) * h, c * w:(c + 1) * w] = img
        sheets.append(sheet)
    return sheets


class Verifier:
    """Scores every frame of a dataset against the render at its recorded joint angles and camera pose.
      dataset      a name (open_dataset: 'synthetic:...' too) or an opened Dataset / SyntheticDataset
      batch        frames per device batch: one render, one upload of depth maps, one rope_frame_agreement call
      tol          metres within which a recorded depth counts as agreeing with the render (the 'close' share); a power of two,
                   so that its Q32 form is exact.  The flag rule does not depend on it
      ds_renderer  a DatasetRenderer of the dataset to draw with; made when first needed otherwise"""

    def __init__(self, dataset, batch: int = 64, tol: float = 2 ** -5, ds_renderer=None):
        if batch < 1:
            raise ValueError("batch must be at least 1")
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError(f"tol must be finite and not negative, got {tol}")
        self.batch, self.tol = int(batch), float(tol)
        self._rend = ds_renderer
        if ds_renderer is not None and not isinstance(dataset, str):
            self.ds = dataset
        elif ds_renderer is not None:
            self.ds = ds_renderer.ds
        else:
            from .dataset import open_dataset
            self.ds = open_dataset(dataset) if isinstance(dataset, str) else dataset
        self.sums = self.table = None

    def _renderer(self, mode: str):
        if self._rend is None:
            from ..simulation.render import DatasetRenderer
            self._rend = DatasetRenderer(self.ds, mode)
        self._rend.setMode(mode)
        return self._rend

    @property
    def thumbnail_size(self):
        """(h, w) of an overlay: the dataset's thumbnails (the frame over THUMBNAIL_DS_FACTOR) times VERIFIER_SCALER
        (verification.py:48)."""
        pv = getattr(self.ds, 'preview_img', None)
        th, tw = pv.shape[1:3] if pv is not None else (s // THUMBNAIL_DS_FACTOR for s in self.ds.og_img.shape[1:3])
        return max(1, int(th * VERIFIER_SCALER)), max(1, int(tw * VERIFIER_SCALER))

    def run(self) -> dict:
        """Every frame against its render -> agreement_table of the (N, 28) sums (kept in .sums / .table)."""
        import torch
        rend = self._renderer('seg')
        n, (H, W) = self.ds.length, rend.resolution
        angles, poses = rend._ds_angles, rend._ds_poses
        device = torch.device('cuda', rend.engine.device)
        sums = np.zeros((n, AGREE_WORDS), np.uint64)
        for a in range(0, n, self.batch):
            b = min(n, a + self.batch)
            recorded = np.ascontiguousarray(self.ds.depthmaps[a:b], np.float32)
            if recorded.shape != (b - a, H, W):
                raise ValueError(f"depth maps of frames {a}..{b - 1} are {recorded.shape[1:]}, the intrinsics say {(H, W)}")
            depth_t, ids_t = rend.render_ids_batch_device(angles[a:b], poses[a:b])
            sums[a:b] = rend.engine.frame_agreement(depth_t, ids_t, torch.from_numpy(recorded).to(device), rend.n_render, self.tol)
        self.sums, self.table = sums, agreement_table(sums, rend.n_render)
        return self.table

    def _table(self) -> dict:
        return self.table if self.table is not None else self.run()

    def flagged(self) -> np.ndarray:
        """The frames whose recorded pose is to be questioned (flag_frames), ascending."""
        return flag_frames(self._table())[0]

    def unrendered(self) -> np.ndarray:
        """The frames whose render is empty (the robot out of view at the recorded pose): not flagged, nothing to compare."""
        return flag_frames(self._table())[1]

    def summary(self) -> str:
        t = self._table()
        flagged, unrendered = flag_frames(t)
        m = t['mean_abs_diff'][t['both'] > 0]
        lines = [f"{self.ds.length} frames, {len(m)} scored, {len(unrendered)} with nothing rendered, tolerance {self.tol:g} m"]
        if len(m):
            lines.append(f"\tmean |render - recorded| per frame: median {np.median(m):.6f} m, max {m.max():.6f} m, "
                         f"upper fence {upper_fence(m):.6f} m")
            for name in ('coverage', 'close', 'front', 'behind'):
                lines.append(f"\t{name:>8}: mean {np.nanmean(t[name]):.4f}  min {np.nanmin(t[name]):.4f}")
        if t['bad_ids'].any():
            lines.append(f"\t{int(t['bad_ids'].sum())} rendered pixels carry the id of no link")
        lines.append(f"flagged ({len(flagged)}): {flagged.tolist()}")
        if len(unrendered):
            lines.append(f"nothing rendered ({len(unrendered)}): {unrendered.tolist()}")
        return '\n'.join(lines)

    def overlays(self, idxs) -> np.ndarray:
        """The reference's picture of the frames idxs (verification.py:62-67, :222): thumbnail and 'seg_full' render, both resized
        to thumbnail_size, blended VERIFIER_ALPHA : 1 - VERIFIER_ALPHA.  -> (K, h, w, 3) uint8.  Host work, for the few flagged frames."""
        from ..imgproc import resize_linear
        idxs = np.asarray(idxs, np.int64).reshape(-1)
        h, w = self.thumbnail_size
        out = np.zeros((len(idxs), h, w, 3), np.uint8)
        if not len(idxs):
            return out
        colours, _ = self._renderer('seg_full').render_indices(idxs)
        pv = getattr(self.ds, 'preview_img', None)
        for k, i in enumerate(idxs):
            photo = np.asarray(pv[int(i)] if pv is not None else self.ds.og_img[int(i)], np.uint8)
            out[k] = blend(resize_linear(photo, w, h), VERIFIER_ALPHA, resize_linear(colours[k], w, h), 1 - VERIFIER_ALPHA, 0)
        return out

    def sheets(self, folder: str, idxs) -> list:
        """overlays(idxs) as VERIFIER_ROWS x VERIFIER_COLUMNS contact sheets, folder/sheet_000.png ... in the order of idxs, and
        folder/frames.txt naming the frame in every cell.  -> the PNG paths."""
        from .annotation import encode_png
        idxs = np.asarray(idxs, np.int64).reshape(-1)
        os.makedirs(folder, exist_ok=True)
        paths = []
        for k, sheet in enumerate(contact_sheets(self.overlays(idxs))):
            paths.append(os.path.join(folder, f'sheet_{k:03d}.png'))
            with open(paths[-1], 'wb') as f:
                f.write(encode_png(sheet))
        per = VERIFIER_ROWS * VERIFIER_COLUMNS
        with open(os.path.join(folder, 'frames.txt'), 'w') as f:
            for k in range(len(paths)):
                f.write(f"sheet_{k:03d}.png: {idxs[k * per:(k + 1) * per].tolist()}\n")
        return paths

    def remove(self, idxs, inplace: bool = False, name: str = None) -> str:
        """The set without the frames idxs, in the storage form it has (.h5 or .npy arrays), order and attributes kept, 'length'
        and 'name' set anew (Builder.remove_idxs, building.py:77-91).  Written beside the original as <name>_verified, or to
        `name` (a dataset name or a directory); inplace=True replaces the original, and this Verifier then holds the new set.
        In place is refused (ValueError) while the folder holds anything but the set's own files: annotations, splits and other
        derived data are numbered by the old frames and would no longer fit.  The new files are written completely before the
        first old one is replaced, but the replacement itself goes file by file: a crash inside it leaves a .npy set mixed.
        An .h5 file's `paths/*` bookkeeping is not carried over (write_h5_dataset).  -> the directory of the new set."""
        from .dataset import _ARRAYS, Dataset, write_dataset, write_h5_dataset
        ds = self.ds
        drop = np.unique(np.asarray(idxs, np.int64).reshape(-1))
        if len(drop) and (drop[0] < 0 or drop[-1] >= ds.length):
            raise IndexError(f"frames {drop[0]}..{drop[-1]} of a set of {ds.length}")
        keep = np.setdiff1d(np.arange(ds.length), drop)
        stored = os.path.isdir(str(ds.dataset_dir))
        if inplace and (name is not None or not stored):
            raise ValueError("inplace rewrites a stored set under its own name")
        if name is None and not stored:
            raise ValueError(f"{ds.dataset_dir} is not stored anywhere: give the new set a name")
        src = os.path.abspath(str(ds.dataset_dir))
        as_h5 = getattr(ds, 'file', None) is not None
        if inplace:
            own = {os.path.basename(src) + '.h5'} if as_h5 else set(_ARRAYS.values()) | {'attrs.json'}
            derived = sorted(set(os.listdir(src)) - own)
            if derived:
                raise ValueError(f"{src} also holds {derived}, made for the frames as they are numbered now: remove to a new name, "
                                 "or move them away first")
            dst = src + '.verifier_tmp'
            shutil.rmtree(dst, ignore_errors=True)
        else:
            dst = src + '_verified' if name is None else name

        def take(arr):
            if arr is None:
                return None
            if not len(keep):
                return np.zeros((0,) + tuple(arr.shape[1:]), arr.dtype)
            return np.stack([np.asarray(arr[int(i)]) for i in keep])
        arrays = {k: take(getattr(ds, k, None)) for k in ('og_img', 'depthmaps', 'angles', 'camera_pose', 'positions', 'preview_img')}
        attrs = {k: (v.tolist() if isinstance(v, np.ndarray) else v.item() if isinstance(v, np.generic) else v) for k, v in ds.attrs.items()}
        attrs['length'] = int(len(keep))
        writer = write_h5_dataset if as_h5 else write_dataset
        out = writer(dst, arrays['og_img'], arrays['depthmaps'], arrays['angles'], arrays['camera_pose'], str(attrs['color_intrinsics']),
                     positions=arrays['positions'], extra_attrs=dict(attrs, name=os.path.basename(src if inplace else os.path.normpath(dst))),
                     preview=arrays['preview_img'])
        new_dir = os.path.dirname(out) if as_h5 else out
        if inplace:
            base = os.path.basename(src)
            for attr in ('og_img', 'depthmaps', 'angles', 'camera_pose', 'positions', 'preview_img'):       # let go of the maps of the files
                setattr(ds, attr, None)
            ds.close()
            for fn in os.listdir(new_dir):
                target = base + '.h5' if as_h5 and fn == os.path.basename(new_dir) + '.h5' else fn
                os.replace(os.path.join(new_dir, fn), os.path.join(src, target))
            os.rmdir(new_dir)
            if self._rend is not None and getattr(self._rend, 'ds', None) is ds:
                self._rend.close()
            self._rend, self.sums, self.table = None, None, None
            self.ds = Dataset(src, permissions=getattr(ds, 'permissions', 'r'))
            new_dir = src
        return new_dir
