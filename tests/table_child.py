"""Drives tests/table_shim.hip: the stored lookup table's launch helpers on torch tensors between guard bytes.  Imported by
tests/test_gpu_table_kernels.py, and run by it as a program for the table_score_frames_kernel<F, LANES> instantiations that
ROPE_TABLE_FRAMES / ROPE_TABLE_LANES select — the library reads them once per process, so each variant is a fresh process:

    python tests/table_child.py in.npz out.npz

in.npz: shim (path of the built shim), rows (C, ch, cw) float32, planes (N, H, W) float32, geom (W, H, r0, r1, c0, c1) and one
index array batch_<n> per batch of frames; out.npz: scores_<n> (n, C) and best_<n> (n, 2) of each."""
import ctypes as C
import sys

import numpy as np
import torch

GUARD = 0xA5
PAD = 256                                                # guard bytes on either side; keeps float4 alignment


def load_shim(path):
    torch.cuda.init()                                   # one HIP runtime in the process: torch's, loaded first
    lib = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int
    lib.shim_crop_words.restype = C.c_longlong
    lib.shim_crop_words.argtypes = [i32] * 6
    lib.shim_table_count.argtypes = [i32, i32, vp, i32, vp, vp, vp, vp]
    lib.shim_table_fill.argtypes = [i32, i32, vp, i32, vp, vp, vp, vp]
    lib.shim_table_score.argtypes = [i32] * 6 + [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.shim_table_score_frames.argtypes = [i32] * 6 + [vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.shim_argmin_sets.argtypes = [vp, i32, i32, vp, vp]
    lib.shim_finalize_lookup.argtypes = [vp, vp, i32, C.c_double, vp, vp]
    return lib


class Out:
    """An output buffer of n elements of dtype between guard bytes, itself filled with the guard byte (an element the kernel
    skips shows); host() checks the guards and returns the elements."""

    def __init__(self, name, n, dtype, zero=False):
        self.name, self.n, self.dtype = name, int(n), np.dtype(dtype)
        self.nbytes = self.n * self.dtype.itemsize
        self.t = torch.full((self.nbytes + 2 * PAD,), GUARD, dtype=torch.uint8, device='cuda')
        if zero:
            self.t[PAD:PAD + self.nbytes] = 0
        self.ptr = self.t.data_ptr() + PAD

    def host(self):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:PAD] == GUARD).all(), f"{self.name}: bytes before the buffer were written"
        assert (h[PAD + self.nbytes:] == GUARD).all(), f"{self.name}: bytes after the buffer were written"
        return h[PAD:PAD + self.nbytes].copy().view(self.dtype)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build_table(lib, rows):
    """launch_table_count + launch_table_fill on dense rows (C, ch, cw) -> dict of the device buffers and their host copies."""
    n_rows, ch, cw = rows.shape
    d_rows = dev(rows.astype(np.float32))
    counts, offs, used = Out('counts', n_rows, np.uint32), Out('offs', n_rows, np.uint64), Out('used', 1, np.uint64, zero=True)
    rc = lib.shim_table_count(cw, ch, d_rows.data_ptr(), n_rows, counts.ptr, offs.ptr, used.ptr, None)
    assert rc == 0, rc
    n_used = int(used.host()[0])
    h_counts, h_offs = counts.host(), offs.host()
    assert n_used == int(h_counts.sum()) <= n_rows * ch * ((cw + 3) // 4), (n_used, h_counts)      # before anything is sized by it
    assert all(int(o) + int(c) <= n_used for o, c in zip(h_offs, h_counts)), (h_offs, h_counts, n_used)
    goff, gval = Out('goff', max(n_used, 1), np.uint32), Out('gval', 4 * max(n_used, 1), np.float32)
    rc = lib.shim_table_fill(cw, ch, d_rows.data_ptr(), n_rows, offs.ptr, goff.ptr, gval.ptr, None)
    assert rc == 0, rc
    return dict(C=n_rows, cw=cw, ch=ch, counts=counts, offs=offs, goff=goff, gval=gval, used=n_used, h_counts=h_counts, h_offs=h_offs,
                h_goff=goff.host(), h_gval=gval.host().reshape(-1, 4))


def score_one(lib, tbl, geom, plane, sum_words):
    """launch_table_score + launch_finalize(ROPE_LOSS_LOOKUP, zero totals) on one plane -> (sums (C, words) as table_score left
    them, scores (C,), best score, best row)."""
    W, H, r0, r1, c0, c1 = (int(v) for v in geom)
    n_rows = tbl['C']
    assert plane.shape == (H, W) and (r1 - r0 + 1, c1 - c0 + 1) == (tbl['ch'], tbl['cw']) and 0 <= r0 and r1 < H and 0 <= c0 and c1 < W
    words = lib.shim_crop_words(W, H, r0, r1, c0, c1)
    d_plane = dev(plane.astype(np.float32))
    t32c, total, sums = Out('t32c', words, np.float32), Out('total', sum_words, np.uint64), Out('sums', n_rows * sum_words, np.uint64)
    rc = lib.shim_table_score(W, H, r0, r1, c0, c1, tbl['counts'].ptr, tbl['offs'].ptr, tbl['goff'].ptr, tbl['gval'].ptr, n_rows,
                              d_plane.data_ptr(), t32c.ptr, total.ptr, sums.ptr, None)
    assert rc == 0, rc
    h_sums = sums.host().reshape(n_rows, sum_words)
    t32c.host(), total.host()
    zero = torch.zeros(sum_words, dtype=torch.int64, device='cuda')
    err = Out('err', n_rows + 2, np.float64)
    rc = lib.shim_finalize_lookup(sums.ptr, zero.data_ptr(), n_rows, float(tbl['cw'] * tbl['ch']), err.ptr, None)
    assert rc == 0, rc
    h_err = err.host()
    sums.host()
    return h_sums, h_err[:n_rows], h_err[n_rows], int(h_err[n_rows + 1])


def score_frames(lib, tbl, geom, planes, sum_words):
    """launch_table_score_frames on planes (n, H, W) -> (scores (n, C), best (n, 2))."""
    W, H, r0, r1, c0, c1 = (int(v) for v in geom)
    n, n_rows = len(planes), tbl['C']
    assert planes.shape == (n, H, W) and (r1 - r0 + 1, c1 - c0 + 1) == (tbl['ch'], tbl['cw']) and 0 <= r0 and r1 < H and 0 <= c0 and c1 < W
    words = lib.shim_crop_words(W, H, r0, r1, c0, c1)
    d_planes = dev(planes.astype(np.float32))
    t32c, totals = Out('t32c', n * words, np.float32), Out('totals', n * sum_words, np.uint64)
    scores, best = Out('scores', n * n_rows, np.float64), Out('best', 2 * n, np.float64)
    rc = lib.shim_table_score_frames(W, H, r0, r1, c0, c1, tbl['counts'].ptr, tbl['offs'].ptr, tbl['goff'].ptr, tbl['gval'].ptr, n_rows,
                                     d_planes.data_ptr(), n, t32c.ptr, totals.ptr, scores.ptr, best.ptr, None)
    assert rc == 0, rc
    t32c.host(), totals.host()
    for k in ('counts', 'offs', 'goff', 'gval'):
        tbl[k].host()
    return scores.host().reshape(n, n_rows), best.host().reshape(n, 2)


def main(src, dst):
    with np.load(src) as z:
        data = {k: z[k] for k in z.files}
    lib = load_shim(str(data['shim']))
    sum_words = lib.shim_sum_words()
    tbl = build_table(lib, data['rows'])
    out = {}
    for key, idx in data.items():
        if key.startswith('batch_'):
            sc, best = score_frames(lib, tbl, data['geom'], data['planes'][idx], sum_words)
            out['scores_' + key[6:]], out['best_' + key[6:]] = sc, best
    np.savez(dst, **out)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
