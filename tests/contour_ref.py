"""A second, separately written border follower for the tests: Suzuki & Abe's Algorithm 1 ("Topological structural analysis of
digitized binary images by border following", CVGIP 30, 1985) as the paper states it, with its NBD numbering and (row, column)
indexing, 8-connected foreground.  The chain is followed in full first and compressed afterwards (CHAIN_APPROX_SIMPLE: keep a
point where the direction of the step leaving it differs from the step before).  Slow and plain on purpose; the library's
rope_trace_contours is compared against it."""
import numpy as np

# (d_row, d_col) in counter-clockwise order on the screen (rows grow downwards), starting east
_CCW = [(0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)]


def _code(dr, dc):
    return _CCW.index((dr, dc))


def find_contours(mask: np.ndarray):
    """-> list of (contour (k, 2) int32 (x, y) points, is_hole) in the order the raster scan meets their starting pixels."""
    h, w = mask.shape
    f = np.zeros((h + 2, w + 2), np.int64)
    f[1:-1, 1:-1] = np.asarray(mask) != 0
    f = f.tolist()
    nbd = 1
    out = []
    for i in range(1, h + 1):
        for j in range(1, w + 1):
            if f[i][j] == 1 and f[i][j - 1] == 0:                    # (1a) outer border
                i2, j2, hole = i, j - 1, False
            elif f[i][j] >= 1 and f[i][j + 1] == 0:                  # (1b) hole border
                i2, j2, hole = i, j + 1, True
            else:
                continue
            nbd += 1
            out.append((_follow(f, i, j, i2, j2, nbd), hole))
    return out


def _follow(f, i, j, i2, j2, nbd):
    """Steps (3.1)-(3.5) from (i, j), entered from the 0-pixel (i2, j2).  -> compressed (x, y) points."""
    k0 = _code(i2 - i, j2 - j)
    found = None
    for t in range(1, 8):                                           # (3.1) clockwise from (i2, j2)
        dr, dc = _CCW[(k0 - t) % 8]
        if f[i + dr][j + dc] != 0:
            found = (i + dr, j + dc)
            break
    if found is None:
        f[i][j] = -nbd
        return np.array([[j - 1, i - 1]], np.int32)               # the frame is one pixel wide
    i1, j1 = found
    i2, j2, i3, j3 = i1, j1, i, j                                   # (3.2)
    pixels, moves = [], []
    first_dir = _code(i1 - i, j1 - j)
    while True:
        k = _code(i2 - i3, j2 - j3)                                 # (3.3) counter-clockwise from the element after (i2, j2)
        right_examined = False
        for t in range(1, 9):
            dr, dc = _CCW[(k + t) % 8]
            if f[i3 + dr][j3 + dc] != 0:
                i4, j4 = i3 + dr, j3 + dc
                break
            if (dr, dc) == (0, 1):
                right_examined = True
        if right_examined:                                          # (3.4)
            f[i3][j3] = -nbd
        elif f[i3][j3] == 1:
            f[i3][j3] = nbd
        pixels.append((j3 - 1, i3 - 1))
        moves.append(_code(i4 - i3, j4 - j3))
        if (i4, j4) == (i, j) and (i3, j3) == (i1, j1):             # (3.5)
            break
        i2, j2, i3, j3 = i3, j3, i4, j4
    keep = []
    before = first_dir ^ 4                                          # as if it had arrived from the side of (i1, j1)
    for p, m in zip(pixels, moves):
        if m != before:
            keep.append(p)
        before = m
    return np.array(keep, np.int32).reshape(-1, 2)
