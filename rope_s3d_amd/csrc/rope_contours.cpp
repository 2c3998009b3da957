// Border following for the annotator: the contours of one label of a mask plane, as the reference gets them from
// cv2.findContours(mask, cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE) in Annotator._get_contour (robotpose/data/annotation.py:125-127,
// OpenCV 4.5.1 pinned).
//
// Suzuki & Abe, "Topological structural analysis of digitized binary images by border following" (CVGIP 30, 1985), in the
// form OpenCV runs it on 8-bit images: the image gets a frame of zero pixels, a raster scan starts an outer border at a
// 0 -> 1 step and a hole border at a (>= 1) -> 0 step, and each border is followed with 8-connected foreground, marking its
// pixels 2, or -126 where the pixel to the right was examined and found 0 (that mark keeps a later hole start off the
// pixels of a border already followed).  CHAIN_APPROX_SIMPLE keeps the start point and every point where the chain
// direction changes.  The hierarchy is not needed: outer and hole borders are both returned, in the order the scan finds them.
//
// Sequential work per border pixel: this stays on host threads (the device hands over one byte per pixel, already dilated).
#include <cstdint>
#include <vector>

#include "../../include/rope_s3d.h"

namespace {

// chain code k: step (DX[k], DY[k]); 0 = +x, then counter-clockwise on screen (y grows downwards)
const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
const int DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

constexpr int8_t MARK = 2, MARK_RIGHT = -126;

// one border from *i0 at (x, y); hole: the pixel right of the start is the background that was stepped into
void follow(int8_t *i0, int step, int x, int y, bool hole, std::vector<int32_t> &pts)
{
    int delta[16];
    for (int k = 0; k < 16; k++) delta[k] = DX[k & 7] + DY[k & 7] * step;
    int s_end = hole ? 0 : 4, s = s_end;
    int8_t *i1;
    do {                                                        // clockwise from the known background neighbour
        s = (s - 1) & 7;
        i1 = i0 + delta[s];
    } while (*i1 == 0 && s != s_end);
    if (s == s_end) {                                           // an isolated pixel
        *i0 = MARK_RIGHT;
        pts.push_back(x);
        pts.push_back(y);
        return;
    }
    int8_t *i3 = i0, *i4 = nullptr;
    int prev_s = s ^ 4;
    for (;;) {
        s_end = s;
        while (s < 15) {                                        // counter-clockwise from the pixel we came from
            i4 = i3 + delta[++s];
            if (*i4 != 0) break;
        }
        s &= 7;
        if ((unsigned)(s - 1) < (unsigned)s_end) *i3 = MARK_RIGHT;    // the right neighbour was examined: background
        else if (*i3 == 1) *i3 = MARK;
        if (s != prev_s) {
            pts.push_back(x);
            pts.push_back(y);
            prev_s = s;
        }
        x += DX[s];
        y += DY[s];
        if (i4 == i0 && i3 == i1) break;
        i3 = i4;
        s = (s + 4) & 7;
    }
}

}  // namespace

extern "C" int rope_trace_contours(const uint8_t *mask, int H, int W, int bit, const int32_t *box, int min_points, int32_t *points,
                                   int points_cap, int32_t *starts, int starts_cap, int *n_points, int *n_contours)
{
    if (!mask || H < 1 || W < 1 || bit < 0 || bit > 7 || !n_points || !n_contours || points_cap < 0 || starts_cap < 0)
        return ROPE_E_ARG;
    if ((points_cap && !points) || (starts_cap && !starts)) return ROPE_E_ARG;
    *n_points = 0;
    *n_contours = 0;
    int r0 = 0, r1 = H - 1, c0 = 0, c1 = W - 1;
    if (box) {
        if (box[0] == -1 && box[1] == -1 && box[2] == -1 && box[3] == -1) {
            if (starts_cap < 1) return ROPE_E_NOMEM;
            starts[0] = 0;
            return ROPE_OK;
        }
        r0 = box[0]; r1 = box[1]; c0 = box[2]; c1 = box[3];
        if (r0 < 0 || r1 >= H || r0 > r1 || c0 < 0 || c1 >= W || c0 > c1) return ROPE_E_ARG;
    }
    // the box's pixels as 0 / 1 inside a frame of zeros (the copyMakeBorder of cv::findContours)
    const int w = c1 - c0 + 1, h = r1 - r0 + 1, step = w + 2;
    std::vector<int8_t> img((size_t)(h + 2) * step, 0);
    for (int y = 0; y < h; y++) {
        const uint8_t *src = mask + (size_t)(r0 + y) * W + c0;
        int8_t *dst = img.data() + (size_t)(y + 1) * step + 1;
        for (int x = 0; x < w; x++) dst[x] = (int8_t)((src[x] >> bit) & 1);
    }
    std::vector<int32_t> pts, contour;
    std::vector<int32_t> offs{0};
    for (int y = 1; y < h + 1; y++) {
        int8_t *row = img.data() + (size_t)y * step;
        int prev = 0;
        for (int x = 1; x < step; x++) {
            const int p = row[x];
            if (p != prev) {
                const bool outer = prev == 0 && p == 1, hole = !outer && p == 0 && prev >= 1;
                if (outer || hole) {
                    contour.clear();
                    follow(row + x - hole, step, x - hole - 1 + c0, y - 1 + r0, hole, contour);
                    if ((int)contour.size() / 2 >= min_points) {
                        pts.insert(pts.end(), contour.begin(), contour.end());
                        offs.push_back((int32_t)(pts.size() / 2));
                    }
                }
            }
            prev = row[x];                                      // as marked by the border just followed
        }
    }
    *n_points = (int)(pts.size() / 2);
    *n_contours = (int)offs.size() - 1;
    if (*n_points > points_cap || (int)offs.size() > starts_cap) return ROPE_E_NOMEM;
    for (size_t i = 0; i < pts.size(); i++) points[i] = pts[i];
    for (size_t i = 0; i < offs.size(); i++) starts[i] = offs[i];
    return ROPE_OK;
}
