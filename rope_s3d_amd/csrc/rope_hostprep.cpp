// rope_hostprep.cpp — the entry points of librope_hip.so that are plain CPU code: no context, no runtime call, nothing but the
// arrays they are handed.  Standard headers and include/rope_s3d.h only, so any C++17 compiler builds this file, and
// tests/hostprep_main.cpp runs it under AddressSanitizer and UBSan.  Like the rest of the library it is meant to be compiled
// with -ffp-contract=off: every step below is one IEEE operation.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rope_s3d.h"

// numpy's rint (round half to even) of a double in [0, 2^51) without a library call: adding and taking away 2^52 leaves the
// nearest integer, ties to even, under the default rounding mode (every step one IEEE operation: -ffp-contract=off, no fast-math).
// Beyond 2^51 the result is only used to be clipped to 2^39 - 1.
static inline double rint_nonneg(double x)
{
    double t = x + 4503599627370496.0;
    asm volatile("" : "+x"(t));                          // the sum is rounded to a double here: the two operations stay two operations
    return t - 4503599627370496.0;
}

// depth in metres -> Q32, as rope_pack_target documents it
static inline uint64_t q32_of_depth(double d)
{
    const double Q32 = 4294967296.0, top = 549755813887.0;          // 2^32, 2^39 - 1
    double q = (d > 0.0 && d <= 1.7976931348623157e308) ? rint_nonneg(d * Q32) : 0.0;     // NaN, inf, zero and negatives: no depth
    q = q < top ? q : top;
    return (uint64_t)q;
}

// Host only: float64 metres + link-mask bits -> the packed plane of rope_set_target.  Rounding is numpy's rint (round half to even).
extern "C" int rope_pack_target(const double *depth, const uint8_t *mask_bits, int64_t n, uint64_t *out)
{
    if (!depth || !out || n < 0) return ROPE_E_ARG;
    for (int64_t i = 0; i < n; i++) out[i] = q32_of_depth(depth[i]) | (mask_bits ? (uint64_t)mask_bits[i] << 40 : 0);
    return ROPE_OK;
}

// Host only: cv2.resize(img, (W/f, H/f)) with INTER_LINEAR for an EVEN integer factor f (Predictor._downsample,
// predict.py:378-381).  The source coordinate of every output sample falls exactly between the two central taps of its
// f x f block (f/2-1 and f/2), both with weight 1/2, so the general interpolation collapses to four taps per sample:
//   kind 0  uint8 : OpenCV's fixed-point path — horizontal pass with 11-bit weights, >> 4, vertical pass >> 16, + 2 >> 2
//   kind 1  float32, kind 2 float64 : (a*w + b*w) per row, then (top*w + bottom*w), w = 0.5 in the image's own type
// `channels` interleaved values per pixel; rows are `row_stride` BYTES apart (a strided view is fine).
extern "C" int rope_downsample_even(const void *src, int H, int W, int channels, int64_t row_stride, int f, int kind, void *dst)
{
    if (!src || !dst || H < 1 || W < 1 || channels < 1 || f < 2 || (f & 1) || H % f || W % f || kind < 0 || kind > 2) return ROPE_E_ARG;
    const int oh = H / f, ow = W / f, a = f / 2 - 1, b = f / 2;
    const char *base = (const char *)src;
    for (int y = 0; y < oh; y++) {
        const char *r0 = base + (int64_t)(y * f + a) * row_stride, *r1 = base + (int64_t)(y * f + b) * row_stride;
        for (int x = 0; x < ow; x++)
            for (int ch = 0; ch < channels; ch++) {
                const size_t ia = (size_t)(x * f + a) * channels + ch, ib = (size_t)(x * f + b) * channels + ch;
                const size_t o = ((size_t)y * ow + x) * channels + ch;
                if (kind == 0) {
                    const uint8_t *p0 = (const uint8_t *)r0, *p1 = (const uint8_t *)r1;
                    const int64_t t = ((int64_t)p0[ia] * 1024 + (int64_t)p0[ib] * 1024) >> 4, u = ((int64_t)p1[ia] * 1024 + (int64_t)p1[ib] * 1024) >> 4;
                    int64_t v = (((1024 * t) >> 16) + ((1024 * u) >> 16) + 2) >> 2;
                    ((uint8_t *)dst)[o] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
                } else if (kind == 1) {
                    const float *p0 = (const float *)r0, *p1 = (const float *)r1;
                    const float top = p0[ia] * 0.5f + p0[ib] * 0.5f, bot = p1[ia] * 0.5f + p1[ib] * 0.5f;
                    ((float *)dst)[o] = top * 0.5f + bot * 0.5f;
                } else {
                    const double *p0 = (const double *)r0, *p1 = (const double *)r1;
                    const double top = p0[ia] * 0.5 + p0[ib] * 0.5, bot = p1[ia] * 0.5 + p1[ib] * 0.5;
                    ((double *)dst)[o] = top * 0.5 + bot * 0.5;
                }
            }
    }
    return ROPE_OK;
}

// Host only: one frame of the synthetic path from the camera's arrays to what rope_set_target(s) takes, in one pass — the
// down-sampling of Predictor._downsample (predict.py:378-381: cv2.resize INTER_LINEAR; the taps and roundings of
// rope_downsample_even), the link masks read off channel 0 of the colour render and the lookup depth of _loadSynthetic
// (predict.py:445-469), the per-link flags and the packing of _load_target (predict.py:397-413, rope_pack_target).
extern "C" int rope_prepare_synthetic(const uint8_t *color, int64_t color_stride, const void *depth, int depth_kind, int64_t depth_stride,
                                      int H0, int W0, int f, const int32_t *link_blue, int n_links, int n_lookup_links,
                                      uint64_t *tq, float *lookup_f32, double *tgt_depth, uint8_t *flags)
{
    if (!color || !depth || !link_blue || !tq || !lookup_f32 || !flags) return ROPE_E_ARG;
    if (H0 < 1 || W0 < 1 || f < 1 || (f > 1 && (f & 1)) || H0 % f || W0 % f || (depth_kind != 1 && depth_kind != 2)) return ROPE_E_ARG;
    if (n_links < 1 || n_links > ROPE_MAX_LINKS || n_lookup_links < 0 || n_lookup_links > n_links) return ROPE_E_ARG;
    const int H = H0 / f, W = W0 / f, a = f / 2 - 1, b = f / 2;
    // what a channel-0 value says about a pixel, looked up instead of compared link by link: the links whose colour it is (two
    // links may share one), and whether one of them is a lookup link; the counts are kept per value and folded per link at the end
    uint8_t bits_of[256] = {}, hit_of[256] = {};
    int64_t n_val[256] = {}, n_val_depth[256] = {};
    for (int l = 0; l < n_links; l++)
        if (link_blue[l] >= 0 && link_blue[l] <= 255) {
            bits_of[link_blue[l]] |= (uint8_t)(1u << l);
            if (l < n_lookup_links) hit_of[link_blue[l]] = 1;
        }
    int cur = -1;                                                  // counts are kept for the run of equal values and flushed when it ends:
    int64_t run = 0, run_depth = 0;                                // a colour-coded frame is long runs, and a counter in memory per pixel is a chain of store-to-load stalls
    for (int y = 0; y < H; y++) {
        const int ya = f > 1 ? y * f + a : y, yb = f > 1 ? y * f + b : y;
        const uint8_t *c0 = color + (int64_t)ya * color_stride, *c1 = color + (int64_t)yb * color_stride;
        const char *d0 = (const char *)depth + (int64_t)ya * depth_stride, *d1 = (const char *)depth + (int64_t)yb * depth_stride;
        for (int x = 0; x < W; x++) {
            const size_t xa = f > 1 ? (size_t)(x * f + a) : (size_t)x, xb = f > 1 ? (size_t)(x * f + b) : (size_t)x;
            int blue;
            double d;
            if (f > 1) {
                // OpenCV's fixed-point path for uint8 (rope_downsample_even, kind 0); channel 0 of three interleaved
                const int64_t t = ((int64_t)c0[3 * xa] * 1024 + (int64_t)c0[3 * xb] * 1024) >> 4, u = ((int64_t)c1[3 * xa] * 1024 + (int64_t)c1[3 * xb] * 1024) >> 4;
                const int64_t v = (((1024 * t) >> 16) + ((1024 * u) >> 16) + 2) >> 2;
                blue = (int)(v < 0 ? 0 : (v > 255 ? 255 : v));
                if (depth_kind == 1) {
                    const float *p0 = (const float *)d0, *p1 = (const float *)d1;
                    const float tp = p0[xa] * 0.5f + p0[xb] * 0.5f, bt = p1[xa] * 0.5f + p1[xb] * 0.5f;
                    d = (double)(tp * 0.5f + bt * 0.5f);
                } else {
                    const double *p0 = (const double *)d0, *p1 = (const double *)d1;
                    const double tp = p0[xa] * 0.5 + p0[xb] * 0.5, bt = p1[xa] * 0.5 + p1[xb] * 0.5;
                    d = tp * 0.5 + bt * 0.5;
                }
            } else {
                blue = c0[3 * xa];
                d = depth_kind == 1 ? (double)((const float *)d0)[xa] : ((const double *)d0)[xa];
            }
            const unsigned bits = bits_of[blue];
            if (blue != cur) {
                if (cur >= 0) { n_val[cur] += run; n_val_depth[cur] += run_depth; }
                cur = blue; run = 0; run_depth = 0;
            }
            run++;
            run_depth += (d != 0.0);                               // NaN counts, as `depth != 0` does
            const size_t o = (size_t)y * W + x;
            if (tgt_depth) tgt_depth[o] = d;
            lookup_f32[o] = (float)(d * (hit_of[blue] ? 1.0 : 0.0));     // target_depth * hit (predict.py:449-454): NaN stays NaN
            tq[o] = q32_of_depth(d) | ((uint64_t)bits << 40);
        }
    }
    if (cur >= 0) { n_val[cur] += run; n_val_depth[cur] += run_depth; }
    std::memset(flags, 0, 8);
    for (int l = 0; l < n_links; l++) {
        if (link_blue[l] < 0 || link_blue[l] > 255) continue;
        const int64_t n_mask = n_val[link_blue[l]], n_depth = n_val_depth[link_blue[l]];
        if (n_mask > 0) {                                          // np.sum(mask) > 0 (predict.py:465)
            flags[l] |= 1;
            if ((double)n_depth > 0.05 * (double)n_mask) flags[l] |= 2;      // predict.py:495, a fact of the target alone
        }
    }
    return ROPE_OK;
}

// The camera-to-world rotation of a pose [x, y, z, a3, a4, a5]: rope_camera_matrix's R below, and what rope_refine_poses
// (rope_polish.hip) turns into the kernels' camera axes.  One IEEE double operation per written step, sin / cos from libm.
void rope_pose_rotation(const double *pose, double R[3][3])
{
    const double yaw = pose[5], pitch = pose[3], roll = pose[4] + 3.141592653589793 / 2;
    const double c0 = std::cos(yaw), c1 = std::cos(pitch), c2 = std::cos(roll), s0 = std::sin(yaw), s1 = std::sin(pitch), s2 = std::sin(roll);
    R[0][0] = c0 * c1;
    R[1][0] = c1 * s0;
    R[2][0] = -1 * s1;
    R[0][1] = c0 * s1 * s2 - c2 * s0;
    R[1][1] = c0 * c2 + (s0 * s1) * s2;
    R[2][1] = c1 * s2;
    R[0][2] = s0 * s2 + c0 * c2 * s1;
    R[1][2] = c2 * s0 * s1 - c0 * s2;
    R[2][2] = c1 * c2;
}

// Host only: camera pose + pinhole intrinsics -> P·V, the matrix rope_set_camera takes.  Every step is one IEEE double operation in
// the written order (the library is built with -ffp-contract=off), sin / cos from libm.
//   pose   [x, y, z, a3, a4, a5] as Renderer.setCameraPose takes it (render.py:107-111): roll = a4 + pi/2, pitch = a3, yaw = a5,
//          camera-to-world R = Rz(yaw)·Ry(pitch)·Rx(roll) by the element formulas of angToPoseArr (render_utils.py:56-85),
//          t = (x, y, z); the camera looks along its -Z, +Y up (OpenGL); V = the rigid inverse [R^T | -R^T t]
//   P      pyrender 0.1.45's IntrinsicsCamera.get_projection_matrix (projection.py:161-169): P00 = 2fx/W, P11 = 2fy/H,
//          P02 = 1 - 2cx/W, P12 = 2cy/H - 1, P22 = (f+n)/(n-f), P23 = 2fn/(n-f), P32 = -1
extern "C" int rope_camera_matrix(const double *pose, double fx, double fy, double cx, double cy, int W, int H, double znear, double zfar,
                                  double *PV)
{
    if (!pose || !PV || W < 1 || H < 1 || !(znear > 0.0) || !(zfar > znear)) return ROPE_E_ARG;
    double R[3][3];
    rope_pose_rotation(pose, R);
    double V[4][4] = {};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) V[i][j] = R[j][i];
        V[i][3] = -((R[0][i] * pose[0] + R[1][i] * pose[1]) + R[2][i] * pose[2]);
    }
    V[3][3] = 1.0;
    const double w = (double)W, h = (double)H;
    const double P00 = 2.0 * fx / w, P11 = 2.0 * fy / h, P02 = 1.0 - 2.0 * cx / w, P12 = 2.0 * cy / h - 1.0;
    const double P22 = (zfar + znear) / (znear - zfar), P23 = (2.0 * zfar * znear) / (znear - zfar);
    for (int j = 0; j < 4; j++) {
        PV[j] = P00 * V[0][j] + P02 * V[2][j];
        PV[4 + j] = P11 * V[1][j] + P12 * V[2][j];
        PV[8 + j] = P22 * V[2][j] + P23 * V[3][j];
        PV[12 + j] = -V[2][j];
    }
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(PV[k])) return ROPE_E_ARG;
    return ROPE_OK;
}

// Host only: the Lookup stage's pose grid in the reference's order (lookup.py:39-66).  divisions[j] >= 1: joint j takes that many
// samples between its limits (np.linspace: lo + i * step, the last one hi itself; a single sample is lo), clipped to
// LOOKUP_MAX_DIV_PER_LINK = 200 (constants.py:30); divisions[j] <= 0: joint j is not part of the grid and stays 0.  Joint 0 varies
// fastest.  Returns the number of rows (the product of the sample counts); writes them when `out` is given and `capacity` rows fit
// (ROPE_E_ARG otherwise).
extern "C" int64_t rope_lookup_grid(const double *limits, const int32_t *divisions, double *out, int64_t capacity)
{
    if (!limits || !divisions) return ROPE_E_ARG;
    int64_t div[6], n = 1;
    for (int j = 0; j < 6; j++) {
        div[j] = divisions[j] < 1 ? 1 : (divisions[j] > 200 ? 200 : divisions[j]);
        n *= div[j];
    }
    if (!out) return n;
    if (capacity < n) return ROPE_E_ARG;
    int64_t repeat = 1;
    for (int j = 0; j < 6; j++) {
        const double lo = limits[2 * j], hi = limits[2 * j + 1], dv = (double)(div[j] - 1), delta = hi - lo;
        const double step = div[j] > 1 ? delta / dv : 0.0;
        for (int64_t r = 0; r < n; r++) {
            const int64_t i = (r / repeat) % div[j];
            double v = 0.0;                                         // not part of the grid: np.zeros
            if (divisions[j] >= 1) {
                if (div[j] == 1) v = lo;
                else if (i == div[j] - 1) v = hi;
                else v = step == 0.0 ? ((double)i / dv) * delta + lo : (double)i * step + lo;
            }
            out[6 * r + j] = v;
        }
        repeat *= div[j];
    }
    return n;
}

// Host only: the divisions of the pose grid Crop renders to find the image bounds of the first `num_links` links
// (robotpose/crop.py:114-146), in rope_lookup_grid's convention — feed them to rope_lookup_grid for the poses.  Weights 6:3:3:0:1
// over the joints S L U R B (constants.py:19: CROP_RENDER_WEIGHTING), a budget of 20 s at the reference's cost model of
// pixels x 1.2e-8 + 0.002 s per render (crop.py:121-123), at most 50 samples per joint; joints beyond the rendered links sit at
// their lower limit (np.linspace(lo, hi, 1)), R and T are not part of the grid (CROP_VARYING = 'SLUB') and stay 0.
extern "C" int rope_crop_divisions(int64_t n_pixels, int num_links, int32_t *divisions)
{
    if (!divisions || n_pixels < 1 || num_links < 2 || num_links > 6) return ROPE_E_ARG;
    const double weighting[6] = {6, 3, 3, 0, 1, 0};
    const int n = num_links - 1;
    double w[6], sum = 0.0, prod = 1.0;
    int nz = 0;
    for (int j = 0; j < n; j++) sum += weighting[j];
    for (int j = 0; j < n; j++) {
        w[j] = weighting[j] / sum;
        if (w[j] != 0.0) { prod *= w[j]; nz++; }
    }
    const double num_poses = 20.0 / ((double)n_pixels * 1.2 * 1.0e-8 + .002);
    const double scale = std::pow(num_poses / prod, 1.0 / (double)nz);
    const bool varying[6] = {true, true, true, false, true, false};          // S L U B
    for (int j = 0; j < 6; j++) {
        int d = 1;
        if (j < n) {
            double b = w[j] * scale;
            if (b < 1.0) b = 1.0;
            if (b > 50.0) b = 50.0;
            d = (int)b;
        }
        divisions[j] = varying[j] ? d : 0;
    }
    return ROPE_OK;
}

// cv2.dilate / cv2.erode of a binary image with a ones(k, k) kernel, default anchor (k / 2, k / 2), a border that never wins
// (predict.py:428,437): separable, rows then columns; `grow` true: a pixel is set when any pixel of its window is (outside counts
// as clear), false: when all are (outside counts as set)
static void box_morph(const uint8_t *src, uint8_t *dst, uint8_t *tmp, int H, int W, int k, bool grow)
{
    const int a = k / 2, b = k - 1 - a;                  // the window of x reaches from x - a to x + b
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const int lo = x - a < 0 ? 0 : x - a, hi = x + b > W - 1 ? W - 1 : x + b;
            uint8_t v = grow ? 0 : 1;
            for (int i = lo; i <= hi; i++) v = grow ? (uint8_t)(v | src[(size_t)y * W + i]) : (uint8_t)(v & src[(size_t)y * W + i]);
            tmp[(size_t)y * W + x] = v;
        }
    for (int y = 0; y < H; y++) {
        const int lo = y - a < 0 ? 0 : y - a, hi = y + b > H - 1 ? H - 1 : y + b;
        for (int x = 0; x < W; x++) {
            uint8_t v = grow ? 0 : 1;
            for (int i = lo; i <= hi; i++) v = grow ? (uint8_t)(v | tmp[(size_t)i * W + x]) : (uint8_t)(v & tmp[(size_t)i * W + x]);
            dst[(size_t)y * W + x] = v;
        }
    }
}

// Host only: one frame of the SEGMENTATION path from the segmenter's instance masks to what rope_set_target(s) takes — the merge of
// a class's instances (_reorganize_by_link, predict.py:383-395), the body mask erode7(dilate8(sum of the masks)) that zeroes the
// depth outside the robot, once over all classes and once over the lookup links (predict.py:419-438), the depth's own
// down-sampling (predict.py:378-381), the per-link flags and the packing of _load_target (predict.py:397-413).
//   masks     H x W x K bytes (non-zero = inside instance k), as the segmenter returns them;  link_of: K link indices (0..n_links-1),
//             or -1 for an instance of a class that is not one of the rendered links (it still counts for the body mask)
extern "C" int rope_prepare_segmented(const void *depth, int depth_kind, int64_t depth_stride, int H0, int W0, int f, const uint8_t *masks,
                                      int K, const int32_t *link_of, int n_links, int n_lookup_links, uint64_t *tq, float *lookup_f32,
                                      double *tgt_depth, uint8_t *flags)
{
    if (!depth || (K > 0 && (!masks || !link_of)) || !tq || !lookup_f32 || !flags || K < 0) return ROPE_E_ARG;
    if (H0 < 1 || W0 < 1 || f < 1 || (f > 1 && (f & 1)) || H0 % f || W0 % f || (depth_kind != 1 && depth_kind != 2)) return ROPE_E_ARG;
    if (n_links < 1 || n_links > ROPE_MAX_LINKS || n_lookup_links < 0 || n_lookup_links > n_links) return ROPE_E_ARG;
    for (int k = 0; k < K; k++)
        if (link_of[k] < -1 || link_of[k] >= n_links) return ROPE_E_ARG;
    const int H = H0 / f, W = W0 / f, a = f / 2 - 1, b = f / 2;
    const size_t n = (size_t)H * W;
    std::vector<uint8_t> bits(n, 0), any(n, 0), look(n, 0), body(n), body_look(n), t1(n), t2(n);
    for (size_t i = 0; i < n; i++) {
        const uint8_t *m = masks + i * (size_t)K;
        for (int k = 0; k < K; k++)
            if (m[k]) {
                any[i] = 1;
                if (link_of[k] >= 0) {
                    bits[i] |= (uint8_t)(1u << link_of[k]);
                    if (link_of[k] < n_lookup_links) look[i] = 1;
                }
            }
    }
    box_morph(any.data(), t1.data(), t2.data(), H, W, 8, true);
    box_morph(t1.data(), body.data(), t2.data(), H, W, 7, false);
    box_morph(look.data(), t1.data(), t2.data(), H, W, 8, true);
    box_morph(t1.data(), body_look.data(), t2.data(), H, W, 7, false);
    int64_t n_mask[ROPE_MAX_LINKS] = {}, n_depth[ROPE_MAX_LINKS] = {};
    bool present[ROPE_MAX_LINKS] = {};
    for (int k = 0; k < K; k++)
        if (link_of[k] >= 0) present[link_of[k]] = true;             // a class that was detected has a mask, however empty (predict.py:408-413)
    for (int y = 0; y < H; y++) {
        const int ya = f > 1 ? y * f + a : y, yb = f > 1 ? y * f + b : y;
        const char *d0 = (const char *)depth + (int64_t)ya * depth_stride, *d1 = (const char *)depth + (int64_t)yb * depth_stride;
        for (int x = 0; x < W; x++) {
            const size_t xa = f > 1 ? (size_t)(x * f + a) : (size_t)x, xb = f > 1 ? (size_t)(x * f + b) : (size_t)x, o = (size_t)y * W + x;
            double d;
            if (f > 1) {
                if (depth_kind == 1) {
                    const float *p0 = (const float *)d0, *p1 = (const float *)d1;
                    const float tp = p0[xa] * 0.5f + p0[xb] * 0.5f, bt = p1[xa] * 0.5f + p1[xb] * 0.5f;
                    d = (double)(tp * 0.5f + bt * 0.5f);
                } else {
                    const double *p0 = (const double *)d0, *p1 = (const double *)d1;
                    const double tp = p0[xa] * 0.5 + p0[xb] * 0.5, bt = p1[xa] * 0.5 + p1[xb] * 0.5;
                    d = tp * 0.5 + bt * 0.5;
                }
            } else {
                d = depth_kind == 1 ? (double)((const float *)d0)[xa] : ((const double *)d0)[xa];
            }
            d = d * (body[o] ? 1.0 : 0.0);                           // target_depth *= body (predict.py:429)
            const double dl = d * (body_look[o] ? 1.0 : 0.0);        // lookup_depth = the copy, *= the lookup links' body (predict.py:432-438)
            for (int l = 0; l < n_links; l++)
                if ((bits[o] >> l) & 1) {
                    n_mask[l]++;
                    if (d != 0.0) n_depth[l]++;
                }
            if (tgt_depth) tgt_depth[o] = d;
            lookup_f32[o] = (float)dl;
            tq[o] = q32_of_depth(d) | ((uint64_t)bits[o] << 40);
        }
    }
    std::memset(flags, 0, 8);
    for (int l = 0; l < n_links; l++)
        if (present[l]) {
            flags[l] |= 1;
            if ((double)n_depth[l] > 0.05 * (double)n_mask[l]) flags[l] |= 2;
        }
    return ROPE_OK;
}

// Host only: the thresholds of the depth holes' seed bits.  Dilation j has size d = 3 (j + 1) < max_size (np.arange(3, max_size, 3),
// noise.py:16); a pixel is a seed of it when |N(0, std)| >= 1 - thresh_factor / d, with probability p = erfc(thresh / (std sqrt 2));
// T = floor(p 2^32), the whole range when p reaches 1.  Every step one IEEE double operation, erfc and sqrt from libm.
extern "C" int rope_hole_thresholds(double sigma, double thresh_factor, int max_size, uint32_t *T_out, int *n_out)
{
    if (!n_out || !(sigma > 0.0) || !std::isfinite(sigma) || !std::isfinite(thresh_factor)) return ROPE_E_ARG;
    // what rope_depth_holes takes: ROPE_HOLE_MAX_DILATIONS and ROPE_HOLE_MAX_WINDOW of rope_kernels.h, a HIP header this file does
    // without (tests/test_hostprep_host.py holds the two pairs equal)
    constexpr int HOLE_MAX_DILATIONS = 16, HOLE_MAX_WINDOW = 32;
    const int n = max_size > 3 ? (max_size - 1) / 3 : 0;
    if (n > HOLE_MAX_DILATIONS || 3 * n > HOLE_MAX_WINDOW) return ROPE_E_ARG;
    *n_out = n;
    if (!T_out) return ROPE_OK;
    for (int j = 0; j < n; j++) {
        const double d = 3.0 * (j + 1);
        const double thresh = 1.0 - thresh_factor / d;
        const double p = std::erfc(thresh / (sigma * std::sqrt(2.0)));
        const double t = std::floor(p * 4294967296.0);
        T_out[j] = t >= 4294967295.0 ? 0xFFFFFFFFu : (t > 0.0 ? (uint32_t)t : 0u);
    }
    return ROPE_OK;
}
