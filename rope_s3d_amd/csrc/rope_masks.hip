// rope_masks.hip — label masks of rendered poses for the annotator, for gfx950: the link-id planes a MODE_DUMP launch wrote
// -> per-pixel label bits (a lookup table over the 256 id values, 255 = background -> 0), dilated by a pad x pad window,
// and per (pose, bit) the bounding box of the dilated mask.
//
// Reference: robotpose/data/annotation.py:117-127 (Annotator._mask_color: np.all(render == colour) then expandRegion, which is
// cv2.dilate(mask, ones((pad, pad))) with the default anchor (pad/2, pad/2) and a border that never adds a pixel).
// dst(x, y) = OR of src over columns x - pad/2 .. x - pad/2 + pad - 1 and the same rows; the bits of one byte are the labels,
// so one byte-wise OR dilates all eight label masks at once.
//
// One workgroup per (128 x 16 output tile, pose).  The tile and its halo of pad - 1 columns and rows go to LDS as label bytes,
// then two separable passes: along rows (four output bytes per 32-bit word, the window's bytes brought in by funnel shifts of
// neighbouring words), then along columns (a word-wise OR of pad rows).  Stores are one word per lane where the plane's width
// is a multiple of four, bytes otherwise.  Boxes: the OR of the tile's output per row and per column goes through LDS, one wave
// turns those into ballots per bit, and lane b issues the (at most) four atomics of bit b.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rope_kernels.h"

namespace rope {
namespace {

constexpr int MASK_TW = 128;                                   // output tile: columns (a multiple of 4, at most 128)
constexpr int MASK_TH = 16;                                    // output tile: rows (at most 64)
constexpr int MASK_THREADS = 256;
constexpr int MASK_TW_WORDS = MASK_TW / 4;
constexpr int MASK_ROWS_PER_THREAD = MASK_TH * MASK_TW_WORDS / MASK_THREADS;
constexpr int MASK_IN_ROWS = MASK_TH + ROPE_MASK_MAX_PAD - 1;
constexpr int MASK_IN_WORDS = (MASK_TW + ROPE_MASK_MAX_PAD - 1 + 3) / 4 + 1;  // + 1: the funnel shift reads one word past
static_assert(MASK_ROWS_PER_THREAD * MASK_THREADS == MASK_TH * MASK_TW_WORDS, "column pass: whole rows per thread");
static_assert(MASK_TW <= 128 && MASK_TH <= 64, "box ballots: two column bytes and one row per lane of one wave");

__global__ void __launch_bounds__(MASK_THREADS)
label_mask_kernel(const uint8_t *__restrict__ ids, int H, int W, const uint8_t *__restrict__ lut, int pad,
                  uint8_t *__restrict__ masks, int32_t *__restrict__ boxes)
{
    __shared__ uint8_t s_lut[256];
    __shared__ uint32_t s_in[MASK_IN_ROWS * MASK_IN_WORDS];    // label bytes of the tile and its halo
    __shared__ uint32_t s_h[MASK_IN_ROWS * MASK_TW_WORDS];     // after the row pass
    __shared__ uint32_t s_col[MASK_TW_WORDS];                  // OR over the tile's rows: one byte per column
    __shared__ uint32_t s_row[MASK_TH];                        // OR over the tile's columns, per row

    const int t = threadIdx.x;
    const int x0 = blockIdx.x * MASK_TW, y0 = blockIdx.y * MASK_TH;
    const size_t plane = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    const int a = pad / 2;                                      // cv2's default anchor
    const int rows = MASK_TH + pad - 1;
    const int in_words = (MASK_TW + pad - 1 + 3) / 4 + 1;
    const int in_bytes = 4 * in_words, used_bytes = MASK_TW + pad - 1;

    s_lut[t] = lut[t];
    if (t < MASK_TW_WORDS) s_col[t] = 0;
    if (t < MASK_TH) s_row[t] = 0;
    __syncthreads();

    // stage: rows y0 - a .., columns x0 - a .. of the id plane as label bytes, 0 outside the image and past the window
    uint8_t *s_in8 = reinterpret_cast<uint8_t *>(s_in);
    const uint8_t *src = ids + plane;
    for (int i = t; i < rows * in_bytes; i += MASK_THREADS) {
        const int r = i / in_bytes, c = i - r * in_bytes;
        const int y = y0 - a + r, x = x0 - a + c;
        uint8_t v = 0;
        if (c < used_bytes && y >= 0 && y < H && x >= 0 && x < W) v = s_lut[src[(size_t)y * W + x]];
        s_in8[i] = v;
    }
    __syncthreads();

    // row pass: output byte 4k + i of a row = OR of input bytes 4k + i .. 4k + i + pad - 1
    for (int i = t; i < rows * MASK_TW_WORDS; i += MASK_THREADS) {
        const int r = i / MASK_TW_WORDS, k = i - r * MASK_TW_WORDS;
        const uint32_t *w = s_in + r * in_words + k;
        uint32_t lo = w[0], acc = 0;
        for (int m = 0; 4 * m < pad; m++) {
            const uint32_t hi = w[m + 1];
            const uint64_t pair = ((uint64_t)hi << 32) | lo;
            const int left = pad - 4 * m;                       // window bytes that start in this word
            acc |= lo;
            if (left > 1) acc |= (uint32_t)(pair >> 8);
            if (left > 2) acc |= (uint32_t)(pair >> 16);
            if (left > 3) acc |= (uint32_t)(pair >> 24);
            lo = hi;
        }
        s_h[i] = acc;
    }
    __syncthreads();

    // column pass, stores, and the OR of the output per row and per column
    const int k = t % MASK_TW_WORDS;
    const int x = x0 + 4 * k;
    uint32_t col_or = 0;
    for (int rr = 0; rr < MASK_ROWS_PER_THREAD; rr++) {
        const int r = (t / MASK_TW_WORDS) * MASK_ROWS_PER_THREAD + rr;
        const int y = y0 + r;
        if (y >= H || x >= W) continue;
        uint32_t v = 0;
        for (int j = 0; j < pad; j++) v |= s_h[(r + j) * MASK_TW_WORDS + k];
        const int n = W - x < 4 ? W - x : 4;                    // bytes of this word inside the image
        if (n < 4) v &= 0xFFFFFFFFu >> (8 * (4 - n));
        uint8_t *dst = masks + plane + (size_t)y * W + x;
        if ((W & 3) == 0) {
            *reinterpret_cast<uint32_t *>(dst) = v;             // plane, row and tile starts are all 4-byte aligned
        } else {
            for (int b = 0; b < n; b++) dst[b] = (uint8_t)(v >> (8 * b));
        }
        col_or |= v;
        const uint32_t row_bits = (v | (v >> 8) | (v >> 16) | (v >> 24)) & 0xFFu;
        if (row_bits) atomicOr(&s_row[r], row_bits);
    }
    if (col_or) atomicOr(&s_col[k], col_or);
    __syncthreads();

    if (t < 64) {                                               // one wave: boxes by ballot, four atomics per bit present
        const uint8_t *col8 = reinterpret_cast<const uint8_t *>(s_col);
        const uint32_t c_lo = col8[t], c_hi = col8[64 + t];
        const uint32_t rw = t < MASK_TH ? s_row[t] : 0u;
        for (int b = 0; b < 8; b++) {
            const uint64_t mr = __ballot((rw >> b) & 1u);
            if (!mr) continue;                                  // uniform across the wave
            const uint64_t m0 = __ballot((c_lo >> b) & 1u), m1 = __ballot((c_hi >> b) & 1u);
            if (t == b) {
                const int r0 = y0 + __builtin_ctzll(mr), r1 = y0 + 63 - __builtin_clzll(mr);
                const int c0 = x0 + (m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1));
                const int c1 = x0 + (m1 ? 127 - __builtin_clzll(m1) : 63 - __builtin_clzll(m0));
                int32_t *box = boxes + ((size_t)blockIdx.z * 8 + b) * 4;
                // every field starts at -1: as unsigned that is above any row or column, as signed below
                atomicMin(reinterpret_cast<unsigned int *>(box + 0), (unsigned int)r0);
                atomicMax(box + 1, r1);
                atomicMin(reinterpret_cast<unsigned int *>(box + 2), (unsigned int)c0);
                atomicMax(box + 3, c1);
            }
        }
    }
}

}  // namespace

hipError_t launch_masks(hipStream_t st, const uint8_t *ids, int n, int H, int W, const uint8_t *lut, int pad, uint8_t *masks,
                        int32_t *boxes)
{
    if (n < 1 || H < 1 || W < 1 || pad < 1 || pad > ROPE_MASK_MAX_PAD) return hipErrorInvalidValue;
    const dim3 grid((W + MASK_TW - 1) / MASK_TW, (H + MASK_TH - 1) / MASK_TH, n);
    hipLaunchKernelGGL(label_mask_kernel, grid, dim3(MASK_THREADS), 0, st, ids, H, W, lut, pad, masks, boxes);
    return hipGetLastError();
}

}  // namespace rope
