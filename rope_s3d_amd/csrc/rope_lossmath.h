// rope_lossmath.h — device code the kernel files share: the loss terms of one pixel and of one tile as exact integer sums, and
// the mean / deviation step of the finalize.  Included by rope_kernels.hip (raster, gtile, layer sums, empty tile, finalize),
// rope_fragments.hip and rope_table.hip; device functions only, no kernel and no launch function.
//
// Arithmetic contract: all floating point steps are single IEEE-754 operations in the written order, pixel
// reductions are exact integer sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rope_kernels.h"

namespace rope {

// --------------------------------------------------------------- pixel maths ----
__device__ static inline float linear_depth(uint32_t d24, float c_num, float c_sum, float c_dif)
{
    float d = (float)d24 / 16777215.0f;
    float t = 2.0f * d - 1.0f;
    float u = t * c_dif;
    float den = c_sum - u;
    return c_num / den;
}

// floor(z * 2^32) for a finite z >= 0 (same value as (uint64_t)((double)z * 2^32)).
// Any size: by shifting the significand.
__device__ static inline uint64_t q32_of_f32_wide(float z)
{
    const uint32_t b = __float_as_uint(z);
    const int ex = (int)(b >> 23) & 0xFF;
    // zero and denormals are below one unit of 2^-32; no branches: both shifts are always executed, one of them by 0
    const uint64_t m = ex ? (uint64_t)((b & 0x7FFFFFu) | 0x800000u) : 0ull;
    const int sh = ex - 127 - 23 + 32;                        // z = m * 2^(ex-150)
    return (m << min(max(sh, 0), 63)) >> min(max(-sh, 0), 63);
}

// Below 2^32 (every depth and depth difference there is: the far plane is at 100 m) in five full-rate operations instead of a
// dozen with 64-bit shifts: z = trunc(z) + fraction, both parts exact in float32; the integer part is the high word, and
// fraction * 2^32 — a power-of-two scaling, exact, below 2^32 — truncated is the low word.
__device__ static inline uint64_t q32_of_f32(float z)
{
    if (__builtin_expect(!(z < 4294967296.0f), 0)) return q32_of_f32_wide(z);
    const float whole = truncf(z);
    const uint32_t hi = (uint32_t)whole, lo = (uint32_t)((z - whole) * 4294967296.0f);
    return ((uint64_t)hi << 32) | lo;
}

// floor(sqrt(x) * 2^32) for x given in Q32: sqrt(dq * 2^-32) * 2^32 = sqrt(dq) * 2^16; one correctly rounded
// float64 square root (dq < 2^39 converts exactly), then truncation
__device__ static inline uint64_t sqrt_q32(uint64_t dq) { return (uint64_t)(sqrt((double)dq) * 65536.0); }

// NEG subtracts instead of adds (modulo 2^64): lets "sums(tile) - sums(base)" live in one set of registers
template <bool NEG>
__device__ static inline void acc(uint64_t &w, uint64_t x) { if (NEG) w -= x; else w += x; }

template <bool NEG>
__device__ static inline void acc_sq(uint64_t *s, uint64_t dq)
{
    uint32_t a = (uint32_t)(dq >> 20), b = (uint32_t)(dq & 0xFFFFFu);
    acc<NEG>(s[SUM_S1], dq);
    acc<NEG>(s[SUM_AA], (uint64_t)a * a);
    acc<NEG>(s[SUM_AB], (uint64_t)a * b);
    acc<NEG>(s[SUM_BB], (uint64_t)b * b);
}

// The same for the differences of the float losses, which reach 2^32 (a lookup target just below it where nothing is drawn):
// a = dq >> 20 has up to 44 bits there, and the products are taken modulo 2^64 as the oracle takes them.
template <bool NEG>
__device__ static inline void acc_sq_wide(uint64_t *s, uint64_t dq)
{
    const uint64_t a = dq >> 20, b = dq & 0xFFFFFu;
    acc<NEG>(s[SUM_S1], dq);
    acc<NEG>(s[SUM_AA], a * a);
    acc<NEG>(s[SUM_AB], a * b);
    acc<NEG>(s[SUM_BB], b * b);
}

// Loss terms of one pixel given its z-buffer key.  `pix` indexes the H x W target planes.
template <int LOSS, bool NEG = false>
__device__ static inline void score_pixel(uint32_t key, size_t pix, int n_render, const uint64_t t /* tq[pix] */,
                                          const float ta /* t32[pix] */, const uint64_t *__restrict__ tl, size_t plane,
                                          float c_num, float c_sum, float c_dif, uint64_t *s, uint64_t *pk = nullptr,
                                          unsigned link_mask = 0xFFu /* ROPE_LOSS_FULL: the links whose terms are wanted (uniform) */)
{
    const bool empty = (key == KEY_EMPTY);
    float z = empty ? 0.0f : linear_depth(key >> 8, c_num, c_sum, c_dif);
    if (LOSS == ROPE_LOSS_LOOKUP || LOSS == ROPE_LOSS_TSWEEP) {
        float a = ta;
        if (LOSS == ROPE_LOSS_TSWEEP) a = sqrtf(a);
        float diff = fabsf(a - sqrtf(z));
        uint64_t dq = q32_of_f32(diff);
        if (dq) acc_sq_wide<NEG>(s, dq);
        return;
    }
    if (LOSS == ROPE_LOSS_CAMFULL) {
        // CameraPredictor._error (camera_pose_prediction.py:933-970): every difference enters as its square root;
        // per link (base_link included) mask mismatches and the mean of sqrt|T_l - D*R_l| over its non-zero entries
        const uint64_t T = t & 0x7FFFFFFFFFull, zq = q32_of_f32(z);
        const uint64_t dq = T > zq ? T - zq : zq - T;
        if (dq) { acc<NEG>(s[SUM_CNT], 1); acc<NEG>(s[SUM_S1], dq); acc<NEG>(s[SUM_AA], sqrt_q32(dq)); }
        const int id = empty ? 255 : (int)(key & 0xFF);
#pragma unroll
        for (int l = 0; l < ROPE_MAX_LINKS; l++) {
            if (l < n_render) {
                const uint64_t tll = tl[(size_t)l * plane + pix];
                // the reference compares blue values (:943-946), and base_link's blue is 0 — the black background's too
                // (constants.py:82-89): its render mask also holds every pixel nothing was drawn on
                const bool M = (tll >> 40) & 1, R = (id == l) || (l == 0 && empty);
                if (!M && !R && !(tll & 0x7FFFFFFFFFull)) continue;
                const uint64_t a = tll & 0x7FFFFFFFFFull, b = R ? zq : 0;
                const uint64_t dl = a > b ? a - b : b - a;
                pk[NEG ? 1 : 0] += (uint64_t)(M != R) << (10 * l);          // six 10-bit fields (see ROPE_LOSS_FULL below)
                pk[NEG ? 3 : 2] += (uint64_t)(dl != 0) << (10 * l);
                if (dl) acc<NEG>(s[SUM_LINK0 + 3 * l + 2], sqrt_q32(dl));
            }
        }
        return;
    }
    if (empty && t == 0) return;                  // nothing rendered, no target: every term is zero
    const uint64_t T = t & 0x7FFFFFFFFFull, zq = q32_of_f32(z);
    const uint64_t dq = T > zq ? T - zq : zq - T;
    acc<NEG>(s[SUM_CNT], (uint64_t)(dq != 0));    // unconditional: a zero difference adds zeros
    acc_sq<NEG>(s, dq);
    if (LOSS == ROPE_LOSS_FULL) {
        const unsigned mask = (unsigned)(t >> 40) & 0xFFu;
        const int id = empty ? 255 : (int)(key & 0xFF);
#pragma unroll
        for (int l = 1; l < ROPE_MAX_LINKS; l++) {
            if (l < n_render && ((link_mask >> l) & 1u)) {
                const bool M = (mask >> l) & 1, R = (id == l);
                const uint64_t a = M ? T : 0, b = R ? zq : 0;
                const uint64_t dl = a > b ? a - b : b - a;
                // the two counts of every link live as 12-bit fields of packed words (a thread of score_tile meets at most 16 samples;
                // fragment_score_kernel, whose threads meet any number, empties the words before a field can fill up):
                // pk[0]/pk[1] mask mismatches added / subtracted, pk[2]/pk[3] non-zero link differences added / subtracted
                pk[NEG ? 1 : 0] += (uint64_t)(M != R) << (12 * (l - 1));
                pk[NEG ? 3 : 2] += (uint64_t)(dl != 0) << (12 * (l - 1));
                acc<NEG>(s[SUM_LINK0 + 3 * l + 2], dl);
            }
        }
    }
}

// Pixels of a tile that take part in the loss: inside the image and, for the lookup loss, the crop.
__device__ static inline bool pixel_active(int row, int col, int W, int H, int r0, int r1, int c0, int c1)
{
    return row < H && col < W && row >= r0 && row <= r1 && col >= c0 && col <= c1;
}

// Loss sums of one tile.  DELTA = false: plain sums of a tile with nothing rendered.
// DELTA = true: sums(tile) - sums(base tile), which only the samples whose key differs contribute to —
// all others are skipped without touching the target planes.  Arithmetic is
// modulo 2^64, the frame total of the "nothing rendered" sums is added back by finalize_argmin_kernel.
// Rows [r_lo, r_hi] and 4-sample column groups [g_lo, g_hi] of a tile that a launch may have drawn into.
struct TileRect { int r_lo, r_hi, g_lo, g_hi; int block_g; };   // block_g: log2 of a wave's block width in groups (3, 4 or 5)

template <int LOSS, bool DELTA>
__device__ static inline void score_tile(const uint32_t *tile, const uint32_t *__restrict__ base /* global, or nullptr = nothing */,
                                         int row0, int col0, const FrameParams &fp, int n_render,
                                         const uint64_t *__restrict__ tq, const float *__restrict__ t32,
                                         const uint64_t *__restrict__ tl, uint64_t *lds_sums, const TileRect rc)
{
    const size_t plane = (size_t)fp.W * fp.H;
    uint64_t s[ROPE_SUM_WORDS];
#pragma unroll
    for (int k = 0; k < ROPE_SUM_WORDS; k++) s[k] = 0;
    uint64_t pk[4] = {0, 0, 0, 0};                      // ROPE_LOSS_FULL: packed per-link counts (score_pixel)
    if (DELTA) {
        // Only samples whose key differs from the base tile (the shared layer, or nothing) change the sums, and only
        // the rectangle this launch could draw into can hold any.  The z-test is a minimum over keys, so the tile
        // holds this launch's own samples and min(tile, base) is the finished image: the base is never copied to LDS.
        // A wave takes a compact block of the tile — 2^BLOCK_G groups wide, 64 >> BLOCK_G rows high — instead of two
        // whole rows: the robot's image is a blob, and the blocks inside it keep all their lanes busy.
        static_assert((TILE_W / 4) == 32, "block mapping below assumes 32 four-sample groups per tile row");
        const int bg = rc.block_g, brows = 64 >> bg, bpr_sh = 5 - bg;            // blocks per band of rows: 32 >> bg
        const int n_items = (rc.r_hi - rc.r_lo + 1) * (TILE_W / 4);
        for (int it = threadIdx.x; it < n_items; it += blockDim.x) {
            const int b = it >> 6, l = it & 63;
            const int g = ((b & ((1 << bpr_sh) - 1)) << bg) | (l & ((1 << bg) - 1));
            const int i4 = (rc.r_lo + (b >> bpr_sh) * brows + (l >> bg)) * (TILE_W / 4) + g;
            uint4 k4 = reinterpret_cast<const uint4 *>(tile)[i4];
            const uint4 b4 = base ? reinterpret_cast<const uint4 *>(base)[i4] : make_uint4(KEY_EMPTY, KEY_EMPTY, KEY_EMPTY, KEY_EMPTY);
            k4.x = min(k4.x, b4.x); k4.y = min(k4.y, b4.y); k4.z = min(k4.z, b4.z); k4.w = min(k4.w, b4.w);
            if (k4.x == b4.x && k4.y == b4.y && k4.z == b4.z && k4.w == b4.w) continue;
            const uint32_t keys[4] = {k4.x, k4.y, k4.z, k4.w}, bas[4] = {b4.x, b4.y, b4.z, b4.w};
            const int row = row0 + (4 * i4) / TILE_W, colg = col0 + (4 * i4) % TILE_W;
            if (row >= fp.H || colg >= fp.W) continue;
            const size_t pixg = (size_t)row * fp.W + colg;
            // the four samples sit side by side: fetch their target words together, one wait instead of four
            constexpr bool USE_F = (LOSS == ROPE_LOSS_LOOKUP || LOSS == ROPE_LOSS_TSWEEP);
            uint64_t tw[4] = {0, 0, 0, 0};
            float tf[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (colg + 3 < fp.W && !(fp.W & 3)) {
                if (USE_F) {
                    const float4 f = *reinterpret_cast<const float4 *>(t32 + pixg);
                    tf[0] = f.x; tf[1] = f.y; tf[2] = f.z; tf[3] = f.w;
                } else {
                    const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(tq + pixg), b = *reinterpret_cast<const ulonglong2 *>(tq + pixg + 2);
                    tw[0] = a.x; tw[1] = a.y; tw[2] = b.x; tw[3] = b.y;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (colg + j < fp.W) { if (USE_F) tf[j] = t32[pixg + j]; else tw[j] = tq[pixg + j]; }
            }
            // ROPE_LOSS_FULL: a link's terms at a sample depend on the image only through "is this the link drawn here", so in
            // sums(tile) - sums(base) every link that is drawn in neither cancels, sample by sample and exactly.  The links that
            // are drawn somewhere in this wave's block (usually one or two of the five) are the only ones whose terms are worked
            // out: a uniform branch per link, taken from a vote.
            unsigned links = 0xFFu;
            if (LOSS == ROPE_LOSS_FULL) {
                unsigned mine = 0;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (keys[j] != bas[j]) mine |= (keys[j] == KEY_EMPTY ? 0u : 1u << (keys[j] & 7u)) | (bas[j] == KEY_EMPTY ? 0u : 1u << (bas[j] & 7u));
                links = 0;
#pragma unroll
                for (int l = 1; l < ROPE_MAX_LINKS; l++) links |= __ballot((mine >> l) & 1u) ? 1u << l : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (keys[j] == bas[j]) continue;
                if (!pixel_active(row, colg + j, fp.W, fp.H, fp.r0, fp.r1, fp.c0, fp.c1)) continue;
                score_pixel<LOSS, false>(keys[j], pixg + j, n_render, tw[j], tf[j], tl, plane, fp.c_num, fp.c_sum, fp.c_dif, s, pk, links);
                score_pixel<LOSS, true>(bas[j], pixg + j, n_render, tw[j], tf[j], tl, plane, fp.c_num, fp.c_sum, fp.c_dif, s, pk, links);
            }
        }
    } else {
        for (int i = threadIdx.x; i < TILE_W * TILE_H; i += blockDim.x) {
            int row = row0 + i / TILE_W, col = col0 + i % TILE_W;
            if (!pixel_active(row, col, fp.W, fp.H, fp.r0, fp.r1, fp.c0, fp.c1)) continue;
            const size_t pix = (size_t)row * fp.W + col;
            constexpr bool USE_F = (LOSS == ROPE_LOSS_LOOKUP || LOSS == ROPE_LOSS_TSWEEP);
            score_pixel<LOSS>(KEY_EMPTY, pix, n_render, USE_F ? 0ull : tq[pix], USE_F ? t32[pix] : 0.0f, tl, plane, fp.c_num, fp.c_sum, fp.c_dif, s, pk);
        }
    }
    if (LOSS == ROPE_LOSS_CAMFULL) {
#pragma unroll
        for (int l = 0; l < ROPE_MAX_LINKS; l++) {
            s[SUM_LINK0 + 3 * l] = ((pk[0] >> (10 * l)) & 0x3FFull) - ((pk[1] >> (10 * l)) & 0x3FFull);
            s[SUM_LINK0 + 3 * l + 1] = ((pk[2] >> (10 * l)) & 0x3FFull) - ((pk[3] >> (10 * l)) & 0x3FFull);
        }
    }
    if (LOSS == ROPE_LOSS_FULL) {
#pragma unroll
        for (int l = 1; l < ROPE_MAX_LINKS; l++) {
            s[SUM_LINK0 + 3 * l] = ((pk[0] >> (12 * (l - 1))) & 0xFFFull) - ((pk[1] >> (12 * (l - 1))) & 0xFFFull);
            s[SUM_LINK0 + 3 * l + 1] = ((pk[2] >> (12 * (l - 1))) & 0xFFFull) - ((pk[3] >> (12 * (l - 1))) & 0xFFFull);
        }
    }
    // one LDS atomic per word and wave: the partial sums (modulo 2^64) are added up across the lanes first, and
    // waves that met no sample skip the whole step
    bool any = false;
#pragma unroll
    for (int k = 0; k < ROPE_SUM_WORDS; k++) any = any || s[k] != 0;
    if (__ballot(any) == 0) return;
#pragma unroll
    for (int k = 0; k < ROPE_SUM_WORDS; k++) {
        const bool used = (LOSS == ROPE_LOSS_FULL || LOSS == ROPE_LOSS_CAMFULL) ? true : (k < SUM_LINK0);
        if (!used) continue;
        uint64_t v = s[k];
        // a word nobody in the wave added to (the terms of a link that is drawn nowhere in the wave's block: most of the 20 words
        // of the full loss) needs no exchange — the twelve steps of one cost more than a thread's share of the samples
        if ((LOSS == ROPE_LOSS_FULL || LOSS == ROPE_LOSS_CAMFULL) && __ballot(v != 0) == 0) continue;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long *)&lds_sums[k], (unsigned long long)v);
    }
}

// ---------------------------------------------------------------- finalize -----
__device__ static inline double mean_std_parts(const uint64_t *s, double N, double &m1)
{
    m1 = ((double)s[SUM_S1] * 0x1p-32) / N;
    double S2 = ((double)s[SUM_AA] * 0x1p40 + (double)s[SUM_AB] * 0x1p21) + (double)s[SUM_BB];
    double m2 = (S2 * 0x1p-64) / N;
    double var = m2 - m1 * m1;
    if (var < 0.0) var = 0.0;
    return sqrt(var);
}

}  // namespace rope
