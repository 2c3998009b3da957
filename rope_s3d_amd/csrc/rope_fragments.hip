// rope_fragments.hip — the kept fragments of a fixed grid (rope_ctx::frags, rope_fragstore.h): count, fill and score kernels and
// their launch functions.  The loss terms are rope_lossmath.h's; the key tiles come from a MODE_LAYER launch of rope_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rope_kernels.h"
#include "rope_lossmath.h"
#include "rope_launch.h"

namespace rope {

// ----------------------------------------------------------- kept fragments -----
// What the scoring launch draws of a row — its own links l_begin .. n_render - 1 into a tile, tested against the row's shared layer —
// is a function of geometry alone, and of all the samples of a (row, tile) pair only those where the row's own links
// beat the layer enter the row's sums: score_tile<.., DELTA> skips every 16-byte group in which min(own, base) == base.  A grid
// that is scored again and again keeps exactly those groups (rope_ctx::frags): a MODE_LAYER launch over the rows' own links leaves
// whole key tiles in a scratch, chunk of rows by chunk of rows, fragment_count_kernel / fragment_fill_kernel compact them into one
// store (the pattern of the lookup table's kernels, rope_table.hip), and fragment_score_kernel streams a row's groups against the target.

// the row's shared layer over this tile, or nullptr where the layer's representative has no mask_lo bit (raster_tile's layer_tile)
__device__ static inline const uint4 *fragment_base_tile(const RasterArgs &ra, int cand, int tile_id, int n_tiles)
{
    const int layer = ra.layer_of[cand];
    const bool lo = (ra.mask_lo[(size_t)ra.layer_rep[layer] * ra.mask_words + (tile_id >> 5)] >> (tile_id & 31)) & 1u;
    return lo ? reinterpret_cast<const uint4 *>(ra.layers + ((size_t)layer * n_tiles + tile_id) * (TILE_W * TILE_H)) : nullptr;
}

__device__ static inline bool fragment_beats(const uint4 k, const uint4 b) { return k.x < b.x || k.y < b.y || k.z < b.z || k.w < b.w; }

// Grid = (tiles, rows of the chunk): own = the chunk's key tiles (rows x tiles x TILE_W*TILE_H, written by the MODE_LAYER launch
// for the pairs whose mask_hi bit is set; the others hold anything and are not read).  counts: C x tiles, zeroed before the first chunk.
__global__ void __launch_bounds__(256)
fragment_count_kernel(RasterArgs ra, const uint32_t *__restrict__ own, int row0, int n_tiles, uint32_t *__restrict__ counts)
{
    __shared__ int s_n;
    const int tile_id = blockIdx.x, cand = row0 + (int)blockIdx.y;
    if (!((ra.mask_hi[(size_t)cand * ra.mask_words + (tile_id >> 5)] >> (tile_id & 31)) & 1u)) return;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint4 *k4 = reinterpret_cast<const uint4 *>(own + ((size_t)blockIdx.y * n_tiles + tile_id) * (TILE_W * TILE_H));
    const uint4 *b4 = fragment_base_tile(ra, cand, tile_id, n_tiles);
    const uint4 none = make_uint4(KEY_EMPTY, KEY_EMPTY, KEY_EMPTY, KEY_EMPTY);
    int mine = 0;
    for (int g = threadIdx.x; g < TILE_W * TILE_H / 4; g += blockDim.x) mine += fragment_beats(k4[g], b4 ? b4[g] : none);
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0) counts[(size_t)cand * n_tiles + tile_id] = (uint32_t)s_n;
}

// The same walk, writing: the groups of a (row, tile) pair from offs[row * tiles + tile] on, IN ORDER of their place in the tile
// (table_fill_kernel's compaction), so that a row's list is ordered by tile, then group, and neighbouring lanes of the scorer read
// neighbouring pieces of the target.
__global__ void __launch_bounds__(256)
fragment_fill_kernel(RasterArgs ra, const uint32_t *__restrict__ own, int row0, int n_tiles, const unsigned long long *__restrict__ offs,
                     uint32_t *__restrict__ where, uint4 *__restrict__ finished, uint4 *__restrict__ base_keys)
{
    __shared__ int s_wave[4];
    const int tile_id = blockIdx.x, cand = row0 + (int)blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!((ra.mask_hi[(size_t)cand * ra.mask_words + (tile_id >> 5)] >> (tile_id & 31)) & 1u)) return;
    const size_t slot = (size_t)cand * n_tiles + tile_id;
    const unsigned long long first = offs[slot], last = offs[slot + 1];
    if (last == first) return;                                                         // nothing of this pair is kept (uniform)
    const uint4 *k4 = reinterpret_cast<const uint4 *>(own + ((size_t)blockIdx.y * n_tiles + tile_id) * (TILE_W * TILE_H));
    const uint4 *b4 = fragment_base_tile(ra, cand, tile_id, n_tiles);
    const uint4 none = make_uint4(KEY_EMPTY, KEY_EMPTY, KEY_EMPTY, KEY_EMPTY);
    static_assert((TILE_W * TILE_H / 4) % 256 == 0 && TILE_W * TILE_H / 4 <= 4096, "whole rounds of 256 groups; a group index fits 12 bits");
    int running = 0;
    for (int g0 = 0; g0 < TILE_W * TILE_H / 4; g0 += 256) {
        const int g = g0 + (int)threadIdx.x;
        uint4 k = k4[g];
        const uint4 b = b4 ? b4[g] : none;
        const bool any = fragment_beats(k, b);
        const unsigned long long m = __ballot(any);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; w++) { before += w < wave ? s_wave[w] : 0; all += s_wave[w]; }
        const unsigned long long pos = first + (unsigned long long)(running + before + __popcll(m & ((1ull << lane) - 1ull)));
        if (any && pos < last) {                                // never past the place the count pass reserved for this pair
            k.x = min(k.x, b.x); k.y = min(k.y, b.y); k.z = min(k.z, b.z); k.w = min(k.w, b.w);
            where[pos] = ((uint32_t)tile_id << 12) | (uint32_t)g;
            finished[pos] = k;
            base_keys[pos] = b;
        }
        running += all;
        __syncthreads();
    }
}

// One workgroup per row: the row's kept groups against the target — the body of score_tile's delta loop on stored keys instead of
// an LDS tile (score_pixel on the finished key, score_pixel<.., NEG> on the base key, for the samples where they differ and that
// take part in the loss; the full loss's vote over the links drawn in the wave, its packed counts) — then the loss sums of the row's
// layer over every tile the layer reaches (ra.layer_sums, this pass's), and the row's 23 words stored whole: nothing is accumulated
// into, so nothing has to be cleared.  Integer sums modulo 2^64: the words of raster_queue_kernel<LOSS, SCORE>, bit for bit.
template <int LOSS>
__global__ void __launch_bounds__(256)
fragment_score_kernel(FrameParams fp, RasterArgs ra, const unsigned long long *__restrict__ offs, const uint32_t *__restrict__ where,
                      const uint4 *__restrict__ finished, const uint4 *__restrict__ base_keys)
{
    __shared__ uint64_t lds_sums[ROPE_SUM_WORDS];
    const int tid = threadIdx.x, cand = blockIdx.x, n_tiles = fp.tiles_x * fp.tiles_y;
    const size_t plane = (size_t)fp.W * fp.H;
    const uint64_t *__restrict__ tq = ra.tq;
    const float *__restrict__ t32 = ra.t32;
    const int n_render = ra.n_render;
    if (tid < ROPE_SUM_WORDS) lds_sums[tid] = 0;
    __syncthreads();
    uint64_t s[ROPE_SUM_WORDS];
#pragma unroll
    for (int k = 0; k < ROPE_SUM_WORDS; k++) s[k] = 0;
    uint64_t pk[4] = {0, 0, 0, 0};
    const unsigned long long begin = offs[(size_t)cand * n_tiles], end = offs[(size_t)(cand + 1) * n_tiles];
    constexpr bool USE_F = (LOSS == ROPE_LOSS_LOOKUP || LOSS == ROPE_LOSS_TSWEEP);
    // The full loss's packed counts are 12-bit fields and a round adds at most 4 to one: they are emptied into the sums every
    // FRAGMENT_PK_ROUNDS rounds (4 x 1000 < 4096), since nothing bounds the rounds of a row — a 4K frame gives a thread thousands.
    constexpr int FRAGMENT_PK_ROUNDS = 1000;
    int rounds = 0;
    for (unsigned long long i0 = begin; i0 < end; i0 += 256) {                        // uniform: every lane takes every round
        if (LOSS == ROPE_LOSS_FULL && ++rounds > FRAGMENT_PK_ROUNDS) {
#pragma unroll
            for (int l = 1; l < ROPE_MAX_LINKS; l++) {
                s[SUM_LINK0 + 3 * l] += ((pk[0] >> (12 * (l - 1))) & 0xFFFull) - ((pk[1] >> (12 * (l - 1))) & 0xFFFull);
                s[SUM_LINK0 + 3 * l + 1] += ((pk[2] >> (12 * (l - 1))) & 0xFFFull) - ((pk[3] >> (12 * (l - 1))) & 0xFFFull);
            }
            pk[0] = pk[1] = pk[2] = pk[3] = 0;
            rounds = 1;
        }
        const unsigned long long i = i0 + (unsigned long long)tid;
        bool use = i < end;
        uint32_t w = 0;
        uint4 k4 = make_uint4(KEY_EMPTY, KEY_EMPTY, KEY_EMPTY, KEY_EMPTY), b4 = k4;
        if (use) { w = where[i]; k4 = finished[i]; b4 = base_keys[i]; }
        const int tile_id = (int)(w >> 12), i4 = (int)(w & 0xFFFu);
        const int row = (tile_id / fp.tiles_x) * TILE_H + (4 * i4) / TILE_W, colg = (tile_id % fp.tiles_x) * TILE_W + (4 * i4) % TILE_W;
        use = use && row < fp.H && colg < fp.W;
        const uint32_t keys[4] = {k4.x, k4.y, k4.z, k4.w}, bas[4] = {b4.x, b4.y, b4.z, b4.w};
        const size_t pixg = (size_t)row * fp.W + colg;
        uint64_t tw[4] = {0, 0, 0, 0};
        float tf[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (use) {
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
        }
        unsigned links = 0xFFu;
        if (LOSS == ROPE_LOSS_FULL) {
            unsigned mine = 0;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (use && keys[j] != bas[j]) mine |= (keys[j] == KEY_EMPTY ? 0u : 1u << (keys[j] & 7u)) | (bas[j] == KEY_EMPTY ? 0u : 1u << (bas[j] & 7u));
            links = 0;
#pragma unroll
            for (int l = 1; l < ROPE_MAX_LINKS; l++) links |= __ballot((mine >> l) & 1u) ? 1u << l : 0u;
        }
        if (!use) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (keys[j] == bas[j]) continue;
            if (!pixel_active(row, colg + j, fp.W, fp.H, fp.r0, fp.r1, fp.c0, fp.c1)) continue;
            score_pixel<LOSS, false>(keys[j], pixg + j, n_render, tw[j], tf[j], nullptr, plane, fp.c_num, fp.c_sum, fp.c_dif, s, pk, links);
            score_pixel<LOSS, true>(bas[j], pixg + j, n_render, tw[j], tf[j], nullptr, plane, fp.c_num, fp.c_sum, fp.c_dif, s, pk, links);
        }
    }
    if (LOSS == ROPE_LOSS_FULL) {
#pragma unroll
        for (int l = 1; l < ROPE_MAX_LINKS; l++) {
            s[SUM_LINK0 + 3 * l] += ((pk[0] >> (12 * (l - 1))) & 0xFFFull) - ((pk[1] >> (12 * (l - 1))) & 0xFFFull);
            s[SUM_LINK0 + 3 * l + 1] += ((pk[2] >> (12 * (l - 1))) & 0xFFFull) - ((pk[3] >> (12 * (l - 1))) & 0xFFFull);
        }
    }
#pragma unroll
    for (int k = 0; k < ROPE_SUM_WORDS; k++) {
        if (LOSS != ROPE_LOSS_FULL && k >= SUM_LINK0) continue;
        uint64_t v = s[k];
        if (__ballot(v != 0) == 0) continue;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0 && v) atomicAdd((unsigned long long *)&lds_sums[k], (unsigned long long)v);
    }
    __syncthreads();
    if (tid < ROPE_SUM_WORDS) {
        uint64_t v = lds_sums[tid];
        const int layer = ra.layer_of[cand];
        const uint32_t *lo = ra.mask_lo + (size_t)ra.layer_rep[layer] * ra.mask_words;
        for (int wd = 0; 32 * wd < n_tiles; wd++)
            for (uint32_t m = lo[wd]; m; m &= m - 1)
                v += ra.layer_sums[((size_t)layer * n_tiles + 32 * wd + __ffs((int)m) - 1) * ROPE_SUM_WORDS + tid];
        ra.sums[(size_t)cand * ROPE_SUM_WORDS + tid] = v;
    }
}

// ------------------------------------------------------------ launch helpers ---
hipError_t launch_fragment_count(hipStream_t st, const RasterArgs &a, const uint32_t *own, int row0, int rows, int n_tiles, uint32_t *counts)
{
    hipLaunchKernelGGL(fragment_count_kernel, dim3(n_tiles, rows), dim3(256), 0, st, a, own, row0, n_tiles, counts);
    return hipGetLastError();
}

hipError_t launch_fragment_fill(hipStream_t st, const RasterArgs &a, const uint32_t *own, int row0, int rows, int n_tiles,
                                const unsigned long long *offs, uint32_t *where, uint4 *finished, uint4 *base_keys)
{
    hipLaunchKernelGGL(fragment_fill_kernel, dim3(n_tiles, rows), dim3(256), 0, st, a, own, row0, n_tiles, offs, where, finished, base_keys);
    return hipGetLastError();
}

hipError_t launch_fragment_score(int loss, int rows, hipStream_t st, const FrameParams &fp, const RasterArgs &a, const unsigned long long *offs,
                                 const uint32_t *where, const uint4 *finished, const uint4 *base_keys)
{
    const dim3 grid(rows);
    if (!with_loss<LOSSES_LAYERED>(loss, [&](auto l) {
            hipLaunchKernelGGL(fragment_score_kernel<decltype(l)::value>, grid, dim3(256), 0, st, fp, a, offs, where, finished, base_keys);
        }))
        return hipErrorInvalidValue;               // the camera-pose loss has no shared layers, so no kept fragments either
    return hipGetLastError();
}

}  // namespace rope
