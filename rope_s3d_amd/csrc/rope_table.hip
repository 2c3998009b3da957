// rope_table.hip — the stored lookup table: the kernels that build it from dense rows, the kernels that score it against one
// frame's or many frames' targets, and their launch functions.  Pure streaming: nothing is drawn here (the rows come from a
// MODE_TABLE launch of rope_kernels.hip); the Q32 sums are rope_lossmath.h's, the argmin is rope_kernels.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "rope_kernels.h"
#include "rope_lossmath.h"

namespace rope {

// ------------------------------------------------------------- lookup table -----
// Lookup stage against a stored table (predict.py:165-171): per row k of the table, the exact sums of |T - sqrtD_k| in Q32
// over the crop.  The crop is the box of every pose of the grid; one pose covers a fraction of it, and where a row holds
// nothing the term is |T - 0|, the same for every row.  So a row is stored as the groups of samples that hold something
// (table_count_kernel / table_fill_kernel), the sums of |T| over the whole crop are taken once per frame (crop_total_kernel), and
// a row's sums are total + sum over its groups of (|T - D| - |T|) — integers, so exactly the sums over the whole crop.

// One workgroup: the crop of the target plane as one contiguous array — rows padded with zeros to a multiple of four samples, so
// that a group of the table (columns 4k .. 4k+3 of a crop row) is one aligned float4 at offset 4 x (its number) — and the sums of |T|
// over it.  (The same sums group by group, for a table row to subtract instead of working them out again per (row, frame), made the
// scoring kernel half as slow again, 9.8 against 6.6 ms for 256 frames x 15 625 rows: it waits for its gathers, not for its arithmetic.)
// grid = frames: frame f's plane starts f planes into t32, its crop f crops into t32c, its totals f x ROPE_SUM_WORDS into total
__global__ void __launch_bounds__(1024)
crop_total_kernel(FrameParams fp, const float *__restrict__ t32, float *__restrict__ t32c, uint64_t *__restrict__ total /* ROPE_SUM_WORDS */)
{
    __shared__ uint64_t lds[4];
    const int cw = fp.c1 - fp.c0 + 1, ch = fp.r1 - fp.r0 + 1, gw = (cw + 3) >> 2, n_groups = gw * ch;
    t32 += (size_t)blockIdx.x * fp.W * fp.H;
    t32c += (size_t)blockIdx.x * n_groups * 4;
    total += (size_t)blockIdx.x * ROPE_SUM_WORDS;
    if (threadIdx.x < 4) lds[threadIdx.x] = 0;
    __syncthreads();
    uint64_t s[ROPE_SUM_WORDS];
    s[SUM_S1] = s[SUM_AA] = s[SUM_AB] = s[SUM_BB] = 0;
    for (int g = threadIdx.x; g < n_groups; g += blockDim.x) {
        const int r = g / gw, c = 4 * (g - r * gw);
        const float *src = t32 + (size_t)(fp.r0 + r) * fp.W + fp.c0 + c;
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            t[j] = c + j < cw ? src[j] : 0.0f;
            acc_sq_wide<false>(s, q32_of_f32(fabsf(t[j] - 0.0f)));
        }
        reinterpret_cast<float4 *>(t32c)[g] = make_float4(t[0], t[1], t[2], t[3]);
    }
    const int words[4] = {SUM_S1, SUM_AA, SUM_AB, SUM_BB};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint64_t v = s[words[k]];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long *)&lds[k], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < ROPE_SUM_WORDS) {
        uint64_t v = 0;
        for (int k = 0; k < 4; k++) if ((int)threadIdx.x == words[k]) v = lds[k];
        total[threadIdx.x] = v;
    }
}

// Build time.  A dense row (the cropped sqrt-depth image of one grid pose) is mostly zeros: the crop is the box of every pose of the
// grid together, one pose covers a fraction of it, and the robot a fraction of its own bounding box.  A sample that holds nothing
// contributes |T - 0| - |T| = 0 to the row's sums, exactly — so the stored table keeps only the GROUPS of four consecutive samples
// of a crop row (columns 4k .. 4k+3) in which anything was drawn: per group four times its number — the offset of its first
// sample in a crop whose rows are padded to whole groups (crop_total_kernel's layout) — and its four values (columns past the
// crop's edge read as 0).  table_count_kernel counts a row's groups and reserves their place,
// table_fill_kernel writes them (in the order of their place in the crop: neighbouring lanes then read neighbouring samples).
__global__ void __launch_bounds__(256)
table_count_kernel(int cw, int ch, const float *__restrict__ table, uint32_t *__restrict__ counts, unsigned long long *__restrict__ offs,
                   unsigned long long *__restrict__ used)
{
    __shared__ int s_n;
    const int gw = (cw + 3) >> 2, n_groups = gw * ch;
    const float *row = table + (size_t)blockIdx.x * cw * ch;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int mine = 0;
    for (int g = threadIdx.x; g < n_groups; g += blockDim.x) {
        const int r = g / gw, c = 4 * (g - r * gw);
        bool any = false;
        for (int j = 0; j < 4; j++) any = any || (c + j < cw && row[(size_t)r * cw + c + j] != 0.0f);
        mine += any;
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = (uint32_t)s_n;
        offs[blockIdx.x] = s_n ? atomicAdd(used, (unsigned long long)s_n) : 0ull;
    }
}

__global__ void __launch_bounds__(256)
table_fill_kernel(int cw, int ch, const float *__restrict__ table, const unsigned long long *__restrict__ offs, uint32_t *__restrict__ goff,
                  float4 *__restrict__ gval)
{
    // The groups of a row are written IN ORDER of their place in the crop: the scoring kernels hand consecutive groups to
    // consecutive lanes, and a run of groups inside the robot's outline is then a run of neighbouring 16-byte pieces of the target —
    // eight lanes to a cache line instead of one line per lane.
    __shared__ int s_wave[4];
    const int gw = (cw + 3) >> 2, n_groups = gw * ch, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *row = table + (size_t)blockIdx.x * cw * ch;
    const unsigned long long base = offs[blockIdx.x];
    int running = 0;
    for (int g0 = 0; g0 < n_groups; g0 += 256) {
        const int g = g0 + (int)threadIdx.x;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool any = false;
        if (g < n_groups) {
            const int r = g / gw, c = 4 * (g - r * gw);
            for (int j = 0; j < 4; j++) { v[j] = c + j < cw ? row[(size_t)r * cw + c + j] : 0.0f; any = any || v[j] != 0.0f; }
        }
        const unsigned long long b = __ballot(any);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; w++) { before += w < wave ? s_wave[w] : 0; all += s_wave[w]; }
        if (any) {
            const int pos = running + before + __popcll(b & ((1ull << lane) - 1ull));
            goff[base + pos] = (uint32_t)(4 * g);
            gval[base + pos] = make_float4(v[0], v[1], v[2], v[3]);
        }
        running += all;
        __syncthreads();
    }
}

// One group against one cropped target: s += sum of |T - D| minus sum of |T| over its four samples (words S1, AA, AB, BB), modulo 2^64.
__device__ static inline void table_group_delta(const float4 t, const float4 d, uint64_t *s)
{
    acc_sq_wide<false>(s, q32_of_f32(fabsf(t.x - d.x))); acc_sq_wide<true>(s, q32_of_f32(fabsf(t.x - 0.0f)));
    acc_sq_wide<false>(s, q32_of_f32(fabsf(t.y - d.y))); acc_sq_wide<true>(s, q32_of_f32(fabsf(t.y - 0.0f)));
    acc_sq_wide<false>(s, q32_of_f32(fabsf(t.z - d.z))); acc_sq_wide<true>(s, q32_of_f32(fabsf(t.z - 0.0f)));
    acc_sq_wide<false>(s, q32_of_f32(fabsf(t.w - d.w))); acc_sq_wide<true>(s, q32_of_f32(fabsf(t.w - 0.0f)));
}

__global__ void __launch_bounds__(256)
table_score_kernel(const uint32_t *__restrict__ counts, const unsigned long long *__restrict__ offs, const uint32_t *__restrict__ goff,
                   const float4 *__restrict__ gval, const float *__restrict__ t32c, const uint64_t *__restrict__ total, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t lds[4];
    if (threadIdx.x < 4) lds[threadIdx.x] = 0;
    __syncthreads();
    const int n = (int)counts[blockIdx.x];
    const unsigned long long base = offs[blockIdx.x];
    uint64_t s[ROPE_SUM_WORDS];
    s[SUM_S1] = s[SUM_AA] = s[SUM_AB] = s[SUM_BB] = 0;
    for (int g = threadIdx.x; g < n; g += blockDim.x) table_group_delta(*reinterpret_cast<const float4 *>(t32c + goff[base + g]), gval[base + g], s);
    const int words[4] = {SUM_S1, SUM_AA, SUM_AB, SUM_BB};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint64_t v = s[words[k]];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long *)&lds[k], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < ROPE_SUM_WORDS) {
        uint64_t v = 0;
        for (int k = 0; k < 4; k++) if ((int)threadIdx.x == words[k]) v = total[words[k]] + lds[k];
        sums[(size_t)blockIdx.x * ROPE_SUM_WORDS + threadIdx.x] = v;
    }
}

// The same for the targets of many frames (rope_lookup_score_targets): grid = (table rows, frame chunks), and inside a workgroup
// one group of LANES lanes per (row, TABLE_FRAMES frames) — a row's few hundred groups are a handful per lane, so this needs no
// barrier and no LDS: a lane reads a group of the row once and holds it against TABLE_FRAMES frames' samples at that place (their
// loads in flight together), the lanes' partial sums meet by lane exchange and the group's first lane writes the finished lookup
// scores (finalize_one's steps for ROPE_LOSS_LOOKUP on the same sums: same bits) to scores[frame x rows + row].  The kernel lives on its arithmetic
// (two Q32 conversions and six 64-bit multiply-adds per sample) and on the waves in flight: few frames per wave, see the launch.
template <int TABLE_FRAMES, int LANES /* of a wave that share one frame: 64, or 16 (four frames side by side in a wave) */>
__global__ void __launch_bounds__(256)
table_score_frames_kernel(int crop_px /* padded: 4 x groups */, const uint32_t *__restrict__ counts, const unsigned long long *__restrict__ offs,
                          const uint32_t *__restrict__ goff, const float4 *__restrict__ gval, const float *__restrict__ t32c /* frames x crop_px */,
                          const uint64_t *__restrict__ totals /* frames x ROPE_SUM_WORDS */, int n_frames, double n_pix,
                          double *__restrict__ scores)
{
    // With LANES = 16 a wave holds four frame groups side by side: a row's few hundred groups are then twenty per lane instead of
    // five with the last step a third empty, the lane exchange is four steps instead of six and serves four times the frames, and
    // the float64 epilogue of four frames runs in four lanes at once.
    constexpr int PARTS = 64 / LANES, PER_WAVE = PARTS * TABLE_FRAMES;
    const int n = (int)counts[blockIdx.x], lane = threadIdx.x & 63, wave = threadIdx.x >> 6, part = lane / LANES, sub = lane % LANES;
    const unsigned long long base = offs[blockIdx.x];
    const int per = (n_frames + (int)gridDim.y - 1) / (int)gridDim.y, f_lo = (int)blockIdx.y * per, f_hi = min(f_lo + per, n_frames);
    for (int fw = f_lo + wave * PER_WAVE; fw < f_hi; fw += 4 * PER_WAVE) {
        const int f0 = fw + part * TABLE_FRAMES;                 // this lane group's first frame
        const int nf = max(0, min(TABLE_FRAMES, f_hi - f0));
        uint64_t s[TABLE_FRAMES][SUM_BB + 1];
#pragma unroll
        for (int j = 0; j < TABLE_FRAMES; j++)
#pragma unroll
            for (int k = 0; k <= SUM_BB; k++) s[j][k] = 0;
        const float *__restrict__ t0 = t32c + (size_t)min(f0, n_frames - 1) * crop_px;
        if (nf > 0)
            for (int g = sub; g < n; g += LANES) {
                const uint32_t off = goff[base + g];
                const float4 d = gval[base + g];
                float4 t[TABLE_FRAMES];
#pragma unroll
                for (int j = 0; j < TABLE_FRAMES; j++)
                    t[j] = j < nf ? *reinterpret_cast<const float4 *>(t0 + (size_t)j * crop_px + off) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int j = 0; j < TABLE_FRAMES; j++) table_group_delta(t[j], d, s[j]);
            }
#pragma unroll
        for (int j = 0; j < TABLE_FRAMES; j++) {
            uint64_t r[ROPE_SUM_WORDS];
#pragma unroll
            for (int k = SUM_S1; k <= SUM_BB; k++) {
                uint64_t v = s[j][k];
#pragma unroll
                for (int off = LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);      // stays inside the lane group
                r[k] = v;
            }
            if (sub == 0 && j < nf) {
                const uint64_t *total = totals + (size_t)(f0 + j) * ROPE_SUM_WORDS;
#pragma unroll
                for (int k = SUM_S1; k <= SUM_BB; k++) r[k] += total[k];
                double m1;
                const double sd = mean_std_parts(r, n_pix, m1);
                scores[(size_t)(f0 + j) * gridDim.x + blockIdx.x] = m1 * sd;
            }
        }
    }
}

// ------------------------------------------------------------ launch helpers ---
hipError_t launch_table_score_frames(hipStream_t st, const FrameParams &fp, const uint32_t *counts, const unsigned long long *offs,
                                     const uint32_t *goff, const float4 *gval, int C, const float *t32, int n_frames, float *t32c, uint64_t *totals,
                                     double *scores, double *best)
{
    const int cw = fp.c1 - fp.c0 + 1, ch = fp.r1 - fp.r0 + 1;
    hipLaunchKernelGGL(crop_total_kernel, dim3(n_frames), dim3(1024), 0, st, fp, t32, t32c, totals);
    // A workgroup takes 4 x F frames (F per wave), and the grid walks the table once per such chunk of frames (rows fastest): the
    // chunk's cropped targets stay in L2 while every row gathers from them, and the table streams past once per chunk.
    // Measured for 256 frames x 15 625 rows at 160x90 (tools/r03_tbl_run.sh), a whole wave per frame group: F = 8 7.2 ms (221
    // registers, two waves per SIMD), F = 4 5.1 ms, F = 2 4.8-5.0 ms; one frame per wave and every frame in one workgroup (round 3's
    // first form) 6.6 ms.  With F = 2 and the wave split into lane groups of 32 / 16 / 8: 4.0 / 3.4 / 3.2 ms.
    static const int F = [] { const char *e = std::getenv("ROPE_TABLE_FRAMES"); const int v = e ? std::atoi(e) : 2; return v == 4 || v == 8 ? v : 2; }();
    static const int LANES = [] { const char *e = std::getenv("ROPE_TABLE_LANES"); const int v = e ? std::atoi(e) : 16; return v == 64 || v == 8 ? v : 16; }();
    const int per_wg = 4 * F * (64 / LANES);
    const int chunks = std::max(1, (n_frames + per_wg - 1) / per_wg);
    const dim3 grid(C, chunks);
    const int words = (int)table_crop_words(fp);
    const double n_pix = (double)cw * (double)ch;
#define ROPE_TABLE_LAUNCH(F_, L_) hipLaunchKernelGGL((table_score_frames_kernel<F_, L_>), grid, dim3(256), 0, st, words, counts, offs, goff, gval, t32c, totals, n_frames, n_pix, scores)
    if (LANES == 16) { if (F == 2) ROPE_TABLE_LAUNCH(2, 16); else if (F == 4) ROPE_TABLE_LAUNCH(4, 16); else ROPE_TABLE_LAUNCH(8, 16); }
    else if (LANES == 8) { if (F == 2) ROPE_TABLE_LAUNCH(2, 8); else ROPE_TABLE_LAUNCH(4, 8); }
    else { if (F == 2) ROPE_TABLE_LAUNCH(2, 64); else if (F == 4) ROPE_TABLE_LAUNCH(4, 64); else ROPE_TABLE_LAUNCH(8, 64); }
#undef ROPE_TABLE_LAUNCH
    return launch_argmin_sets(st, scores, C, n_frames, best);      // rope_kernels.hip: one workgroup per frame's C scores
}

hipError_t launch_table_count(hipStream_t st, int cw, int ch, const float *table, int C, uint32_t *counts, unsigned long long *offs,
                              unsigned long long *used)
{
    hipLaunchKernelGGL(table_count_kernel, dim3(C), dim3(256), 0, st, cw, ch, table, counts, offs, used);
    return hipGetLastError();
}

hipError_t launch_table_fill(hipStream_t st, int cw, int ch, const float *table, int C, const unsigned long long *offs, uint32_t *goff, float4 *gval)
{
    hipLaunchKernelGGL(table_fill_kernel, dim3(C), dim3(256), 0, st, cw, ch, table, offs, goff, gval);
    return hipGetLastError();
}

hipError_t launch_table_score(hipStream_t st, const FrameParams &fp, const uint32_t *counts, const unsigned long long *offs, const uint32_t *goff,
                              const float4 *gval, int C, const float *t32, float *t32c, uint64_t *total, uint64_t *sums)
{
    hipLaunchKernelGGL(crop_total_kernel, dim3(1), dim3(1024), 0, st, fp, t32, t32c, total);
    hipLaunchKernelGGL(table_score_kernel, dim3(C), dim3(256), 0, st, counts, offs, goff, gval, t32c, total, sums);
    return hipGetLastError();
}

}  // namespace rope
