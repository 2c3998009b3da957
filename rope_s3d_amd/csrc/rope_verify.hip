// rope_verify.hip — does a recorded frame agree with the render at its recorded pose?  For gfx950.  Per frame, from the render's
// depth R (float32 metres), its link ids (a byte, 255 = background) and the recorded depth T (float32 metres), the 28 exact integer
// sums of include/rope_s3d.h (rope_frame_agreement): how many pixels are measured, how many are drawn, and per link how many of
// its pixels are measured at all, lie within the tolerance of the render, or have something in front of them; plus the summed
// absolute difference in Q32 metres.  The rule that turns the sums into flagged frames is host arithmetic (data/verification.py).
//
// The work is a stream: 9 bytes per pixel, each read once.  A frame's planes start at i H W elements, so for H W no multiple of
// four the float planes of most frames are not 16-byte aligned (they are always 4-byte aligned: the entry point refuses other
// pointers) and an id plane is aligned to nothing.  A frame is cut as rope_eval.hip cuts a plane: a head of 0..3 pixels up to the
// first 16-byte boundary of the render plane's ADDRESS, a body of quads (four pixels: one 16-byte load of R, one of T at the same
// offset and at whatever alignment it has there — the same as R's when both allocations are aligned alike, as torch's are — and
// one 4-byte load of the ids) and a tail of 0..3 pixels.  Head and tail go through the same counting step as quads of one pixel.
//
// Counting: the depths are compared per pixel in 64-bit integers (q(x) = floor(x 2^32), exact for a float32 in [0, 128)); what a
// pixel is — measured, close, in front — becomes bit 0 of its byte in three dword masks, and the per-link counters are then taken
// on the id dword as a whole: the bytes equal to l, one AND and one popcount per counter, as rope_eval.hip counts labels.
// Counters stay in registers (32 bits per lane: the entry point holds H W to 2^24), are summed across the wave with shuffles,
// across the workgroup through LDS, and reach memory as ONE 64-bit integer atomic per word and workgroup.  Integer adds commute:
// the sums are the same bytes from run to run.  No floating-point accumulation, no per-pixel atomics.  A frame is split over
// several workgroups so that a few large frames still fill the device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

constexpr int VF_THREADS = 256;
constexpr int VF_WAVES = VF_THREADS / 64;
constexpr int VF_TARGET_GROUPS = 2048;        // workgroups a launch aims for before it stops splitting frames (256 CUs x 8)
constexpr int VF_SLOTS = 3 + 4 * ROPE_MAX_LINKS;      // what a lane counts: measured, not background, the sum, four per link
constexpr uint32_t ONES = 0x01010101u;

struct Counts {
    uint32_t valid, drawn;                    // pixels with a measured T; pixels whose id is not the background's
    uint64_t sum;                             // |q(R) - q(T)| over the pixels both drawn (id < n_links) and measured
    uint32_t link[ROPE_MAX_LINKS][4];         // per link: rendered, both, close, front
};

// bit 0 of every byte of x that is zero
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x)
{
    return (~(x | ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u) >> 7;
}

// floor(x 2^32) of a depth held to [0, 128): NaN and negatives to 0, anything larger to the last float below 128
__device__ __forceinline__ int64_t q32(float x)
{
    const float c = fminf(fmaxf(x, 0.0f), 0x1.fffffep6f);                               // fmaxf(NaN, 0) = 0; the constant is 128 - 2^-17
    return (int64_t)__float2ull_rz(c * 4294967296.0f);                                  // a power of two: the product is exact
}

// four pixels: depths r and t, the four id bytes in one dword
__device__ __forceinline__ void count_quad(Counts &n, const float r[4], uint32_t ids, const float t[4], int n_links, int64_t tol_q)
{
    uint32_t valid = 0, close = 0, front = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool ok = t[j] > 0.0f && t[j] < 128.0f;                                   // false for NaN, inf, zero and negatives
        const int64_t d = q32(r[j]) - q32(t[j]);
        const int64_t a = d < 0 ? -d : d;
        const bool both = ok && (int)((ids >> (8 * j)) & 0xFFu) < n_links;
        valid |= (uint32_t)ok << (8 * j);
        close |= (uint32_t)(ok && a <= tol_q) << (8 * j);
        front |= (uint32_t)(ok && d > tol_q) << (8 * j);
        n.sum += both ? (uint64_t)a : 0ull;
    }
    n.valid += __popc(valid);
    n.drawn += 4 - __popc(zero_bytes(~ids));
#pragma unroll
    for (int l = 0; l < ROPE_MAX_LINKS; l++) {
        if (l < n_links) {                                                              // uniform
            const uint32_t eq = zero_bytes(ids ^ (ONES * (uint32_t)l));
            n.link[l][0] += __popc(eq);
            n.link[l][1] += __popc(eq & valid);
            n.link[l][2] += __popc(eq & close);
            n.link[l][3] += __popc(eq & front);
        }
    }
}

struct Quad { float v[4]; };

// 16 bytes of floats at 4-byte alignment, 4 id bytes at any (the hardware takes unaligned global loads; the compiler is told not
// to assume more)
__device__ __forceinline__ Quad load_floats(const float *p)
{
    Quad q;
    __builtin_memcpy(&q, __builtin_assume_aligned(p, 4), sizeof(q));
    return q;
}

__device__ __forceinline__ uint32_t load_ids(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}

// Workgroup blockIdx.x = frame * splits + part.
__global__ void __launch_bounds__(VF_THREADS)
frame_agreement_kernel(const float *__restrict__ render, const uint8_t *__restrict__ ids, const float *__restrict__ depth, size_t hw,
                       int splits, int n_links, int64_t tol_q, unsigned long long *__restrict__ sums)
{
    __shared__ uint64_t s_part[VF_WAVES][VF_SLOTS];
    const int t = threadIdx.x;
    const int frame = blockIdx.x / splits, part = blockIdx.x - frame * splits;
    const float *const r0 = render + (size_t)frame * hw;
    const float *const t0 = depth + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    // head [0, head), body [head, head + 4 n_vec), tail [head + 4 n_vec, hw): pixels of the frame
    size_t head = ((size_t)(-(intptr_t)r0) & 15) / 4;
    if (head > hw) head = hw;
    const size_t n_vec = (hw - head) / 4;
    const size_t tail = head + n_vec * 4;

    Counts n = {};
    const size_t per = (n_vec + splits - 1) / splits;
    const size_t v_begin = per * part, v_end = v_begin + per < n_vec ? v_begin + per : n_vec;
    size_t v = v_begin + t;
    for (; v + 3 * VF_THREADS < v_end; v += 4 * VF_THREADS) {                           // four loads of each stream in flight per lane
        float4 r[4];
        Quad d[4];
        uint32_t id[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t o = head + (v + u * VF_THREADS) * 4;
            r[u] = *reinterpret_cast<const float4 *>(r0 + o);
            d[u] = load_floats(t0 + o);
            id[u] = load_ids(i0 + o);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const float rr[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
            count_quad(n, rr, id[u], d[u].v, n_links, tol_q);
        }
    }
    for (; v < v_end; v += VF_THREADS) {
        const size_t o = head + v * 4;
        const float4 r = *reinterpret_cast<const float4 *>(r0 + o);
        const Quad d = load_floats(t0 + o);
        const float rr[4] = {r.x, r.y, r.z, r.w};
        count_quad(n, rr, load_ids(i0 + o), d.v, n_links, tol_q);
    }
    if (part == 0 && t < 8) {                                                           // lanes 0-3 the head, 4-7 the tail: a pixel each
        const size_t o = t < 4 ? (size_t)t : tail + (size_t)(t - 4);
        if (t < 4 ? o < head : o < hw) {
            const float rr[4] = {r0[o], 0.0f, 0.0f, 0.0f}, tt[4] = {t0[o], 0.0f, 0.0f, 0.0f};     // T = 0, background: counted nowhere
            count_quad(n, rr, 0xFFFFFF00u | i0[o], tt, n_links, tol_q);
        }
    }

    uint64_t slot[VF_SLOTS];
    slot[0] = n.valid;
    slot[1] = n.drawn;
    slot[2] = n.sum;
#pragma unroll
    for (int j = 0; j < 4 * ROPE_MAX_LINKS; j++) slot[3 + j] = n.link[j / 4][j % 4];
#pragma unroll
    for (int j = 0; j < VF_SLOTS; j++) {
        uint64_t s = slot[j];
        if (j == 2) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, d, 64);
        } else {                                                                        // a count: at most 2^24 per frame
            uint32_t c = (uint32_t)s;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
            s = c;
        }
        if ((t & 63) == 0) s_part[t >> 6][j] = s;
    }
    __syncthreads();
    if (t < ROPE_AGREE_WORDS) {
        // word 0 measured, 1 rendered (all links), 2 the sum, 3 ids that are neither a link's nor the background's, 4.. per link
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < VF_WAVES; w++) {
            uint64_t rendered = 0;
            for (int l = 0; l < ROPE_MAX_LINKS; l++) rendered += s_part[w][3 + 4 * l];
            s += t == 1 ? rendered : t == 3 ? s_part[w][1] - rendered : s_part[w][t < 3 ? t : t - 1];
        }
        atomicAdd(&sums[(size_t)frame * ROPE_AGREE_WORDS + t], (unsigned long long)s);
    }
}

}  // namespace

extern "C" int rope_frame_agreement(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames,
                                    int H, int W, int n_links, float tol_m, uint64_t *sums_dev, void *stream)
{
    static_assert(ROPE_AGREE_WORDS == 4 + 4 * ROPE_MAX_LINKS && ROPE_AGREE_WORDS == VF_SLOTS + 1, "the words of a frame");
    if (n_frames < 1 || H < 1 || W < 1 || n_links < 1 || n_links > ROPE_MAX_LINKS) return ROPE_E_ARG;
    if (!isfinite(tol_m) || tol_m < 0.0f) return ROPE_E_ARG;
    if (!render_depth_dev || !render_ids_dev || !frame_depth_dev || !sums_dev) return ROPE_E_ARG;
    if (((uintptr_t)render_depth_dev & 3) || ((uintptr_t)frame_depth_dev & 3) || ((uintptr_t)sums_dev & 7)) return ROPE_E_ARG;
    const size_t hw = (size_t)H * (size_t)W;
    if (hw > ((size_t)1 << 24)) return ROPE_E_ARG;                                     // 2^39 a pixel: word 2 and the 32-bit lane counters hold
    if (n_frames > 0x7FFFFFFF - VF_TARGET_GROUPS) return ROPE_E_ARG;                    // frames x splits is a grid size
    // q(tol); at 2^39 and beyond every pair of depths below 128 m is close, so larger tolerances need no more bits
    const double tq = floor((double)tol_m * 4294967296.0);
    const int64_t tol_q = tq >= 549755813888.0 ? ((int64_t)1 << 39) : (int64_t)tq;

    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums_dev, 0, (size_t)n_frames * ROPE_AGREE_WORDS * sizeof(uint64_t), st) != hipSuccess) return ROPE_E_HIP;
    // enough workgroups to fill the device, never less than one pass of the workgroup (256 quads) each
    const long long passes = (long long)((hw / 4 + VF_THREADS - 1) / VF_THREADS);
    long long splits = (VF_TARGET_GROUPS + (long long)n_frames - 1) / n_frames;
    if (splits > passes) splits = passes;
    if (splits < 1) splits = 1;                                                         // frames * splits < frames + VF_TARGET_GROUPS
    hipLaunchKernelGGL(frame_agreement_kernel, dim3((unsigned)((long long)n_frames * splits)), dim3(VF_THREADS), 0, st, render_depth_dev,
                       render_ids_dev, frame_depth_dev, hw, (int)splits, n_links, tol_q, (unsigned long long *)sums_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
