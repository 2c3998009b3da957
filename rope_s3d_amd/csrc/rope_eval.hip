// rope_eval.hip — evaluation of the segmentation stage, for gfx950: how far the instance planes a detector left in HBM overlap the
// ground-truth labels of their frames, as exact pixel counts.  Per plane k of frame i and label bit b:
//   inter[k][b]   = #{ pixels : pred_k != 0 and bit b of gt_i set }      area_pred[k] = #{ pixels : pred_k != 0 }
//   area_gt[i][b] = #{ pixels : bit b of gt_i set }
// Matching and average precision (rope_s3d_amd/evaluation.py) are a few hundred numbers per frame and stay on the host.
//
// The work is a stream over bytes.  A plane starts at byte k H W of the stack, so for odd H W most planes are not 16-byte aligned:
// a plane is cut into a head (up to the first 16-byte boundary of its ADDRESS), a body of whole 16-byte vectors and a tail.  The
// body is read once from HBM with one 16-byte load per lane; the frame's label plane is read alongside it (16 bytes at the same
// offset, at whatever alignment that has there: it is small and stays in L2 across the frame's planes); head and tail go byte by
// byte through the same counting step.  Counting is done on whole dwords: bit 0 of every non-zero byte -> that mask times 255
// keeps the label bytes under the instance -> one AND and one popcount per label.  Nine counters per lane (area, eight labels),
// summed across the wave in registers, across the workgroup through LDS, then ONE integer atomic add per counter and workgroup:
// integer adds commute, so the counts are the same bytes from run to run.  A large plane is split over several workgroups, so
// that one frame with few instances still fills the device.  No floating point, no per-pixel atomics.
//
// The same kernel counts area_gt: with no instance plane every byte counts as set and the eight label counters are the areas.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int EV_FRAMES = 64;                 // frames per launch: their plane offsets travel as kernel arguments
constexpr int EV_TARGET_GROUPS = 2048;        // workgroups a launch aims for before it stops splitting planes (256 CUs x 8)

// first[i] .. first[i + 1] - 1 are the planes of the launch's i-th frame; the entries past n_frames repeat the last one
struct FrameTable { int32_t first[EV_FRAMES + 1]; };

struct Counts { uint32_t c[9]; };             // [0] non-zero bytes, [1 + b] of them with label bit b

// four bytes of an instance plane and the four label bytes of the same pixels
__device__ __forceinline__ void count_dword(Counts &n, uint32_t p, uint32_t g)
{
    const uint32_t high = (p | ((p & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u;      // bit 7 of every non-zero byte
    const uint32_t one = high >> 7;
    const uint32_t under = g & ((high - one) | high);                                  // 0xFF where the byte is non-zero
    n.c[0] += __popc(one);
#pragma unroll
    for (int b = 0; b < 8; b++) n.c[1 + b] += __popc(under & (0x01010101u << b));
}

__device__ __forceinline__ void count_vector(Counts &n, const uint4 p, const uint4 g)
{
    count_dword(n, p.x, g.x);
    count_dword(n, p.y, g.y);
    count_dword(n, p.z, g.z);
    count_dword(n, p.w, g.w);
}

// 16 bytes at any alignment (the hardware takes unaligned global loads; the compiler is told not to assume more than bytes)
__device__ __forceinline__ uint4 load_unaligned(const uint8_t *p)
{
    uint4 v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}

// Workgroup blockIdx.x = plane * splits + part.  HAS_PRED: planes are the instance planes k0 + plane, their frames found in the
// table; otherwise plane IS the frame (f0 + plane), every byte counts as set, and the label counters go to area_gt.
template <bool HAS_PRED>
__global__ void __launch_bounds__(EV_THREADS)
mask_overlaps_kernel(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, const FrameTable tab, int n_frames, int f0,
                     size_t hw, int splits, uint32_t *__restrict__ inter, uint32_t *__restrict__ area_pred, uint32_t *__restrict__ area_gt)
{
    __shared__ uint32_t s_part[EV_WAVES][9];
    const int t = threadIdx.x;
    const int plane = blockIdx.x / splits, part = blockIdx.x - plane * splits;
    int frame = plane, k = 0;
    if (HAS_PRED) {
        k = tab.first[0] + plane;
        frame = 0;
        while (frame + 1 < n_frames && tab.first[frame + 1] <= k) frame++;             // uniform: scalar loads of the arguments
    }
    const uint8_t *const g0 = gt + (size_t)(f0 + frame) * hw;
    const uint8_t *const p0 = HAS_PRED ? pred + (size_t)k * hw : g0;                   // without planes the cut follows the label plane
    // head [0, head), body [head, head + 16 n_vec), tail [head + 16 n_vec, hw): offsets into the plane
    size_t head = (size_t)(-(intptr_t)p0) & 15;
    if (head > hw) head = hw;
    const size_t n_vec = (hw - head) / 16;
    const size_t tail = head + n_vec * 16;

    Counts n = {};
    const size_t per = (n_vec + splits - 1) / splits;
    const size_t v_begin = per * part, v_end = v_begin + per < n_vec ? v_begin + per : n_vec;
    const uint4 all = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
    size_t v = v_begin + t;
    for (; v + 3 * EV_THREADS < v_end; v += 4 * EV_THREADS) {                          // four loads of each stream in flight per lane
        uint4 p[4], g[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t o = head + (v + u * EV_THREADS) * 16;
            p[u] = HAS_PRED ? *reinterpret_cast<const uint4 *>(p0 + o) : all;
            g[u] = HAS_PRED ? load_unaligned(g0 + o) : *reinterpret_cast<const uint4 *>(g0 + o);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) count_vector(n, p[u], g[u]);
    }
    for (; v < v_end; v += EV_THREADS) {
        const size_t o = head + v * 16;
        const uint4 p = HAS_PRED ? *reinterpret_cast<const uint4 *>(p0 + o) : all;
        const uint4 g = HAS_PRED ? load_unaligned(g0 + o) : *reinterpret_cast<const uint4 *>(g0 + o);
        count_vector(n, p, g);
    }
    if (part == 0 && t < 32) {                                                         // lanes 0-15 the head, 16-31 the tail: a byte each
        const size_t o = t < 16 ? (size_t)t : tail + (size_t)(t - 16);
        if (t < 16 ? o < head : o < hw) count_dword(n, HAS_PRED ? p0[o] : 1u, g0[o]);
    }

#pragma unroll
    for (int j = 0; j < 9; j++) {
        uint32_t s = n.c[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if ((t & 63) == 0) s_part[t >> 6][j] = s;
    }
    __syncthreads();
    if (t < 9) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < EV_WAVES; w++) s += s_part[w][t];
        if (HAS_PRED) {
            atomicAdd(t == 0 ? &area_pred[k] : &inter[(size_t)k * 8 + (t - 1)], s);
        } else if (t > 0) {
            atomicAdd(&area_gt[(size_t)(f0 + frame) * 8 + (t - 1)], s);
        }
    }
}

// into how many workgroups a plane of hw bytes is cut when the launch has n_planes of them: enough to fill the device, never
// less than one pass of the workgroup (256 vectors) each
int splits_of(size_t hw, long long n_planes)
{
    const long long passes = (long long)((hw / 16 + EV_THREADS - 1) / EV_THREADS);
    long long s = (EV_TARGET_GROUPS + n_planes - 1) / n_planes;
    if (s > passes) s = passes;
    return s < 1 ? 1 : (int)s;
}

}  // namespace

extern "C" int rope_seg_mask_overlaps(const uint8_t *pred_dev, const int32_t *inst_first, int n_frames, const uint8_t *gt_bits_dev, int H,
                                      int W, uint32_t *inter_dev, uint32_t *area_pred_dev, uint32_t *area_gt_dev, void *stream)
{
    if (n_frames < 0 || H < 1 || W < 1 || !inst_first || inst_first[0] != 0) return ROPE_E_ARG;
    for (int i = 0; i < n_frames; i++)
        if (inst_first[i + 1] < inst_first[i]) return ROPE_E_ARG;
    const size_t hw = (size_t)H * (size_t)W;
    if (hw > 0xFFFFFFFFull) return ROPE_E_ARG;                                         // the counters are 32 bits wide
    const int K = inst_first[n_frames];
    if (K > 0x7FFFFFFF - EV_TARGET_GROUPS) return ROPE_E_ARG;                          // planes x splits is a grid size
    if (n_frames > 0 && (!gt_bits_dev || !area_gt_dev)) return ROPE_E_ARG;
    if (K > 0 && (!pred_dev || !inter_dev || !area_pred_dev)) return ROPE_E_ARG;
    if (n_frames == 0) return ROPE_OK;

    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(area_gt_dev, 0, (size_t)n_frames * 8 * sizeof(uint32_t), st) != hipSuccess) return ROPE_E_HIP;
    if (K > 0 && (hipMemsetAsync(inter_dev, 0, (size_t)K * 8 * sizeof(uint32_t), st) != hipSuccess ||
                  hipMemsetAsync(area_pred_dev, 0, (size_t)K * sizeof(uint32_t), st) != hipSuccess))
        return ROPE_E_HIP;
    for (int f0 = 0; f0 < n_frames; f0 += EV_FRAMES) {
        const int nf = n_frames - f0 < EV_FRAMES ? n_frames - f0 : EV_FRAMES;
        FrameTable tab;
        for (int i = 0; i <= EV_FRAMES; i++) tab.first[i] = inst_first[f0 + (i < nf ? i : nf)];
        const int s_gt = splits_of(hw, nf);
        hipLaunchKernelGGL(mask_overlaps_kernel<false>, dim3((unsigned)(nf * s_gt)), dim3(EV_THREADS), 0, st, nullptr, gt_bits_dev, tab, nf,
                           f0, hw, s_gt, nullptr, nullptr, area_gt_dev);
        const long long planes = (long long)tab.first[nf] - tab.first[0];
        if (planes > 0) {
            const int s = splits_of(hw, planes);                                       // planes * s < planes + EV_TARGET_GROUPS
            hipLaunchKernelGGL(mask_overlaps_kernel<true>, dim3((unsigned)(planes * s)), dim3(EV_THREADS), 0, st, pred_dev, gt_bits_dev, tab,
                               nf, f0, hw, s, inter_dev, area_pred_dev, nullptr);
        }
    }
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
