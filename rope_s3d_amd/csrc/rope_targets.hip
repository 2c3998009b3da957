// rope_targets.hip — the segmentation path's targets built on the device, for gfx950: instance masks that are already in HBM
// (the segmenter's (K, H, W) planes) and the frame's depth -> the packed plane, the lookup plane, the TensorSweep plane and the
// per-link flags of rope_set_targets, with no trip through host memory.  Per frame exactly what the host function
// rope_prepare_segmented (rope_hostprep.cpp) computes at f == 1:
//   merge      any |= m_k;  bits |= 1 << link_of[k] (link_of[k] >= 0);  look |= m_k (0 <= link_of[k] < n_lookup_links)
//   body       erode7(dilate8(any)), body_look = erode7(dilate8(look)): cv2's box kernels with their default anchors (the dilate
//              window of x is x-4..x+3, the erode window x-3..x+3, in both axes) and borders that never win: outside the image is
//              clear for the dilation and SET for the erosion of the dilated image
//   depth      d = (double)depth * (body ? 1 : 0);  dl = d * (body_look ? 1 : 0);  tq = q32(d) | bits << 40;  t32 = (float)dl;
//              tsweep = (float)d — one IEEE operation per written step (-ffp-contract=off)
//   flags      per link n_mask = pixels of its merged mask, n_depth = those with d != 0.0 (true for NaN): integer counts, so the
//              order of the additions does not matter; bit 0: the link has an instance, bit 1: n_depth > 0.05 n_mask in double
//
// One workgroup per (64 x 32 output tile, frame).  The tile and its halo (7 before, 6 after, per axis: 4 + 3 and 3 + 3) are merged
// into LDS as one byte per position, bit 0 = any, bit 1 = look: OR and AND are bitwise, so both masks ride through ONE morphology
// pass.  Four separable passes in LDS: rows then columns of the dilation, the positions of the dilated image that lie outside the
// frame set to "set", rows then columns of the erosion.  Global loads and stores run along x, one wave per tile row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rope_kernels.h"

namespace rope {
namespace {

constexpr int TG_TW = ROPE_TARGET_TILE_W, TG_TH = ROPE_TARGET_TILE_H;
constexpr int TG_THREADS = 256;
constexpr int TG_IN_W = TG_TW + 13, TG_IN_H = TG_TH + 13;      // merged masks: columns x0 - 7 .. x0 + TW + 5, rows likewise
constexpr int TG_DIL_W = TG_TW + 6, TG_DIL_H = TG_TH + 6;      // dilated image: columns x0 - 3 .. x0 + TW + 2, rows likewise
constexpr int TG_IN_PITCH = TG_IN_W + 3, TG_DIL_PITCH = TG_DIL_W + 2;
static_assert(TG_TW == 64, "one wave per tile row: the flag counts are ballots over a row");
static_assert((TG_TW * TG_TH) % TG_THREADS == 0, "whole rows per pass of the workgroup");

// depth in metres -> Q32 with the rounding and clipping of rope_pack_target (q32_of_depth, rope_hostprep.cpp): round half to even,
// NaN, inf, zero and negatives are "no depth", clipped to 2^39 - 1.  rint is exact where the host's 2^52 trick is, and beyond
// 2^52 both end at the clip.
__device__ inline uint64_t q32_of_depth_dev(double d)
{
    const double Q32 = 4294967296.0, top = 549755813887.0;
    double q = (d > 0.0 && d <= 1.7976931348623157e308) ? rint(d * Q32) : 0.0;
    q = q < top ? q : top;
    return (uint64_t)q;
}

template <typename DEPTH>
__global__ void __launch_bounds__(TG_THREADS)
segmented_targets_kernel(const DEPTH *__restrict__ depth, const uint8_t *__restrict__ masks, const int32_t *__restrict__ meta, int n_frames,
                         int H, int W, int n_links, uint64_t *__restrict__ tq, float *__restrict__ t32, float *__restrict__ ts,
                         unsigned long long *__restrict__ counts)
{
    __shared__ uint8_t s_src[TG_IN_H * TG_IN_PITCH];           // bit 0 any, bit 1 look; 0 outside the image
    __shared__ uint8_t s_bits[TG_TH * TG_TW];                  // link bits of the tile itself
    __shared__ uint8_t s_row[TG_IN_H * TG_DIL_PITCH];          // after the dilation's row pass
    __shared__ uint8_t s_dil[TG_DIL_H * TG_DIL_PITCH];         // the dilated image, 3 outside the frame
    __shared__ uint8_t s_ero[TG_DIL_H * TG_TW];                // after the erosion's row pass
    __shared__ unsigned int s_cnt[2 * ROPE_MAX_LINKS];

    const int t = threadIdx.x, frame = blockIdx.z;
    const int x0 = blockIdx.x * TG_TW, y0 = blockIdx.y * TG_TH;
    const size_t plane = (size_t)H * (size_t)W;
    const int k0 = meta[frame], k1 = meta[frame + 1];          // this frame's instance planes
    const int32_t *code = meta + 2 * n_frames + 1;             // per plane: link bit | 0x100 lookup link | 0x200 (any)

    if (t < 2 * ROPE_MAX_LINKS) s_cnt[t] = 0;

    for (int i = t; i < TG_IN_H * TG_IN_W; i += TG_THREADS) {
        const int r = i / TG_IN_W, c = i - r * TG_IN_W;
        const int y = y0 - 7 + r, x = x0 - 7 + c;
        int acc = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const uint8_t *m = masks + (size_t)y * W + x;
            for (int k = k0; k < k1; k++)
                if (m[(size_t)k * plane]) acc |= code[k];
        }
        s_src[r * TG_IN_PITCH + c] = (uint8_t)(((acc >> 9) & 1) | ((acc >> 7) & 2));
        if (r >= 7 && r < 7 + TG_TH && c >= 7 && c < 7 + TG_TW) s_bits[(r - 7) * TG_TW + (c - 7)] = (uint8_t)acc;
    }
    __syncthreads();

    // dilation, rows: the dilated column x0 - 3 + j looks at columns x0 - 7 + j .. x0 + j
    for (int i = t; i < TG_IN_H * TG_DIL_W; i += TG_THREADS) {
        const int r = i / TG_DIL_W, j = i - r * TG_DIL_W;
        const uint8_t *s = s_src + r * TG_IN_PITCH + j;
        s_row[r * TG_DIL_PITCH + j] = (uint8_t)(s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7]);
    }
    __syncthreads();
    // dilation, columns; what lies outside the frame is not computed but "set": the erosion's border never wins
    for (int i = t; i < TG_DIL_H * TG_DIL_W; i += TG_THREADS) {
        const int r = i / TG_DIL_W, j = i - r * TG_DIL_W;
        const int y = y0 - 3 + r, x = x0 - 3 + j;
        uint8_t v = 3;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            v = 0;
            for (int a = 0; a < 8; a++) v |= s_row[(r + a) * TG_DIL_PITCH + j];
        }
        s_dil[r * TG_DIL_PITCH + j] = v;
    }
    __syncthreads();
    // erosion, rows: column x0 + c looks at the dilated columns x0 + c - 3 .. x0 + c + 3
    for (int i = t; i < TG_DIL_H * TG_TW; i += TG_THREADS) {
        const int r = i / TG_TW, c = i - r * TG_TW;
        const uint8_t *s = s_dil + r * TG_DIL_PITCH + c;
        s_ero[i] = (uint8_t)(s[0] & s[1] & s[2] & s[3] & s[4] & s[5] & s[6]);
    }
    __syncthreads();

    // erosion, columns, then the depth, the planes and the counts: a wave per tile row
    unsigned int n_mask[ROPE_MAX_LINKS] = {}, n_depth[ROPE_MAX_LINKS] = {};       // wave-uniform
    const size_t out0 = (size_t)frame * plane;
    for (int i = t; i < TG_TH * TG_TW; i += TG_THREADS) {
        const int r = i / TG_TW, c = i - r * TG_TW;
        const int y = y0 + r, x = x0 + c;
        const bool inside = y < H && x < W;
        uint8_t body = 3;
        for (int a = 0; a < 7; a++) body &= s_ero[(r + a) * TG_TW + c];
        unsigned int bits = 0;
        bool has_depth = false;
        if (inside) {
            const size_t o = out0 + (size_t)y * W + x;
            bits = s_bits[i];
            const double d = (double)depth[o] * ((body & 1) ? 1.0 : 0.0);
            const double dl = d * ((body & 2) ? 1.0 : 0.0);
            has_depth = d != 0.0;
            tq[o] = q32_of_depth_dev(d) | ((uint64_t)bits << 40);
            t32[o] = (float)dl;
            if (ts) ts[o] = (float)d;
        }
        for (int l = 0; l < ROPE_MAX_LINKS; l++) {
            if (l >= n_links) break;
            const bool in_mask = (bits >> l) & 1u;
            n_mask[l] += (unsigned int)__popcll(__ballot(in_mask));
            n_depth[l] += (unsigned int)__popcll(__ballot(in_mask && has_depth));
        }
    }
    if ((t & 63) == 0)
        for (int l = 0; l < n_links; l++) {
            if (n_mask[l]) atomicAdd(&s_cnt[2 * l], n_mask[l]);
            if (n_depth[l]) atomicAdd(&s_cnt[2 * l + 1], n_depth[l]);
        }
    __syncthreads();
    if (t < 2 * n_links && s_cnt[t]) atomicAdd(&counts[(size_t)frame * 2 * ROPE_MAX_LINKS + t], (unsigned long long)s_cnt[t]);
}

// the flags of every frame from its counts: bit 0 for a link that has an instance, however empty its mask, bit 1 by the host's
// expression in double
__global__ void segmented_flags_kernel(const unsigned long long *__restrict__ counts, const int32_t *__restrict__ meta, int n_frames,
                                       int n_links, LinkFlags *__restrict__ flags)
{
    const int frame = blockIdx.x * blockDim.x + threadIdx.x;
    if (frame >= n_frames) return;
    const int present = meta[n_frames + 1 + frame];
    LinkFlags f = {};
    for (int l = 0; l < n_links; l++)
        if ((present >> l) & 1) {
            const unsigned long long n_mask = counts[(size_t)frame * 2 * ROPE_MAX_LINKS + 2 * l];
            const unsigned long long n_depth = counts[(size_t)frame * 2 * ROPE_MAX_LINKS + 2 * l + 1];
            f.f[l] = (uint8_t)(1 | (((double)n_depth > 0.05 * (double)n_mask) ? 2 : 0));
        }
    flags[frame] = f;
}

}  // namespace

hipError_t launch_segmented_targets(hipStream_t st, int H, int W, int n_frames, const void *depth, int depth_kind, const uint8_t *masks,
                                    const int32_t *meta, int n_links, uint64_t *tq, float *t32, float *ts, unsigned long long *counts,
                                    LinkFlags *flags)
{
    if (H < 1 || W < 1 || n_frames < 1 || n_frames > 65535 || n_links < 1 || n_links > ROPE_MAX_LINKS || (depth_kind != 1 && depth_kind != 2))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_frames * 2 * ROPE_MAX_LINKS * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const dim3 grid((W + TG_TW - 1) / TG_TW, (H + TG_TH - 1) / TG_TH, n_frames);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (depth_kind == 1)
        hipLaunchKernelGGL(segmented_targets_kernel<float>, grid, dim3(TG_THREADS), 0, st, static_cast<const float *>(depth), masks, meta, n_frames,
                           H, W, n_links, tq, t32, ts, counts);
    else
        hipLaunchKernelGGL(segmented_targets_kernel<double>, grid, dim3(TG_THREADS), 0, st, static_cast<const double *>(depth), masks, meta, n_frames,
                           H, W, n_links, tq, t32, ts, counts);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(segmented_flags_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, st, counts, meta, n_frames, n_links, flags);
    return hipGetLastError();
}

}  // namespace rope
