// rope_synth.hip — the synthetic path's frames kept on the device, for gfx950: depth holes punched into rendered depth planes, and
// the targets of rope_prepare_synthetic built from full-size depth and link-id planes that are in HBM already.
//
// depth holes (launch_depth_holes), the integer contract of DESIGN.md §3a:
//   seed bit   of pixel i = y W + x, frame k, dilation index j: word (j & 3) of Philox4x32-10, key (seed low 32, seed high 32),
//              counter (i, k, j >> 2, 0), compared as word < T[j].  Only integers reach the device: the thresholds T come from the
//              host (rope_hole_thresholds).
//   union      U = OR_j dilate_{d_j}(seed_j): ones(d, d), anchor d / 2, so a seed at s covers s - (d - 1 - d/2) .. s + d/2 per axis
//   close      hole = erode_k(dilate_k(U)), k = connection: the window of x is x - k/2 .. x - k/2 + k - 1 in both; outside the image
//              is clear for the dilation and SET for the erosion of the dilated image (borders never win)
//   depth      0 where hole is set, untouched elsewhere
// One workgroup per (64 x 64 output tile, frame).  Everything a tile's holes depend on lies within a halo of 2 (k - 1) + max d - 1
// pixels, so the tile is self-contained: its threads draw the bits of every pixel of tile + halo (two generator calls for eight
// dilations), the few seeds scatter their d x d block into a byte plane in LDS (same-value stores: the union does not depend on
// their order), and the close runs as four separable passes through LDS.  No global scratch, no atomics, no second launch.
//
// synthetic targets (launch_synthetic_targets): per output pixel the four taps of the even-factor down-sampling (f == 1: the pixel
// itself) of the colour plane blue_of_id[ids] (OpenCV's fixed-point rounding) and of the depth (float32, one IEEE operation per
// written step: -ffp-contract=off), then what rope_prepare_synthetic writes: the link bits of blue == link_blue[l], the lookup
// depth, the Q32 packing, the TensorSweep plane, and per link the counts the flags are made of.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rope_kernels.h"

namespace rope {
namespace {

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
struct Philox4 { uint32_t w[4]; };

__device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

constexpr int HT = 64;                                           // output tile, both axes
constexpr int HOLE_THREADS = 256;
constexpr int HK = ROPE_HOLE_MAX_WINDOW;                         // largest window of the close and of a dilation
constexpr int HU = HT + 2 * (HK - 1), HU_PITCH = HU + 2;         // the union plane: tile + 2 (k - 1)
constexpr int HD = HT + HK - 1, HD_PITCH = HD + 1;               // the dilated image: tile + k - 1

struct HoleParams {
    uint32_t T[ROPE_HOLE_MAX_DILATIONS];
    int32_t d[ROPE_HOLE_MAX_DILATIONS];
    int n_d, k;
    int reach_before, reach_after;                               // a pixel of U is reached by seeds x - reach_before .. x + reach_after
    uint32_t key0, key1, frame0;
};

__global__ void __launch_bounds__(HOLE_THREADS)
depth_holes_kernel(float *__restrict__ depth, int H, int W, HoleParams p)
{
    __shared__ uint8_t s_u[HU * HU_PITCH];                       // U; 0 outside the image
    __shared__ uint8_t s_row[HU * HD_PITCH];                     // after the dilation's row pass
    __shared__ uint8_t s_dil[HD * HD_PITCH];                     // the dilated image, 1 outside the image
    __shared__ uint8_t s_ero[HD * HT];                           // after the erosion's row pass

    const int t = threadIdx.x, frame = blockIdx.z;
    const int x0 = blockIdx.x * HT, y0 = blockIdx.y * HT;
    const int k = p.k, a = k / 2;
    const int nu = HT + 2 * (k - 1), nd = HT + k - 1;            // sides of U and of the dilated image in use
    const int ux0 = x0 - 2 * a, uy0 = y0 - 2 * a;                // image position of U's first column / row

    for (int i = t; i < nu * HU_PITCH; i += HOLE_THREADS) s_u[i] = 0;
    __syncthreads();

    // the seeds: every image pixel that can reach U draws its bits; a set bit scatters its block, clipped to U and to the image
    const int sx0 = max(ux0 - p.reach_before, 0), sx1 = min(ux0 + nu - 1 + p.reach_after, W - 1);
    const int sy0 = max(uy0 - p.reach_before, 0), sy1 = min(uy0 + nu - 1 + p.reach_after, H - 1);
    const int sw = sx1 - sx0 + 1, sh = sy1 - sy0 + 1;
    const int cx0 = max(ux0, 0), cx1 = min(ux0 + nu - 1, W - 1), cy0 = max(uy0, 0), cy1 = min(uy0 + nu - 1, H - 1);
    const int n_calls = (p.n_d + 3) >> 2;
    for (int i = t; i < sw * sh; i += HOLE_THREADS) {
        const int r = i / sw, sy = sy0 + r, sx = sx0 + (i - r * sw);
        const uint32_t pixel = (uint32_t)sy * (uint32_t)W + (uint32_t)sx;
        for (int call = 0; call < n_calls; call++) {
            const Philox4 g = philox4x32_10(pixel, p.frame0 + (uint32_t)frame, (uint32_t)call, 0u, p.key0, p.key1);
            for (int wd = 0; wd < 4; wd++) {
                const int j = 4 * call + wd;
                if (j >= p.n_d || !(g.w[wd] < p.T[j])) continue;
                const int d = p.d[j], ad = d / 2;
                const int bx0 = max(sx - (d - 1 - ad), cx0), bx1 = min(sx + ad, cx1);
                const int by0 = max(sy - (d - 1 - ad), cy0), by1 = min(sy + ad, cy1);
                for (int y = by0; y <= by1; y++)
                    for (int x = bx0; x <= bx1; x++) s_u[(y - uy0) * HU_PITCH + (x - ux0)] = 1;
            }
        }
    }
    __syncthreads();

    // dilation, rows: the dilated column x0 - a + j looks at U's columns j .. j + k - 1
    for (int i = t; i < nu * nd; i += HOLE_THREADS) {
        const int r = i / nd, j = i - r * nd;
        const uint8_t *s = s_u + r * HU_PITCH + j;
        uint8_t v = 0;
        for (int b = 0; b < k; b++) v |= s[b];
        s_row[r * HD_PITCH + j] = v;
    }
    __syncthreads();
    // dilation, columns; what lies outside the image is not computed but "set": the erosion's border never wins
    for (int i = t; i < nd * nd; i += HOLE_THREADS) {
        const int r = i / nd, j = i - r * nd;
        const int y = y0 - a + r, x = x0 - a + j;
        uint8_t v = 1;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            v = 0;
            for (int b = 0; b < k; b++) v |= s_row[(r + b) * HD_PITCH + j];
        }
        s_dil[r * HD_PITCH + j] = v;
    }
    __syncthreads();
    // erosion, rows: column x0 + c looks at the dilated columns c .. c + k - 1
    for (int i = t; i < nd * HT; i += HOLE_THREADS) {
        const int r = i / HT, c = i - r * HT;
        const uint8_t *s = s_dil + r * HD_PITCH + c;
        uint8_t v = 1;
        for (int b = 0; b < k; b++) v &= s[b];
        s_ero[i] = v;
    }
    __syncthreads();
    // erosion, columns, and the depth
    float *plane = depth + (size_t)frame * (size_t)H * (size_t)W;
    for (int i = t; i < HT * HT; i += HOLE_THREADS) {
        const int r = i / HT, c = i - r * HT;
        const int y = y0 + r, x = x0 + c;
        if (y >= H || x >= W) continue;
        uint8_t v = 1;
        for (int b = 0; b < k; b++) v &= s_ero[(r + b) * HT + c];
        if (v) plane[(size_t)y * W + x] = 0.0f;
    }
}

// ---- synthetic targets
struct SynthTables {
    uint8_t blue_of_id[256];
    int32_t link_blue[ROPE_MAX_LINKS];
};

constexpr int ST_THREADS = 256;

__device__ inline uint64_t q32_of_depth_dev(double d)              // as rope_targets.hip: rope_pack_target's rounding and clipping
{
    const double Q32 = 4294967296.0, top = 549755813887.0;
    double q = (d > 0.0 && d <= 1.7976931348623157e308) ? rint(d * Q32) : 0.0;
    q = q < top ? q : top;
    return (uint64_t)q;
}

__global__ void __launch_bounds__(ST_THREADS)
synthetic_targets_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ ids, int H0, int W0, int f, SynthTables tb, int n_links,
                         int n_lookup_links, uint64_t *__restrict__ tq, float *__restrict__ t32, float *__restrict__ ts,
                         unsigned long long *__restrict__ counts)
{
    __shared__ unsigned int s_cnt[2 * ROPE_MAX_LINKS];
    const int t = threadIdx.x, frame = blockIdx.y;
    const int H = H0 / f, W = W0 / f;
    const size_t plane = (size_t)H * (size_t)W, plane0 = (size_t)H0 * (size_t)W0;
    const size_t o = (size_t)blockIdx.x * ST_THREADS + t;
    if (t < 2 * ROPE_MAX_LINKS) s_cnt[t] = 0;
    __syncthreads();

    unsigned int bits = 0;
    bool has_depth = false;
    if (o < plane) {
        const int y = (int)(o / (size_t)W), x = (int)(o - (size_t)y * W);
        const float *dp = depth + (size_t)frame * plane0;
        const uint8_t *ip = ids + (size_t)frame * plane0;
        int blue;
        double d;
        if (f > 1) {
            const int a = f / 2 - 1, b = f / 2;
            const size_t r0 = (size_t)(y * f + a) * W0, r1 = (size_t)(y * f + b) * W0, xa = (size_t)(x * f + a), xb = (size_t)(x * f + b);
            // OpenCV's fixed-point path for uint8, the steps of rope_downsample_even (kind 0)
            const int64_t c00 = tb.blue_of_id[ip[r0 + xa]], c01 = tb.blue_of_id[ip[r0 + xb]], c10 = tb.blue_of_id[ip[r1 + xa]], c11 = tb.blue_of_id[ip[r1 + xb]];
            const int64_t tt = (c00 * 1024 + c01 * 1024) >> 4, u = (c10 * 1024 + c11 * 1024) >> 4;
            const int64_t v = (((1024 * tt) >> 16) + ((1024 * u) >> 16) + 2) >> 2;
            blue = (int)(v < 0 ? 0 : (v > 255 ? 255 : v));
            const float tp = dp[r0 + xa] * 0.5f + dp[r0 + xb] * 0.5f, bt = dp[r1 + xa] * 0.5f + dp[r1 + xb] * 0.5f;
            d = (double)(tp * 0.5f + bt * 0.5f);
        } else {
            blue = tb.blue_of_id[ip[o]];
            d = (double)dp[o];
        }
        bool hit = false;
        for (int l = 0; l < ROPE_MAX_LINKS; l++)
            if (l < n_links && tb.link_blue[l] == blue) {
                bits |= 1u << l;
                hit = hit || l < n_lookup_links;
            }
        has_depth = d != 0.0;                                    // true for NaN, as `depth != 0`
        const size_t out = (size_t)frame * plane + o;
        tq[out] = q32_of_depth_dev(d) | ((uint64_t)bits << 40);
        t32[out] = (float)(d * (hit ? 1.0 : 0.0));
        if (ts) ts[out] = (float)d;
    }
    // integer counts per link, so the order of the additions does not matter: ballots per wave, LDS per workgroup, one global add
    for (int l = 0; l < ROPE_MAX_LINKS; l++) {
        if (l >= n_links) break;
        const bool in_mask = (bits >> l) & 1u;
        const unsigned int n_mask = (unsigned int)__popcll(__ballot(in_mask));
        const unsigned int n_depth = (unsigned int)__popcll(__ballot(in_mask && has_depth));
        if ((t & 63) == 0) {
            if (n_mask) atomicAdd(&s_cnt[2 * l], n_mask);
            if (n_depth) atomicAdd(&s_cnt[2 * l + 1], n_depth);
        }
    }
    __syncthreads();
    if (t < 2 * n_links && s_cnt[t]) atomicAdd(&counts[(size_t)frame * 2 * ROPE_MAX_LINKS + t], (unsigned long long)s_cnt[t]);
}

// the flags of every frame from its counts: bit 0 for a link whose mask has a pixel, bit 1 by the host's expression in double
__global__ void synthetic_flags_kernel(const unsigned long long *__restrict__ counts, int n_frames, int n_links, LinkFlags *__restrict__ flags)
{
    const int frame = blockIdx.x * blockDim.x + threadIdx.x;
    if (frame >= n_frames) return;
    LinkFlags fl = {};
    for (int l = 0; l < n_links; l++) {
        const unsigned long long n_mask = counts[(size_t)frame * 2 * ROPE_MAX_LINKS + 2 * l];
        const unsigned long long n_depth = counts[(size_t)frame * 2 * ROPE_MAX_LINKS + 2 * l + 1];
        if (n_mask > 0) fl.f[l] = (uint8_t)(1 | (((double)n_depth > 0.05 * (double)n_mask) ? 2 : 0));
    }
    flags[frame] = fl;
}

}  // namespace

hipError_t launch_depth_holes(hipStream_t st, float *depth, int N, int H, int W, uint32_t frame0, uint64_t seed, const uint32_t *T,
                              const int32_t *d, int n_d, int connection)
{
    if (!depth || N < 1 || N > 65535 || H < 1 || W < 1 || (uint64_t)H * (uint64_t)W > 0xFFFFFFFFull || n_d < 0 || n_d > ROPE_HOLE_MAX_DILATIONS ||
        connection < 1 || connection > ROPE_HOLE_MAX_WINDOW || (n_d > 0 && (!T || !d)))
        return hipErrorInvalidValue;
    HoleParams p = {};
    p.n_d = n_d;
    p.k = connection;
    for (int j = 0; j < n_d; j++) {
        if (d[j] < 1 || d[j] > ROPE_HOLE_MAX_WINDOW) return hipErrorInvalidValue;
        p.T[j] = T[j];
        p.d[j] = d[j];
        // a seed at s covers s - (d - 1 - d/2) .. s + d/2, so the pixel x is reached from x - d/2 .. x + (d - 1 - d/2)
        p.reach_before = std::max(p.reach_before, d[j] / 2);
        p.reach_after = std::max(p.reach_after, d[j] - 1 - d[j] / 2);
    }
    p.key0 = (uint32_t)seed;
    p.key1 = (uint32_t)(seed >> 32);
    p.frame0 = frame0;
    const dim3 grid((W + HT - 1) / HT, (H + HT - 1) / HT, N);
    if (grid.y > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(depth_holes_kernel, grid, dim3(HOLE_THREADS), 0, st, depth, H, W, p);
    return hipGetLastError();
}

hipError_t launch_synthetic_targets(hipStream_t st, int H0, int W0, int f, int n_frames, const float *depth, const uint8_t *ids,
                                    const uint8_t *blue_of_id, const int32_t *link_blue, int n_links, int n_lookup_links, uint64_t *tq,
                                    float *t32, float *ts, unsigned long long *counts, LinkFlags *flags)
{
    if (H0 < 1 || W0 < 1 || f < 1 || (f > 1 && (f & 1)) || H0 % f || W0 % f || n_frames < 1 || n_frames > 65535 || n_links < 1 ||
        n_links > ROPE_MAX_LINKS || n_lookup_links < 0 || n_lookup_links > n_links)
        return hipErrorInvalidValue;
    SynthTables tb;
    for (int i = 0; i < 256; i++) tb.blue_of_id[i] = blue_of_id[i];
    for (int l = 0; l < ROPE_MAX_LINKS; l++) tb.link_blue[l] = l < n_links ? link_blue[l] : -1;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_frames * 2 * ROPE_MAX_LINKS * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const size_t plane = (size_t)(H0 / f) * (size_t)(W0 / f);
    const size_t blocks = (plane + ST_THREADS - 1) / ST_THREADS;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(synthetic_targets_kernel, dim3((unsigned)blocks, n_frames), dim3(ST_THREADS), 0, st, depth, ids, H0, W0, f, tb, n_links,
                       n_lookup_links, tq, t32, ts, counts);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(synthetic_flags_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, st, counts, n_frames, n_links, flags);
    return hipGetLastError();
}

}  // namespace rope
