// rope_robust.hip — robust weights for the depth term of the bundle polish, for gfx950: rope_bundle_normal_equations_robust sums what
// rope_bundle_normal_equations sums with every inlier's row multiplied by the square root of a Huber or Tukey weight, into the same 96
// words, and rope_residual_histogram counts a frame's residuals in 256 bins up to the truncation, from which the host takes the median
// that scales the weights (prediction/refinement.py, robust_scale_from_histogram).  Everything is float64 with one IEEE operation per
// written operation (-ffp-contract=off); tests/robust_ref.py restates the contract of include/rope_s3d.h in numpy.
//
// This file holds what is particular to the weights: robust_pixel, a pixel's classification, its share of the robust cost and the
// scaled row v' = sqrt(w) (J_0 .. J_11, r).  The surface, the columns, the pack-and-own-words body, the gather, the chunk rule and the
// host checks are rope_neq.h's, so the order of every addition is rope_bundle.hip's.  The histogram adds integers alone.
#include "rope_neq.h"

namespace {

constexpr int RESID_BINS = ROPE_RESID_WORDS - 2;             // 256 bins of |r| <= clip, then: both but beyond, not both
static_assert(RESID_BINS == 256, "the words of a frame's histogram");

// What a call's scale makes of the weights, once on the host: k, k k and the cost share of a pixel beyond the truncation.
struct Robust { double clip, k, kk, beyond; };

// Pixel p of a frame: adds its share of words 0 .. 2 to head and, for an inlier, fills v' = sqrt(w) v and returns true.
template <int KIND>
__device__ __forceinline__ bool robust_pixel(const float *__restrict__ r0, const uint8_t *__restrict__ i0, const float *__restrict__ t0, int p, int H,
                                             int W, int n_links, const Camera &cam, const double *__restrict__ jf, int n_joints,
                                             const double *__restrict__ tf, int n_cols, const Robust &rb, double (&head)[BNEQ_HEAD],
                                             double (&v)[BNEQ_VEC])
{
    const int id = i0[p];
    const float T = t0[p];
    if (id >= n_links || !(T > 0.0f && T < 128.0f)) return false;                       // not BOTH (false for NaN, inf, zero, negatives)
    const double z = (double)r0[p];
    const double r = z - (double)T;
    const double r2 = r * r;
    const double a = fabs(r);
    head[0] += 1.0;
    double w = 1.0;
    bool in;
    if (KIND == ROPE_ROBUST_HUBER) {
        in = a <= rb.clip;                                                              // a NaN is beyond
        if (a <= rb.k) {
            head[1] += r2;
        } else if (in) {
            head[1] += (2.0 * rb.k) * a - rb.kk;
            w = rb.k / a;
        } else {
            head[1] += rb.beyond;
        }
    } else {
        in = a <= rb.k;
        const double u = r2 / rb.kk;
        const double q = 1.0 - u;
        w = q * q;
        head[1] += in ? (rb.kk / 3.0) * (1.0 - (q * q) * q) : rb.beyond;
    }
    if (!in) return false;                                                              // every drawn link counts

    const int y = p / W, x = p - y * W;
    Vec3 P, n;
    double nP;
    if (!depth_surface(r0, i0, p, x, y, H, W, id, z, cam, P, n, nP)) return false;      // no normal, or grazing

    bneq_depth_columns(jf, n_joints, tf, n_cols, id, z, P, n, nP, r, v);
    const double s = sqrt(w);
#pragma unroll
    for (int c = 0; c < BNEQ_VEC; c++) v[c] = s * v[c];
    head[2] += 1.0;
    return true;
}

// Workgroup blockIdx.x = frame * chunks + chunk.
template <int KIND>
__global__ void __launch_bounds__(NEQ_THREADS)
robust_partial_kernel(const float *__restrict__ render, const uint8_t *__restrict__ ids, const float *__restrict__ depth, int H, int W, int chunks,
                      int n_links, Camera cam, const double *__restrict__ joints, int n_joints, const double *__restrict__ twists, int n_cols,
                      Robust rb, double *__restrict__ work)
{
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int hw = H * W;                                                               // at most 2^24
    const float *const r0 = render + (size_t)frame * hw;
    const float *const t0 = depth + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    const double *const jf = joints + (size_t)frame * n_joints * 6;                     // never read when its count is 0
    const double *const tf = twists + (size_t)frame * n_cols * 6;
    bneq_pack_and_own_words(hw, chunk, [&](int p, double (&head)[BNEQ_HEAD], double (&v)[BNEQ_VEC]) {
        return robust_pixel<KIND>(r0, i0, t0, p, H, W, n_links, cam, jf, n_joints, tf, n_cols, rb, head, v);
    }, work + (size_t)blockIdx.x * ROPE_BNEQ_WORDS);
}

// a frame's partials added in index order, two frames a workgroup (rope_neq.h)
__global__ void __launch_bounds__(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS)
robust_gather_kernel(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    neq_gather<ROPE_BNEQ_WORDS>(work, n_frames, chunks, out);
}

// Workgroup blockIdx.x = frame * chunks + chunk counts its chunk in LDS and adds its non-empty bins to the frame's words, which the
// entry point has zeroed: integer adds alone, so the words depend neither on the order of the workgroups nor on the batch.  The
// pixels that are not BOTH — the background, most of a frame — go through a ballot: one add a wave, not 64 on one address.
__global__ void __launch_bounds__(NEQ_THREADS)
resid_histogram_kernel(const float *__restrict__ render, const uint8_t *__restrict__ ids, const float *__restrict__ depth, int hw, int chunks,
                       int n_links, double clip, double inv, uint32_t *__restrict__ hist)
{
    __shared__ unsigned s_hist[ROPE_RESID_WORDS];
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int t = threadIdx.x, lane = t & 63;
    const float *const r0 = render + (size_t)frame * hw;
    const float *const t0 = depth + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    for (int i = t; i < ROPE_RESID_WORDS; i += NEQ_THREADS) s_hist[i] = 0u;
    __syncthreads();
    for (int k = 0; k < NEQ_PER_THREAD; k++) {
        const int p = chunk * NEQ_CHUNK + k * NEQ_THREADS + t;
        bool both = false;
        if (p < hw) {
            const float T = t0[p];
            both = i0[p] < n_links && T > 0.0f && T < 128.0f;
            if (both) {
                const double a = fabs((double)r0[p] - (double)T);
                int b = RESID_BINS;                                                     // beyond the truncation; a NaN too
                if (a <= clip) {
                    b = (int)(a * inv);
                    if (b > RESID_BINS - 1) b = RESID_BINS - 1;
                }
                atomicAdd(&s_hist[b], 1u);
            }
        }
        const unsigned long long m = __ballot(p < hw && !both);
        if (lane == 0 && m) atomicAdd(&s_hist[RESID_BINS + 1], (unsigned)__popcll(m));
    }
    __syncthreads();
    uint32_t *const h = hist + (size_t)frame * ROPE_RESID_WORDS;
    for (int i = t; i < ROPE_RESID_WORDS; i += NEQ_THREADS) {
        const unsigned c = s_hist[i];
        if (c) atomicAdd(&h[i], c);
    }
}

}  // namespace

extern "C" int rope_residual_histogram(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames,
                                       int H, int W, int n_links, float clip_m, uint32_t *hist_dev, void *stream)
{
    static const double aligned = 0.0;                                                  // stands for out and work, which this call has not
    if (neq_bad_args(n_links, 1.0f, 1.0f, 0.0f, 0.0f, render_depth_dev, render_ids_dev, frame_depth_dev, &aligned, &aligned)) return ROPE_E_ARG;
    if (!hist_dev || ((uintptr_t)hist_dev & 3)) return ROPE_E_ARG;
    if (!isfinite(clip_m) || !(clip_m > 0.0f)) return ROPE_E_ARG;
    const long long chunks = neq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist_dev, 0, (size_t)n_frames * ROPE_RESID_WORDS * sizeof(uint32_t), st) != hipSuccess) return ROPE_E_HIP;
    const double clip = (double)clip_m;
    hipLaunchKernelGGL(resid_histogram_kernel, dim3((unsigned)((long long)n_frames * chunks)), dim3(NEQ_THREADS), 0, st, render_depth_dev,
                       render_ids_dev, frame_depth_dev, H * W, (int)chunks, n_links, clip, (double)RESID_BINS / clip, hist_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" size_t rope_bundle_normal_workspace_robust(int n_frames, int H, int W)
{
    return neq_workspace(n_frames, H, W, ROPE_BNEQ_WORDS);
}

extern "C" int rope_bundle_normal_equations_robust(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev,
                                                   int n_frames, int H, int W, int n_links, float fx, float fy, float cx, float cy,
                                                   const double *joints_dev, int n_joints, const double *twists_dev, int n_cols, float clip_m,
                                                   int kind, float scale_m, double *out_dev, double *work_dev, void *stream)
{
    if (neq_bad_args(n_links, fx, fy, cx, cy, render_depth_dev, render_ids_dev, frame_depth_dev, out_dev, work_dev)) return ROPE_E_ARG;
    if (neq_bad_columns12(joints_dev, n_joints, twists_dev, n_cols)) return ROPE_E_ARG;
    if (!isfinite(clip_m) || !(clip_m > 0.0f)) return ROPE_E_ARG;
    if (kind != ROPE_ROBUST_HUBER && kind != ROPE_ROBUST_TUKEY) return ROPE_E_ARG;
    if (!isfinite(scale_m) || !(scale_m > 0.0f && scale_m <= clip_m)) return ROPE_E_ARG;
    const long long chunks = neq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    const Camera cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    const double clip = (double)clip_m, k = (double)scale_m, kk = k * k;
    const Robust rb = {clip, k, kk, kind == ROPE_ROBUST_HUBER ? (2.0 * k) * clip - kk : kk / 3.0};
    const dim3 grid((unsigned)((long long)n_frames * chunks)), block(NEQ_THREADS);
    const double *const joints = n_joints > 0 ? joints_dev : nullptr, *const twists = n_cols > 0 ? twists_dev : nullptr;
    if (kind == ROPE_ROBUST_HUBER)
        hipLaunchKernelGGL(robust_partial_kernel<ROPE_ROBUST_HUBER>, grid, block, 0, st, render_depth_dev, render_ids_dev, frame_depth_dev, H, W,
                           (int)chunks, n_links, cam, joints, n_joints, twists, n_cols, rb, work_dev);
    else
        hipLaunchKernelGGL(robust_partial_kernel<ROPE_ROBUST_TUKEY>, grid, block, 0, st, render_depth_dev, render_ids_dev, frame_depth_dev, H, W,
                           (int)chunks, n_links, cam, joints, n_joints, twists, n_cols, rb, work_dev);
    if (hipGetLastError() != hipSuccess) return ROPE_E_HIP;
    hipLaunchKernelGGL(robust_gather_kernel, dim3(neq_gather_grid(n_frames)), dim3(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS), 0, st, work_dev, n_frames,
                       (int)chunks, out_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
