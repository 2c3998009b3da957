// rope_bundle.hip — the normal equations of joint angles AND camera pose in one system, for gfx950: rope_bundle_normal_equations takes
// what rope_pose_normal_equations and rope_camera_normal_equations take together (the render at a pose, the frame's depth, the joint
// axes and the camera's twists, both in camera axes) and sums per frame J^T J, J^T r and the residual sums of include/rope_s3d.h over
// twelve column slots: 0 .. 5 the joints, 6 .. 11 the camera's parameters.  The cross block (joint x camera) is what neither of the
// two 6-column calls can give.  Everything is float64 with one IEEE operation per written operation (-ffp-contract=off);
// tests/bundle_ref.py restates the contract in numpy.
//
// This file holds what is particular to the depth term over twelve slots: bneq_pixel, the classification of a pixel and its thirteen
// entries v = (J_0 .. J_11, r).  The depth surface and the columns are rope_refine.hip's, and the shape of the kernel — the inliers of
// a pass packed into LDS in pixel order, then the threads owning words — is rope_silhouette.hip's as well: both live in rope_neq.h
// (bneq_pack_and_own_words says how and in which order everything is added), with the gather, the chunk rule and the host checks.
#include "rope_neq.h"

namespace {

// Pixel p of a frame: adds its share of words 0 .. 2 to head and, for an inlier (rule 4'), fills v and returns true.
__device__ __forceinline__ bool bneq_pixel(const float *__restrict__ r0, const uint8_t *__restrict__ i0, const float *__restrict__ t0, int p, int H,
                                           int W, int n_links, const Camera &cam, const double *__restrict__ jf, int n_joints,
                                           const double *__restrict__ tf, int n_cols, double clip, double clip2, double (&head)[BNEQ_HEAD],
                                           double (&v)[BNEQ_VEC])
{
    const int id = i0[p];
    const float T = t0[p];
    if (id >= n_links || !(T > 0.0f && T < 128.0f)) return false;                       // not BOTH (false for NaN, inf, zero, negatives)
    const double z = (double)r0[p];
    const double r = z - (double)T;
    const double r2 = r * r;
    head[0] += 1.0;
    head[1] += r2 <= clip2 ? r2 : clip2;                                                // a NaN counts as clip^2
    if (!(fabs(r) <= clip)) return false;                                               // beyond the truncation; every drawn link counts

    const int y = p / W, x = p - y * W;
    Vec3 P, n;
    double nP;
    if (!depth_surface(r0, i0, p, x, y, H, W, id, z, cam, P, n, nP)) return false;      // no normal, or grazing

    bneq_depth_columns(jf, n_joints, tf, n_cols, id, z, P, n, nP, r, v);                // rope_neq.h: rope_robust.hip fills the same entries
    head[2] += 1.0;
    return true;
}

// Workgroup blockIdx.x = frame * chunks + chunk.
__global__ void __launch_bounds__(NEQ_THREADS)
bneq_partial_kernel(const float *__restrict__ render, const uint8_t *__restrict__ ids, const float *__restrict__ depth, int H, int W, int chunks,
                    int n_links, Camera cam, const double *__restrict__ joints, int n_joints, const double *__restrict__ twists, int n_cols,
                    double clip, double *__restrict__ work)
{
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int hw = H * W;                                                               // at most 2^24
    const float *const r0 = render + (size_t)frame * hw;
    const float *const t0 = depth + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    const double *const jf = joints + (size_t)frame * n_joints * 6;                     // never read when its count is 0
    const double *const tf = twists + (size_t)frame * n_cols * 6;
    const double clip2 = clip * clip;
    bneq_pack_and_own_words(hw, chunk, [&](int p, double (&head)[BNEQ_HEAD], double (&v)[BNEQ_VEC]) {
        return bneq_pixel(r0, i0, t0, p, H, W, n_links, cam, jf, n_joints, tf, n_cols, clip, clip2, head, v);
    }, work + (size_t)blockIdx.x * ROPE_BNEQ_WORDS);
}

// a frame's partials added in index order, two frames a workgroup (rope_neq.h)
__global__ void __launch_bounds__(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS)
bneq_gather_kernel(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    neq_gather<ROPE_BNEQ_WORDS>(work, n_frames, chunks, out);
}

}  // namespace

extern "C" size_t rope_bundle_normal_workspace(int n_frames, int H, int W)
{
    return neq_workspace(n_frames, H, W, ROPE_BNEQ_WORDS);
}

extern "C" int rope_bundle_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames,
                                            int H, int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev, int n_joints,
                                            const double *twists_dev, int n_cols, float clip_m, double *out_dev, double *work_dev, void *stream)
{
    if (neq_bad_args(n_links, fx, fy, cx, cy, render_depth_dev, render_ids_dev, frame_depth_dev, out_dev, work_dev)) return ROPE_E_ARG;
    if (neq_bad_columns12(joints_dev, n_joints, twists_dev, n_cols)) return ROPE_E_ARG;
    if (!isfinite(clip_m) || !(clip_m > 0.0f)) return ROPE_E_ARG;
    const long long chunks = neq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    const Camera cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    hipLaunchKernelGGL(bneq_partial_kernel, dim3((unsigned)((long long)n_frames * chunks)), dim3(NEQ_THREADS), 0, st, render_depth_dev,
                       render_ids_dev, frame_depth_dev, H, W, (int)chunks, n_links, cam, n_joints > 0 ? joints_dev : nullptr, n_joints,
                       n_cols > 0 ? twists_dev : nullptr, n_cols, (double)clip_m, work_dev);
    if (hipGetLastError() != hipSuccess) return ROPE_E_HIP;
    hipLaunchKernelGGL(bneq_gather_kernel, dim3(neq_gather_grid(n_frames)), dim3(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS), 0, st, work_dev, n_frames,
                       (int)chunks, out_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
