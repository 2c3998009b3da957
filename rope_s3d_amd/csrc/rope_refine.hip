// rope_refine.hip — the normal equations of a pose against a depth frame, for gfx950: rope_pose_normal_equations takes the render at
// a pose (depth R, link ids), the frame's depth T and the joint axes of that pose in camera axes, and sums over the pixels of every
// frame J^T J, J^T r and the residual sums of include/rope_s3d.h, J being the derivative of the rendered depth with respect to each
// joint angle.  Solving the system is a Gauss-Newton step of the pose, inverting it its formal covariance; both are host arithmetic
// (prediction/refinement.py).  Everything is float64 with one IEEE operation per written operation (-ffp-contract=off);
// tests/refine_ref.py restates the contract in numpy.
//
// rope_camera_normal_equations is the same reduction with other columns: every frame brings up to six twists (w, v) of the camera
// pose's parameters instead of joint axes, every drawn link moves with every column (the base, link 0, too), and a surface point P
// has the velocity w x P + v per unit of a column.  The two entry points share one kernel body, neq_partial_body<CAMERA>; what
// differs is the MOVING rule and the column of J, nothing in the shape or in the order of the sums.  tests/camera_refine_ref.py
// restates that contract.  The depth surface of a pixel, the columns' velocities, the chunk rule, the gather and the host checks are
// rope_bundle.hip's and rope_silhouette.hip's as well and live in rope_neq.h; this file keeps the 31 register accumulators.
//
// Shape.  A workgroup takes NEQ_CHUNK consecutive pixels of one frame — pixel p = chunk NEQ_CHUNK + k NEQ_THREADS + t for thread t,
// k = 0 .. 7, so a wave's loads are consecutive — and a thread reads its pixel's R, id and T and the R and id of its four
// neighbours straight from memory (9 bytes a pixel from HBM, the neighbours from cache: they are other lanes' pixels or the rows
// above and below).  The six axes (or twists) of the frame are uniform per workgroup and stay in scalar registers.
//
// Determinism.  No floating-point atomics.  The pixels of a workgroup depend on H W alone, never on the batch or on an address.  A
// thread adds its pixels in the order k = 0 .. 7; the 64 threads of a wave are added in a butterfly (xor 32, 16, .. 1: IEEE addition
// commutes, so every lane holds the same bits afterwards); the four waves are added in the order 0 .. 3 out of LDS; the workgroup
// writes ONE partial of ROPE_NEQ_WORDS doubles to the workspace; neq_gather_kernel then adds the partials of a frame in index
// order.  The same planes give the same bytes from run to run, and in one call or in several.
// Lane exchange: every accumulator is defined (zero) in all 256 threads before the loop, no thread leaves early, and pixels beyond
// the frame add nothing instead of branching around the butterfly: no lane reads what an inactive lane made.
#include "rope_neq.h"

namespace {

constexpr int NEQ_USED = 4 + NEQ_JOINTS + NEQ_JOINTS * (NEQ_JOINTS + 1) / 2;       // 31 of the 32 words

static_assert(NEQ_USED <= ROPE_NEQ_WORDS && ROPE_NEQ_WORDS == 32, "the words of a frame");

// Workgroup blockIdx.x = frame * chunks + chunk.  CAMERA = false: `joints` holds (axis, point) per joint and link l moves with the
// joints j < l; CAMERA = true: `joints` holds (w, v) per column and every drawn link moves with every column.
// Three waves a SIMD is what the joint columns get on their own (157 VGPRs); asked for, it keeps the twist columns there too (155
// VGPRs; left to itself the allocator takes 170 and drops to two).
template <bool CAMERA>
__global__ void __launch_bounds__(NEQ_THREADS) __attribute__((amdgpu_waves_per_eu(3)))
neq_partial_kernel(const float *__restrict__ render, const uint8_t *__restrict__ ids, const float *__restrict__ depth, int H, int W, int chunks,
                   int n_links, Camera cam, const double *__restrict__ joints, int n_joints, double clip, double *__restrict__ work)
{
    __shared__ double s_part[NEQ_WAVES][NEQ_USED];
    const int t = threadIdx.x;
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int hw = H * W;                                                               // at most 2^24
    const float *const r0 = render + (size_t)frame * hw;
    const float *const t0 = depth + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    const double *const jf = joints + (size_t)frame * n_joints * 6;
    const double clip2 = clip * clip;

    double acc[NEQ_USED];
#pragma unroll
    for (int j = 0; j < NEQ_USED; j++) acc[j] = 0.0;

    for (int k = 0; k < NEQ_PER_THREAD; k++) {
        const int p = chunk * NEQ_CHUNK + k * NEQ_THREADS + t;
        if (p >= hw) continue;                                                          // adds nothing; the accumulators stay defined
        const int id = i0[p];
        const float T = t0[p];
        if (id >= n_links || !(T > 0.0f && T < 128.0f)) continue;                       // not BOTH (false for NaN, inf, zero, negatives)
        const double z = (double)r0[p];
        const double r = z - (double)T;
        const double r2 = r * r;
        acc[0] += 1.0;
        acc[1] += r2 <= clip2 ? r2 : clip2;                                             // a NaN counts as clip^2
        if (CAMERA) {
            if (!(fabs(r) <= clip)) continue;                                           // beyond the truncation; every drawn link is MOVING
        } else {
            if (id < 1 || id > n_joints || !(fabs(r) <= clip)) continue;                // not MOVING, or beyond the truncation
        }

        const int y = p / W, x = p - y * W;
        Vec3 P, n;
        double nP;
        if (!depth_surface(r0, i0, p, x, y, H, W, id, z, cam, P, n, nP)) continue;      // no normal, or grazing

        double J[NEQ_JOINTS];
#pragma unroll
        for (int j = 0; j < NEQ_JOINTS; j++) {
            J[j] = 0.0;
            if (CAMERA) {
                if (j < n_joints) J[j] = depth_column(z, n, nP, twist_velocity(jf, j, P));      // every column moves every drawn link
            } else if (j < n_joints && j < id) {                                        // joint j moves the links behind it
                J[j] = depth_column(z, n, nP, joint_velocity(jf, j, P));
            }
        }
        acc[2] += 1.0;
        acc[3] += r2;
        int w = 4 + NEQ_JOINTS;
#pragma unroll
        for (int j = 0; j < NEQ_JOINTS; j++) {
            acc[4 + j] += J[j] * r;
#pragma unroll
            for (int i = j; i < NEQ_JOINTS; i++) acc[w++] += J[j] * J[i];
        }
    }

    // every thread of the workgroup is here with all its accumulators defined
#pragma unroll
    for (int j = 0; j < NEQ_USED; j++) {
        double s = acc[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if ((t & 63) == 0) s_part[t >> 6][j] = s;
    }
    __syncthreads();
    if (t < ROPE_NEQ_WORDS) {
        double s = 0.0;
        if (t < NEQ_USED) {
            s = s_part[0][t];
#pragma unroll
            for (int w = 1; w < NEQ_WAVES; w++) s += s_part[w][t];
        }
        work[(size_t)blockIdx.x * ROPE_NEQ_WORDS + t] = s;
    }
}

// a frame's partials added in index order, two frames a workgroup (rope_neq.h)
__global__ void __launch_bounds__(NEQ_GATHER_FRAMES * ROPE_NEQ_WORDS)
neq_gather_kernel(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    neq_gather<ROPE_NEQ_WORDS>(work, n_frames, chunks, out);
}

// the checks and the two launches both entry points share; `columns_dev, n_columns`: joints or twists
template <bool CAMERA>
int neq_launch(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames, int H, int W, int n_links,
               float fx, float fy, float cx, float cy, const double *columns_dev, int n_columns, float clip_m, double *out_dev, double *work_dev,
               void *stream)
{
    if (neq_bad_args(n_links, fx, fy, cx, cy, render_depth_dev, render_ids_dev, frame_depth_dev, out_dev, work_dev)) return ROPE_E_ARG;
    if (n_columns < 1 || n_columns > NEQ_JOINTS || !columns_dev || ((uintptr_t)columns_dev & 7)) return ROPE_E_ARG;
    if (!isfinite(clip_m) || !(clip_m > 0.0f)) return ROPE_E_ARG;
    const long long chunks = neq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    const Camera cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    hipLaunchKernelGGL(neq_partial_kernel<CAMERA>, dim3((unsigned)((long long)n_frames * chunks)), dim3(NEQ_THREADS),
                       0, st, render_depth_dev, render_ids_dev, frame_depth_dev, H, W, (int)chunks, n_links, cam, columns_dev, n_columns,
                       (double)clip_m, work_dev);
    if (hipGetLastError() != hipSuccess) return ROPE_E_HIP;
    hipLaunchKernelGGL(neq_gather_kernel, dim3(neq_gather_grid(n_frames)), dim3(NEQ_GATHER_FRAMES * ROPE_NEQ_WORDS), 0, st, work_dev, n_frames,
                       (int)chunks, out_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

}  // namespace

extern "C" size_t rope_pose_normal_workspace(int n_frames, int H, int W)
{
    return neq_workspace(n_frames, H, W, ROPE_NEQ_WORDS);
}

extern "C" int rope_pose_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames,
                                          int H, int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev, int n_joints,
                                          float clip_m, double *out_dev, double *work_dev, void *stream)
{
    return neq_launch<false>(render_depth_dev, render_ids_dev, frame_depth_dev, n_frames, H, W, n_links, fx, fy, cx, cy, joints_dev, n_joints, clip_m,
                             out_dev, work_dev, stream);
}

extern "C" int rope_camera_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames,
                                            int H, int W, int n_links, float fx, float fy, float cx, float cy, const double *twists_dev, int n_cols,
                                            float clip_m, double *out_dev, double *work_dev, void *stream)
{
    return neq_launch<true>(render_depth_dev, render_ids_dev, frame_depth_dev, n_frames, H, W, n_links, fx, fy, cx, cy, twists_dev, n_cols, clip_m,
                            out_dev, work_dev, stream);
}
