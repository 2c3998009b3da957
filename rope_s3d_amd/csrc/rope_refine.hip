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
// restates that contract.
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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

constexpr int NEQ_THREADS = 256;
constexpr int NEQ_WAVES = NEQ_THREADS / 64;
constexpr int NEQ_PER_THREAD = 8;
constexpr int NEQ_CHUNK = NEQ_THREADS * NEQ_PER_THREAD;      // pixels of a workgroup
constexpr int NEQ_JOINTS = 6;
constexpr int NEQ_USED = 4 + NEQ_JOINTS + NEQ_JOINTS * (NEQ_JOINTS + 1) / 2;       // 31 of the 32 words
constexpr int NEQ_GATHER_THREADS = 64;                       // two frames a workgroup

static_assert(NEQ_USED <= ROPE_NEQ_WORDS && ROPE_NEQ_WORDS == 32, "the words of a frame");

struct Camera { double fx, fy, cx, cy; };

struct Vec3 { double x, y, z; };

__device__ __forceinline__ Vec3 sub(const Vec3 &a, const Vec3 &b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 cross(const Vec3 &a, const Vec3 &b)
{
    return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot(const Vec3 &a, const Vec3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

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
        const double kx = ((double)x - cam.cx) / cam.fx, ky = ((double)y - cam.cy) / cam.fy;
        const Vec3 P = {kx * z, ky * z, z};
        Vec3 dX = {0.0, 0.0, 0.0}, dY = {0.0, 0.0, 0.0};
        if (x + 1 < W && i0[p + 1] == id) {
            const double zn = (double)r0[p + 1], kn = ((double)(x + 1) - cam.cx) / cam.fx;
            dX = sub(Vec3{kn * zn, ky * zn, zn}, P);
        } else if (x > 0 && i0[p - 1] == id) {
            const double zn = (double)r0[p - 1], kn = ((double)(x - 1) - cam.cx) / cam.fx;
            dX = sub(P, Vec3{kn * zn, ky * zn, zn});
        }
        if (y + 1 < H && i0[p + W] == id) {
            const double zn = (double)r0[p + W], kn = ((double)(y + 1) - cam.cy) / cam.fy;
            dY = sub(Vec3{kx * zn, kn * zn, zn}, P);
        } else if (y > 0 && i0[p - W] == id) {
            const double zn = (double)r0[p - W], kn = ((double)(y - 1) - cam.cy) / cam.fy;
            dY = sub(P, Vec3{kx * zn, kn * zn, zn});
        }
        const Vec3 n = cross(dX, dY);
        if (!(isfinite(n.x) && isfinite(n.y) && isfinite(n.z)) || (n.x == 0.0 && n.y == 0.0 && n.z == 0.0)) continue;      // no normal
        const double nn = dot(n, n), nP = dot(n, P), PP = dot(P, P);
        if (!(nP * nP >= 0.01 * (nn * PP)) || nP == 0.0) continue;                      // grazing

        double J[NEQ_JOINTS];
#pragma unroll
        for (int j = 0; j < NEQ_JOINTS; j++) {
            J[j] = 0.0;
            if (CAMERA) {
                if (j < n_joints) {                                                     // every column moves every drawn link
                    const Vec3 w = {jf[6 * j], jf[6 * j + 1], jf[6 * j + 2]}, v = {jf[6 * j + 3], jf[6 * j + 4], jf[6 * j + 5]};
                    const Vec3 c = cross(w, P);
                    J[j] = (z * dot(n, Vec3{c.x + v.x, c.y + v.y, c.z + v.z})) / nP;  // the point moves by w x P + v
                }
            } else if (j < n_joints && j < id) {                                        // joint j moves the links behind it
                const Vec3 a = {jf[6 * j], jf[6 * j + 1], jf[6 * j + 2]}, o = {jf[6 * j + 3], jf[6 * j + 4], jf[6 * j + 5]};
                J[j] = (z * dot(n, cross(a, sub(P, o)))) / nP;
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

// Thread t of workgroup b: word t & 31 of frame 2 b + (t >> 5), the partials of the frame added in index order.
__global__ void __launch_bounds__(NEQ_GATHER_THREADS)
neq_gather_kernel(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    const int frame = blockIdx.x * (NEQ_GATHER_THREADS / ROPE_NEQ_WORDS) + (int)(threadIdx.x / ROPE_NEQ_WORDS);
    const int word = threadIdx.x % ROPE_NEQ_WORDS;
    if (frame >= n_frames) return;
    const double *const w = work + (size_t)frame * chunks * ROPE_NEQ_WORDS + word;
    double s = w[0];
    for (int c = 1; c < chunks; c++) s += w[(size_t)c * ROPE_NEQ_WORDS];
    out[(size_t)frame * ROPE_NEQ_WORDS + word] = s;
}

// chunks of a frame, or 0 when the shape is refused
long long neq_chunks(int n_frames, int H, int W)
{
    if (n_frames < 1 || H < 1 || W < 1) return 0;
    const long long hw = (long long)H * (long long)W;
    if (hw > (1ll << 24)) return 0;
    const long long chunks = (hw + NEQ_CHUNK - 1) / NEQ_CHUNK;
    if ((long long)n_frames * chunks >= (1ll << 24)) return 0;                          // a grid holds fewer than 2^32 threads: 2^24 workgroups of 256
    return chunks;
}

// the checks and the two launches both entry points share; `columns_dev, n_columns`: joints or twists
template <bool CAMERA>
int neq_launch(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames, int H, int W, int n_links,
               float fx, float fy, float cx, float cy, const double *columns_dev, int n_columns, float clip_m, double *out_dev, double *work_dev,
               void *stream)
{
    if (n_links < 1 || n_links > ROPE_MAX_LINKS || n_columns < 1 || n_columns > NEQ_JOINTS) return ROPE_E_ARG;
    if (!isfinite(clip_m) || !(clip_m > 0.0f)) return ROPE_E_ARG;
    if (!isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy) || fx == 0.0f || fy == 0.0f) return ROPE_E_ARG;
    if (!render_depth_dev || !render_ids_dev || !frame_depth_dev || !columns_dev || !out_dev || !work_dev) return ROPE_E_ARG;
    if (((uintptr_t)render_depth_dev & 3) || ((uintptr_t)frame_depth_dev & 3)) return ROPE_E_ARG;
    if (((uintptr_t)columns_dev & 7) || ((uintptr_t)out_dev & 7) || ((uintptr_t)work_dev & 7)) return ROPE_E_ARG;
    const long long chunks = neq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    const Camera cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    hipLaunchKernelGGL(neq_partial_kernel<CAMERA>, dim3((unsigned)((long long)n_frames * chunks)), dim3(NEQ_THREADS),
                       0, st, render_depth_dev, render_ids_dev, frame_depth_dev, H, W, (int)chunks, n_links, cam, columns_dev, n_columns,
                       (double)clip_m, work_dev);
    if (hipGetLastError() != hipSuccess) return ROPE_E_HIP;
    const int per = NEQ_GATHER_THREADS / ROPE_NEQ_WORDS;
    hipLaunchKernelGGL(neq_gather_kernel, dim3((unsigned)((n_frames + per - 1) / per)), dim3(NEQ_GATHER_THREADS), 0, st, work_dev, n_frames,
                       (int)chunks, out_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

}  // namespace

extern "C" size_t rope_pose_normal_workspace(int n_frames, int H, int W)
{
    return (size_t)n_frames * (size_t)neq_chunks(n_frames, H, W) * ROPE_NEQ_WORDS * sizeof(double);
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
