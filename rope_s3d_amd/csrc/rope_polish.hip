// rope_polish.hip — the continuous polish of a batch of poses, natively, for gfx950: what prediction/refinement.py's PoseRefiner does
// around rope_pose_normal_equations with numpy and LAPACK, as three small float64 kernels and a host loop behind the C ABI.
//
//   rope_joint_axes        per frame the six joints' axis and a point on it in camera axes (joint_axes_kernel): fk_mvp_kernel's own
//                          chain (rope_fk.h), so the axes belong to exactly the transforms the render was drawn with
//   rope_levenberg_step    per frame (A + lam diag A) d = -g on the live joints by Gaussian elimination with partial pivoting, and the
//                          clip to the joint limits (levenberg_step_kernel)
//   rope_formal_variance   per frame s^2 diag(A^-1) by the same elimination (formal_variance_kernel)
//   rope_refine_poses      PoseRefiner.refine's loop: render, axes, equations, cost, then rounds of step -> render -> axes ->
//                          equations -> accept (polish_accept_kernel), then the variances.  Systems, angles, damping, costs and
//                          step counts stay on the device between rounds; a round's trial angles come down once because the raster
//                          path takes host rows (rope_render_batch_device).
//
// Everything is float64 with one IEEE operation per written operation (-ffp-contract=off, no fma); include/rope_s3d.h is the
// contract and tests/polish_ref.py restates it with Python floats.
//
// Shape.  One frame per thread, 64 threads a workgroup.  A frame's system is at most 6 x 7 doubles (M | b) and the pivot search
// indexes its rows at run time: a per-thread array indexed that way would live in scratch, so the systems of a workgroup lie in
// LDS element-major, s_m[element][thread] — lane t reads word t of a row of 64 consecutive 8-byte words, whatever element its
// own control flow has reached, so a wave's access is at unit stride.  21.5 KB (step) and 24.6 KB (variance) a workgroup of one
// wave; a batch is a few hundred frames, so occupancy is not what these kernels wait for.  No thread reads another's words and
// there is no barrier: a thread beyond the batch simply leaves.  The elimination itself, the clip, the cost and the checks of masks
// and limits are rope_bundle_polish.hip's as well and live in rope_solve.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rope_ctx.h"
#include "rope_fk.h"
#include "rope_solve.h"

namespace {

constexpr int POLISH_THREADS = 64;
constexpr int POLISH_COLS = 7;                  // six columns of M and the right-hand side
constexpr int POLISH_ELEMS = 6 * POLISH_COLS;

struct PolishCamera { double R[9], t[3]; };     // X_c = R (X_w - t)

// word of A[i][j], i <= j, among a frame's ROPE_NEQ_WORDS: the upper triangle row by row from word 10
__device__ __forceinline__ int tri_word(int i, int j) { return 10 + 6 * i - (i * (i - 1)) / 2 + (j - i); }

// The live joints of a frame: those of active_mask with a positive diagonal entry, ascending, three bits each -> p.
__device__ __forceinline__ int live_joints(const double *__restrict__ w, int active_mask, uint32_t &packed)
{
    int p = 0;
    packed = 0;
#pragma unroll
    for (int j = 0; j < 6; j++)
        if (((active_mask >> j) & 1) && w[tri_word(j, j)] > 0.0) packed |= (uint32_t)j << (3 * p++);
    return p;
}

// M = A[idx][idx] into the thread's column of s_m, the diagonal damped when lam is given: M_kk = A_kk + lam A_kk
__device__ __forceinline__ void load_block(double (*s_m)[POLISH_THREADS], int t, const double *__restrict__ w, uint32_t packed, int p, bool damp, double lam)
{
    for (int r = 0; r < p; r++) {
        const int jr = (packed >> (3 * r)) & 7;
        for (int c = 0; c < p; c++) {
            const int jc = (packed >> (3 * c)) & 7;
            const double a = w[jr <= jc ? tri_word(jr, jc) : tri_word(jc, jr)];
            s_m[r * POLISH_COLS + c][t] = (damp && r == c) ? a + lam * a : a;
        }
    }
}

__global__ void __launch_bounds__(POLISH_THREADS)
levenberg_step_kernel(const double *__restrict__ words, const double *__restrict__ q, const double *__restrict__ lam_dev, int n_frames,
                      int active_mask, JointLimits lim, double *__restrict__ trial)
{
    __shared__ double s_m[POLISH_ELEMS][POLISH_THREADS];
    const int t = threadIdx.x;
    const int f = blockIdx.x * POLISH_THREADS + t;
    if (f >= n_frames) return;
    const double *const w = words + (size_t)f * ROPE_NEQ_WORDS;
    uint32_t packed;
    const int p = live_joints(w, active_mask, packed);
    bool ok = p > 0;
    if (ok) {
        load_block(s_m, t, w, packed, p, true, lam_dev[f]);
        for (int r = 0; r < p; r++) s_m[r * POLISH_COLS + 6][t] = -w[4 + ((packed >> (3 * r)) & 7)];
        ok = eliminate<6, POLISH_COLS, POLISH_THREADS>(s_m, t, p, 1);
        for (int r = 0; ok && r < p; r++) ok = isfinite(s_m[r * POLISH_COLS + 6][t]);
    }
    int k = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const bool live = ((active_mask >> j) & 1) && w[tri_word(j, j)] > 0.0;
        const double d = (ok && live) ? s_m[k * POLISH_COLS + 6][t] : 0.0;
        k += live ? 1 : 0;
        trial[(size_t)f * 6 + j] = clip_to(q[(size_t)f * 6 + j] + d, lim.lo[j], lim.hi[j]);
    }
}

__global__ void __launch_bounds__(POLISH_THREADS)
formal_variance_kernel(const double *__restrict__ words, int n_frames, int active_mask, double *__restrict__ var)
{
    __shared__ double s_m[POLISH_ELEMS][POLISH_THREADS];
    __shared__ double s_v[6][POLISH_THREADS];
    const int t = threadIdx.x;
    const int f = blockIdx.x * POLISH_THREADS + t;
    if (f >= n_frames) return;
    const double *const w = words + (size_t)f * ROPE_NEQ_WORDS;
    uint32_t packed;
    const int p = live_joints(w, active_mask, packed);
    bool ok = p > 0 && !(w[2] < (double)(p + 1));
    if (ok) {
        const double s2 = w[3] / (w[2] - (double)p);
        for (int k = 0; ok && k < p; k++) {                     // A x = e_k: the elimination of the block again, with another right-hand side
            load_block(s_m, t, w, packed, p, false, 0.0);
            for (int r = 0; r < p; r++) s_m[r * POLISH_COLS + 6][t] = r == k ? 1.0 : 0.0;
            ok = eliminate<6, POLISH_COLS, POLISH_THREADS>(s_m, t, p, 1);
            if (ok) {
                const double v = s2 * s_m[k * POLISH_COLS + 6][t];
                s_v[k][t] = v;
                ok = isfinite(v) && v >= 0.0;
            }
        }
    }
    int k = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const bool active = (active_mask >> j) & 1;
        const bool live = active && w[tri_word(j, j)] > 0.0;
        double v = active ? (double)INFINITY : (double)NAN;
        if (ok && live) v = s_v[k][t];
        k += live ? 1 : 0;
        var[(size_t)f * 6 + j] = v;
    }
}

__device__ __forceinline__ double dot3(double ux, double uy, double uz, double vx, double vy, double vz) { return (ux * vx + uy * vy) + uz * vz; }

// One thread per frame: fk_mvp_kernel's chain over the six joints, and after link j + 1's transform the joint's axis and origin
__global__ void __launch_bounds__(POLISH_THREADS)
joint_axes_kernel(const double *__restrict__ q, int n_frames, const double *__restrict__ joint_fixed, const double *__restrict__ joint_axes,
                  PolishCamera cam, double *__restrict__ out)
{
    const int f = blockIdx.x * POLISH_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double A[12], N[12];
        rope::joint_matrix(q[(size_t)f * 6 + j], j, joint_fixed, joint_axes, A);
        rope::aff_mul(T, A, N);
#pragma unroll
        for (int k = 0; k < 12; k++) T[k] = N[k];
        const double ax = joint_axes[3 * j], ay = joint_axes[3 * j + 1], az = joint_axes[3 * j + 2];
        const double wx = dot3(T[0], T[1], T[2], ax, ay, az), wy = dot3(T[4], T[5], T[6], ax, ay, az), wz = dot3(T[8], T[9], T[10], ax, ay, az);
        const double ox = T[3] - cam.t[0], oy = T[7] - cam.t[1], oz = T[11] - cam.t[2];
        double *const o = out + ((size_t)f * 6 + j) * 6;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            o[r] = dot3(cam.R[3 * r], cam.R[3 * r + 1], cam.R[3 * r + 2], wx, wy, wz);
            o[3 + r] = dot3(cam.R[3 * r], cam.R[3 * r + 1], cam.R[3 * r + 2], ox, oy, oz);
        }
    }
}

// The state of rope_refine_poses at the start: the cost of the systems at q, no step taken, the damping every frame starts with
__global__ void __launch_bounds__(POLISH_THREADS)
polish_init_kernel(const double *__restrict__ words, int n_frames, double damping, double *__restrict__ cost, double *__restrict__ cost_before,
                   double *__restrict__ lam, int32_t *__restrict__ steps)
{
    const int f = blockIdx.x * POLISH_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const double c = mean_cost(words + (size_t)f * ROPE_NEQ_WORDS);
    cost[f] = cost_before[f] = c;
    lam[f] = damping;
    steps[f] = 0;
}

// A round's verdict per frame: the trial is kept when its cost is strictly smaller — angles, system, cost, one more step —
// and otherwise the frame's damping grows tenfold
__global__ void __launch_bounds__(POLISH_THREADS)
polish_accept_kernel(const double *__restrict__ words_t, const double *__restrict__ trial, int n_frames, double *__restrict__ words,
                     double *__restrict__ q, double *__restrict__ cost, double *__restrict__ lam, int32_t *__restrict__ steps)
{
    const int f = blockIdx.x * POLISH_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const double *const wt = words_t + (size_t)f * ROPE_NEQ_WORDS;
    const double c = mean_cost(wt);
    if (c < cost[f]) {
        for (int k = 0; k < ROPE_NEQ_WORDS; k++) words[(size_t)f * ROPE_NEQ_WORDS + k] = wt[k];
        for (int j = 0; j < 6; j++) q[(size_t)f * 6 + j] = trial[(size_t)f * 6 + j];
        cost[f] = c;
        steps[f] = steps[f] + 1;
    } else {
        lam[f] = lam[f] * 10.0;
    }
}

__global__ void __launch_bounds__(POLISH_THREADS)
polish_inliers_kernel(const double *__restrict__ words, int n_frames, double *__restrict__ inliers)
{
    const int f = blockIdx.x * POLISH_THREADS + threadIdx.x;
    if (f < n_frames) inliers[f] = words[(size_t)f * ROPE_NEQ_WORDS + 2];
}

inline unsigned polish_grid(int n_frames) { return (unsigned)((n_frames + POLISH_THREADS - 1) / POLISH_THREADS); }

// The pieces of rope_refine_poses' work_dev, in bytes from its start; every piece 8-byte aligned.  `total` 0: a shape refused.
// What the caller gets back lies in one run, q .. steps and then the systems, so that it comes down in one copy.
struct PolishLayout {
    size_t depth, ids, neq, axes, words_t, trial, lam, q, var, cost_before, cost, inliers, steps, words, total;
};
PolishLayout polish_layout(int n_frames, int H, int W)
{
    PolishLayout l{};
    const size_t neq = n_frames < 1 ? 0 : rope_pose_normal_workspace(n_frames, H, W);
    if (neq == 0) return l;
    const size_t n = (size_t)n_frames, px = (size_t)H * (size_t)W;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += (bytes + 7) & ~(size_t)7; return here; };
    l.depth = take(n * px * sizeof(float));
    l.ids = take(n * px);
    l.neq = take(neq);
    l.axes = take(n * 36 * sizeof(double));
    l.words_t = take(n * ROPE_NEQ_WORDS * sizeof(double));
    l.trial = take(n * 6 * sizeof(double));
    l.lam = take(n * sizeof(double));
    l.q = take(n * 6 * sizeof(double));
    l.var = take(n * 6 * sizeof(double));
    l.cost_before = take(n * sizeof(double));
    l.cost = take(n * sizeof(double));
    l.inliers = take(n * sizeof(double));
    l.steps = take(n * sizeof(int32_t));
    l.words = take(n * ROPE_NEQ_WORDS * sizeof(double));
    l.total = at;
    return l;
}

}  // namespace

extern "C" int rope_joint_axes(rope_ctx *c, const double *q_dev, int n_frames, const double *Rwc, const double *tc, double *joints_dev, void *stream)
{
    if (!c) return ROPE_E_ARG;
    if (!c->have_robot) ARG_FAIL(c, "rope_joint_axes: call rope_set_robot first");
    if (n_frames < 1 || !q_dev || !Rwc || !tc || !joints_dev || misaligned8(q_dev) || misaligned8(joints_dev))
        ARG_FAIL(c, "rope_joint_axes: need n_frames >= 1 and 8-byte aligned q_dev and joints_dev, Rwc and tc");
    PolishCamera cam;
    for (int k = 0; k < 9; k++) cam.R[k] = Rwc[k];
    for (int k = 0; k < 3; k++) cam.t[k] = tc[k];
    for (int k = 0; k < 9; k++) if (!std::isfinite(cam.R[k])) ARG_FAIL(c, "rope_joint_axes: Rwc is not finite");
    for (int k = 0; k < 3; k++) if (!std::isfinite(cam.t[k])) ARG_FAIL(c, "rope_joint_axes: tc is not finite");
    hipLaunchKernelGGL(joint_axes_kernel, dim3(polish_grid(n_frames)), dim3(POLISH_THREADS), 0, (hipStream_t)stream, q_dev, n_frames,
                       c->d_joint_fixed.get(), c->d_joint_axes.get(), cam, joints_dev);
    HIP_TRY(c, hipGetLastError());
    return ROPE_OK;
}

extern "C" int rope_levenberg_step(const double *words_dev, const double *q_dev, const double *lam_dev, int n_frames, int active_mask,
                                   const double *limits, double *trial_dev, void *stream)
{
    if (n_frames < 1 || !words_dev || !q_dev || !lam_dev || !trial_dev || bad_mask6(active_mask) || bad_limits(limits)) return ROPE_E_ARG;
    if (misaligned8(words_dev) || misaligned8(q_dev) || misaligned8(lam_dev) || misaligned8(trial_dev)) return ROPE_E_ARG;
    hipLaunchKernelGGL(levenberg_step_kernel, dim3(polish_grid(n_frames)), dim3(POLISH_THREADS), 0, (hipStream_t)stream, words_dev, q_dev, lam_dev,
                       n_frames, active_mask, JointLimits(limits), trial_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" int rope_formal_variance(const double *words_dev, int n_frames, int active_mask, double *var_dev, void *stream)
{
    if (n_frames < 1 || !words_dev || !var_dev || bad_mask6(active_mask) || misaligned8(words_dev) || misaligned8(var_dev)) return ROPE_E_ARG;
    hipLaunchKernelGGL(formal_variance_kernel, dim3(polish_grid(n_frames)), dim3(POLISH_THREADS), 0, (hipStream_t)stream, words_dev, n_frames,
                       active_mask, var_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" size_t rope_refine_workspace(rope_ctx *c, int n_frames)
{
    if (!c || !c->have_camera) return 0;
    return polish_layout(n_frames, c->fp.H, c->fp.W).total;
}

extern "C" int rope_refine_poses(rope_ctx *c, const double *q, const float *frame_depth_dev, int n_frames, const double *camera_pose6, float fx,
                                 float fy, float cx, float cy, int active_mask, const double *limits, float clip_m, int iterations, double damping,
                                 void *work_dev, double *angles_out, double *var_out, double *cost_before, double *cost_after, int32_t *steps_out,
                                 double *inliers_out, double *words_out)
{
    if (!c) return ROPE_E_ARG;
    // everything any part would refuse is refused here, before the first command
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "rope_refine_poses: robot and camera must be set first");
    if (n_frames < 1) ARG_FAIL(c, "rope_refine_poses: need n_frames >= 1");
    if (!q || !frame_depth_dev || !camera_pose6 || !work_dev || !angles_out || !var_out || !cost_before || !cost_after || !steps_out || !inliers_out)
        ARG_FAIL(c, "rope_refine_poses: null pointer");
    if (((uintptr_t)frame_depth_dev & 3) || misaligned8(work_dev)) ARG_FAIL(c, "rope_refine_poses: misaligned device pointer");
    if (bad_mask6(active_mask)) ARG_FAIL(c, "rope_refine_poses: active_mask outside 0 .. 63");
    if (bad_limits(limits)) ARG_FAIL(c, "rope_refine_poses: limits must be finite with lo <= hi");
    if (iterations < 0 || !std::isfinite(damping) || damping < 0.0) ARG_FAIL(c, "rope_refine_poses: iterations and damping must not be negative");
    if (!std::isfinite(clip_m) || !(clip_m > 0.0f)) ARG_FAIL(c, "rope_refine_poses: clip_m must be finite and positive");
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || fx == 0.0f || fy == 0.0f)
        ARG_FAIL(c, "rope_refine_poses: camera terms must be finite, fx and fy not 0");
    for (int k = 0; k < 6; k++) if (!std::isfinite(camera_pose6[k])) ARG_FAIL(c, "rope_refine_poses: camera pose is not finite");
    for (size_t i = 0; i < 6 * (size_t)n_frames; i++)
        if (!std::isfinite(q[i]) || std::fabs(q[i]) > 1.0e4) ARG_FAIL(c, "rope_refine_poses: joint angle not finite or |q| > 1e4 rad");
    const int H = c->fp.H, W = c->fp.W;
    const PolishLayout l = polish_layout(n_frames, H, W);
    if (l.total == 0 || n_frames > MAX_ROWS) ARG_FAIL(c, "rope_refine_poses: too many frames, or pixels, for one call");

    // the camera in the kernels' axes (x right, y down, z forward): X_c = Rwc (X_w - tc), Rwc = diag(1, -1, -1) R^T
    double R[3][3], Rwc[9], tc[3] = {camera_pose6[0], camera_pose6[1], camera_pose6[2]};
    rope_pose_rotation(camera_pose6, R);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rwc[3 * i + j] = i == 0 ? R[j][i] : -R[j][i];

    unsigned char *const base = static_cast<unsigned char *>(work_dev);
    float *const d_depth = reinterpret_cast<float *>(base + l.depth);
    uint8_t *const d_ids = base + l.ids;
    auto dbl = [base](size_t off) { return reinterpret_cast<double *>(base + off); };
    double *const d_neq = dbl(l.neq), *const d_axes = dbl(l.axes), *const d_words = dbl(l.words), *const d_words_t = dbl(l.words_t),
                 *const d_q = dbl(l.q), *const d_trial = dbl(l.trial), *const d_lam = dbl(l.lam), *const d_cost = dbl(l.cost),
                 *const d_cost0 = dbl(l.cost_before), *const d_var = dbl(l.var), *const d_inl = dbl(l.inliers);
    int32_t *const d_steps = reinterpret_cast<int32_t *>(base + l.steps);
    const int n_render = std::min(c->n_links, ROPE_MAX_LINKS);
    const dim3 grid(polish_grid(n_frames)), block(POLISH_THREADS);
    const size_t row = 6 * (size_t)n_frames * sizeof(double);

    // render at the host rows `at`, then the axes and the equations of the same angles on the device -> `words`
    auto equations = [&](const double *at, const double *at_dev, double *words) -> int {
        int rc = rope_render_batch_device(c, at, nullptr, n_frames, n_render, d_depth, d_ids);
        if (rc) return rc;
        if ((rc = rope_joint_axes(c, at_dev, n_frames, Rwc, tc, d_axes, c->stream))) return rc;
        rc = rope_pose_normal_equations(d_depth, d_ids, frame_depth_dev, n_frames, H, W, n_render, fx, fy, cx, cy, d_axes, 6, clip_m, words, d_neq,
                                        c->stream);
        if (rc) c->err = "rope_refine_poses: rope_pose_normal_equations refused the frames";
        return rc;
    };

    HIP_TRY(c, hipSetDevice(c->device));
    int rc = copy_h2d_staged(c, d_q, q, row);
    if (rc) return rc;
    if ((rc = equations(q, d_q, d_words))) return rc;
    hipLaunchKernelGGL(polish_init_kernel, grid, block, 0, c->stream, d_words, n_frames, damping, d_cost, d_cost0, d_lam, d_steps);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> trial(6 * (size_t)n_frames);
    for (int it = 0; it < iterations; it++) {
        if ((rc = rope_levenberg_step(d_words, d_q, d_lam, n_frames, active_mask, limits, d_trial, c->stream))) {
            c->err = "rope_refine_poses: rope_levenberg_step failed";
            return rc;
        }
        if ((rc = copy_d2h_staged(c, trial.data(), d_trial, row))) return rc;       // the round's one wait: the raster path takes host rows
        if ((rc = equations(trial.data(), d_trial, d_words_t))) return rc;
        hipLaunchKernelGGL(polish_accept_kernel, grid, block, 0, c->stream, d_words_t, d_trial, n_frames, d_words, d_q, d_cost, d_lam, d_steps);
        HIP_TRY(c, hipGetLastError());
    }
    if ((rc = rope_formal_variance(d_words, n_frames, active_mask, d_var, c->stream))) {
        c->err = "rope_refine_poses: rope_formal_variance failed";
        return rc;
    }
    hipLaunchKernelGGL(polish_inliers_kernel, grid, block, 0, c->stream, d_words, n_frames, d_inl);
    HIP_TRY(c, hipGetLastError());
    // one copy for everything the caller gets, and the call is complete when it is down
    const size_t n = (size_t)n_frames, end = words_out ? l.total : l.words;
    std::vector<unsigned char> back(end - l.q);
    if ((rc = copy_d2h_staged(c, back.data(), base + l.q, back.size()))) return rc;
    auto from = [&](size_t off) { return back.data() + (off - l.q); };
    std::memcpy(angles_out, from(l.q), row);
    std::memcpy(var_out, from(l.var), row);
    std::memcpy(cost_before, from(l.cost_before), n * sizeof(double));
    std::memcpy(cost_after, from(l.cost), n * sizeof(double));
    std::memcpy(inliers_out, from(l.inliers), n * sizeof(double));
    std::memcpy(steps_out, from(l.steps), n * sizeof(int32_t));
    if (words_out) std::memcpy(words_out, from(l.words), n * ROPE_NEQ_WORDS * sizeof(double));
    return ROPE_OK;
}
