// rope_bundle_polish.hip — the camera polish and the bundle polish, natively, for gfx950: what prediction/refinement.py's
// BundleRefiner does around rope_bundle_normal_equations with numpy and LAPACK (pool_bundle, schur_step, schur_sigma,
// bundle_columns_step, bundle_columns_sigma and the loop around them), as small float64 kernels and a host loop behind the C ABI.
//
//   rope_camera_twists             host: a camera pose -> the kernels' camera axes (Rwc, tc) and the six twists of its parameters
//   rope_bundle_pool               the frames' 96 words added in frame order, one thread a word (bundle_pool_kernel)
//   rope_bundle_schur_step         the Levenberg step of the block-arrow system: per frame X_f = D_f^-1 [B_f | g_f] and its share
//                                  P_f = B_f^T X_f (schur_frame_kernel), the frame-order sum and the camera's solve in one
//                                  workgroup (schur_reduce_kernel), the frames' own steps and the clip (schur_back_kernel)
//   rope_bundle_schur_variance     the formal variances of the same system at lam = 0, the same three parts
//                                  (schur_var_frame_kernel, schur_var_reduce_kernel, schur_var_back_kernel)
//   rope_bundle_columns_step / _variance   the pooled twelve-column system of 'offset' mode, solved by one thread
//   rope_refine_bundle             BundleRefiner.refine's depth loop: words, pooled words, angles, offsets, pose, damping, cost and
//                                  the step count stay on the device between rounds; a round's trial pose and trial angles come
//                                  down once because the raster path takes host rows (rope_render_batch_device)
//
// Everything is float64 with one IEEE operation per written operation (-ffp-contract=off, no fma); include/rope_s3d.h is the
// contract and tests/bundle_polish_ref.py restates it with Python floats.
//
// Shape.  The per-frame kernels take one frame per thread, 64 threads a workgroup, and hold a workgroup's systems in LDS
// element-major, s_m[element][thread], as rope_polish.hip does and for its reason: the pivot search indexes rows at run time, and
// a per-thread array indexed that way would live in scratch.  A frame's system is 6 x 13 doubles for the step (D | B | g) and
// 6 x 18 for the variances (A | B | I): 39 936 and 55 296 bytes a workgroup of one wave.  The systems one thread solves (the
// camera's 6 x 7 and 6 x 12, the pooled 12 x 13 and 12 x 24) lie in LDS as well, one word an element.  No kernel uses scratch.
// THE ELIMINATION of all of them is one function, eliminate<MW, RW, TS> in rope_solve.h, which rope_polish.hip calls too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rope_ctx.h"
#include "rope_solve.h"

namespace {

constexpr int BP_THREADS = 64;
constexpr int BW = ROPE_BNEQ_WORDS;
constexpr int STEP_RW = 13, STEP_ELEMS = 6 * STEP_RW;        // D (6) | B (<= 6) | g
constexpr int VAR_RW = 18, VAR_ELEMS = 6 * VAR_RW;           // A (6) | B (<= 6) | I (<= 6)
constexpr int CAM_RW = 7, CAM_ELEMS = 6 * CAM_RW;            // S (6) | -rhs
constexpr int COV_RW = 12, COV_ELEMS = 6 * COV_RW;           // S0 (6) | I (6)
constexpr int COL_RW = 13, COL_ELEMS = 12 * COL_RW;          // M (12) | b
constexpr int COLV_RW = 24, COLV_ELEMS = 12 * COLV_RW;       // A (12) | I (12)
// a frame's record between the three kernels of a call, in doubles
constexpr int REC = 88;
constexpr int REC_X = 0, REC_P = 42, REC_OK = 84;                            // step: X (r 7 + m; m = 6: g), P (a 7 + b; b = 6: rhs)
constexpr int REC_Y = 0, REC_AINV = 36, REC_VP = 42, REC_VOK = 78, REC_NP = 79;   // variance: Y (r 6 + a), diag A^-1, P (a 6 + b), ok, p
constexpr int STATE = 48;                                                    // the reduce kernel's words for the back kernel

struct BundleTwists { double v[36]; };

// word of A[i][j], i <= j, among the 96: the upper triangle over the twelve slots row by row from word 16
__device__ __forceinline__ int tri12(int i, int j) { return 16 + 12 * i - (i * (i - 1)) / 2 + (j - i); }
__device__ __forceinline__ int sym12(int i, int j) { return i <= j ? tri12(i, j) : tri12(j, i); }

// the slots first .. first + count - 1 of `mask` (bit k = slot first + k) with a positive diagonal, ascending, four bits each -> p
__device__ __forceinline__ int live_slots(const double *__restrict__ w, int mask, int first, int count, uint64_t &packed)
{
    int p = 0;
    packed = 0;
    for (int k = 0; k < count; k++)
        if (((mask >> k) & 1) && w[tri12(first + k, first + k)] > 0.0) packed |= (uint64_t)k << (4 * p++);
    return p;
}
__device__ __forceinline__ int slot_of(uint64_t packed, int r) { return (int)((packed >> (4 * r)) & 15); }

// ---------------------------------------------------------------------------------------------- the pool
__global__ void __launch_bounds__(BP_THREADS)
bundle_pool_kernel(const double *__restrict__ words, int n_frames, double *__restrict__ pooled)
{
    const int k = blockIdx.x * BP_THREADS + threadIdx.x;
    if (k >= BW) return;
    double s = 0.0;
    for (int f = 0; f < n_frames; f++) s = s + words[(size_t)f * BW + k];
    pooled[k] = s;
}

// ---------------------------------------------------------------------------------------------- the arrow step
__global__ void __launch_bounds__(BP_THREADS)
schur_frame_kernel(const double *__restrict__ words, const double *__restrict__ pooled, const double *__restrict__ lam_dev, int n_frames,
                   int joint_mask, int camera_mask, double *__restrict__ rec)
{
    __shared__ double s_m[STEP_ELEMS][BP_THREADS];
    const int t = threadIdx.x;
    const int f = blockIdx.x * BP_THREADS + t;
    if (f >= n_frames) return;
    const double *const w = words + (size_t)f * BW;
    double *const o = rec + (size_t)f * REC;
    uint64_t pj, pc;
    const int nk = live_slots(pooled, camera_mask, 6, 6, pc);
    const int p = live_slots(w, joint_mask, 0, 6, pj);
    const double lam = lam_dev[0];
    bool ok = p > 0;
    if (ok) {
        for (int r = 0; r < p; r++) {
            const int jr = slot_of(pj, r);
            for (int c = 0; c < p; c++) {
                const double a = w[sym12(jr, slot_of(pj, c))];
                s_m[r * STEP_RW + c][t] = r == c ? a + lam * a : a;
            }
            for (int a = 0; a < nk; a++) s_m[r * STEP_RW + 6 + a][t] = w[tri12(jr, 6 + slot_of(pc, a))];
            s_m[r * STEP_RW + 6 + nk][t] = w[4 + jr];
        }
        ok = eliminate<6, STEP_RW, BP_THREADS>(s_m, t, p, nk + 1) && all_finite<6, STEP_RW, BP_THREADS>(s_m, t, p, nk + 1);
    }
    o[REC_OK] = ok ? 1.0 : 0.0;
    if (!ok) return;
    for (int r = 0; r < p; r++) {
        for (int a = 0; a < nk; a++) o[REC_X + r * 7 + a] = s_m[r * STEP_RW + 6 + a][t];
        o[REC_X + r * 7 + 6] = s_m[r * STEP_RW + 6 + nk][t];
    }
    for (int a = 0; a < nk; a++) {                              // P_f = B_f^T X_f, r ascending from the first product
        const int ca = 6 + slot_of(pc, a);
        for (int b = 0; b <= nk; b++) {
            double s = w[tri12(slot_of(pj, 0), ca)] * s_m[6 + b][t];
            for (int r = 1; r < p; r++) s = s + w[tri12(slot_of(pj, r), ca)] * s_m[r * STEP_RW + 6 + b][t];
            o[REC_P + a * 7 + (b < nk ? b : 6)] = s;
        }
    }
}

// One workgroup: S = C + lam diag C and rhs = gc, less the frames' shares in frame order (a thread an entry), then S d = -rhs by
// thread 0 -> state[a] = d[a] over the live camera slots, trial_pose = pose + dc
__global__ void __launch_bounds__(BP_THREADS)
schur_reduce_kernel(const double *__restrict__ rec, const double *__restrict__ pooled, const double *__restrict__ lam_dev, int n_frames,
                    int camera_mask, const double *__restrict__ pose, double *__restrict__ state, double *__restrict__ trial_pose)
{
    __shared__ double s_s[CAM_ELEMS][1];
    const int e = threadIdx.x;
    uint64_t pc;
    const int nk = live_slots(pooled, camera_mask, 6, 6, pc);
    const double lam = lam_dev[0];
    if (e < CAM_ELEMS) {
        const int a = e / 7, b = e % 7;
        if (a < nk && (b < nk || b == 6)) {
            double v;
            if (b < nk) {
                const double c = pooled[sym12(6 + slot_of(pc, a), 6 + slot_of(pc, b))];
                v = a == b ? c + lam * c : c;
            } else {
                v = pooled[4 + 6 + slot_of(pc, a)];
            }
            for (int f = 0; f < n_frames; f++)
                if (rec[(size_t)f * REC + REC_OK] != 0.0) v = v - rec[(size_t)f * REC + REC_P + e];
            s_s[e][0] = v;
        }
    }
    __syncthreads();
    if (e != 0) return;
    for (int a = 0; a < nk; a++) s_s[a * 7 + 6][0] = -s_s[a * 7 + 6][0];
    const bool ok = nk > 0 && eliminate<6, CAM_RW, 1>(s_s, 0, nk, 1) && all_finite<6, CAM_RW, 1>(s_s, 0, nk, 1);
    for (int k = 0; k < 6; k++) state[6 + k] = 0.0;
    for (int a = 0; a < 6; a++) {
        const double d = (ok && a < nk) ? s_s[a * 7 + 6][0] : 0.0;
        state[a] = d;
        if (a < nk) state[6 + slot_of(pc, a)] = d;
    }
    for (int k = 0; k < 6; k++) trial_pose[k] = pose[k] + state[6 + k];
}

__global__ void __launch_bounds__(BP_THREADS)
schur_back_kernel(const double *__restrict__ words, const double *__restrict__ pooled, const double *__restrict__ rec,
                  const double *__restrict__ state, const double *__restrict__ q, int n_frames, int joint_mask, int camera_mask, JointLimits lim,
                  double *__restrict__ trial)
{
    const int f = blockIdx.x * BP_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const double *const w = words + (size_t)f * BW;
    const double *const x = rec + (size_t)f * REC + REC_X;
    uint64_t pc;
    const int nk = live_slots(pooled, camera_mask, 6, 6, pc);
    const bool ok = rec[(size_t)f * REC + REC_OK] != 0.0;
    int k = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const bool live = ((joint_mask >> j) & 1) && w[tri12(j, j)] > 0.0;
        double d = 0.0;
        if (ok && live) {
            double s = 0.0;
            for (int a = 0; a < nk; a++) {
                const double pr = x[k * 7 + a] * state[a];
                s = a == 0 ? pr : s + pr;
            }
            d = -(x[k * 7 + 6] + s);
        }
        k += live ? 1 : 0;
        trial[(size_t)f * 6 + j] = clip_to(q[(size_t)f * 6 + j] + d, lim.lo[j], lim.hi[j]);
    }
}

// ---------------------------------------------------------------------------------------------- the arrow variances
__global__ void __launch_bounds__(BP_THREADS)
schur_var_frame_kernel(const double *__restrict__ words, const double *__restrict__ pooled, int n_frames, int joint_mask, int camera_mask,
                       double *__restrict__ rec)
{
    __shared__ double s_m[VAR_ELEMS][BP_THREADS];
    const int t = threadIdx.x;
    const int f = blockIdx.x * BP_THREADS + t;
    if (f >= n_frames) return;
    const double *const w = words + (size_t)f * BW;
    double *const o = rec + (size_t)f * REC;
    uint64_t pj, pc;
    const int nk = live_slots(pooled, camera_mask, 6, 6, pc);
    const int p = live_slots(w, joint_mask, 0, 6, pj);
    bool ok = p > 0;
    if (ok) {
        for (int r = 0; r < p; r++) {
            const int jr = slot_of(pj, r);
            for (int c = 0; c < p; c++) s_m[r * VAR_RW + c][t] = w[sym12(jr, slot_of(pj, c))];
            for (int a = 0; a < nk; a++) s_m[r * VAR_RW + 6 + a][t] = w[tri12(jr, 6 + slot_of(pc, a))];
            for (int c = 0; c < p; c++) s_m[r * VAR_RW + 6 + nk + c][t] = r == c ? 1.0 : 0.0;
        }
        ok = eliminate<6, VAR_RW, BP_THREADS>(s_m, t, p, nk + p) && all_finite<6, VAR_RW, BP_THREADS>(s_m, t, p, nk + p);
    }
    o[REC_VOK] = ok ? 1.0 : 0.0;
    o[REC_NP] = (double)p;
    if (!ok) return;
    for (int r = 0; r < p; r++) {
        for (int a = 0; a < nk; a++) o[REC_Y + r * 6 + a] = s_m[r * VAR_RW + 6 + a][t];
        o[REC_AINV + r] = s_m[r * VAR_RW + 6 + nk + r][t];
    }
    for (int a = 0; a < nk; a++) {
        const int ca = 6 + slot_of(pc, a);
        for (int b = 0; b < nk; b++) {
            double s = w[tri12(slot_of(pj, 0), ca)] * s_m[6 + b][t];
            for (int r = 1; r < p; r++) s = s + w[tri12(slot_of(pj, r), ca)] * s_m[r * VAR_RW + 6 + b][t];
            o[REC_VP + a * 6 + b] = s;
        }
    }
}

// One workgroup: p over all frames, S0 = C less the frames' shares in frame order, its inverse by thread 0 ->
// state[0 .. 35] cov_c (a 6 + b), [36] s^2, [37] 1 when the frames may go on, and var_pose
__global__ void __launch_bounds__(BP_THREADS)
schur_var_reduce_kernel(const double *__restrict__ rec, const double *__restrict__ pooled, int n_frames, int camera_mask,
                        double *__restrict__ state, double *__restrict__ var_pose)
{
    __shared__ double s_s[COV_ELEMS][1];
    __shared__ int s_p[BP_THREADS];
    const int e = threadIdx.x;
    uint64_t pc;
    const int nk = live_slots(pooled, camera_mask, 6, 6, pc);
    int count = 0;
    for (int f = e; f < n_frames; f += BP_THREADS) count += (int)rec[(size_t)f * REC + REC_NP];
    s_p[e] = count;
    if (e < 36) {
        const int a = e / 6, b = e % 6;
        if (a < nk && b < nk) {
            double v = pooled[sym12(6 + slot_of(pc, a), 6 + slot_of(pc, b))];
            for (int f = 0; f < n_frames; f++)
                if (rec[(size_t)f * REC + REC_VOK] != 0.0) v = v - rec[(size_t)f * REC + REC_VP + e];
            s_s[a * COV_RW + b][0] = v;
            s_s[a * COV_RW + 6 + b][0] = a == b ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    if (e != 0) return;
    int p = nk;
    for (int k = 0; k < BP_THREADS; k++) p += s_p[k];
    for (int k = 0; k < 6; k++) var_pose[k] = ((camera_mask >> k) & 1) ? (double)INFINITY : (double)NAN;
    bool go = p > 0 && !(pooled[2] < (double)(p + 1));
    const double s2 = go ? pooled[3] / (pooled[2] - (double)p) : 0.0;
    if (go && nk > 0) go = eliminate<6, COV_RW, 1>(s_s, 0, nk, nk) && all_finite<6, COV_RW, 1>(s_s, 0, nk, nk);
    state[36] = s2;
    state[37] = go ? 1.0 : 0.0;
    if (!go) return;
    bool fine = true;
    for (int a = 0; a < nk; a++) {
        for (int b = 0; b < nk; b++) state[a * 6 + b] = s_s[a * COV_RW + 6 + b][0];
        const double v = s2 * s_s[a * COV_RW + 6 + a][0];
        fine = fine && isfinite(v) && v >= 0.0;
    }
    if (fine)
        for (int a = 0; a < nk; a++) var_pose[slot_of(pc, a)] = s2 * s_s[a * COV_RW + 6 + a][0];
}

__global__ void __launch_bounds__(BP_THREADS)
schur_var_back_kernel(const double *__restrict__ words, const double *__restrict__ pooled, const double *__restrict__ rec,
                      const double *__restrict__ state, int n_frames, int joint_mask, int camera_mask, double *__restrict__ var)
{
    const int f = blockIdx.x * BP_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const double *const w = words + (size_t)f * BW;
    const double *const o = rec + (size_t)f * REC;
    uint64_t pc;
    const int nk = live_slots(pooled, camera_mask, 6, 6, pc);
    const bool ok = state[37] != 0.0 && o[REC_VOK] != 0.0;
    const double s2 = state[36];
    double v[6];
    bool fine = ok;
    int k = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const bool live = ((joint_mask >> j) & 1) && w[tri12(j, j)] > 0.0;
        v[j] = 0.0;
        if (ok && live) {
            double u = 0.0;
            for (int a = 0; a < nk; a++) {                      // u = Y_r cov_c Y_r^T: t_a = sum_b cov_c[a][b] Y[r][b], u = sum_a Y[r][a] t_a
                double ta = 0.0;
                for (int b = 0; b < nk; b++) {
                    const double pr = state[a * 6 + b] * o[REC_Y + k * 6 + b];
                    ta = b == 0 ? pr : ta + pr;
                }
                const double pr = o[REC_Y + k * 6 + a] * ta;
                u = a == 0 ? pr : u + pr;
            }
            v[j] = s2 * (o[REC_AINV + k] + u);
            fine = fine && isfinite(v[j]) && v[j] >= 0.0;
        }
        k += live ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const bool active = (joint_mask >> j) & 1;
        const bool live = active && w[tri12(j, j)] > 0.0;
        double out = active ? (double)INFINITY : (double)NAN;
        if (fine && live) out = v[j];
        var[(size_t)f * 6 + j] = out;
    }
}

// ---------------------------------------------------------------------------------------------- the pooled twelve columns
// Every workgroup solves the same system by its thread 0 (the same operations, the same bytes) and clips its 64 frames; workgroup 0
// writes the trial pose and offsets
__global__ void __launch_bounds__(BP_THREADS)
columns_step_kernel(const double *__restrict__ pooled, const double *__restrict__ lam_dev, int slot_mask, const double *__restrict__ pose,
                    const double *__restrict__ off, const double *__restrict__ q0, int n_frames, JointLimits lim,
                    double *__restrict__ trial_pose, double *__restrict__ trial_off, double *__restrict__ trial)
{
    __shared__ double s_s[COL_ELEMS][1];
    __shared__ double s_off[6];
    const int t = threadIdx.x;
    if (t == 0) {
        uint64_t ps;
        const int p = live_slots(pooled, slot_mask, 0, 12, ps);
        const double lam = lam_dev[0];
        for (int r = 0; r < p; r++) {
            const int sr = slot_of(ps, r);
            for (int c = 0; c < p; c++) {
                const double a = pooled[sym12(sr, slot_of(ps, c))];
                s_s[r * COL_RW + c][0] = r == c ? a + lam * a : a;
            }
            s_s[r * COL_RW + 12][0] = -pooled[4 + sr];
        }
        const bool ok = p > 0 && eliminate<12, COL_RW, 1>(s_s, 0, p, 1) && all_finite<12, COL_RW, 1>(s_s, 0, p, 1);
        int k = 0;
        for (int c = 0; c < 12; c++) {
            const bool live = ((slot_mask >> c) & 1) && pooled[tri12(c, c)] > 0.0;
            const double d = (ok && live) ? s_s[k * COL_RW + 12][0] : 0.0;
            k += live ? 1 : 0;
            if (c < 6) {
                const double v = off[c] + d;
                s_off[c] = v;
                if (blockIdx.x == 0) trial_off[c] = v;
            } else if (blockIdx.x == 0) {
                trial_pose[c - 6] = pose[c - 6] + d;
            }
        }
    }
    __syncthreads();
    const int f = blockIdx.x * BP_THREADS + t;
    if (f >= n_frames) return;
#pragma unroll
    for (int j = 0; j < 6; j++) trial[(size_t)f * 6 + j] = clip_to(q0[(size_t)f * 6 + j] + s_off[j], lim.lo[j], lim.hi[j]);
}

__global__ void __launch_bounds__(BP_THREADS)
columns_variance_kernel(const double *__restrict__ pooled, int slot_mask, double *__restrict__ var)
{
    __shared__ double s_s[COLV_ELEMS][1];
    if (threadIdx.x != 0) return;
    uint64_t ps;
    const int p = live_slots(pooled, slot_mask, 0, 12, ps);
    bool ok = p > 0 && !(pooled[2] < (double)(p + 1));
    double s2 = 0.0;
    if (ok) {
        s2 = pooled[3] / (pooled[2] - (double)p);
        for (int r = 0; r < p; r++) {
            const int sr = slot_of(ps, r);
            for (int c = 0; c < p; c++) {
                s_s[r * COLV_RW + c][0] = pooled[sym12(sr, slot_of(ps, c))];
                s_s[r * COLV_RW + 12 + c][0] = r == c ? 1.0 : 0.0;
            }
        }
        ok = eliminate<12, COLV_RW, 1>(s_s, 0, p, p) && all_finite<12, COLV_RW, 1>(s_s, 0, p, p);
        for (int r = 0; ok && r < p; r++) {
            const double v = s2 * s_s[r * COLV_RW + 12 + r][0];
            ok = isfinite(v) && v >= 0.0;
        }
    }
    int k = 0;
    for (int c = 0; c < 12; c++) {
        const bool active = (slot_mask >> c) & 1;
        const bool live = active && pooled[tri12(c, c)] > 0.0;
        double v = active ? (double)INFINITY : (double)NAN;
        if (ok && live) v = s2 * s_s[k * COLV_RW + 12 + k][0];
        k += live ? 1 : 0;
        var[c] = v;
    }
}

// ---------------------------------------------------------------------------------------------- the loop's own kernels
// head, in doubles: the scalars of rope_refine_bundle's state, brought down with the rest in one copy
constexpr int HD_POSE = 0, HD_OFF = 6, HD_VPOSE = 12, HD_VOFF = 18, HD_COST0 = 24, HD_COST = 25, HD_INL = 26, HD_STEPS = 27, HD_LAM = 28,
              HD_ACCEPT = 29, HD_WORDS = 32;

__global__ void bundle_init_kernel(const double *__restrict__ pooled, BundleTwists pose, double damping, double *__restrict__ head)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < 6; k++) { head[HD_POSE + k] = pose.v[k]; head[HD_OFF + k] = 0.0; }
    const double c = mean_cost(pooled);
    head[HD_COST0] = head[HD_COST] = c;
    head[HD_STEPS] = 0.0;
    head[HD_LAM] = damping;
    head[HD_ACCEPT] = 0.0;
}

// A round's verdict: the trial is kept when its pooled cost is strictly smaller — pooled words, pose, offsets, cost, one more
// step — and otherwise the damping grows tenfold.  The frames' words and angles follow in bundle_take_kernel.
__global__ void __launch_bounds__(BP_THREADS)
bundle_verdict_kernel(const double *__restrict__ pooled_t, const double *__restrict__ trial_pose, const double *__restrict__ trial_off,
                      double *__restrict__ pooled, double *__restrict__ head)
{
    __shared__ int s_take;
    const int t = threadIdx.x;
    if (t == 0) {
        const double c = mean_cost(pooled_t);
        const bool take = c < head[HD_COST];
        s_take = take ? 1 : 0;
        head[HD_ACCEPT] = take ? 1.0 : 0.0;
        if (take) {
            head[HD_COST] = c;
            head[HD_STEPS] = head[HD_STEPS] + 1.0;
            for (int k = 0; k < 6; k++) { head[HD_POSE + k] = trial_pose[k]; head[HD_OFF + k] = trial_off[k]; }
        } else {
            head[HD_LAM] = head[HD_LAM] * 10.0;
        }
    }
    __syncthreads();
    if (s_take)
        for (int k = t; k < BW; k += BP_THREADS) pooled[k] = pooled_t[k];
}

__global__ void __launch_bounds__(BP_THREADS)
bundle_take_kernel(const double *__restrict__ head, const double *__restrict__ words_t, const double *__restrict__ trial, int n_frames,
                   double *__restrict__ words, double *__restrict__ q)
{
    const int f = blockIdx.x * BP_THREADS + threadIdx.x;
    if (f >= n_frames || head[HD_ACCEPT] == 0.0) return;
    for (int k = 0; k < BW; k++) words[(size_t)f * BW + k] = words_t[(size_t)f * BW + k];
    for (int j = 0; j < 6; j++) q[(size_t)f * 6 + j] = trial[(size_t)f * 6 + j];
}

__global__ void __launch_bounds__(BP_THREADS)
bundle_finish_kernel(const double *__restrict__ words, const double *__restrict__ pooled, const double *__restrict__ var12, int n_frames,
                     double *__restrict__ head, double *__restrict__ frame_cost)
{
    const int f = blockIdx.x * BP_THREADS + threadIdx.x;
    if (f == 0) {
        head[HD_INL] = pooled[2];
        if (var12)
            for (int k = 0; k < 6; k++) { head[HD_VOFF + k] = var12[k]; head[HD_VPOSE + k] = var12[6 + k]; }
        else
            for (int k = 0; k < 6; k++) head[HD_VOFF + k] = (double)NAN;
    }
    if (f < n_frames) frame_cost[f] = mean_cost(words + (size_t)f * BW);
}

__global__ void __launch_bounds__(BP_THREADS)
tile_twists_kernel(BundleTwists tw, int n_frames, double *__restrict__ out)
{
    const int f = blockIdx.x * BP_THREADS + threadIdx.x;
    if (f >= n_frames) return;
#pragma unroll
    for (int k = 0; k < 36; k++) out[(size_t)f * 36 + k] = tw.v[k];
}

inline unsigned frame_grid(int n_frames) { return (unsigned)((n_frames + BP_THREADS - 1) / BP_THREADS); }
inline int launched() { return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP; }

// The pieces of rope_refine_bundle's work_dev, in bytes from its start; every piece 8-byte aligned.  `total` 0: a shape refused.
// What the caller gets back lies in one run, head .. words; what comes down between rounds in another, trial .. trial_pose.
struct BundleLayout {
    size_t depth, ids, neq, axes, twists, words_t, pooled, pooled_t, rec, state, q0, var12, trial_off, trial, trial_pose, head, q, var, frame_cost,
        words, total;
};
BundleLayout bundle_layout(int n_frames, int H, int W)
{
    BundleLayout l{};
    const size_t neq = n_frames < 1 ? 0 : rope_bundle_normal_workspace(n_frames, H, W);
    if (neq == 0) return l;
    const size_t n = (size_t)n_frames, px = (size_t)H * (size_t)W, d = sizeof(double);
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += (bytes + 7) & ~(size_t)7; return here; };
    l.depth = take(n * px * sizeof(float));
    l.ids = take(n * px);
    l.neq = take(neq);
    l.axes = take(n * 36 * d);
    l.twists = take(n * 36 * d);
    l.words_t = take(n * BW * d);
    l.pooled = take(BW * d);
    l.pooled_t = take(BW * d);
    l.rec = take(rope_bundle_schur_workspace(n_frames));
    l.state = take(STATE * d);
    l.q0 = take(n * 6 * d);
    l.var12 = take(12 * d);
    l.trial_off = take(6 * d);
    l.trial = take(n * 6 * d);
    l.trial_pose = take(6 * d);
    l.head = take(HD_WORDS * d);
    l.q = take(n * 6 * d);
    l.var = take(n * 6 * d);
    l.frame_cost = take(n * d);
    l.words = take(n * BW * d);
    l.total = at;
    return l;
}

}  // namespace

extern "C" int rope_camera_twists(const double *pose6, double *Rwc9, double *tc3, double *twists36)
{
    if (!pose6 || !Rwc9 || !tc3 || !twists36) return ROPE_E_ARG;
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(pose6[k])) return ROPE_E_ARG;
    double R[3][3];
    rope_pose_rotation(pose6, R);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rwc9[3 * i + j] = i == 0 ? R[j][i] : -R[j][i];
    for (int k = 0; k < 3; k++) tc3[k] = pose6[k];
    const double yaw = pose6[5], pitch = pose6[3];
    const double cy = std::cos(yaw), sy = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch);
    const double axis[3][3] = {{-sy, cy, 0.0}, {cy * cp, sy * cp, -sp}, {0.0, 0.0, 1.0}};      // of a3 (pitch), a4 (roll), a5 (yaw)
    for (int k = 0; k < 36; k++) twists36[k] = 0.0;
    for (int k = 0; k < 3; k++)
        for (int r = 0; r < 3; r++) twists36[6 * k + 3 + r] = -Rwc9[3 * r + k];
    for (int k = 0; k < 3; k++)
        for (int r = 0; r < 3; r++)
            twists36[6 * (3 + k) + r] = -((Rwc9[3 * r] * axis[k][0] + Rwc9[3 * r + 1] * axis[k][1]) + Rwc9[3 * r + 2] * axis[k][2]);
    return ROPE_OK;
}

extern "C" int rope_bundle_pool(const double *words_dev, int n_frames, double *pooled_dev, void *stream)
{
    if (n_frames < 1 || !words_dev || !pooled_dev || misaligned8(words_dev) || misaligned8(pooled_dev)) return ROPE_E_ARG;
    hipLaunchKernelGGL(bundle_pool_kernel, dim3((BW + BP_THREADS - 1) / BP_THREADS), dim3(BP_THREADS), 0, (hipStream_t)stream, words_dev, n_frames,
                       pooled_dev);
    return launched();
}

extern "C" size_t rope_bundle_schur_workspace(int n_frames)
{
    return n_frames < 1 ? 0 : ((size_t)n_frames * REC + STATE) * sizeof(double);
}

extern "C" int rope_bundle_schur_step(const double *words_dev, const double *pooled_dev, const double *q_dev, const double *pose_dev,
                                      const double *lam_dev, int n_frames, int joint_mask, int camera_mask, const double *limits, void *work_dev,
                                      double *trial_q_dev, double *trial_pose_dev, void *stream)
{
    if (n_frames < 1 || !words_dev || !pooled_dev || !q_dev || !pose_dev || !lam_dev || !work_dev || !trial_q_dev || !trial_pose_dev) return ROPE_E_ARG;
    if (bad_mask6(joint_mask) || bad_mask6(camera_mask) || bad_limits(limits)) return ROPE_E_ARG;
    if (misaligned8(words_dev) || misaligned8(pooled_dev) || misaligned8(q_dev) || misaligned8(pose_dev) || misaligned8(lam_dev) ||
        misaligned8(work_dev) || misaligned8(trial_q_dev) || misaligned8(trial_pose_dev))
        return ROPE_E_ARG;
    double *const rec = static_cast<double *>(work_dev), *const state = rec + (size_t)n_frames * REC;
    const dim3 grid(frame_grid(n_frames)), block(BP_THREADS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(schur_frame_kernel, grid, block, 0, s, words_dev, pooled_dev, lam_dev, n_frames, joint_mask, camera_mask, rec);
    hipLaunchKernelGGL(schur_reduce_kernel, dim3(1), block, 0, s, rec, pooled_dev, lam_dev, n_frames, camera_mask, pose_dev, state, trial_pose_dev);
    hipLaunchKernelGGL(schur_back_kernel, grid, block, 0, s, words_dev, pooled_dev, rec, state, q_dev, n_frames, joint_mask, camera_mask,
                       JointLimits(limits), trial_q_dev);
    return launched();
}

extern "C" int rope_bundle_schur_variance(const double *words_dev, const double *pooled_dev, int n_frames, int joint_mask, int camera_mask,
                                          void *work_dev, double *var_q_dev, double *var_pose_dev, void *stream)
{
    if (n_frames < 1 || !words_dev || !pooled_dev || !work_dev || !var_q_dev || !var_pose_dev || bad_mask6(joint_mask) || bad_mask6(camera_mask)) return ROPE_E_ARG;
    if (misaligned8(words_dev) || misaligned8(pooled_dev) || misaligned8(work_dev) || misaligned8(var_q_dev) || misaligned8(var_pose_dev)) return ROPE_E_ARG;
    double *const rec = static_cast<double *>(work_dev), *const state = rec + (size_t)n_frames * REC;
    const dim3 grid(frame_grid(n_frames)), block(BP_THREADS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(schur_var_frame_kernel, grid, block, 0, s, words_dev, pooled_dev, n_frames, joint_mask, camera_mask, rec);
    hipLaunchKernelGGL(schur_var_reduce_kernel, dim3(1), block, 0, s, rec, pooled_dev, n_frames, camera_mask, state, var_pose_dev);
    hipLaunchKernelGGL(schur_var_back_kernel, grid, block, 0, s, words_dev, pooled_dev, rec, state, n_frames, joint_mask, camera_mask, var_q_dev);
    return launched();
}

extern "C" int rope_bundle_columns_step(const double *pooled_dev, const double *lam_dev, int slot_mask, const double *pose_dev, const double *off_dev,
                                        const double *q0_dev, int n_frames, const double *limits, double *trial_pose_dev, double *trial_off_dev,
                                        double *trial_q_dev, void *stream)
{
    if (n_frames < 1 || !pooled_dev || !lam_dev || !pose_dev || !off_dev || !q0_dev || !trial_pose_dev || !trial_off_dev || !trial_q_dev) return ROPE_E_ARG;
    if (slot_mask < 0 || slot_mask > 4095 || bad_limits(limits)) return ROPE_E_ARG;
    if (misaligned8(pooled_dev) || misaligned8(lam_dev) || misaligned8(pose_dev) || misaligned8(off_dev) || misaligned8(q0_dev) ||
        misaligned8(trial_pose_dev) || misaligned8(trial_off_dev) || misaligned8(trial_q_dev))
        return ROPE_E_ARG;
    hipLaunchKernelGGL(columns_step_kernel, dim3(frame_grid(n_frames)), dim3(BP_THREADS), 0, (hipStream_t)stream, pooled_dev, lam_dev, slot_mask,
                       pose_dev, off_dev, q0_dev, n_frames, JointLimits(limits), trial_pose_dev, trial_off_dev, trial_q_dev);
    return launched();
}

extern "C" int rope_bundle_columns_variance(const double *pooled_dev, int slot_mask, double *var_dev, void *stream)
{
    if (!pooled_dev || !var_dev || slot_mask < 0 || slot_mask > 4095 || misaligned8(pooled_dev) || misaligned8(var_dev)) return ROPE_E_ARG;
    hipLaunchKernelGGL(columns_variance_kernel, dim3(1), dim3(BP_THREADS), 0, (hipStream_t)stream, pooled_dev, slot_mask, var_dev);
    return launched();
}

extern "C" size_t rope_refine_bundle_workspace(rope_ctx *c, int n_frames)
{
    if (!c || !c->have_camera) return 0;
    return bundle_layout(n_frames, c->fp.H, c->fp.W).total;
}

extern "C" int rope_refine_bundle(rope_ctx *c, int mode, const double *camera_pose6, const double *q, const float *frame_depth_dev, int n_frames,
                                  double fx, double fy, double cx, double cy, double znear, double zfar, int joint_mask, int camera_mask,
                                  const double *limits, float clip_m, int iterations, double damping, void *work_dev, double *pose_out,
                                  double *angles_out, double *offsets_out, double *var_pose_out, double *var_joints_out, double *costs_out,
                                  int32_t *steps_out, double *frame_cost_out, double *words_out)
{
    if (!c) return ROPE_E_ARG;
    // everything any part would refuse is refused here, before the first command
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "rope_refine_bundle: robot and camera must be set first");
    if (mode != ROPE_BUNDLE_FRAME && mode != ROPE_BUNDLE_OFFSET) ARG_FAIL(c, "rope_refine_bundle: mode is ROPE_BUNDLE_FRAME or ROPE_BUNDLE_OFFSET");
    if (n_frames < 1 || n_frames > MAX_ROWS) ARG_FAIL(c, "rope_refine_bundle: need 1 <= n_frames <= 65535");
    if (!camera_pose6 || !q || !frame_depth_dev || !work_dev || !pose_out || !angles_out || !offsets_out || !var_pose_out || !var_joints_out ||
        !costs_out || !steps_out || !frame_cost_out)
        ARG_FAIL(c, "rope_refine_bundle: null pointer");
    if (((uintptr_t)frame_depth_dev & 3) || misaligned8(work_dev)) ARG_FAIL(c, "rope_refine_bundle: misaligned device pointer");
    if (bad_mask6(joint_mask) || bad_mask6(camera_mask) || (joint_mask == 0 && camera_mask == 0))
        ARG_FAIL(c, "rope_refine_bundle: joint_mask and camera_mask are 0 .. 63, not both 0");
    if (bad_limits(limits)) ARG_FAIL(c, "rope_refine_bundle: limits must be finite with lo <= hi");
    if (iterations < 0 || !std::isfinite(damping) || damping < 0.0) ARG_FAIL(c, "rope_refine_bundle: iterations and damping must not be negative");
    if (!std::isfinite(clip_m) || !(clip_m > 0.0f)) ARG_FAIL(c, "rope_refine_bundle: clip_m must be finite and positive");
    const float ffx = (float)fx, ffy = (float)fy, fcx = (float)cx, fcy = (float)cy;
    if (!std::isfinite(ffx) || !std::isfinite(ffy) || !std::isfinite(fcx) || !std::isfinite(fcy) || ffx == 0.0f || ffy == 0.0f)
        ARG_FAIL(c, "rope_refine_bundle: camera terms must be finite, fx and fy not 0");
    if (!(znear > 0.0) || !(zfar > znear) || !std::isfinite(zfar)) ARG_FAIL(c, "rope_refine_bundle: need 0 < znear < zfar");
    for (int k = 0; k < 6; k++) if (!std::isfinite(camera_pose6[k])) ARG_FAIL(c, "rope_refine_bundle: camera pose is not finite");
    for (size_t i = 0; i < 6 * (size_t)n_frames; i++)
        if (!std::isfinite(q[i]) || std::fabs(q[i]) > 1.0e4) ARG_FAIL(c, "rope_refine_bundle: joint angle not finite or |q| > 1e4 rad");
    const int H = c->fp.H, W = c->fp.W;
    const BundleLayout l = bundle_layout(n_frames, H, W);
    if (l.total == 0 || n_frames > MAX_ROWS) ARG_FAIL(c, "rope_refine_bundle: too many frames, or pixels, for one call");
    double PV[16];
    if (rope_camera_matrix(camera_pose6, fx, fy, cx, cy, W, H, znear, zfar, PV)) ARG_FAIL(c, "rope_refine_bundle: the camera has no finite matrix");

    unsigned char *const base = static_cast<unsigned char *>(work_dev);
    float *const d_depth = reinterpret_cast<float *>(base + l.depth);
    uint8_t *const d_ids = base + l.ids;
    auto dbl = [base](size_t off) { return reinterpret_cast<double *>(base + off); };
    double *const d_neq = dbl(l.neq), *const d_axes = dbl(l.axes), *const d_twists = dbl(l.twists), *const d_words = dbl(l.words),
                 *const d_words_t = dbl(l.words_t), *const d_pooled = dbl(l.pooled), *const d_pooled_t = dbl(l.pooled_t), *const d_rec = dbl(l.rec),
                 *const d_q0 = dbl(l.q0), *const d_var12 = dbl(l.var12), *const d_trial_off = dbl(l.trial_off), *const d_trial = dbl(l.trial),
                 *const d_trial_pose = dbl(l.trial_pose), *const d_head = dbl(l.head), *const d_q = dbl(l.q), *const d_var = dbl(l.var),
                 *const d_frame_cost = dbl(l.frame_cost);
    const int n_render = std::min(c->n_links, ROPE_MAX_LINKS);
    const int n_joints = joint_mask ? 6 : 0, n_cols = camera_mask ? 6 : 0;
    const bool frame_mode = mode == ROPE_BUNDLE_FRAME;
    const dim3 grid(frame_grid(n_frames)), block(BP_THREADS);
    const size_t row = 6 * (size_t)n_frames * sizeof(double);
    std::vector<double> rows_pv(16 * (size_t)n_frames);

    // render the host rows `at` under the camera `pose`, then the axes, the twists, the equations and their pool on the device
    auto equations = [&](const double *pose, const double *at, const double *at_dev, double *words, double *pooled) -> int {
        double Rwc[9], tc[3];
        BundleTwists tw;
        if (rope_camera_twists(pose, Rwc, tc, tw.v) || rope_camera_matrix(pose, fx, fy, cx, cy, W, H, znear, zfar, PV)) {
            c->err = "rope_refine_bundle: a trial camera pose is not finite";
            return ROPE_E_ARG;
        }
        for (int f = 0; f < n_frames; f++) std::memcpy(rows_pv.data() + 16 * (size_t)f, PV, sizeof PV);
        int rc = rope_render_batch_device(c, at, rows_pv.data(), n_frames, n_render, d_depth, d_ids);
        if (rc) return rc;
        if (n_joints && (rc = rope_joint_axes(c, at_dev, n_frames, Rwc, tc, d_axes, c->stream))) return rc;
        if (n_cols) {
            hipLaunchKernelGGL(tile_twists_kernel, grid, block, 0, c->stream, tw, n_frames, d_twists);
            HIP_TRY(c, hipGetLastError());
        }
        rc = rope_bundle_normal_equations(d_depth, d_ids, frame_depth_dev, n_frames, H, W, n_render, ffx, ffy, fcx, fcy, n_joints ? d_axes : nullptr,
                                          n_joints, n_cols ? d_twists : nullptr, n_cols, clip_m, words, d_neq, c->stream);
        if (!rc) rc = rope_bundle_pool(words, n_frames, pooled, c->stream);
        if (rc) c->err = "rope_refine_bundle: rope_bundle_normal_equations refused the frames";
        return rc;
    };

    HIP_TRY(c, hipSetDevice(c->device));
    int rc = copy_h2d_staged(c, d_q, q, row);
    if (rc) return rc;
    if ((rc = copy_h2d_staged(c, d_q0, q, row))) return rc;
    if ((rc = equations(camera_pose6, q, d_q, d_words, d_pooled))) return rc;
    BundleTwists start{};
    for (int k = 0; k < 6; k++) start.v[k] = camera_pose6[k];
    hipLaunchKernelGGL(bundle_init_kernel, dim3(1), dim3(1), 0, c->stream, d_pooled, start, damping, d_head);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> trial(6 * (size_t)n_frames + 6);
    for (int it = 0; it < iterations; it++) {
        if (frame_mode) {
            rc = rope_bundle_schur_step(d_words, d_pooled, d_q, d_head + HD_POSE, d_head + HD_LAM, n_frames, joint_mask, camera_mask, limits, d_rec,
                                        d_trial, d_trial_pose, c->stream);
            if (!rc) HIP_TRY(c, hipMemcpyAsync(d_trial_off, d_head + HD_OFF, 6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        } else {
            rc = rope_bundle_columns_step(d_pooled, d_head + HD_LAM, joint_mask | (camera_mask << 6), d_head + HD_POSE, d_head + HD_OFF, d_q0,
                                          n_frames, limits, d_trial_pose, d_trial_off, d_trial, c->stream);
        }
        if (rc) {
            c->err = "rope_refine_bundle: the step failed";
            return rc;
        }
        // the round's one wait: the raster path takes host rows.  trial and trial_pose lie next to each other
        if ((rc = copy_d2h_staged(c, trial.data(), d_trial, row + 6 * sizeof(double)))) return rc;
        if ((rc = equations(trial.data() + 6 * (size_t)n_frames, trial.data(), d_trial, d_words_t, d_pooled_t))) return rc;
        hipLaunchKernelGGL(bundle_verdict_kernel, dim3(1), block, 0, c->stream, d_pooled_t, d_trial_pose, d_trial_off, d_pooled, d_head);
        hipLaunchKernelGGL(bundle_take_kernel, grid, block, 0, c->stream, d_head, d_words_t, d_trial, n_frames, d_words, d_q);
        HIP_TRY(c, hipGetLastError());
    }
    if (frame_mode)
        rc = rope_bundle_schur_variance(d_words, d_pooled, n_frames, joint_mask, camera_mask, d_rec, d_var, d_head + HD_VPOSE, c->stream);
    else
        rc = rope_bundle_columns_variance(d_pooled, joint_mask | (camera_mask << 6), d_var12, c->stream);
    if (rc) {
        c->err = "rope_refine_bundle: the variances failed";
        return rc;
    }
    hipLaunchKernelGGL(bundle_finish_kernel, grid, block, 0, c->stream, d_words, d_pooled, frame_mode ? nullptr : d_var12, n_frames, d_head,
                       d_frame_cost);
    HIP_TRY(c, hipGetLastError());
    // one copy for everything the caller gets, and the call is complete when it is down
    const size_t n = (size_t)n_frames, end = words_out ? l.total : l.words;
    std::vector<unsigned char> back(end - l.head);
    if ((rc = copy_d2h_staged(c, back.data(), base + l.head, back.size()))) return rc;
    auto from = [&](size_t off) { return reinterpret_cast<const double *>(back.data() + (off - l.head)); };
    const double *const head = from(l.head);
    std::memcpy(pose_out, head + HD_POSE, 6 * sizeof(double));
    std::memcpy(angles_out, from(l.q), row);
    std::memcpy(var_pose_out, head + HD_VPOSE, 6 * sizeof(double));
    if (frame_mode) {
        for (int k = 0; k < 6; k++) offsets_out[k] = (double)NAN;
        std::memcpy(var_joints_out, from(l.var), row);
    } else {
        std::memcpy(offsets_out, head + HD_OFF, 6 * sizeof(double));
        std::memcpy(var_joints_out, head + HD_VOFF, 6 * sizeof(double));
    }
    costs_out[0] = head[HD_COST0];
    costs_out[1] = head[HD_COST];
    costs_out[2] = head[HD_INL];
    *steps_out = (int32_t)head[HD_STEPS];
    std::memcpy(frame_cost_out, from(l.frame_cost), n * sizeof(double));
    if (words_out) std::memcpy(words_out, from(l.words), n * BW * sizeof(double));
    return ROPE_OK;
}
