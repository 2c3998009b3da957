// rope_bundle.hip — the normal equations of joint angles AND camera pose in one system, for gfx950: rope_bundle_normal_equations takes
// what rope_pose_normal_equations and rope_camera_normal_equations take together (the render at a pose, the frame's depth, the joint
// axes and the camera's twists, both in camera axes) and sums per frame J^T J, J^T r and the residual sums of include/rope_s3d.h over
// twelve column slots: 0 .. 5 the joints, 6 .. 11 the camera's parameters.  The cross block (joint x camera) is what neither of the
// two 6-column calls can give.  Everything is float64 with one IEEE operation per written operation (-ffp-contract=off);
// tests/bundle_ref.py restates the contract in numpy.  The geometry helpers are copies of rope_refine.hip's: that file is untouched.
//
// Shape.  94 sums a pixel do not fit a thread's registers (rope_refine.hip's 31 take 157 VGPRs), so the threads change what they own
// halfway.  A workgroup takes BNEQ_CHUNK consecutive pixels of one frame in 8 passes of 256, as neq_partial_kernel does.  In a pass
//   a) thread t owns pixel p = chunk BNEQ_CHUNK + k 256 + t: it reads the planes, adds words 0 .. 2 to three accumulators of its own and,
//      for an inlier, works out v = (J_0 .. J_11, r);
//   b) the inliers are packed into LDS in pixel order (a ballot and a prefix count per wave, the waves' counts through LDS): row i of
//      s_v is the v of the pass's i-th inlier;
//   c) the threads own WORDS: v_a v_b for a <= b over the 13 entries are 91 sums — 78 of J^T J, 12 of J^T r (b = 12) and r r (a = b =
//      12).  Waves 0 and 1 hold one accumulator each for the first half of the rows, waves 2 and 3 for the second half, and walk their
//      rows in index order: every lane of a wave reads the same row, two LDS reads, one product, one sum.
// Background and outliers cost step (a) alone.  One accumulator a thread: nothing to spill.
//
// Determinism.  No floating-point atomics.  A workgroup's pixels depend on H W alone.  Rows are packed in pixel order, so what a
// word's accumulator adds, and in which order, depends on the planes alone; the two halves are added first + second; words 0 .. 2 go
// through rope_refine.hip's butterfly and the waves in the order 0 .. 3; the workgroup writes ONE partial of ROPE_BNEQ_WORDS doubles,
// and bneq_gather_kernel adds a frame's partials in index order.  No thread leaves before the last barrier.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

constexpr int BNEQ_THREADS = 256;
constexpr int BNEQ_WAVES = BNEQ_THREADS / 64;
constexpr int BNEQ_PER_THREAD = 8;
constexpr int BNEQ_CHUNK = BNEQ_THREADS * BNEQ_PER_THREAD;  // pixels of a workgroup: rope_refine.hip's
constexpr int BNEQ_HALF = 6;                                 // joint slots; as many camera slots
constexpr int BNEQ_SLOTS = 2 * BNEQ_HALF;
constexpr int BNEQ_VEC = BNEQ_SLOTS + 1;                     // J_0 .. J_11 and r
constexpr int BNEQ_PAIRS = BNEQ_VEC * (BNEQ_VEC + 1) / 2;    // 91
constexpr int BNEQ_HEAD = 3;                                 // words 0 .. 2: per-pixel sums that are no product of two entries of v
constexpr int BNEQ_SEG_THREADS = BNEQ_THREADS / 2;           // threads of a half
constexpr int BNEQ_GATHER_FRAMES = 2;                        // frames a gather workgroup

static_assert(ROPE_BNEQ_WORDS == 96 && BNEQ_HEAD + BNEQ_PAIRS + 2 == ROPE_BNEQ_WORDS, "the words of a frame");
static_assert(BNEQ_PAIRS <= BNEQ_SEG_THREADS, "a thread a word in each half");

struct Camera { double fx, fy, cx, cy; };

struct Vec3 { double x, y, z; };

__device__ __forceinline__ Vec3 sub(const Vec3 &a, const Vec3 &b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 cross(const Vec3 &a, const Vec3 &b)
{
    return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot(const Vec3 &a, const Vec3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

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
    if (!(isfinite(n.x) && isfinite(n.y) && isfinite(n.z)) || (n.x == 0.0 && n.y == 0.0 && n.z == 0.0)) return false;      // no normal
    const double nn = dot(n, n), nP = dot(n, P), PP = dot(P, P);
    if (!(nP * nP >= 0.01 * (nn * PP)) || nP == 0.0) return false;                      // grazing

#pragma unroll
    for (int j = 0; j < BNEQ_HALF; j++) {
        v[j] = 0.0;
        if (j < n_joints && j < id) {                                                   // joint j moves the links behind it; the base none
            const Vec3 a = {jf[6 * j], jf[6 * j + 1], jf[6 * j + 2]}, o = {jf[6 * j + 3], jf[6 * j + 4], jf[6 * j + 5]};
            v[j] = (z * dot(n, cross(a, sub(P, o)))) / nP;
        }
        v[BNEQ_HALF + j] = 0.0;
        if (j < n_cols) {                                                               // every column moves every drawn link
            const Vec3 w = {tf[6 * j], tf[6 * j + 1], tf[6 * j + 2]}, u = {tf[6 * j + 3], tf[6 * j + 4], tf[6 * j + 5]};
            const Vec3 c = cross(w, P);
            v[BNEQ_HALF + j] = (z * dot(n, Vec3{c.x + u.x, c.y + u.y, c.z + u.z})) / nP;
        }
    }
    v[BNEQ_SLOTS] = r;
    head[2] += 1.0;
    return true;
}

// Workgroup blockIdx.x = frame * chunks + chunk.
__global__ void __launch_bounds__(BNEQ_THREADS)
bneq_partial_kernel(const float *__restrict__ render, const uint8_t *__restrict__ ids, const float *__restrict__ depth, int H, int W, int chunks,
                    int n_links, Camera cam, const double *__restrict__ joints, int n_joints, const double *__restrict__ twists, int n_cols,
                    double clip, double *__restrict__ work)
{
    __shared__ double s_v[BNEQ_THREADS * BNEQ_VEC];             // the packed inliers of a pass, a row each
    __shared__ double s_head[BNEQ_WAVES][BNEQ_HEAD];
    __shared__ double s_second[BNEQ_PAIRS];                     // the second half's sums
    __shared__ int s_count[BNEQ_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int hw = H * W;                                                               // at most 2^24
    const float *const r0 = render + (size_t)frame * hw;
    const float *const t0 = depth + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    const double *const jf = joints + (size_t)frame * n_joints * 6;                     // never read when its count is 0
    const double *const tf = twists + (size_t)frame * n_cols * 6;
    const double clip2 = clip * clip;

    // the word of this thread in step (c): entries a <= b of v, row by row over the 13, and the word of the frame they belong to
    const int half = t / BNEQ_SEG_THREADS, pair = t - half * BNEQ_SEG_THREADS;
    int a = 0, b = 0;
    if (pair < BNEQ_PAIRS) {
        int w = pair;
        while (w >= BNEQ_VEC - a) { w -= BNEQ_VEC - a; a++; }
        b = a + w;
    }
    const int word = b < BNEQ_SLOTS ? 4 + BNEQ_SLOTS + (a * BNEQ_SLOTS - a * (a - 1) / 2) + (b - a) : (a < BNEQ_SLOTS ? 4 + a : 3);

    double head[BNEQ_HEAD] = {0.0, 0.0, 0.0};
    double acc = 0.0;
    for (int k = 0; k < BNEQ_PER_THREAD; k++) {
        const int p = chunk * BNEQ_CHUNK + k * BNEQ_THREADS + t;
        double v[BNEQ_VEC];
        const bool in = p < hw && bneq_pixel(r0, i0, t0, p, H, W, n_links, cam, jf, n_joints, tf, n_cols, clip, clip2, head, v);
        const unsigned long long m = __ballot(in);
        if (lane == 0) s_count[wave] = __popcll(m);
        __syncthreads();
        int row = __popcll(m & ((1ull << lane) - 1ull)), rows = 0;
#pragma unroll
        for (int w = 0; w < BNEQ_WAVES; w++) {
            const int c = s_count[w];
            if (w < wave) row += c;
            rows += c;
        }
        if (in) {                                                                       // row < rows <= 256
#pragma unroll
            for (int c = 0; c < BNEQ_VEC; c++) s_v[row * BNEQ_VEC + c] = v[c];
        }
        __syncthreads();
        if (pair < BNEQ_PAIRS) {
            const int mid = (rows + 1) >> 1;
            const int first = half ? mid : 0, last = half ? rows : mid;
            for (int i = first; i < last; i++) acc += s_v[i * BNEQ_VEC + a] * s_v[i * BNEQ_VEC + b];
        }
        __syncthreads();                                                                // the next pass writes s_count and s_v again
    }

    // every thread of the workgroup is here with its accumulators defined
#pragma unroll
    for (int j = 0; j < BNEQ_HEAD; j++) {
        double s = head[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0) s_head[wave][j] = s;
    }
    if (half == 1 && pair < BNEQ_PAIRS) s_second[pair] = acc;
    __syncthreads();
    double *const out = work + (size_t)blockIdx.x * ROPE_BNEQ_WORDS;
    if (half == 0) {
        if (pair < BNEQ_PAIRS) out[word] = acc + s_second[pair];                        // words 3 .. 93, each once
    } else if (pair < BNEQ_HEAD) {
        double s = s_head[0][pair];
#pragma unroll
        for (int w = 1; w < BNEQ_WAVES; w++) s += s_head[w][pair];
        out[pair] = s;
    } else if (pair < BNEQ_HEAD + 2) {
        out[ROPE_BNEQ_WORDS - 2 + (pair - BNEQ_HEAD)] = 0.0;
    }
}

// Thread t of workgroup b: word t % 96 of frame 2 b + t / 96, the partials of the frame added in index order.
__global__ void __launch_bounds__(BNEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS)
bneq_gather_kernel(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    const int frame = blockIdx.x * BNEQ_GATHER_FRAMES + (int)(threadIdx.x / ROPE_BNEQ_WORDS);
    const int word = threadIdx.x % ROPE_BNEQ_WORDS;
    if (frame >= n_frames) return;
    const double *const w = work + (size_t)frame * chunks * ROPE_BNEQ_WORDS + word;
    double s = w[0];
    for (int c = 1; c < chunks; c++) s += w[(size_t)c * ROPE_BNEQ_WORDS];
    out[(size_t)frame * ROPE_BNEQ_WORDS + word] = s;
}

// chunks of a frame, or 0 when the shape is refused: rope_refine.hip's rule
long long bneq_chunks(int n_frames, int H, int W)
{
    if (n_frames < 1 || H < 1 || W < 1) return 0;
    const long long hw = (long long)H * (long long)W;
    if (hw > (1ll << 24)) return 0;
    const long long chunks = (hw + BNEQ_CHUNK - 1) / BNEQ_CHUNK;
    if ((long long)n_frames * chunks >= (1ll << 24)) return 0;                          // a grid holds fewer than 2^32 threads
    return chunks;
}

}  // namespace

extern "C" size_t rope_bundle_normal_workspace(int n_frames, int H, int W)
{
    return (size_t)n_frames * (size_t)bneq_chunks(n_frames, H, W) * ROPE_BNEQ_WORDS * sizeof(double);
}

extern "C" int rope_bundle_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames,
                                            int H, int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev, int n_joints,
                                            const double *twists_dev, int n_cols, float clip_m, double *out_dev, double *work_dev, void *stream)
{
    if (n_links < 1 || n_links > ROPE_MAX_LINKS) return ROPE_E_ARG;
    if (n_joints < 0 || n_joints > BNEQ_HALF || n_cols < 0 || n_cols > BNEQ_HALF || n_joints + n_cols < 1) return ROPE_E_ARG;
    if (!isfinite(clip_m) || !(clip_m > 0.0f)) return ROPE_E_ARG;
    if (!isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy) || fx == 0.0f || fy == 0.0f) return ROPE_E_ARG;
    if (!render_depth_dev || !render_ids_dev || !frame_depth_dev || !out_dev || !work_dev) return ROPE_E_ARG;
    if ((n_joints > 0 && !joints_dev) || (n_cols > 0 && !twists_dev)) return ROPE_E_ARG;
    if (((uintptr_t)render_depth_dev & 3) || ((uintptr_t)frame_depth_dev & 3)) return ROPE_E_ARG;
    if ((n_joints > 0 && ((uintptr_t)joints_dev & 7)) || (n_cols > 0 && ((uintptr_t)twists_dev & 7))) return ROPE_E_ARG;
    if (((uintptr_t)out_dev & 7) || ((uintptr_t)work_dev & 7)) return ROPE_E_ARG;
    const long long chunks = bneq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    const Camera cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    hipLaunchKernelGGL(bneq_partial_kernel, dim3((unsigned)((long long)n_frames * chunks)), dim3(BNEQ_THREADS), 0, st, render_depth_dev,
                       render_ids_dev, frame_depth_dev, H, W, (int)chunks, n_links, cam, n_joints > 0 ? joints_dev : nullptr, n_joints,
                       n_cols > 0 ? twists_dev : nullptr, n_cols, (double)clip_m, work_dev);
    if (hipGetLastError() != hipSuccess) return ROPE_E_HIP;
    hipLaunchKernelGGL(bneq_gather_kernel, dim3((unsigned)((n_frames + BNEQ_GATHER_FRAMES - 1) / BNEQ_GATHER_FRAMES)),
                       dim3(BNEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS), 0, st, work_dev, n_frames, (int)chunks, out_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
