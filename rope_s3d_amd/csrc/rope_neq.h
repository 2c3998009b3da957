// rope_neq.h — what the normal-equation files (rope_refine.hip, rope_bundle.hip, rope_silhouette.hip,
// rope_silhouette_reverse.hip, rope_robust.hip) have in common, once:
// the camera and vector helpers, the depth surface of a pixel, the velocity of a surface point per unit of a column and the two ways
// it becomes an entry of J, the workgroup shape and the chunk rule, the gather body, the pack-and-own-words body of the twelve-slot
// kernels, and the host checks every entry point makes.  Everything is float64 with one IEEE operation per written operation
// (-ffp-contract=off), and every expression below is part of a contract that tests/test_gpu_neq_terms.py holds bit for bit: the
// parentheses and the order of the operations are not style.  Each file keeps what is particular to its term.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

// ---------------------------------------------------------------------------------------------- shape
// A workgroup takes NEQ_CHUNK consecutive pixels of one frame in NEQ_PER_THREAD passes of NEQ_THREADS: pixel
// p = chunk NEQ_CHUNK + k NEQ_THREADS + t for thread t in pass k, so a wave's loads are consecutive.
constexpr int NEQ_THREADS = 256;
constexpr int NEQ_WAVES = NEQ_THREADS / 64;
constexpr int NEQ_PER_THREAD = 8;
constexpr int NEQ_CHUNK = NEQ_THREADS * NEQ_PER_THREAD;      // pixels of a workgroup
constexpr int NEQ_JOINTS = 6;                                // columns of a group: the joint slots, and as many camera slots
constexpr int NEQ_GATHER_FRAMES = 2;                         // frames a gather workgroup
// the twelve-slot layout (ROPE_BNEQ_WORDS): v = (J_0 .. J_11, residual) a pixel, and the products v_a v_b for a <= b
constexpr int BNEQ_SLOTS = 2 * NEQ_JOINTS;
constexpr int BNEQ_VEC = BNEQ_SLOTS + 1;
constexpr int BNEQ_PAIRS = BNEQ_VEC * (BNEQ_VEC + 1) / 2;    // 91
constexpr int BNEQ_HEAD = 3;                                 // words 0 .. 2: per-pixel sums that are no product of two entries of v
constexpr int BNEQ_SEG_THREADS = NEQ_THREADS / 2;            // threads of a half

static_assert(ROPE_BNEQ_WORDS == 96 && BNEQ_HEAD + BNEQ_PAIRS + 2 == ROPE_BNEQ_WORDS, "the words of a frame");
static_assert(BNEQ_PAIRS <= BNEQ_SEG_THREADS, "a thread a word in each half");

// chunks of a frame, or 0 when the shape is refused
inline long long neq_chunks(int n_frames, int H, int W)
{
    if (n_frames < 1 || H < 1 || W < 1) return 0;
    const long long hw = (long long)H * (long long)W;
    if (hw > (1ll << 24)) return 0;
    const long long chunks = (hw + NEQ_CHUNK - 1) / NEQ_CHUNK;
    if ((long long)n_frames * chunks >= (1ll << 24)) return 0;                          // a grid holds fewer than 2^32 threads: 2^24 workgroups of 256
    return chunks;
}

// bytes of a call's workspace: one partial of `words` doubles a workgroup; 0 when the shape is refused
inline size_t neq_workspace(int n_frames, int H, int W, int words)
{
    return (size_t)n_frames * (size_t)neq_chunks(n_frames, H, W) * (size_t)words * sizeof(double);
}

inline unsigned neq_gather_grid(int n_frames) { return (unsigned)((n_frames + NEQ_GATHER_FRAMES - 1) / NEQ_GATHER_FRAMES); }

// ---------------------------------------------------------------------------------------------- host checks
// What every entry point refuses whatever its term: the links, the camera terms, a null or misaligned plane, `out` or `work`.
// `plane3`: the frame's depth or the distance field, four bytes a pixel as the render's depth.
inline bool neq_bad_args(int n_links, float fx, float fy, float cx, float cy, const float *render_depth, const uint8_t *render_ids, const void *plane3,
                         const double *out, const double *work)
{
    if (n_links < 1 || n_links > ROPE_MAX_LINKS) return true;
    if (!isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy) || fx == 0.0f || fy == 0.0f) return true;
    if (!render_depth || !render_ids || !plane3 || !out || !work) return true;
    if (((uintptr_t)render_depth & 3) || ((uintptr_t)plane3 & 3)) return true;
    return ((uintptr_t)out & 7) || ((uintptr_t)work & 7);
}

// The columns of a twelve-slot call: either group may be absent (count 0, its pointer then unused), not both
inline bool neq_bad_columns12(const double *joints, int n_joints, const double *twists, int n_cols)
{
    if (n_joints < 0 || n_joints > NEQ_JOINTS || n_cols < 0 || n_cols > NEQ_JOINTS || n_joints + n_cols < 1) return true;
    if ((n_joints > 0 && !joints) || (n_cols > 0 && !twists)) return true;
    return (n_joints > 0 && ((uintptr_t)joints & 7)) || (n_cols > 0 && ((uintptr_t)twists & 7));
}

// ---------------------------------------------------------------------------------------------- geometry
struct Camera { double fx, fy, cx, cy; };

struct Vec3 { double x, y, z; };

__device__ __forceinline__ Vec3 vec3_at(const double *p) { return Vec3{p[0], p[1], p[2]}; }
__device__ __forceinline__ Vec3 sub(const Vec3 &a, const Vec3 &b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 cross(const Vec3 &a, const Vec3 &b)
{
    return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot(const Vec3 &a, const Vec3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// The depth surface at pixel p = (x, y) of a frame's render (r0 depth, i0 link ids), the pixel drawn at depth z by link id: the
// point P, the normal n from one-sided differences to the neighbours of the same link (+1 before -1, on either axis) and n . P.
// false: no normal (a difference missing on an axis, or not finite), or a surface seen at grazing incidence.
__device__ __forceinline__ bool depth_surface(const float *r0, const uint8_t *i0, int p, int x, int y, int H, int W, int id,
                                              double z, const Camera &cam, Vec3 &P, Vec3 &n, double &nP)
{
    const double kx = ((double)x - cam.cx) / cam.fx, ky = ((double)y - cam.cy) / cam.fy;
    P = Vec3{kx * z, ky * z, z};
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
    n = cross(dX, dY);
    const bool no_normal = !(isfinite(n.x) && isfinite(n.y) && isfinite(n.z)) || (n.x == 0.0 && n.y == 0.0 && n.z == 0.0);
    const double nn = dot(n, n);
    nP = dot(n, P);
    const double PP = dot(P, P);
    // one exit: with a return of its own for "no normal" neq_partial_kernel takes two registers and four instructions more
    return !(no_normal || !(nP * nP >= 0.01 * (nn * PP)) || nP == 0.0);                 // the second and third: grazing (a NaN too)
}

// The velocity of the surface point P per unit of a column: a joint with axis a through the point o, a twist (w, v) of the camera
__device__ __forceinline__ Vec3 joint_velocity(const Vec3 &a, const Vec3 &o, const Vec3 &P) { return cross(a, sub(P, o)); }
__device__ __forceinline__ Vec3 twist_velocity(const Vec3 &w, const Vec3 &v, const Vec3 &P)
{
    const Vec3 c = cross(w, P);
    return Vec3{c.x + v.x, c.y + v.y, c.z + v.z};
}
// column j of a frame's joints (axis, point) or twists (w, v), six doubles a column
__device__ __forceinline__ Vec3 joint_velocity(const double *jf, int j, const Vec3 &P)
{
    return joint_velocity(vec3_at(jf + 6 * j), vec3_at(jf + 6 * j + 3), P);
}
__device__ __forceinline__ Vec3 twist_velocity(const double *tf, int j, const Vec3 &P)
{
    return twist_velocity(vec3_at(tf + 6 * j), vec3_at(tf + 6 * j + 3), P);
}

// What a velocity u is in J.  Depth: the rendered depth at a fixed pixel changes by z (n . u) / (n . P).  Silhouette: the point's
// image moves by (vx, vy) pixels, along which the distance field has the slope (gx, gy); kx, ky are the pixel's ray, P = (kx z, ky z, z).
__device__ __forceinline__ double depth_column(double z, const Vec3 &n, double nP, const Vec3 &u) { return (z * dot(n, u)) / nP; }
__device__ __forceinline__ double silhouette_column(double gx, double gy, const Camera &cam, double kx, double ky, double z, const Vec3 &u)
{
    const double vx = (cam.fx * (u.x - kx * u.z)) / z, vy = (cam.fy * (u.y - ky * u.z)) / z;
    return gx * vx + gy * vy;
}

// The thirteen entries v = (J_0 .. J_11, r) of an inlier pixel of the DEPTH term over twelve slots (rope_bundle.hip and
// rope_robust.hip): the pixel on link id at depth z with the surface (P, n, nP) and the residual r; jf, tf the frame's joints and twists.
__device__ __forceinline__ void bneq_depth_columns(const double *__restrict__ jf, int n_joints, const double *__restrict__ tf, int n_cols, int id,
                                                   double z, const Vec3 &P, const Vec3 &n, double nP, double r, double (&v)[BNEQ_VEC])
{
#pragma unroll
    for (int j = 0; j < NEQ_JOINTS; j++) {
        v[j] = 0.0;
        if (j < n_joints && j < id) v[j] = depth_column(z, n, nP, joint_velocity(jf, j, P));       // joint j moves the links behind it; the base none
        v[NEQ_JOINTS + j] = 0.0;
        if (j < n_cols) v[NEQ_JOINTS + j] = depth_column(z, n, nP, twist_velocity(tf, j, P));      // every column moves every drawn link
    }
    v[BNEQ_SLOTS] = r;
}

// The outline terms' phi (rope_silhouette.hip, rope_silhouette_reverse.hip): the signed distance to the boundary in pixels, from a
// distance field's integer (rope_mask_distance); beyond the truncation it is that of FAR, far2 = R R + 1
__device__ __forceinline__ double sil_phi(int32_t sd, int far2)
{
    const long long a = sd < 0 ? -(long long)sd : (long long)sd;
    const int m = a > far2 ? far2 : (int)a;
    const double d = sqrt((double)m) - 0.5;
    return sd < 0 ? -d : d;
}

// ---------------------------------------------------------------------------------------------- the gather
// Thread t of workgroup b: word t % WORDS of frame NEQ_GATHER_FRAMES b + t / WORDS, the partials of the frame added in index order.
template <int WORDS>
__device__ __forceinline__ void neq_gather(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    const int frame = blockIdx.x * NEQ_GATHER_FRAMES + (int)(threadIdx.x / WORDS);
    const int word = threadIdx.x % WORDS;
    if (frame >= n_frames) return;
    const double *const w = work + (size_t)frame * chunks * WORDS + word;
    double s = w[0];
    for (int c = 1; c < chunks; c++) s += w[(size_t)c * WORDS];
    out[(size_t)frame * WORDS + word] = s;
}

// ---------------------------------------------------------------------------------------------- pack and own words
// The body of a twelve-slot partial kernel.  94 sums a pixel do not fit a thread's registers (rope_refine.hip's 31 take 157 VGPRs),
// so the threads change what they own halfway.  In each of the 8 passes over the workgroup's chunk (`chunk` of a frame of hw pixels)
//   a) thread t owns a pixel p: pixel(p, head, v) adds the pixel's share of words 0 .. 2 to the thread's `head` and, for an inlier,
//      fills v = (J_0 .. J_11, residual) and returns true;
//   b) the inliers are packed into LDS in pixel order (a ballot and a prefix count per wave, the waves' counts through LDS): row i of
//      s_v is the v of the pass's i-th inlier;
//   c) the threads own WORDS: v_a v_b for a <= b over the 13 entries are 91 sums — 78 of J^T J, 12 of J^T r (b = 12) and r r (a = b =
//      12).  Waves 0 and 1 hold one accumulator each for the first half of the rows, waves 2 and 3 for the second half, and walk their
//      rows in index order: every lane of a wave reads the same row, two LDS reads, one product, one sum.
// Pixels that are no inliers cost step (a) alone.  One accumulator a thread: nothing to spill.
// Determinism.  Rows are packed in pixel order, so what a word's accumulator adds, and in which order, depends on the planes alone;
// the two halves are added first + second; words 0 .. 2 go through a butterfly (xor 32 .. 1) and the waves in the order 0 .. 3; the
// workgroup writes ONE partial of ROPE_BNEQ_WORDS doubles to `out`.  No thread leaves before the last barrier.
template <typename Pixel>
__device__ __forceinline__ void bneq_pack_and_own_words(int hw, int chunk, const Pixel &pixel, double *__restrict__ out)
{
    __shared__ double s_v[NEQ_THREADS * BNEQ_VEC];              // the packed inliers of a pass, a row each
    __shared__ double s_head[NEQ_WAVES][BNEQ_HEAD];
    __shared__ double s_second[BNEQ_PAIRS];                     // the second half's sums
    __shared__ int s_count[NEQ_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

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
    for (int k = 0; k < NEQ_PER_THREAD; k++) {
        const int p = chunk * NEQ_CHUNK + k * NEQ_THREADS + t;
        double v[BNEQ_VEC];
        const bool in = p < hw && pixel(p, head, v);
        const unsigned long long m = __ballot(in);
        if (lane == 0) s_count[wave] = __popcll(m);
        __syncthreads();
        int row = __popcll(m & ((1ull << lane) - 1ull)), rows = 0;
#pragma unroll
        for (int w = 0; w < NEQ_WAVES; w++) {
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
    if (half == 0) {
        if (pair < BNEQ_PAIRS) out[word] = acc + s_second[pair];                        // words 3 .. 93, each once
    } else if (pair < BNEQ_HEAD) {
        double s = s_head[0][pair];
#pragma unroll
        for (int w = 1; w < NEQ_WAVES; w++) s += s_head[w][pair];
        out[pair] = s;
    } else if (pair < BNEQ_HEAD + 2) {
        out[ROPE_BNEQ_WORDS - 2 + (pair - BNEQ_HEAD)] = 0.0;
    }
}

}  // namespace
