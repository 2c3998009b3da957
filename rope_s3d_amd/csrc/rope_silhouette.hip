// rope_silhouette.hip — the outline term of render-and-compare for gfx950, in two calls of include/rope_s3d.h:
//   rope_mask_distance                 the truncated signed squared distance of every pixel to its mask's boundary, exact integers;
//   rope_silhouette_normal_equations   per frame J^T J, J^T e and the residual sums of the render's CONTOUR pixels against that field,
//                                      over rope_bundle_normal_equations' twelve column slots and in its 96-word layout.
// Everything floating is float64 with one IEEE operation per written operation (-ffp-contract=off); tests/silhouette_ref.py restates
// both contracts in numpy.  The normal-equation half holds what is particular to the outline term, sneq_pixel; the vector helpers,
// the columns' velocities and the body of the kernel are rope_bundle.hip's as well and live in rope_neq.h, and so does sil_phi, which
// rope_silhouette_reverse.hip (the mask's outline against a field of the render) reads its field through as well.
//
// Distance.  A workgroup takes a tile of 32 x 32 pixels of one plane.  With R <= 16 the tile and its halo are 64 columns wide: a row
// of it is ONE 64-bit word.  Each wave reads rows of 64 mask bytes, a lane a byte, and two ballots turn the row into the word of its
// inside pixels and the word of its outside pixels (a pixel beyond the image is in neither: the image edge is no boundary).  A thread
// then walks the 2 R + 1 rows about its pixel: in the word of the OTHER state the nearest set bit to the left and to the right of its
// column are one count of leading and one of trailing zeros, so a row costs a handful of integer operations whatever R is, and
// m = min over the rows of dy^2 + dx^2.  All lanes of a half wave read the same word of LDS (a broadcast).  No floating point at all.
//
// Normal equations.  The shape is bneq_partial_kernel's (bneq_pack_and_own_words, rope_neq.h): a workgroup takes NEQ_CHUNK
// consecutive pixels of a frame in 8 passes of 256; a thread classifies its pixel (contour pixels are a perimeter, a few in a hundred), adds words 0 .. 2 to accumulators of its
// own and, for an inlier, works out v = (J_0 .. J_11, e); the inliers of a pass are packed into LDS in pixel order (a ballot and a
// prefix count per wave, the waves' counts through LDS); then the threads own WORDS, v_a v_b for a <= b over the 13 entries, the two
// halves of the workgroup half of the rows each.  Background and interior pixels cost the classification alone.
//
// Determinism.  No floating-point atomics.  A workgroup's pixels depend on H W alone; rows are packed in pixel order; the halves are
// added first + second; words 0 .. 2 go through a butterfly and the waves in the order 0 .. 3; the workgroup writes ONE partial of
// ROPE_BNEQ_WORDS doubles and sneq_gather_kernel adds a frame's partials in index order.  No thread leaves before the last barrier.
#include "rope_neq.h"

namespace {

// ---------------------------------------------------------------------------------------------- the distance field
constexpr int MD_THREADS = 256;
constexpr int MD_WAVES = MD_THREADS / 64;
constexpr int MD_TILE = 32;                                  // output pixels a side
constexpr int MD_HALO = ROPE_SIL_MAX_RADIUS;
constexpr int MD_SPAN = MD_TILE + 2 * MD_HALO;               // rows and columns of the tile with its halo
constexpr int MD_MAX_PLANES_Y = 32768;                       // gridDim.y; more planes are walked by the workgroups

static_assert(MD_SPAN == 64, "a row of the tile with its halo is one ballot");
static_assert(MD_THREADS % MD_TILE == 0 && MD_TILE % (MD_THREADS / MD_TILE) == 0, "a thread a column, whole passes of rows");

// Workgroup (blockIdx.x, blockIdx.y): tile blockIdx.x of the planes blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ void __launch_bounds__(MD_THREADS)
mask_distance_kernel(const uint8_t *__restrict__ mask, int n_planes, int H, int W, int tiles_x, int R, int32_t *__restrict__ sd2)
{
    __shared__ unsigned long long s_in[MD_SPAN], s_out[MD_SPAN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
    const long long y0 = (long long)tile_y * MD_TILE, x0 = (long long)tile_x * MD_TILE;     // H W < 2^31, H + 64 may not fit an int
    const size_t hw = (size_t)H * (size_t)W;
    const int far2 = R * R + 1;
    const int tx = t & (MD_TILE - 1), c = MD_HALO + tx;
    for (int plane = blockIdx.y; plane < n_planes; plane += gridDim.y) {
        const uint8_t *const m0 = mask + (size_t)plane * hw;
        for (int r = MD_HALO - R + wave; r < MD_HALO + MD_TILE + R; r += MD_WAVES) {       // the rows a pixel of the tile can ask for
            const long long y = y0 - MD_HALO + r, x = x0 - MD_HALO + lane;
            const bool inside = y >= 0 && y < H && x >= 0 && x < W;
            const bool on = inside && m0[(size_t)y * (size_t)W + (size_t)x] != 0;
            const unsigned long long bi = __ballot(on), bo = __ballot(inside && !on);
            if (lane == 0) {
                s_in[r] = bi;
                s_out[r] = bo;
            }
        }
        __syncthreads();
        for (int ty = t / MD_TILE; ty < MD_TILE; ty += MD_THREADS / MD_TILE) {
            const long long y = y0 + ty, x = x0 + tx;
            if (y < H && x < W) {
                const bool v = (s_in[MD_HALO + ty] >> c) & 1ull;
                int m = far2;
                for (int dy = -R; dy <= R; dy++) {
                    const int r = MD_HALO + ty + dy;                                        // 0 .. 63
                    const unsigned long long w = v ? s_out[r] : s_in[r];                    // the pixels of the other state in that row
                    const unsigned long long right = w >> c, left = w << (63 - c);          // bit 0 / bit 63: the pixel's own column
                    int d = 2 * MD_SPAN;
                    if (right) d = __builtin_ctzll(right);
                    if (left) {
                        const int dl = __builtin_clzll(left);
                        d = dl < d ? dl : d;
                    }
                    const int q = dy * dy + d * d;
                    m = q < m ? q : m;                                                      // |dx| > R gives q > R R: it never wins
                }
                sd2[(size_t)plane * hw + (size_t)y * (size_t)W + (size_t)x] = v ? -m : m;
            }
        }
        __syncthreads();                                                                    // the next plane writes the words again
    }
}

// ---------------------------------------------------------------------------------------------- the normal equations
// Pixel p of a frame: adds its share of words 0 .. 2 to head and, for an inlier, fills v and returns true.
__device__ __forceinline__ bool sneq_pixel(const float *__restrict__ r0, const uint8_t *__restrict__ i0, const int32_t *__restrict__ d0, int p, int H,
                                           int W, int n_links, const Camera &cam, const double *__restrict__ jf, int n_joints,
                                           const double *__restrict__ tf, int n_cols, int near2, double (&head)[BNEQ_HEAD], double (&v)[BNEQ_VEC])
{
    const int id = i0[p];
    if (id >= n_links) return false;                                                    // not rendered
    const int y = p / W, x = p - y * W;
    const bool left = x > 0, right = x + 1 < W, up = y > 0, down = y + 1 < H;
    const bool contour = (left && i0[p - 1] >= n_links) || (right && i0[p + 1] >= n_links) || (up && i0[p - W] >= n_links) ||
                         (down && i0[p + W] >= n_links);                                // the frame's edge is no outline
    if (!contour) return false;
    const int far2 = near2 + 1;
    const int32_t sd = d0[p];
    const double phi = sil_phi(sd, far2);
    const double e = phi + 0.5;
    head[0] += 1.0;
    head[1] += e * e;
    if (!(sd <= near2 && sd >= -near2)) return false;                                   // beyond the truncation

    double gx = 0.0, gy = 0.0;
    if (left && right) gx = (sil_phi(d0[p + 1], far2) - sil_phi(d0[p - 1], far2)) / 2.0;
    else if (right) gx = sil_phi(d0[p + 1], far2) - phi;
    else if (left) gx = phi - sil_phi(d0[p - 1], far2);
    if (up && down) gy = (sil_phi(d0[p + W], far2) - sil_phi(d0[p - W], far2)) / 2.0;
    else if (down) gy = sil_phi(d0[p + W], far2) - phi;
    else if (up) gy = phi - sil_phi(d0[p - W], far2);

    const double z = (double)r0[p];
    const double kx = ((double)x - cam.cx) / cam.fx, ky = ((double)y - cam.cy) / cam.fy;
    const Vec3 P = {kx * z, ky * z, z};
#pragma unroll
    for (int j = 0; j < NEQ_JOINTS; j++) {
        v[j] = 0.0;
        if (j < n_joints && j < id) v[j] = silhouette_column(gx, gy, cam, kx, ky, z, joint_velocity(jf, j, P));    // joint j moves the links behind it
        v[NEQ_JOINTS + j] = 0.0;
        if (j < n_cols) v[NEQ_JOINTS + j] = silhouette_column(gx, gy, cam, kx, ky, z, twist_velocity(tf, j, P));   // every column moves every drawn link
    }
    v[BNEQ_SLOTS] = e;
    head[2] += 1.0;
    return true;
}

// Workgroup blockIdx.x = frame * chunks + chunk.
__global__ void __launch_bounds__(NEQ_THREADS)
sneq_partial_kernel(const float *__restrict__ render, const uint8_t *__restrict__ ids, const int32_t *__restrict__ sd2, int H, int W, int chunks,
                    int n_links, Camera cam, const double *__restrict__ joints, int n_joints, const double *__restrict__ twists, int n_cols,
                    int near2, double *__restrict__ work)
{
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int hw = H * W;                                                               // at most 2^24
    const float *const r0 = render + (size_t)frame * hw;
    const int32_t *const d0 = sd2 + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    const double *const jf = joints + (size_t)frame * n_joints * 6;                     // never read when its count is 0
    const double *const tf = twists + (size_t)frame * n_cols * 6;
    bneq_pack_and_own_words(hw, chunk, [&](int p, double (&head)[BNEQ_HEAD], double (&v)[BNEQ_VEC]) {
        return sneq_pixel(r0, i0, d0, p, H, W, n_links, cam, jf, n_joints, tf, n_cols, near2, head, v);
    }, work + (size_t)blockIdx.x * ROPE_BNEQ_WORDS);
}

// a frame's partials added in index order, two frames a workgroup (rope_neq.h)
__global__ void __launch_bounds__(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS)
sneq_gather_kernel(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    neq_gather<ROPE_BNEQ_WORDS>(work, n_frames, chunks, out);
}

}  // namespace

extern "C" int rope_mask_distance(const uint8_t *mask_dev, int N, int H, int W, int radius, int32_t *sd2_dev, void *stream)
{
    if (N < 0 || H < 1 || W < 1 || (long long)H * (long long)W >= (1ll << 31)) return ROPE_E_ARG;
    if (radius < 1 || radius > ROPE_SIL_MAX_RADIUS) return ROPE_E_ARG;
    if (N > 0 && (!mask_dev || !sd2_dev || ((uintptr_t)sd2_dev & 3))) return ROPE_E_ARG;
    if (N == 0) return ROPE_OK;
    const long long tiles_x = ((long long)W + MD_TILE - 1) / MD_TILE, tiles_y = ((long long)H + MD_TILE - 1) / MD_TILE;    // their product < 2^27
    hipLaunchKernelGGL(mask_distance_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)(N < MD_MAX_PLANES_Y ? N : MD_MAX_PLANES_Y)),
                       dim3(MD_THREADS), 0, (hipStream_t)stream, mask_dev, N, H, W, (int)tiles_x, radius, sd2_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" size_t rope_silhouette_normal_workspace(int n_frames, int H, int W)
{
    return neq_workspace(n_frames, H, W, ROPE_BNEQ_WORDS);
}

extern "C" int rope_silhouette_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const int32_t *sd2_dev, int n_frames,
                                                int H, int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev,
                                                int n_joints, const double *twists_dev, int n_cols, int radius, double *out_dev, double *work_dev,
                                                void *stream)
{
    if (neq_bad_args(n_links, fx, fy, cx, cy, render_depth_dev, render_ids_dev, sd2_dev, out_dev, work_dev)) return ROPE_E_ARG;
    if (neq_bad_columns12(joints_dev, n_joints, twists_dev, n_cols)) return ROPE_E_ARG;
    if (radius < 1 || radius > ROPE_SIL_MAX_RADIUS) return ROPE_E_ARG;
    const long long chunks = neq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    const Camera cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    hipLaunchKernelGGL(sneq_partial_kernel, dim3((unsigned)((long long)n_frames * chunks)), dim3(NEQ_THREADS), 0, st, render_depth_dev,
                       render_ids_dev, sd2_dev, H, W, (int)chunks, n_links, cam, n_joints > 0 ? joints_dev : nullptr, n_joints,
                       n_cols > 0 ? twists_dev : nullptr, n_cols, radius * radius, work_dev);
    if (hipGetLastError() != hipSuccess) return ROPE_E_HIP;
    hipLaunchKernelGGL(sneq_gather_kernel, dim3(neq_gather_grid(n_frames)), dim3(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS), 0, st, work_dev, n_frames,
                       (int)chunks, out_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
