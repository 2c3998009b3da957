// rope_silhouette_reverse.hip — the outline term's SECOND direction for gfx950, in two calls of include/rope_s3d.h:
//   rope_render_nearest                        for every pixel of a render's id plane the nearest pixel of the other state (rendered /
//                                              not rendered) as one int16 code, exact integers: rope_mask_distance's field of the
//                                              render's coverage and, with it, WHERE that distance is reached;
//   rope_silhouette_normal_equations_reverse   per frame J^T J, J^T e and the residual sums of the MASK's contour pixels against that
//                                              field of the render, over the twelve column slots and in the 96-word layout of
//                                              rope_silhouette_normal_equations, so that the two directions' words add.
// rope_silhouette.hip measures the render's outline against a field of the mask, made once; here the mask's outline is measured
// against a field of the render, made every round — hence two bytes a pixel and no mask plane in between.  The file is a sibling and
// not a template over rope_silhouette.hip's kernels: those keep their machine code.  tests/silhouette_reverse_ref.py restates both
// contracts in numpy.  Everything floating is float64 with one IEEE operation per written operation (-ffp-contract=off).
//
// Nearest.  mask_distance_kernel's structure: a workgroup takes a tile of 32 x 32 pixels of one plane, the tile with its halo of 16 is
// 64 columns wide, a row of it ONE 64-bit ballot word of the rendered pixels and one of the unrendered ones (a pixel beyond the image
// is in neither), and a thread walks the 2 R + 1 rows about its pixel with one count of leading and one of trailing zeros a row.
// The TIE-BREAK among the pixels at the least distance is the first in raster order, smallest y, then smallest x, and it comes from
// two rules below: the rows are scanned from dy = -R upward and a row replaces the best so far only when it is STRICTLY nearer; in
// a row the left bit is taken when it is as near as the right one.  tests/test_silhouette_reverse_refs.py pins it.  Integers only.
//
// Normal equations.  bneq_pack_and_own_words (rope_neq.h) with rneq_pixel in sneq_pixel's place, and neq_gather: the shape, the
// determinism and the workspace are the forward term's.
#include "rope_neq.h"

namespace {

// ---------------------------------------------------------------------------------------------- the nearest pixel of the other state
constexpr int RN_THREADS = 256;
constexpr int RN_WAVES = RN_THREADS / 64;
constexpr int RN_TILE = 32;                                  // output pixels a side
constexpr int RN_HALO = ROPE_SIL_MAX_RADIUS;
constexpr int RN_SPAN = RN_TILE + 2 * RN_HALO;               // rows and columns of the tile with its halo
constexpr int RN_MAX_PLANES_Y = 32768;                       // gridDim.y; more planes are walked by the workgroups
constexpr int RN_CODE_SIDE = 2 * ROPE_SIL_MAX_RADIUS + 1;    // 33: code = (dy + 16) 33 + (dx + 16)

static_assert(RN_SPAN == 64, "a row of the tile with its halo is one ballot");
static_assert(RN_THREADS % RN_TILE == 0 && RN_TILE % (RN_THREADS / RN_TILE) == 0, "a thread a column, whole passes of rows");
static_assert(RN_CODE_SIDE * RN_CODE_SIDE - 1 == ROPE_SIL_NEAREST_MAX, "the largest code");

// Workgroup (blockIdx.x, blockIdx.y): tile blockIdx.x of the planes blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ void __launch_bounds__(RN_THREADS)
render_nearest_kernel(const uint8_t *__restrict__ ids, int n_planes, int H, int W, int tiles_x, int n_links, int R, int16_t *__restrict__ near)
{
    __shared__ unsigned long long s_in[RN_SPAN], s_out[RN_SPAN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
    const long long y0 = (long long)tile_y * RN_TILE, x0 = (long long)tile_x * RN_TILE;     // H W < 2^31, H + 64 may not fit an int
    const size_t hw = (size_t)H * (size_t)W;
    const int far2 = R * R + 1;
    const int tx = t & (RN_TILE - 1), c = RN_HALO + tx;
    for (int plane = blockIdx.y; plane < n_planes; plane += gridDim.y) {
        const uint8_t *const i0 = ids + (size_t)plane * hw;
        for (int r = RN_HALO - R + wave; r < RN_HALO + RN_TILE + R; r += RN_WAVES) {       // the rows a pixel of the tile can ask for
            const long long y = y0 - RN_HALO + r, x = x0 - RN_HALO + lane;
            const bool inside = y >= 0 && y < H && x >= 0 && x < W;
            const bool on = inside && (int)i0[(size_t)y * (size_t)W + (size_t)x] < n_links;
            const unsigned long long bi = __ballot(on), bo = __ballot(inside && !on);
            if (lane == 0) {
                s_in[r] = bi;
                s_out[r] = bo;
            }
        }
        __syncthreads();
        for (int ty = t / RN_TILE; ty < RN_TILE; ty += RN_THREADS / RN_TILE) {
            const long long y = y0 + ty, x = x0 + tx;
            if (y < H && x < W) {
                const bool v = (s_in[RN_HALO + ty] >> c) & 1ull;
                int m = far2, code = -1;
                for (int dy = -R; dy <= R; dy++) {                                          // upward in y: the first row at the least distance stays
                    const int r = RN_HALO + ty + dy;                                        // 0 .. 63
                    const unsigned long long w = v ? s_out[r] : s_in[r];                    // the pixels of the other state in that row
                    const unsigned long long right = w >> c, left = w << (63 - c);          // bit 0 / bit 63: the pixel's own column
                    int d = 2 * RN_SPAN, dx = 0;
                    if (right) {
                        d = __builtin_ctzll(right);
                        dx = d;
                    }
                    if (left) {
                        const int dl = __builtin_clzll(left);
                        if (dl <= d) {                                                      // as near as the right one: the left, smaller x
                            d = dl;
                            dx = -dl;
                        }
                    }
                    const int q = dy * dy + d * d;
                    if (q < m) {                                                            // |dx| > R gives q > R R + 1: it never wins
                        m = q;
                        code = (dy + ROPE_SIL_MAX_RADIUS) * RN_CODE_SIDE + (dx + ROPE_SIL_MAX_RADIUS);
                    }
                }
                near[(size_t)plane * hw + (size_t)y * (size_t)W + (size_t)x] = (int16_t)code;
            }
        }
        __syncthreads();                                                                    // the next plane writes the words again
    }
}

// ---------------------------------------------------------------------------------------------- the normal equations
// What a code says: the offset (dx, dy) to the nearest pixel of the other state and m = dx dx + dy dy; false for FAR — the code -1, and
// as well whatever rope_render_nearest never writes at this radius (a code beyond the table, m = 0, m > R R): such a plane is read
// as FAR there and no address is made from it.
__device__ __forceinline__ bool near_offset(int code, int near2, int &dx, int &dy, int &m)
{
    dx = dy = 0;
    m = near2 + 1;
    if (code < 0 || code > ROPE_SIL_NEAREST_MAX) return false;
    const int oy = code / RN_CODE_SIDE - ROPE_SIL_MAX_RADIUS, ox = code - (code / RN_CODE_SIDE) * RN_CODE_SIDE - ROPE_SIL_MAX_RADIUS;
    const int q = ox * ox + oy * oy;
    if (q < 1 || q > near2) return false;
    dx = ox;
    dy = oy;
    m = q;
    return true;
}

// the signed squared distance rope_mask_distance writes for the render's coverage at pixel q, from the code and the id there
__device__ __forceinline__ int32_t near_sd(const int16_t *__restrict__ n0, const uint8_t *__restrict__ i0, int q, int n_links, int near2)
{
    int dx, dy, m;
    near_offset(n0[q], near2, dx, dy, m);
    return i0[q] < n_links ? -m : m;
}

// Pixel p of a frame: adds its share of words 0 .. 2 to head and, for an inlier, fills v and returns true.
__device__ __forceinline__ bool rneq_pixel(const uint8_t *__restrict__ m0, const int16_t *__restrict__ n0, const float *__restrict__ r0,
                                           const uint8_t *__restrict__ i0, int p, int H, int W, int n_links, const Camera &cam,
                                           const double *__restrict__ jf, int n_joints, const double *__restrict__ tf, int n_cols, int near2,
                                           double (&head)[BNEQ_HEAD], double (&v)[BNEQ_VEC])
{
    if (m0[p] == 0) return false;                                                       // not of the mask
    const int y = p / W, x = p - y * W;
    const bool left = x > 0, right = x + 1 < W, up = y > 0, down = y + 1 < H;
    const bool contour = (left && m0[p - 1] == 0) || (right && m0[p + 1] == 0) || (up && m0[p - W] == 0) || (down && m0[p + W] == 0);
    if (!contour) return false;                                                         // the frame's edge is no outline
    const int far2 = near2 + 1;
    const bool rendered = i0[p] < n_links;
    int dx, dy, m;
    const bool within = near_offset(n0[p], near2, dx, dy, m);
    const double phi = sil_phi(rendered ? -m : m, far2);
    const double e = phi + 0.5;
    head[0] += 1.0;
    head[1] += e * e;
    // the anchor: the rendered pixel that carries the boundary p sees.  p not rendered: its nearest rendered pixel.  p rendered: its
    // nearest unrendered pixel moved one pixel towards p along the longer axis of the offset (x when |dx| >= |dy|) — between p and that
    // pixel and strictly nearer to p than it, so rendered and inside the image
    int ax = x + dx, ay = y + dy;
    if (rendered) {
        const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        if (adx >= ady) ax -= dx > 0 ? 1 : -1;
        else ay -= dy > 0 ? 1 : -1;
    }
    if (!within || ax < 0 || ax >= W || ay < 0 || ay >= H) return false;                  // beyond the truncation (or a code of another plane)
    const int a = ay * W + ax, id = i0[a];
    if (id >= n_links) return false;                                                    // codes of another render: no surface there, FAR as well

    double gx = 0.0, gy = 0.0;
    if (left && right) gx = (sil_phi(near_sd(n0, i0, p + 1, n_links, near2), far2) - sil_phi(near_sd(n0, i0, p - 1, n_links, near2), far2)) / 2.0;
    else if (right) gx = sil_phi(near_sd(n0, i0, p + 1, n_links, near2), far2) - phi;
    else if (left) gx = phi - sil_phi(near_sd(n0, i0, p - 1, n_links, near2), far2);
    if (up && down) gy = (sil_phi(near_sd(n0, i0, p + W, n_links, near2), far2) - sil_phi(near_sd(n0, i0, p - W, n_links, near2), far2)) / 2.0;
    else if (down) gy = sil_phi(near_sd(n0, i0, p + W, n_links, near2), far2) - phi;
    else if (up) gy = phi - sil_phi(near_sd(n0, i0, p - W, n_links, near2), far2);

    const double z = (double)r0[a];
    const double kx = ((double)ax - cam.cx) / cam.fx, ky = ((double)ay - cam.cy) / cam.fy;
    const Vec3 P = {kx * z, ky * z, z};
    // the minus: it is the boundary that moves and not the pixel, d phi(p) / d theta = -grad phi(p) . (the image velocity of the anchor)
#pragma unroll
    for (int j = 0; j < NEQ_JOINTS; j++) {
        v[j] = 0.0;
        if (j < n_joints && j < id) v[j] = -silhouette_column(gx, gy, cam, kx, ky, z, joint_velocity(jf, j, P));   // joint j moves the links behind it
        v[NEQ_JOINTS + j] = 0.0;
        if (j < n_cols) v[NEQ_JOINTS + j] = -silhouette_column(gx, gy, cam, kx, ky, z, twist_velocity(tf, j, P));  // every column moves every drawn link
    }
    v[BNEQ_SLOTS] = e;
    head[2] += 1.0;
    return true;
}

// Workgroup blockIdx.x = frame * chunks + chunk.
__global__ void __launch_bounds__(NEQ_THREADS)
rneq_partial_kernel(const uint8_t *__restrict__ mask, const int16_t *__restrict__ near, const float *__restrict__ render,
                    const uint8_t *__restrict__ ids, int H, int W, int chunks, int n_links, Camera cam, const double *__restrict__ joints,
                    int n_joints, const double *__restrict__ twists, int n_cols, int near2, double *__restrict__ work)
{
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int hw = H * W;                                                               // at most 2^24
    const uint8_t *const m0 = mask + (size_t)frame * hw;
    const int16_t *const n0 = near + (size_t)frame * hw;
    const float *const r0 = render + (size_t)frame * hw;
    const uint8_t *const i0 = ids + (size_t)frame * hw;
    const double *const jf = joints + (size_t)frame * n_joints * 6;                     // never read when its count is 0
    const double *const tf = twists + (size_t)frame * n_cols * 6;
    bneq_pack_and_own_words(hw, chunk, [&](int p, double (&head)[BNEQ_HEAD], double (&v)[BNEQ_VEC]) {
        return rneq_pixel(m0, n0, r0, i0, p, H, W, n_links, cam, jf, n_joints, tf, n_cols, near2, head, v);
    }, work + (size_t)blockIdx.x * ROPE_BNEQ_WORDS);
}

// a frame's partials added in index order, two frames a workgroup (rope_neq.h)
__global__ void __launch_bounds__(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS)
rneq_gather_kernel(const double *__restrict__ work, int n_frames, int chunks, double *__restrict__ out)
{
    neq_gather<ROPE_BNEQ_WORDS>(work, n_frames, chunks, out);
}

}  // namespace

extern "C" int rope_render_nearest(const uint8_t *render_ids_dev, int N, int H, int W, int n_links, int radius, int16_t *near_dev, void *stream)
{
    if (N < 0 || H < 1 || W < 1 || (long long)H * (long long)W >= (1ll << 31)) return ROPE_E_ARG;
    if (radius < 1 || radius > ROPE_SIL_MAX_RADIUS || n_links < 1 || n_links > 255) return ROPE_E_ARG;
    if (N > 0 && (!render_ids_dev || !near_dev || ((uintptr_t)near_dev & 1))) return ROPE_E_ARG;
    if (N == 0) return ROPE_OK;
    const long long tiles_x = ((long long)W + RN_TILE - 1) / RN_TILE, tiles_y = ((long long)H + RN_TILE - 1) / RN_TILE;    // their product < 2^27
    hipLaunchKernelGGL(render_nearest_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)(N < RN_MAX_PLANES_Y ? N : RN_MAX_PLANES_Y)),
                       dim3(RN_THREADS), 0, (hipStream_t)stream, render_ids_dev, N, H, W, (int)tiles_x, n_links, radius, near_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" int rope_silhouette_normal_equations_reverse(const uint8_t *mask_dev, const int16_t *near_dev, const float *render_depth_dev,
                                                        const uint8_t *render_ids_dev, int n_frames, int H, int W, int n_links, float fx, float fy,
                                                        float cx, float cy, const double *joints_dev, int n_joints, const double *twists_dev,
                                                        int n_cols, int radius, double *out_dev, double *work_dev, void *stream)
{
    // the forward call's rules, with the mask and the codes in the place of its field: bytes and 2-byte words, so their own line
    if (!mask_dev || !near_dev || ((uintptr_t)near_dev & 1)) return ROPE_E_ARG;
    if (neq_bad_args(n_links, fx, fy, cx, cy, render_depth_dev, render_ids_dev, render_depth_dev, out_dev, work_dev)) return ROPE_E_ARG;
    if (neq_bad_columns12(joints_dev, n_joints, twists_dev, n_cols)) return ROPE_E_ARG;
    if (radius < 1 || radius > ROPE_SIL_MAX_RADIUS) return ROPE_E_ARG;
    const long long chunks = neq_chunks(n_frames, H, W);
    if (chunks == 0) return ROPE_E_ARG;

    hipStream_t st = (hipStream_t)stream;
    const Camera cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    hipLaunchKernelGGL(rneq_partial_kernel, dim3((unsigned)((long long)n_frames * chunks)), dim3(NEQ_THREADS), 0, st, mask_dev, near_dev,
                       render_depth_dev, render_ids_dev, H, W, (int)chunks, n_links, cam, n_joints > 0 ? joints_dev : nullptr, n_joints,
                       n_cols > 0 ? twists_dev : nullptr, n_cols, radius * radius, work_dev);
    if (hipGetLastError() != hipSuccess) return ROPE_E_HIP;
    hipLaunchKernelGGL(rneq_gather_kernel, dim3(neq_gather_grid(n_frames)), dim3(NEQ_GATHER_FRAMES * ROPE_BNEQ_WORDS), 0, st, work_dev, n_frames,
                       (int)chunks, out_dev);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
