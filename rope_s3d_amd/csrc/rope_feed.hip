// rope_feed.hip — conditioning of raw z16 depth frames before the Predictor sees them, for gfx950: decimation, the edge-preserving
// spatial recurrence, the temporal state machine and the alignment of the depth image to the colour sensor (include/rope_s3d.h,
// rope_depth_*).  The arithmetic is this project's definition: integer steps, float32 steps that are one IEEE
// operation each (-ffp-contract=off) and, in the alignment, double steps in the written order, so that tests/feed_ref.py gives
// the same words.  All planes are uint16 sensor units, 0 = no data, (n_frames, h, w) contiguous.
//
// Decimation and the temporal filter are one lane per output pixel.  The alignment is a scatter: one lane per depth pixel, an
// integer atomic minimum per colour pixel of its footprint on a uint32 plane, then a pass that narrows the plane to uint16;
// a minimum does not depend on the order in which the atomics land.
//
// The spatial filter is a recurrence along a line: sequential along it, parallel across lines, so a launch is bound by the
// chain of dependent steps (w + h of them per sweep and direction), not by bytes, and the kernels are shaped for the latency of
// ONE frame: few lines per wave, many waves.  The vertical sweep has one lane per column — 64 neighbouring columns a wave, which
// is coalesced as it stands — and walks the rows in chunks of SP_VROWS held in registers, the next chunk's loads in flight while
// this one's chain runs.  The horizontal sweep has one lane per row, which would make every global access strided: a wave owns
// SP_ROWS rows and moves them through LDS in tiles of SP_COLS columns, loaded and stored row-wise by all 64 lanes (coalesced)
// and swept column-wise by SP_ROWS lanes; the LDS row pitch is an odd number of dwords so that those lanes hit different banks.
// The next tile is loaded into registers while the chain of this one runs.  A forward pass writes every tile back before the
// backward pass starts at the far end; the value a pass carries from tile to tile is a register of the lane that owns the line.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

constexpr int FD_THREADS = 256;
constexpr size_t FD_MAX_ELEMS = 0x7FFFFFFFu;   // elements of one stack of planes: every index fits 31 bits, every grid 2^23 workgroups

constexpr int SP_ROWS = 16;                    // horizontal sweep: rows of a wave's tile = lanes that walk
constexpr int SP_COLS = 128;                   // columns of a tile
constexpr int SP_PITCH = SP_COLS + 2;          // halfwords: 65 dwords a row, odd, so 16 rows at one column are 16 banks
constexpr int SP_LOADS = SP_ROWS * SP_COLS / 64;   // elements a lane moves per tile
constexpr int SP_VROWS = 32;                   // vertical sweep: rows a lane holds in registers

// one step of the recurrence: a the neighbour already updated in this pass, b the value here
__device__ __forceinline__ uint16_t spatial_step(uint16_t a, uint16_t b, float alpha, float beta, int delta)
{
    const int d = (int)b > (int)a ? (int)b - (int)a : (int)a - (int)b;
    if (a != 0 && b != 0 && d >= 1 && d <= delta) {
        const float v = (float)b * alpha + (float)a * beta + 0.5f;            // two products, a sum, + 0.5: one rounding each
        return (uint16_t)v;                                                  // below 65536: it lies between a and b, + 0.5
    }
    return b;
}

// ------------------------------------------------------------------------------------------------------------------ decimation
__global__ void __launch_bounds__(FD_THREADS)
decimate_kernel(const uint16_t *__restrict__ raw, int H, int W, int k, int h, int w, size_t total, uint16_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * FD_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % (size_t)w), r = (int)((i / (size_t)w) % (size_t)h);
    const size_t f = i / ((size_t)w * (size_t)h);
    const uint16_t *p = raw + (f * (size_t)H + (size_t)r * k) * (size_t)W + (size_t)c * k;     // r k + k <= H, c k + k <= W
    if (k <= 3) {                                                            // the lower median of the valid values
        uint16_t v[9];
        int m = 0;
        for (int y = 0; y < k; y++)
            for (int x = 0; x < k; x++) {
                const uint16_t z = p[(size_t)y * W + x];
                if (z != 0) {                                                // insertion into v[0..m), ascending
                    int j = m++;
                    for (; j > 0 && v[j - 1] > z; j--) v[j] = v[j - 1];
                    v[j] = z;
                }
            }
        out[i] = m ? v[(m - 1) / 2] : (uint16_t)0;
    } else {                                                                 // the mean of the valid values, rounded down
        uint32_t sum = 0, m = 0;                                             // at most 64 x 65535
        for (int y = 0; y < k; y++)
            for (int x = 0; x < k; x++) {
                const uint16_t z = p[(size_t)y * W + x];
                sum += z;
                m += z != 0;
            }
        out[i] = m ? (uint16_t)(sum / m) : (uint16_t)0;
    }
}

// ---------------------------------------------------------------------------------------------------------- spatial, horizontal
// One wave per workgroup: blockIdx.x = a band of SP_ROWS rows out of n h rows (frames stacked: a row is a row).
__device__ __forceinline__ void tile_load(const uint16_t *__restrict__ planes, size_t row0, int rows, int w, int col0, int lane,
                                          uint16_t regs[SP_LOADS])
{
#pragma unroll
    for (int j = 0; j < SP_LOADS; j++) {
        const int e = j * 64 + lane, r = e / SP_COLS, c = col0 + e % SP_COLS;
        regs[j] = r < rows && c < w ? planes[(row0 + r) * (size_t)w + c] : (uint16_t)0;
    }
}

__global__ void __launch_bounds__(64)
spatial_rows_kernel(uint16_t *__restrict__ planes, size_t n_rows, int w, float alpha, float beta, int delta)
{
    __shared__ uint16_t tile[SP_ROWS * SP_PITCH];
    const int lane = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * SP_ROWS;
    const int rows = n_rows - row0 < (size_t)SP_ROWS ? (int)(n_rows - row0) : SP_ROWS;
    const int n_tiles = (w + SP_COLS - 1) / SP_COLS;
    uint16_t regs[SP_LOADS];

    for (int pass = 0; pass < 2; pass++) {                                   // forward, then backward
        uint16_t a = 0;                                                      // nothing before the first element: a zero starts no chain
        tile_load(planes, row0, rows, w, pass ? (n_tiles - 1) * SP_COLS : 0, lane, regs);
        for (int s = 0; s < n_tiles; s++) {
            const int t = pass ? n_tiles - 1 - s : s, col0 = t * SP_COLS;
            const int cols = w - col0 < SP_COLS ? w - col0 : SP_COLS;
#pragma unroll
            for (int j = 0; j < SP_LOADS; j++) {
                const int e = j * 64 + lane;
                tile[(e / SP_COLS) * SP_PITCH + e % SP_COLS] = regs[j];
            }
            __syncthreads();
            if (s + 1 < n_tiles) tile_load(planes, row0, rows, w, (pass ? t - 1 : t + 1) * SP_COLS, lane, regs);
            if (lane < rows) {
                uint16_t *line = tile + lane * SP_PITCH;
                if (!pass)
#pragma unroll 8
                    for (int i = 0; i < cols; i++) line[i] = a = spatial_step(a, line[i], alpha, beta, delta);
                else
#pragma unroll 8
                    for (int i = cols - 1; i >= 0; i--) line[i] = a = spatial_step(a, line[i], alpha, beta, delta);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SP_LOADS; j++) {
                const int e = j * 64 + lane, r = e / SP_COLS, c = e % SP_COLS;
                if (r < rows && c < cols) planes[(row0 + r) * (size_t)w + col0 + c] = tile[r * SP_PITCH + c];
            }
            __syncthreads();                                                 // the tile is free; after the last one, the rows are in memory
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ spatial, vertical
// One lane per column: blockIdx.x = 64 columns, blockIdx.y = frame.
__global__ void __launch_bounds__(64)
spatial_cols_kernel(uint16_t *__restrict__ planes, int h, int w, float alpha, float beta, int delta)
{
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= w) return;
    uint16_t *const p = planes + (size_t)blockIdx.y * (size_t)h * (size_t)w + col;
    const int n_chunks = (h + SP_VROWS - 1) / SP_VROWS;
    uint16_t cur[SP_VROWS], nxt[SP_VROWS];

    for (int pass = 0; pass < 2; pass++) {
        uint16_t a = 0;
        {
            const int r0 = pass ? (n_chunks - 1) * SP_VROWS : 0;
#pragma unroll
            for (int j = 0; j < SP_VROWS; j++) nxt[j] = r0 + j < h ? p[(size_t)(r0 + j) * w] : (uint16_t)0;
        }
        for (int s = 0; s < n_chunks; s++) {
            const int r0 = (pass ? n_chunks - 1 - s : s) * SP_VROWS;
#pragma unroll
            for (int j = 0; j < SP_VROWS; j++) cur[j] = nxt[j];
            if (s + 1 < n_chunks) {                                          // rows of another chunk: untouched by this one's stores
                const int q0 = pass ? r0 - SP_VROWS : r0 + SP_VROWS;
#pragma unroll
                for (int j = 0; j < SP_VROWS; j++) nxt[j] = q0 + j < h ? p[(size_t)(q0 + j) * w] : (uint16_t)0;
            }
            if (!pass) {
#pragma unroll
                for (int j = 0; j < SP_VROWS; j++)
                    if (r0 + j < h) cur[j] = a = spatial_step(a, cur[j], alpha, beta, delta);
            } else {
#pragma unroll
                for (int j = SP_VROWS - 1; j >= 0; j--)
                    if (r0 + j < h) cur[j] = a = spatial_step(a, cur[j], alpha, beta, delta);
            }
#pragma unroll
            for (int j = 0; j < SP_VROWS; j++)
                if (r0 + j < h) p[(size_t)(r0 + j) * w] = cur[j];
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------- temporal
struct Persistence { int need, window; };                                    // window 0 = never, need 0 = always

__global__ void __launch_bounds__(FD_THREADS)
temporal_kernel(uint16_t *__restrict__ planes, int n, size_t hw, float alpha, float beta, int delta, Persistence pers,
                uint16_t *__restrict__ last, uint8_t *__restrict__ history)
{
    const size_t i = (size_t)blockIdx.x * FD_THREADS + threadIdx.x;
    if (i >= hw) return;
    uint16_t p = last[i];
    uint32_t hist = history[i];
    const uint32_t mask = (1u << pers.window) - 1u;
    for (int f = 0; f < n; f++) {
        uint16_t *x = planes + (size_t)f * hw + i;
        const uint16_t c = *x;
        if (c != 0) {
            const int d = (int)c > (int)p ? (int)c - (int)p : (int)p - (int)c;
            if (p != 0 && d <= delta) {
                const float v = alpha * (float)c + beta * (float)p + 0.5f;
                p = (uint16_t)v;
                *x = p;
            } else {
                p = c;
            }
        } else if (p != 0 && pers.window != 0 && __popc(hist & mask) >= pers.need) {
            *x = p;
        }
        hist = ((hist << 1) | (uint32_t)(c != 0)) & 0xFFu;
    }
    last[i] = p;
    history[i] = (uint8_t)hist;
}

// -------------------------------------------------------------------------------------------------------------------- alignment
struct AlignArgs {
    double dfx, dfy, dcx, dcy, cfx, cfy, ccx, ccy, R[9], t[3], scale;
};

// a corner (u, v) of a depth pixel at depth Z metres -> colour image coordinates; false when it lands behind the colour sensor
__device__ __forceinline__ bool align_corner(const AlignArgs &A, double u, double v, double Z, double &pu, double &pv)
{
    const double X = (u - A.dcx) / A.dfx * Z, Y = (v - A.dcy) / A.dfy * Z;
    const double X2 = A.R[0] * X + A.R[1] * Y + A.R[2] * Z + A.t[0];
    const double Y2 = A.R[3] * X + A.R[4] * Y + A.R[5] * Z + A.t[1];
    const double Z2 = A.R[6] * X + A.R[7] * Y + A.R[8] * Z + A.t[2];
    if (!(Z2 > 0.0)) return false;
    pu = X2 / Z2 * A.cfx + A.ccx;
    pv = Y2 / Z2 * A.cfy + A.ccy;
    return true;
}

__global__ void __launch_bounds__(FD_THREADS)
align_scatter_kernel(const uint16_t *__restrict__ planes, int h, int w, size_t total, AlignArgs A, int Hc, int Wc,
                     uint32_t *__restrict__ scratch)
{
    const size_t i = (size_t)blockIdx.x * FD_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint16_t z = planes[i];
    if (z == 0) return;
    const int x = (int)(i % (size_t)w), y = (int)((i / (size_t)w) % (size_t)h);
    const size_t f = i / ((size_t)w * (size_t)h);
    const double Z = (double)z * A.scale;
    double u0, v0, u1, v1;
    if (!align_corner(A, (double)x - 0.5, (double)y - 0.5, Z, u0, v0)) return;
    if (!align_corner(A, (double)x + 0.5, (double)y + 0.5, Z, u1, v1)) return;
    u0 = floor(u0 + 0.5);
    v0 = floor(v0 + 0.5);
    u1 = floor(u1 + 0.5);
    v1 = floor(v1 + 0.5);
    // inside the colour image, all four, before anything becomes an int (a NaN or an infinity fails the comparison)
    if (!(u0 >= 0.0 && u0 < (double)Wc && u1 >= 0.0 && u1 < (double)Wc && v0 >= 0.0 && v0 < (double)Hc && v1 >= 0.0 && v1 < (double)Hc)) return;
    int x0 = (int)u0, x1 = (int)u1, y0 = (int)v0, y1 = (int)v1;
    if (x0 > x1) { const int s = x0; x0 = x1; x1 = s; }
    if (y0 > y1) { const int s = y0; y0 = y1; y1 = s; }
    if (x1 - x0 + 1 > ROPE_ALIGN_MAX_FOOTPRINT || y1 - y0 + 1 > ROPE_ALIGN_MAX_FOOTPRINT) return;
    uint32_t *const plane = scratch + f * (size_t)Hc * (size_t)Wc;
    for (int yy = y0; yy <= y1; yy++)
        for (int xx = x0; xx <= x1; xx++) atomicMin(plane + (size_t)yy * Wc + xx, (uint32_t)z);
}

__global__ void __launch_bounds__(FD_THREADS)
align_narrow_kernel(const uint32_t *__restrict__ scratch, size_t total, uint16_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * FD_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint32_t v = scratch[i];
    out[i] = v > 0xFFFFu ? (uint16_t)0 : (uint16_t)v;                        // still the fill: nothing landed here
}

inline unsigned blocks_for(size_t total) { return (unsigned)((total + FD_THREADS - 1) / FD_THREADS); }

inline bool planes_ok(int n, int h, int w)
{
    return n >= 1 && h >= 1 && w >= 1 && (size_t)n * (size_t)h * (size_t)w <= FD_MAX_ELEMS;
}

inline int launched() { return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP; }

}  // namespace

extern "C" int rope_depth_decimated_shape(int H, int W, int k, int *h, int *w)
{
    if (!h || !w || H < 1 || W < 1 || k < 2 || k > 8) return ROPE_E_ARG;
    const int hh = ((H / k) / 4) * 4, ww = ((W / k) / 4) * 4;
    if (hh == 0 || ww == 0) return ROPE_E_ARG;
    *h = hh;
    *w = ww;
    return ROPE_OK;
}

extern "C" int rope_depth_decimate(const uint16_t *raw_dev, int n_frames, int H, int W, int k, uint16_t *out_dev, void *stream)
{
    int h, w;
    if (!raw_dev || !out_dev || !planes_ok(n_frames, H, W)) return ROPE_E_ARG;
    if (rope_depth_decimated_shape(H, W, k, &h, &w) != ROPE_OK) return ROPE_E_ARG;
    const size_t total = (size_t)n_frames * (size_t)h * (size_t)w;
    hipLaunchKernelGGL(decimate_kernel, dim3(blocks_for(total)), dim3(FD_THREADS), 0, (hipStream_t)stream, raw_dev, H, W, k, h, w, total, out_dev);
    return launched();
}

extern "C" int rope_depth_spatial(uint16_t *planes_dev, int n_frames, int h, int w, float alpha, int delta, int iterations, void *stream)
{
    if (!planes_dev || !planes_ok(n_frames, h, w) || n_frames > 65535) return ROPE_E_ARG;       // a frame is blockIdx.y of the vertical sweep
    if (!(alpha > 0.0f && alpha <= 1.0f) || delta < 1 || delta > 65535 || iterations < 1 || iterations > 5) return ROPE_E_ARG;
    const float beta = 1.0f - alpha;
    const size_t n_rows = (size_t)n_frames * (size_t)h;
    for (int it = 0; it < iterations; it++) {
        if (w > 1) {
            hipLaunchKernelGGL(spatial_rows_kernel, dim3((unsigned)((n_rows + SP_ROWS - 1) / SP_ROWS)), dim3(64), 0, (hipStream_t)stream,
                               planes_dev, n_rows, w, alpha, beta, delta);
            if (launched() != ROPE_OK) return ROPE_E_HIP;
        }
        if (h > 1) {
            hipLaunchKernelGGL(spatial_cols_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)n_frames), dim3(64), 0, (hipStream_t)stream,
                               planes_dev, h, w, alpha, beta, delta);
            if (launched() != ROPE_OK) return ROPE_E_HIP;
        }
    }
    return ROPE_OK;
}

extern "C" int rope_depth_temporal(uint16_t *planes_dev, int n_frames, int h, int w, float alpha, int delta, int persistence,
                                   uint16_t *last_dev, uint8_t *history_dev, void *stream)
{
    static const Persistence table[9] = {{0, 0}, {8, 8}, {2, 3}, {2, 4}, {2, 8}, {1, 2}, {1, 5}, {1, 8}, {0, 8}};
    if (!planes_dev || !last_dev || !history_dev || !planes_ok(n_frames, h, w)) return ROPE_E_ARG;
    if (!(alpha > 0.0f && alpha <= 1.0f) || delta < 1 || delta > 65535 || persistence < 0 || persistence > 8) return ROPE_E_ARG;
    const size_t hw = (size_t)h * (size_t)w;
    hipLaunchKernelGGL(temporal_kernel, dim3(blocks_for(hw)), dim3(FD_THREADS), 0, (hipStream_t)stream, planes_dev, n_frames, hw, alpha,
                       1.0f - alpha, delta, table[persistence], last_dev, history_dev);
    return launched();
}

extern "C" int rope_depth_align(const uint16_t *planes_dev, int n_frames, int h, int w, const double *depth_intrin, const double *color_intrin,
                                const double *extrin, double depth_scale, int Hc, int Wc, uint32_t *scratch_dev, uint16_t *out_dev, void *stream)
{
    if (!planes_dev || !depth_intrin || !color_intrin || !extrin || !scratch_dev || !out_dev) return ROPE_E_ARG;
    if (!planes_ok(n_frames, h, w) || !planes_ok(n_frames, Hc, Wc) || ((uintptr_t)scratch_dev & 3)) return ROPE_E_ARG;
    if (!isfinite(depth_scale) || !(depth_scale > 0.0)) return ROPE_E_ARG;
    for (int i = 0; i < 4; i++)
        if (!isfinite(depth_intrin[i]) || !isfinite(color_intrin[i])) return ROPE_E_ARG;
    if (depth_intrin[0] == 0.0 || depth_intrin[1] == 0.0) return ROPE_E_ARG;                     // the deprojection divides by them
    for (int i = 0; i < 12; i++)
        if (!isfinite(extrin[i])) return ROPE_E_ARG;
    AlignArgs A;
    A.dfx = depth_intrin[0]; A.dfy = depth_intrin[1]; A.dcx = depth_intrin[2]; A.dcy = depth_intrin[3];
    A.cfx = color_intrin[0]; A.cfy = color_intrin[1]; A.ccx = color_intrin[2]; A.ccy = color_intrin[3];
    for (int i = 0; i < 9; i++) A.R[i] = extrin[i];
    for (int i = 0; i < 3; i++) A.t[i] = extrin[9 + i];
    A.scale = depth_scale;
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)n_frames * (size_t)h * (size_t)w, total_c = (size_t)n_frames * (size_t)Hc * (size_t)Wc;
    if (hipMemsetAsync(scratch_dev, 0xFF, total_c * sizeof(uint32_t), st) != hipSuccess) return ROPE_E_HIP;
    hipLaunchKernelGGL(align_scatter_kernel, dim3(blocks_for(total)), dim3(FD_THREADS), 0, st, planes_dev, h, w, total, A, Hc, Wc, scratch_dev);
    if (launched() != ROPE_OK) return ROPE_E_HIP;
    hipLaunchKernelGGL(align_narrow_kernel, dim3(blocks_for(total_c)), dim3(FD_THREADS), 0, st, scratch_dev, total_c, out_dev);
    return launched();
}
