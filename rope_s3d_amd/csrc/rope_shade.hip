// rope_shade.hip — the photograph of a render, for gfx950: rope_shade_frames lights the depth and link-id planes that
// rope_render_batch_device left in HBM, paints them per link, lays them over a background, adds sensor noise and writes the BGR
// picture, with (optionally) a depth map that has a plane behind the robot.  The arithmetic is the contract of include/rope_s3d.h
// (rope_shade_frames), one IEEE float32 operation per written operation (-ffp-contract=off; hipcc's `/` and sqrtf are the correctly
// rounded ones by default, and the build is not asked for anything else); tests/shade_ref.py restates that text in numpy.
//
// Shape.  About 5 bytes in and 3 to 7 out per pixel with a one-pixel neighbourhood, so a workgroup takes a tile of SH_ROWS x SH_COLS
// pixels and stages its depth and ids, with a halo, in LDS: every plane byte is fetched once per tile (18 x 264 for 16 x 256: 1.16
// times the tile) in 16-byte / 4-byte loads where the address allows and element by element where it does not (first and last
// columns, planes whose rows are not 16-byte aligned).  The lane that staged four pixels of the tile proper also writes their
// depth_out, as one 16-byte store where aligned: depth_out follows the depth plane's alignment, not the picture's.
// The picture is 3 bytes a pixel, so 4 pixels are 3 dwords.  Row y of a plane starts at whatever address it does; with
// o = (that address) & 3, the pixels x = o + 4 k start a dword.  A lane therefore takes the 4 pixels from X0 + o + 4 lane of its row
// (o is 0..3 and differs from row to row, which is why the halo is 4 columns wide) and writes 3 dwords; the pixels before o (first
// column tile only) and a chunk that crosses the end of the row go out byte by byte.  The tiles of a row, each shifted by the same o,
// cover o .. W - 1 between them.  Background bytes are read the same way: 3 dwords where the background plane is aligned like the
// picture at that chunk, else bytes.  Philox is computed only for frames whose noise_q is not 0 (uniform per workgroup).
// depth_out may be depth_dev itself: a tile then reads halo pixels a neighbour may have rewritten, but only background pixels change,
// and the depth of a background pixel is used by no other pixel (differences never cross an id boundary).
// The per-frame records travel as kernel arguments, SH_FRAMES to a launch; nothing is allocated, copied or waited for.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr int SH_COLS = 256;                  // pixels of a row per tile: 64 lanes x 4
constexpr int SH_ROWS = 16;                   // rows per tile: SH_WAVES x 4
constexpr int SH_HALO = 4;                    // columns staged before and after the tile (1 for the neighbour + up to 3 of shift)
constexpr int SH_PITCH = SH_COLS + 2 * SH_HALO;       // staged columns: X0 - 4 .. X0 + SH_COLS + 3
constexpr int SH_GROUPS = SH_PITCH / 4;       // 4-pixel groups per staged row
constexpr int SH_FRAMES = 32;                 // records per launch: 2 KiB of kernel arguments

static_assert(sizeof(rope_shade_params) == 64, "rope_shade_params is 64 bytes (engine.SHADE_DTYPE mirrors it)");

struct FrameParams { rope_shade_params p[SH_FRAMES]; };

struct Camera { float fx, fy, cx, cy; };

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), as rope_synth.hip draws the depth holes
struct Philox4 { uint32_t w[4]; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// a value and the channel's noise -> the byte: NaN and anything below 0 give 0
__device__ __forceinline__ uint32_t to_byte(float v, int noise)
{
    const float t = v + (float)noise;
    return (uint32_t)(t > 0.0f ? (t < 255.0f ? t : 255.0f) : 0.0f);
}

__device__ __forceinline__ int noise_of(uint32_t word, int noise_q)
{
    const int s = (int)((word & 0xFFu) + ((word >> 8) & 0xFFu) + ((word >> 16) & 0xFFu) + (word >> 24)) - 510;
    return (s * noise_q) >> 10;
}

// What a lane holds of its neighbourhood: the row of the pixel from one column before its chunk to one after, the rows above and
// below over the chunk.  k is ((float)x - cx) / fx per column and ((float)y - cy) / fy per row.
struct Hood {
    float zc[6], zu[4], zd[4], kx[6], ky[3];
    uint8_t ic[6], iu[4], id[4];
};

// pixel j of the chunk (column index j + 1 of the row arrays) -> its three bytes, B in bits 0-7
__device__ __forceinline__ uint32_t shade_pixel(const Hood &h, int j, bool left, bool right, bool up, bool down, const rope_shade_params &p,
                                                int n_links, uint32_t back, const Philox4 &g)
{
    const int c = j + 1;
    const uint32_t id = h.ic[c];
    const int q = p.noise_q;
    const int n0 = q ? noise_of(g.w[0], q) : 0, n1 = q ? noise_of(g.w[1], q) : 0, n2 = q ? noise_of(g.w[2], q) : 0;
    if (id >= (uint32_t)n_links)
        return to_byte((float)(back & 0xFFu), n0) | (to_byte((float)((back >> 8) & 0xFFu), n1) << 8) | (to_byte((float)(back >> 16), n2) << 16);
    const float z = h.zc[c];
    const float px = h.kx[c] * z, py = h.ky[1] * z;
    float dxx = 0.0f, dxy = 0.0f, dxz = 0.0f, dyx = 0.0f, dyy = 0.0f, dyz = 0.0f;
    if (right && h.ic[c + 1] == id) {
        const float zn = h.zc[c + 1];
        dxx = h.kx[c + 1] * zn - px; dxy = h.ky[1] * zn - py; dxz = zn - z;
    } else if (left && h.ic[c - 1] == id) {
        const float zn = h.zc[c - 1];
        dxx = px - h.kx[c - 1] * zn; dxy = py - h.ky[1] * zn; dxz = z - zn;
    }
    if (down && h.id[j] == id) {
        const float zn = h.zd[j];
        dyx = h.kx[c] * zn - px; dyy = h.ky[2] * zn - py; dyz = zn - z;
    } else if (up && h.iu[j] == id) {
        const float zn = h.zu[j];
        dyx = px - h.kx[c] * zn; dyy = py - h.ky[0] * zn; dyz = z - zn;
    }
    const float nx = dxy * dyz - dxz * dyy, ny = dxz * dyx - dxx * dyz, nz = dxx * dyy - dxy * dyx;
    const float nn = (nx * nx + ny * ny) + nz * nz;
    const float dot = (nx * p.light[0] + ny * p.light[1]) + nz * p.light[2];
    const float lam = nn == 0.0f ? 1.0f : (dot > 0.0f ? dot : 0.0f) / sqrtf(nn);         // a NaN stays one
    const float s = p.ambient + (1.0f - p.ambient) * lam;
    const float shade = s > 1.0f ? 1.0f : s;
    const uint8_t *a = p.albedo[id];
    const float v0 = rintf((float)a[0] * shade * p.gain[0]), v1 = rintf((float)a[1] * shade * p.gain[1]), v2 = rintf((float)a[2] * shade * p.gain[2]);
    return to_byte(v0, n0) | (to_byte(v1, n1) << 8) | (to_byte(v2, n2) << 16);
}

__global__ void __launch_bounds__(SH_THREADS)
shade_frames_kernel(const float *depth, const uint8_t *__restrict__ ids, int H, int W, int tiles_x, int n_links, Camera cam,
                    const FrameParams fp, const uint8_t *__restrict__ bg, uint32_t frame_base, uint32_t key0, uint32_t key1,
                    uint8_t *__restrict__ bgr, float *depth_out)
{
    __shared__ __attribute__((aligned(16))) float s_z[(SH_ROWS + 2) * SH_PITCH];
    __shared__ __attribute__((aligned(4))) uint8_t s_id[(SH_ROWS + 2) * SH_PITCH];

    const int t = threadIdx.x, m = blockIdx.z;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int X0 = tx * SH_COLS, Y0 = ty * SH_ROWS;
    const rope_shade_params &p = fp.p[m];
    const size_t hw = (size_t)H * (size_t)W;
    const float *const zp = depth + (size_t)m * hw;
    const uint8_t *const ip = ids + (size_t)m * hw;
    float *const zo = depth_out ? depth_out + (size_t)m * hw : nullptr;
    const float bg_depth = p.bg_depth;

    // ---- stage rows Y0 - 1 .. Y0 + SH_ROWS, columns X0 - 4 .. X0 + SH_COLS + 3; what lies outside the image is depth 0, id 255
    for (int g = t; g < (SH_ROWS + 2) * SH_GROUPS; g += SH_THREADS) {
        const int r = g / SH_GROUPS, c = g - r * SH_GROUPS;
        const int y = Y0 - 1 + r, x = X0 - SH_HALO + 4 * c;
        float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t id4 = 0xFFFFFFFFu;
        if (y >= 0 && y < H && x + 3 >= 0 && x < W) {
            const size_t o = (size_t)y * W + (size_t)(x < 0 ? 0 : x);                   // offset of the group's first pixel inside the image
            const bool whole = x >= 0 && x + 3 < W;
            if (whole && ((uintptr_t)(zp + o) & 15) == 0) {
                const float4 v = *reinterpret_cast<const float4 *>(zp + o);
                z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (x + j >= 0 && x + j < W) z[j] = zp[(size_t)y * W + (size_t)(x + j)];
            }
            if (whole && ((uintptr_t)(ip + o) & 3) == 0) {
                id4 = *reinterpret_cast<const uint32_t *>(ip + o);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (x + j >= 0 && x + j < W) id4 = (id4 & ~(0xFFu << (8 * j))) | ((uint32_t)ip[(size_t)y * W + (size_t)(x + j)] << (8 * j));
            }
            // the tile proper: its depth with the background plane behind the robot
            if (zo && r >= 1 && r <= SH_ROWS && c >= 1 && c <= SH_COLS / 4) {
                float w[4];
#pragma unroll
                for (int j = 0; j < 4; j++) w[j] = ((id4 >> (8 * j)) & 0xFFu) < (uint32_t)n_links ? z[j] : bg_depth;
                if (whole && ((uintptr_t)(zo + o) & 15) == 0) {
                    *reinterpret_cast<float4 *>(zo + o) = make_float4(w[0], w[1], w[2], w[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x + j < W) zo[(size_t)y * W + (size_t)(x + j)] = w[j];      // x >= X0 >= 0 here
                }
            }
        }
        *reinterpret_cast<float4 *>(&s_z[r * SH_PITCH + 4 * c]) = make_float4(z[0], z[1], z[2], z[3]);
        *reinterpret_cast<uint32_t *>(&s_id[r * SH_PITCH + 4 * c]) = id4;
    }
    __syncthreads();

    // ---- the picture: wave w takes rows w, w + 4, ..; a lane 4 pixels of the row, from a dword boundary of the picture's row
    const int lane = t & 63, wave = t >> 6;
    uint8_t *const out = bgr + (size_t)m * hw * 3;
    const uint8_t *const back = p.bg_index >= 0 ? bg + (size_t)p.bg_index * hw * 3 : nullptr;
    const uint32_t flat = (uint32_t)p.bg_colour[0] | ((uint32_t)p.bg_colour[1] << 8) | ((uint32_t)p.bg_colour[2] << 16);
    const uint32_t frame = frame_base + (uint32_t)m;
    for (int r = wave; r < SH_ROWS; r += SH_WAVES) {
        const int y = Y0 + r;
        if (y >= H) break;
        const size_t row = (size_t)y * W;
        const int shift = (int)((uintptr_t)(out + row * 3) & 3);
        // pass 0: the chunk of four; pass 1 (first column tile, lanes below the shift): one pixel before the first dword boundary
        for (int pass = 0; pass < 2; pass++) {
            const int xs = pass == 0 ? X0 + shift + 4 * lane : lane;
            const int n_px = pass == 0 ? (xs < W ? (W - xs < 4 ? W - xs : 4) : 0) : ((X0 == 0 && lane < shift && lane < W) ? 1 : 0);
            if (n_px == 0) continue;
            Hood h;
            const int lr = r + 1, lc = xs - (X0 - SH_HALO);                             // the chunk's first pixel in the staged tile
#pragma unroll
            for (int j = 0; j < 6; j++) {
                h.zc[j] = s_z[lr * SH_PITCH + lc - 1 + j];
                h.ic[j] = s_id[lr * SH_PITCH + lc - 1 + j];
                h.kx[j] = ((float)(xs - 1 + j) - cam.cx) / cam.fx;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                h.zu[j] = s_z[(lr - 1) * SH_PITCH + lc + j];
                h.iu[j] = s_id[(lr - 1) * SH_PITCH + lc + j];
                h.zd[j] = s_z[(lr + 1) * SH_PITCH + lc + j];
                h.id[j] = s_id[(lr + 1) * SH_PITCH + lc + j];
            }
#pragma unroll
            for (int j = 0; j < 3; j++) h.ky[j] = ((float)(y - 1 + j) - cam.cy) / cam.fy;

            uint8_t *const dst = out + (row + (size_t)xs) * 3;
            uint32_t b[4] = {flat, flat, flat, flat};
            if (back) {
                const uint8_t *const src = back + (row + (size_t)xs) * 3;
                if (n_px == 4 && ((uintptr_t)src & 3) == 0) {
                    const uint32_t d0 = reinterpret_cast<const uint32_t *>(src)[0], d1 = reinterpret_cast<const uint32_t *>(src)[1],
                                   d2 = reinterpret_cast<const uint32_t *>(src)[2];
                    b[0] = d0 & 0xFFFFFFu; b[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8); b[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16); b[3] = d2 >> 8;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (j < n_px) b[j] = (uint32_t)src[3 * j] | ((uint32_t)src[3 * j + 1] << 8) | ((uint32_t)src[3 * j + 2] << 16);
                }
            }
            uint32_t px[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (j >= n_px) continue;
                const int x = xs + j;
                Philox4 g = {};
                if (p.noise_q) g = philox4x32_10((uint32_t)(row + (size_t)x), frame, 0u, 1u, key0, key1);
                px[j] = shade_pixel(h, j, x > 0, x + 1 < W, y > 0, y + 1 < H, p, n_links, b[j], g);
            }
            if (n_px == 4) {                                                            // dst is dword-aligned: that is what the shift is for
                uint32_t *const d = reinterpret_cast<uint32_t *>(dst);
                d[0] = px[0] | (px[1] << 24);
                d[1] = (px[1] >> 8) | (px[2] << 16);
                d[2] = (px[2] >> 16) | (px[3] << 8);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (j < n_px) {
                        dst[3 * j] = (uint8_t)px[j]; dst[3 * j + 1] = (uint8_t)(px[j] >> 8); dst[3 * j + 2] = (uint8_t)(px[j] >> 16);
                    }
            }
        }
    }
}

}  // namespace

extern "C" int rope_shade_frames(const float *depth_dev, const uint8_t *ids_dev, int N, int H, int W, int n_links, float fx, float fy, float cx,
                                 float cy, const rope_shade_params *params, const uint8_t *bg_dev, int n_bg, uint32_t frame0, uint64_t seed,
                                 uint8_t *bgr_dev, float *depth_out_dev, void *stream)
{
    if (N < 0 || H < 1 || W < 1 || n_bg < 0 || n_links < 1 || n_links > ROPE_MAX_LINKS) return ROPE_E_ARG;
    const size_t hw = (size_t)H * (size_t)W;
    if (hw >= ((size_t)1 << 31)) return ROPE_E_ARG;                                     // y W + x is one word of the generator's counter
    if (N > 0 && (!depth_dev || !ids_dev || !bgr_dev || !params)) return ROPE_E_ARG;
    if (((uintptr_t)depth_dev & 3) || ((uintptr_t)depth_out_dev & 3)) return ROPE_E_ARG;
    for (int i = 0; i < N; i++) {
        if (params[i].noise_q < 0 || params[i].noise_q > ROPE_SHADE_MAX_NOISE_Q) return ROPE_E_ARG;
        if (params[i].bg_index < -1 || params[i].bg_index >= n_bg || (params[i].bg_index >= 0 && !bg_dev)) return ROPE_E_ARG;
    }
    if (N == 0) return ROPE_OK;

    hipStream_t st = (hipStream_t)stream;
    const int tiles_x = (W + SH_COLS - 1) / SH_COLS, tiles_y = (H + SH_ROWS - 1) / SH_ROWS;       // at most 2^27 tiles: H W < 2^31
    const Camera cam = {fx, fy, cx, cy};
    for (int f0 = 0; f0 < N; f0 += SH_FRAMES) {
        const int nf = N - f0 < SH_FRAMES ? N - f0 : SH_FRAMES;
        FrameParams fp;
        for (int i = 0; i < SH_FRAMES; i++) fp.p[i] = params[f0 + (i < nf ? i : nf - 1)];
        const size_t o = (size_t)f0 * hw;
        hipLaunchKernelGGL(shade_frames_kernel, dim3((unsigned)(tiles_x * tiles_y), 1, (unsigned)nf), dim3(SH_THREADS), 0, st, depth_dev + o,
                           ids_dev + o, H, W, tiles_x, n_links, cam, fp, bg_dev, frame0 + (uint32_t)f0, (uint32_t)seed, (uint32_t)(seed >> 32),
                           bgr_dev + o * 3, depth_out_dev ? depth_out_dev + o : nullptr);
    }
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
