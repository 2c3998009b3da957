// The first and the last kernels of every evaluation pass (rope_kernels.hip: fk_mvp / bounds / fk_bounds and finalize_only /
// finalize_frames / finalize_argmin), the raster queue's builder (score_queue) and a kept grid's clearing (clear_pass), each launched
// on its own on matrices, meshlet tables, masks and sums the test supplies: the library only ever runs them inside a whole pass, on
// the robot's meshlets at the poses a caller asks for, and entry points of their own in rope_abi.hip would change rope_build_id.  Built by tests/test_gpu_geometry_kernels.py with build.HIPCC_FLAGS into a temporary
// directory and LINKED against the built librope_hip.so (the helpers are plain members of namespace rope and the library is built
// with default visibility), so the kernels that run are the shipped ones; never part of librope_hip.so.
//
// FrameParams is built from (W, H, tiles_x, tiles_y) with every other member zero.  By reading rope_kernels.hip: meshlet_box reads
// fp.W, fp.H (half sizes, clamps, the y flip of the tile rows) and fp.tiles_x (tile index); bounds_kernel reads fp.tiles_x and
// fp.tiles_y besides (their product sizes the weight arrays); fk_bounds_kernel reads fp through meshlet_box only; fk_mvp_kernel and
// the three finalize kernels take no FrameParams.  None of them reads r0, r1, c0, c1, c_num, c_sum or c_dif.
//
// RobotParams is built from device pointers to ml_header and ml_aabb plus n_meshlets; ml_verts and ml_tris are null and link_first
// is zero.  By reading the same code: meshlet_box reads ml_header[8 m + 7] (the link), ml_header[8 m + 6] >> 16 (the triangle
// count, only where a weight array is given) and the two float4 of ml_aabb[8 m ..]; bounds_kernel reads ml_header[8 m + 7] once more
// (the skip of shared links) and n_meshlets; fk_bounds_kernel reads n_meshlets.  ml_verts, ml_tris and link_first are read by the
// raster kernels only.
#include "../rope_s3d_amd/csrc/rope_kernels.h"

static rope::FrameParams frame_of(int W, int H, int tiles_x, int tiles_y)
{
    rope::FrameParams fp = {};
    fp.W = W; fp.H = H; fp.tiles_x = tiles_x; fp.tiles_y = tiles_y;
    return fp;
}

static rope::RobotParams robot_of(const uint32_t *ml_header, const float *ml_aabb, int n_meshlets)
{
    rope::RobotParams rp = {};
    rp.ml_header = ml_header; rp.ml_aabb = ml_aabb; rp.n_meshlets = n_meshlets;
    return rp;
}

// 0 TILE_W, 1 TILE_H, 2 MAX_MASK_WORDS, 3 QUEUE_WEIGHT_TILES, 4 QUEUE_COUNTERS, 5 COMPACT_PX, 6 ROPE_SUM_WORDS, 7 ROPE_MAX_LINKS,
// 8 .. 11 ROPE_LOSS_DEPTH / FULL / LOOKUP / TSWEEP, 12 MAX_MESHLETS, 13 QUEUE_CLASSES, 14 QUEUE_TOP_LOG2; anything else -1
extern "C" int shim_constant(int which)
{
    switch (which) {
    case 0: return rope::TILE_W;
    case 1: return rope::TILE_H;
    case 2: return rope::MAX_MASK_WORDS;
    case 3: return rope::QUEUE_WEIGHT_TILES;
    case 4: return rope::QUEUE_COUNTERS;
    case 5: return rope::COMPACT_PX;
    case 6: return ROPE_SUM_WORDS;
    case 7: return ROPE_MAX_LINKS;
    case 8: return ROPE_LOSS_DEPTH;
    case 9: return ROPE_LOSS_FULL;
    case 10: return ROPE_LOSS_LOOKUP;
    case 11: return ROPE_LOSS_TSWEEP;
    case 12: return rope::MAX_MESHLETS;
    case 13: return rope::QUEUE_CLASSES;
    case 14: return rope::QUEUE_TOP_LOG2;
    }
    return -1;
}

extern "C" int shim_fk(const double *cand, int C, int n_render, const double *joint_fixed, const double *joint_axes, const double *PV,
                       const int32_t *view_of, float *mvp, uint64_t *sums, uint32_t *mask_lo, uint32_t *mask_hi, int mask_words,
                       int *queue_counters, uint32_t *tile_tris, uint32_t *tile_tris_lo, int n_tiles, void *stream)
{
    return (int)rope::launch_fk((hipStream_t)stream, cand, C, n_render, joint_fixed, joint_axes, PV, view_of, mvp, sums, mask_lo, mask_hi,
                                mask_words, queue_counters, tile_tris, tile_tris_lo, n_tiles);
}

extern "C" int shim_bounds(int W, int H, int tiles_x, int tiles_y, const uint32_t *ml_header, const float *ml_aabb, int n_meshlets, int C,
                           int n_render, int n_shared, const float *mvp, void *bounds, uint32_t *mask_lo, uint32_t *mask_hi, int mask_words,
                           const int32_t *layer_of, const int32_t *layer_rep, uint32_t *tile_tris, uint32_t *tile_tris_lo, int lo_first,
                           void *stream)
{
    return (int)rope::launch_bounds((hipStream_t)stream, C, frame_of(W, H, tiles_x, tiles_y), robot_of(ml_header, ml_aabb, n_meshlets),
                                    n_render, n_shared, mvp, (short4 *)bounds, mask_lo, mask_hi, mask_words, layer_of, layer_rep, tile_tris,
                                    tile_tris_lo, lo_first);
}

extern "C" int shim_fk_bounds(int W, int H, int tiles_x, int tiles_y, const uint32_t *ml_header, const float *ml_aabb, int n_meshlets,
                              const double *cand, int C, int n_render, int n_shared, const double *joint_fixed, const double *joint_axes,
                              const double *PV, const int32_t *view_of, float *mvp, void *bounds, uint64_t *sums, uint32_t *mask_lo,
                              uint32_t *mask_hi, int mask_words, void *stream)
{
    return (int)rope::launch_fk_bounds((hipStream_t)stream, cand, C, frame_of(W, H, tiles_x, tiles_y), robot_of(ml_header, ml_aabb, n_meshlets),
                                       n_render, n_shared, joint_fixed, joint_axes, PV, view_of, mvp, (short4 *)bounds, sums, mask_lo,
                                       mask_hi, mask_words);
}

// flags: eight bytes on the host (they travel as a kernel argument); err: C + 2 doubles
extern "C" int shim_finalize(uint64_t *sums, const uint64_t *total_empty, int C, int loss, int n_render, double n_pix,
                             const uint8_t *flags, double *err, void *stream)
{
    rope::LinkFlags lf;
    for (int k = 0; k < 8; k++) lf.f[k] = flags[k];
    return (int)rope::launch_finalize((hipStream_t)stream, sums, total_empty, C, loss, n_render, n_pix, lf, err);
}

// flags: eight bytes per frame on the device; err: C doubles
extern "C" int shim_finalize_frames(uint64_t *sums, const uint64_t *totals, const int32_t *frame_of_row, const uint8_t *flags, int C,
                                    int loss, int n_render, double n_pix, double *err, void *stream)
{
    return (int)rope::launch_finalize_frames((hipStream_t)stream, sums, totals, frame_of_row, (const rope::LinkFlags *)flags, C, loss,
                                             n_render, n_pix, err);
}

// The queue builder alone (launch_score_queue: score_queue_kernel without the drain).  RasterArgs holds the masks, the layer maps,
// the layers' stored sums, the row -> candidate map and the rows' sums; every other member is zero.  By reading rope_kernels.hip:
// score_queue_kernel reads ra.cand_of_row, ra.layer_of, ra.layer_rep, ra.mask_lo, ra.mask_hi, ra.mask_words, ra.layer_sums and
// ra.sums, and nothing else of ra.
extern "C" int shim_score_queue(const uint32_t *mask_lo, const uint32_t *mask_hi, int mask_words, const int32_t *layer_of,
                                const int32_t *layer_rep, uint64_t *layer_sums, const int32_t *cand_of_row, uint64_t *sums, int rows,
                                int n_tiles, uint32_t *items, unsigned long long segment, int *counters, const uint32_t *weights, void *stream)
{
    rope::RasterArgs a = {};
    a.mask_lo = mask_lo; a.mask_hi = mask_hi; a.mask_words = mask_words;
    a.layer_of = layer_of; a.layer_rep = layer_rep; a.layer_sums = layer_sums; a.cand_of_row = cand_of_row; a.sums = sums;
    return (int)rope::launch_score_queue((hipStream_t)stream, a, rows, n_tiles, items, (size_t)segment, counters, weights);
}

extern "C" int shim_clear_pass(uint64_t *sums, int C, int *queue_counters, void *stream)
{
    return (int)rope::launch_clear_pass((hipStream_t)stream, sums, C, queue_counters);
}
