// The stored lookup table's launch helpers (rope_table.hip: table_count / table_fill / crop_total / table_score /
// table_score_frames<F, LANES>; rope_kernels.hip: argmin_sets / finalize) on tables, target planes and errors the test supplies: the library only
// ever feeds them rows the rasteriser has just drawn, and entry points of their own in rope_abi.hip would change rope_build_id.
// Built by tests/test_gpu_table_kernels.py with build.HIPCC_FLAGS into a temporary directory and LINKED against the built
// librope_hip.so (the helpers are plain members of namespace rope and the library is built with default visibility), so the
// kernels that run are the shipped ones; never part of librope_hip.so.
//
// FrameParams is built from (W, H, r0, r1, c0, c1) with every other member zero.  By reading rope_table.hip: crop_total_kernel
// reads fp.W, fp.H, fp.r0, fp.r1, fp.c0, fp.c1 and nothing else; launch_table_score_frames and table_crop_words read r0, r1, c0,
// c1; no other kernel of this group takes a FrameParams.  launch_finalize is given ROPE_LOSS_LOOKUP's arguments: finalize_one
// reads the LinkFlags and n_render only for ROPE_LOSS_FULL, so zero flags and n_render = 0 stand for any.
#include "../rope_s3d_amd/csrc/rope_kernels.h"

static rope::FrameParams frame_of(int W, int H, int r0, int r1, int c0, int c1)
{
    rope::FrameParams fp = {};
    fp.W = W; fp.H = H; fp.r0 = r0; fp.r1 = r1; fp.c0 = c0; fp.c1 = c1;
    return fp;
}

extern "C" int shim_sum_words(void) { return ROPE_SUM_WORDS; }

extern "C" long long shim_crop_words(int W, int H, int r0, int r1, int c0, int c1)
{
    return (long long)rope::table_crop_words(frame_of(W, H, r0, r1, c0, c1));
}

extern "C" int shim_table_count(int cw, int ch, const float *table, int C, uint32_t *counts, unsigned long long *offs,
                                unsigned long long *used, void *stream)
{
    return (int)rope::launch_table_count((hipStream_t)stream, cw, ch, table, C, counts, offs, used);
}

extern "C" int shim_table_fill(int cw, int ch, const float *table, int C, const unsigned long long *offs, uint32_t *goff, void *gval,
                               void *stream)
{
    return (int)rope::launch_table_fill((hipStream_t)stream, cw, ch, table, C, offs, goff, (float4 *)gval);
}

extern "C" int shim_table_score(int W, int H, int r0, int r1, int c0, int c1, const uint32_t *counts, const unsigned long long *offs,
                                const uint32_t *goff, const void *gval, int C, const float *t32, float *t32c, uint64_t *total,
                                uint64_t *sums, void *stream)
{
    return (int)rope::launch_table_score((hipStream_t)stream, frame_of(W, H, r0, r1, c0, c1), counts, offs, goff, (const float4 *)gval, C,
                                         t32, t32c, total, sums);
}

extern "C" int shim_table_score_frames(int W, int H, int r0, int r1, int c0, int c1, const uint32_t *counts, const unsigned long long *offs,
                                       const uint32_t *goff, const void *gval, int C, const float *t32, int n_frames, float *t32c,
                                       uint64_t *totals, double *scores, double *best, void *stream)
{
    return (int)rope::launch_table_score_frames((hipStream_t)stream, frame_of(W, H, r0, r1, c0, c1), counts, offs, goff,
                                                (const float4 *)gval, C, t32, n_frames, t32c, totals, scores, best);
}

extern "C" int shim_argmin_sets(const double *err, int C, int n_sets, double *best, void *stream)
{
    return (int)rope::launch_argmin_sets((hipStream_t)stream, err, C, n_sets, best);
}

// the lookup score of C rows of sums (total_empty: ROPE_SUM_WORDS words) -> err[0..C), err[C] the best score, err[C + 1] its row
extern "C" int shim_finalize_lookup(uint64_t *sums, const uint64_t *total_empty, int C, double n_pix, double *err, void *stream)
{
    const rope::LinkFlags lf = {};
    return (int)rope::launch_finalize((hipStream_t)stream, sums, total_empty, C, ROPE_LOSS_LOOKUP, 0, n_pix, lf, err);
}
