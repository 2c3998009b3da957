// What a pass leaves in the context's layer buffers, read back for tests/test_gpu_geometry_cache.py: the per-(layer, tile) loss
// sums, the layers' representative candidates and the candidates' masks of the tiles their shared links touch.  Built by that test
// with build.HIPCC_FLAGS and LINKED against the built librope_hip.so, as tests/geometry_shim.hip is; it reads the context through
// csrc/rope_ctx.h — the same header, the same flags, so the same layout — and adds no export to the library.
#include "../rope_s3d_amd/csrc/rope_ctx.h"

// out[0] layers, out[1] tiles, out[2] mask words per candidate, out[3] candidates, out[4] ROPE_SUM_WORDS
extern "C" int shim_layer_shape(rope_ctx *c, int32_t *out)
{
    if (!c || !out) return -1;
    out[0] = c->n_layers; out[1] = c->n_tiles; out[2] = c->mask_words; out[3] = c->C; out[4] = ROPE_SUM_WORDS;
    return 0;
}

// sums: layers x tiles x ROPE_SUM_WORDS; layer_rep: layers; mask_lo: candidates x mask words — after everything in the stream
extern "C" int shim_layer_read(rope_ctx *c, uint64_t *sums, int32_t *layer_rep, uint32_t *mask_lo)
{
    if (!c || !sums || !layer_rep || !mask_lo) return -1;
    const size_t n_sums = (size_t)c->n_layers * c->n_tiles * ROPE_SUM_WORDS, n_mask = (size_t)c->C * c->mask_words;
    if (n_sums > c->d_layer_sums.cap() || (size_t)c->n_layers > c->d_layer_rep.cap() || n_mask > c->d_mask_lo.cap()) return -2;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -3;
    if (hipMemcpy(sums, c->d_layer_sums.get(), n_sums * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    if (hipMemcpy(layer_rep, c->d_layer_rep.get(), (size_t)c->n_layers * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    if (hipMemcpy(mask_lo, c->d_mask_lo.get(), n_mask * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return 0;
}
