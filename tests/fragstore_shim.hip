// The kept fragments of the context (rope_ctx::frags, csrc/rope_fragstore.h), read back for tests/test_gpu_kept_fragments.py: per
// (row, tile) where its groups start, and every group's place.  Built by that test with build.HIPCC_FLAGS and LINKED against the
// built librope_hip.so, as tests/geomcache_shim.hip is; it reads the context through csrc/rope_ctx.h and adds no export to the library.
#include "../rope_s3d_amd/csrc/rope_ctx.h"

// out[0] store valid, out[1] rows, out[2] tiles, out[3] groups in all, out[4] declined, out[5] n_shared of the key, out[6] tiles_x
extern "C" int shim_fragment_shape(rope_ctx *c, int64_t *out)
{
    if (!c || !out) return -1;
    out[0] = c->frags.valid; out[1] = c->C; out[2] = c->n_tiles; out[3] = (int64_t)c->frags.groups; out[4] = c->frags.declined;
    out[5] = c->frags.key.n_shared; out[6] = c->fp.tiles_x;
    return 0;
}

// offs: rows x tiles + 1; where: groups (tile << 12 | group index); finished, base: groups x 4 keys — after everything in the stream
extern "C" int shim_fragment_read(rope_ctx *c, uint64_t *offs, uint32_t *where, uint32_t *finished, uint32_t *base)
{
    if (!c || !offs || !where || !finished || !base || !c->frags.valid) return -1;
    const size_t n_slots = (size_t)c->C * c->n_tiles, n = (size_t)c->frags.groups;
    if (n_slots + 1 > c->d_foffs.cap() || n > c->d_fwhere.cap() || n > c->d_ffin.cap() || n > c->d_fbase.cap()) return -2;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -3;
    if (hipMemcpy(offs, c->d_foffs.get(), (n_slots + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    if (n == 0) return 0;
    if (hipMemcpy(where, c->d_fwhere.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    if (hipMemcpy(finished, c->d_ffin.get(), n * sizeof(uint4), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    if (hipMemcpy(base, c->d_fbase.get(), n * sizeof(uint4), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return 0;
}

// The context as a frame of more than QUEUE_WEIGHT_TILES tiles leaves it (ensure_capacity): no pair weights, one queue segment from
// the start of the item buffer — the layout under which draw_own_links takes its unweighted path.  Drops what is kept.
extern "C" int shim_force_unweighted(rope_ctx *c)
{
    if (!c || c->cap < 1) return -1;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -3;
    c->q_weighted = false;
    c->q_segment = 0;
    c->drop_kept();
    return 0;
}

// fragment_score_kernel<loss> on a synthetic store of ONE row: 256 groups — the first eight sample rows of tile 0, link 5 at mid
// depth in front of nothing — listed `rounds` times over, so that every thread meets its group `rounds` times; against the
// context's single target and frame, no layer.  sums: ROPE_SUM_WORDS words out.  The sums of r rounds are r times those of one.
extern "C" int shim_fragment_score_repeat(rope_ctx *c, int loss, int rounds, uint64_t *sums)
{
    if (!c || !sums || rounds < 1 || c->single.n < 1 || c->n_tiles < 1) return -1;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -3;
    const size_t n = (size_t)256 * rounds;
    std::vector<uint32_t> where(n);
    std::vector<uint4> fin(n), bas(n);
    for (size_t i = 0; i < n; i++) {
        where[i] = fragment_where(0, (uint32_t)(i & 255));
        const uint32_t k = (0x800000u << 8) | 5u;
        fin[i] = make_uint4(k, k, k, k);
        bas[i] = make_uint4(KEY_EMPTY, KEY_EMPTY, KEY_EMPTY, KEY_EMPTY);
    }
    std::vector<unsigned long long> offs((size_t)c->n_tiles + 1, (unsigned long long)n);
    offs[0] = 0;
    DevBuf<uint32_t> d_where, d_mask;
    DevBuf<uint4> d_fin, d_bas;
    DevBuf<unsigned long long> d_offs;
    DevBuf<int32_t> d_zero;
    DevBuf<uint64_t> d_sums;
    if (d_where.grow(n) || d_fin.grow(n) || d_bas.grow(n) || d_offs.grow(offs.size()) || d_mask.grow((size_t)c->mask_words) || d_zero.grow(1) ||
        d_sums.grow(ROPE_SUM_WORDS)) return -2;
    if (hipMemcpy(d_where, where.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_fin, fin.data(), n * sizeof(uint4), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_bas, bas.data(), n * sizeof(uint4), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_offs, offs.data(), offs.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_mask, 0, (size_t)c->mask_words * sizeof(uint32_t)) != hipSuccess || hipMemset(d_zero, 0, sizeof(int32_t)) != hipSuccess ||
        hipMemset(d_sums, 0xEE, ROPE_SUM_WORDS * sizeof(uint64_t)) != hipSuccess) return -4;
    RasterArgs a{};
    a.n_render = ROPE_MAX_LINKS;
    a.mask_lo = d_mask; a.mask_words = c->mask_words;
    a.layer_of = d_zero; a.layer_rep = d_zero;
    a.tq = c->single.tq; a.t32 = c->single.plane32(loss);
    a.sums = d_sums;
    if (launch_fragment_score(loss, 1, c->stream, c->fp, a, d_offs, d_where, d_fin, d_bas) != hipSuccess) return -5;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -6;
    if (hipMemcpy(sums, d_sums.get(), ROPE_SUM_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return 0;
}
