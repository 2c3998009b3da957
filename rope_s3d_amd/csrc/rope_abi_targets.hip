// rope_abi_targets.hip — the targets of many frames behind the C ABI: the resident set (rope_set_targets), its staged twin
// (rope_stage_targets*, rope_commit_targets), the calls that score against them (rope_eval_targets, rope_lookup_score_targets),
// and the camera-pose frames that live in the resident set's planes (rope_set_frames, rope_eval_views).  The context: rope_ctx.h.
#include <algorithm>
#include <cmath>

#include "rope_ctx.h"

extern "C" int rope_set_frames(rope_ctx *c, int n_frames, const double *q, const uint64_t *tq, const float *t32,
                               const uint64_t *link_planes)
{
    if (!c) return ROPE_E_ARG;
    if (!c->have_camera) ARG_FAIL(c, "rope_set_frames: call rope_set_camera first (image size)");
    if (!q || !tq || n_frames < 1 || n_frames > 4096) ARG_FAIL(c, "rope_set_frames: need 1 <= n_frames <= 4096, q and tq");
    for (size_t i = 0; i < 6 * (size_t)n_frames; i++)
        if (!std::isfinite(q[i]) || std::fabs(q[i]) > 1.0e4) ARG_FAIL(c, "rope_set_frames: joint angle not finite or |q| > 1e4 rad");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TargetSet &r = c->resident;
    r.n = 0;                                      // the planes are the camera-pose path's from here on
    const size_t n = (size_t)c->fp.W * c->fp.H * (size_t)n_frames;
    // buffers only ever grow: a predictor calls this once per run with the same shapes
    HIP_TRY(c, r.grow(c->fp.W, c->fp.H, n_frames, t32 != nullptr, false, false));
    int rc = copy_h2d_staged(c, r.tq, tq, n * sizeof(uint64_t));
    if (!rc && t32) rc = copy_h2d_staged(c, r.t32, t32, n * sizeof(float));
    if (rc) return rc;
    if (link_planes) {
        HIP_TRY(c, c->d_ftl.grow(n * ROPE_MAX_LINKS));
        rc = copy_h2d_staged(c, c->d_ftl, link_planes, n * ROPE_MAX_LINKS * sizeof(uint64_t));
        if (rc) return rc;
    }
    HIP_TRY(c, c->resident_empty.grow((size_t)n_frames, (size_t)c->n_tiles));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->h_fq.assign(q, q + 6 * (size_t)n_frames);
    r.has_t32 = (t32 != nullptr);
    r.has_ts = false;
    c->frames_tl = (link_planes != nullptr);
    c->resident_empty.invalidate();
    c->holds = rope_ctx::FRAMES;
    r.n = n_frames;
    return ROPE_OK;
}

extern "C" int rope_eval_views(rope_ctx *c, const double *PV, int K, int n_render, int loss, uint64_t *sums_out)
{
    if (!c) return ROPE_E_ARG;
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "rope_eval_views: robot and camera must be set first");
    if (c->n_frames() < 1) ARG_FAIL(c, "rope_eval_views: no frames set");
    if (!PV || !sums_out || K < 1) ARG_FAIL(c, "rope_eval_views: bad arguments");
    if ((long long)K * c->n_frames() > 65535) ARG_FAIL(c, "rope_eval_views: views x frames must not exceed 65535");
    if (n_render < 1 || n_render > c->n_links) ARG_FAIL(c, "rope_eval_views: n_render out of range");
    if (loss != ROPE_LOSS_DEPTH && loss != ROPE_LOSS_TSWEEP && loss != ROPE_LOSS_CAMFULL) ARG_FAIL(c, "rope_eval_views: loss must be DEPTH, TSWEEP or CAMFULL");
    if (loss == ROPE_LOSS_TSWEEP && !c->resident.has_t32) ARG_FAIL(c, "rope_eval_views: this loss needs the frames' float32 planes");
    if (loss == ROPE_LOSS_CAMFULL && !c->frames_tl) ARG_FAIL(c, "rope_eval_views: this loss needs the frames' link planes");
    for (size_t i = 0; i < 16 * (size_t)K; i++)
        if (!std::isfinite(PV[i])) ARG_FAIL(c, "rope_eval_views: non-finite view matrix");
    HIP_TRY(c, hipSetDevice(c->device));
    c->clip_views = false;
    for (int k = 0; k < K; k++) c->clip_views = c->clip_views || near_plane_in_reach(c, PV + 16 * (size_t)k);
    const TargetSet &r = c->resident;
    const int N = r.n, C = K * N;
    int rc = ensure_capacity(c, C);
    if (rc) return rc;
    // One pinned block -> one copy: candidate (k, i) = view k, frame i (joint vector of frame i, scored against frame
    // i's planes) | the K view matrices | view index | frame index
    const size_t off_pv = 6 * (size_t)C * sizeof(double), off_vo = off_pv + 16 * (size_t)K * sizeof(double),
                 off_fo = off_vo + (size_t)C * sizeof(int32_t), bytes = off_fo + (size_t)C * sizeof(int32_t);
    rc = sync_grow(c, c->h_vstage, bytes, c->d_vstage, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // the block may still feed the previous call's copy
    double *hc = reinterpret_cast<double *>(c->h_vstage.get());
    int32_t *hvo = reinterpret_cast<int32_t *>(c->h_vstage + off_vo), *hfo = reinterpret_cast<int32_t *>(c->h_vstage + off_fo);
    for (int k = 0; k < K; k++)
        for (int i = 0; i < N; i++) {
            std::memcpy(hc + 6 * ((size_t)k * N + i), &c->h_fq[6 * (size_t)i], 6 * sizeof(double));
            hvo[(size_t)k * N + i] = k;
            hfo[(size_t)k * N + i] = i;
        }
    std::memcpy(c->h_vstage + off_pv, PV, 16 * (size_t)K * sizeof(double));
    HIP_TRY(c, hipMemcpyAsync(c->d_vstage, c->h_vstage, bytes, hipMemcpyHostToDevice, c->stream));
    c->dv_cand = reinterpret_cast<const double *>(c->d_vstage.get());
    c->dv_PV = reinterpret_cast<const double *>(c->d_vstage + off_pv);
    c->dv_view_of = reinterpret_cast<const int32_t *>(c->d_vstage + off_vo);
    c->dv_frame_of = reinterpret_cast<const int32_t *>(c->d_vstage + off_fo);
    c->C = C;
    c->cand_valid = false;                            // the rows are (view, frame) pairs now: cand_dev / err_on_host describe nothing
    c->results_valid = false;
    c->cand_dev = nullptr;
    c->n_layers = C;                                  // every (view, frame) candidate is its own layer: nothing shared
    const size_t plane = (size_t)c->fp.W * c->fp.H;
    const uint64_t *tl = c->frames_tl ? c->d_ftl.get() : nullptr;
    uint64_t *ftotal = c->resident_empty.total(loss);
    if (!c->resident_empty.fresh(loss, c->fp)) {
        // sums of every frame with nothing rendered: the raster launch only adds what the render changes (frame by frame: the
        // link planes of a frame lie together)
        for (int i = 0; i < N; i++)
            HIP_TRY(c, launch_empty(loss, c->stream, c->fp, r.tq + (size_t)i * plane, r.has_t32 ? r.t32 + (size_t)i * plane : nullptr,
                                    tl ? tl + (size_t)i * plane * ROPE_MAX_LINKS : nullptr, c->resident_empty.scratch,
                                    ftotal + (size_t)i * ROPE_SUM_WORDS));
        c->resident_empty.filled(loss, c->fp);
    }
    rc = enqueue_eval(c, n_render, loss, c->fp, (double)plane, {r.tq, r.plane32(loss), tl, c->dv_frame_of}, EVAL_VIEWS);
    if (rc) return rc;
    const size_t n_sums = (size_t)C * ROPE_SUM_WORDS, n_tot = (size_t)N * ROPE_SUM_WORDS;
    HIP_TRY(c, c->h_vsums.grow(n_sums + n_tot));
    HIP_TRY(c, hipMemcpyAsync(c->h_vsums, c->d_sums, n_sums * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_vsums + n_sums, ftotal, n_tot * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t *total = c->h_vsums + n_sums;
    std::memcpy(sums_out, c->h_vsums, n_sums * sizeof(uint64_t));
    const bool links = (loss == ROPE_LOSS_CAMFULL);
    for (int k = 0; k < K; k++)
        for (int i = 0; i < N; i++)
            for (int w = 0; w < ROPE_SUM_WORDS; w++) {
                uint64_t &o = sums_out[((size_t)k * N + i) * ROPE_SUM_WORDS + w];
                const bool live = w < SUM_LINK0 || (links && w < SUM_LINK0 + 3 * n_render);
                o = live ? o + total[(size_t)i * ROPE_SUM_WORDS + w] : 0;      // modulo 2^64, as the kernel's deltas are
            }
    return ROPE_OK;
}

// per-frame scratch of the batched prediction, sized for n_frames resident targets
static int size_target_scratch(rope_ctx *c, int n_frames)
{
    HIP_TRY(c, c->resident_empty.grow((size_t)n_frames, (size_t)c->n_tiles));
    HIP_TRY(c, c->d_tg_ltotal.grow((size_t)n_frames * ROPE_SUM_WORDS));
    HIP_TRY(c, c->d_tg_best.grow(2 * (size_t)n_frames));
    return ROPE_OK;
}

// ---- batched prediction: the targets of many frames resident at once, every row of a batch scored against its own frame's
extern "C" int rope_set_targets(rope_ctx *c, int n_frames, const uint64_t *tq, const float *t32, const float *t32_tsweep, const uint8_t *link_flags)
{
    if (!c) return ROPE_E_ARG;
    if (!c->have_camera) ARG_FAIL(c, "rope_set_targets: call rope_set_camera first (image size)");
    if (!tq || !link_flags || n_frames < 1 || n_frames > 65535) ARG_FAIL(c, "rope_set_targets: need 1 <= n_frames <= 65535, tq and link_flags");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TargetSet &r = c->resident;
    r.n = 0;                                      // whatever it held, targets or the camera-pose path's frames
    const size_t n = (size_t)c->fp.W * c->fp.H * (size_t)n_frames;
    HIP_TRY(c, r.grow(c->fp.W, c->fp.H, n_frames, t32 != nullptr, t32_tsweep != nullptr, true));
    int rc = copy_h2d_staged(c, r.tq, tq, n * sizeof(uint64_t));
    if (!rc && t32) rc = copy_h2d_staged(c, r.t32, t32, n * sizeof(float));
    if (!rc && t32_tsweep) rc = copy_h2d_staged(c, r.ts, t32_tsweep, n * sizeof(float));
    static_assert(sizeof(LinkFlags) == 8, "link flags travel as 8 bytes per frame");
    if (!rc) rc = copy_h2d_staged(c, r.flags, link_flags, 8 * (size_t)n_frames);
    if (!rc) rc = size_target_scratch(c, n_frames);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    r.has_t32 = (t32 != nullptr);
    r.has_ts = (t32_tsweep != nullptr);
    c->resident_empty.invalidate();
    c->holds = rope_ctx::TARGETS;
    r.n = n_frames;
    return ROPE_OK;
}

// rope_stage_targets and the slot-filling calls may run beside an evaluation on another thread, so nothing in them waits on, or
// reports through, anything the evaluation calls use.

// waits for everything rope_stage_targets_segmented enqueued on its callers' streams
static int drain_stage_events(rope_ctx *c)
{
    int rc = ROPE_OK;
    for (hipEvent_t e : c->stage_events) {
        if (hipEventSynchronize(e) != hipSuccess) rc = ROPE_E_HIP;
        (void)hipEventDestroy(e);
    }
    c->stage_events.clear();
    return rc;
}

// The same targets as rope_set_targets, but into the context's SECOND set of planes and on a stream of its own: returns once the
// copies are enqueued (page-locked sources, rope_host_alloc) — the resident set stays in use meanwhile, from this or another thread
// (this call touches nothing the evaluation calls use).  The host buffers belong to the copy until rope_commit_targets returns.
extern "C" int rope_stage_targets(rope_ctx *c, int n_frames, const uint64_t *tq, const float *t32, const float *t32_tsweep, const uint8_t *link_flags)
{
    if (!c) return ROPE_E_ARG;
    // this call may run beside an evaluation on another thread: its failures are reported through the return code and a message of its own
    auto fail = [&](int code, const char *msg) { c->stage_err = msg; return code; };
    c->stage_err.clear();
    if (!c->have_camera) return fail(ROPE_E_ARG, "rope_stage_targets: call rope_set_camera first (image size)");
    if (!tq || !link_flags || n_frames < 1 || n_frames > 65535) return fail(ROPE_E_ARG, "rope_stage_targets: need 1 <= n_frames <= 65535, tq and link_flags");
    if (hipSetDevice(c->device) != hipSuccess) return fail(ROPE_E_HIP, "rope_stage_targets: hipSetDevice failed");
    if (!c->copy_stream && hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) return fail(ROPE_E_HIP, "rope_stage_targets: no stream");
    if (hipStreamSynchronize(c->copy_stream) != hipSuccess) return fail(ROPE_E_HIP, "rope_stage_targets: the upload stream failed");
    if (drain_stage_events(c)) return fail(ROPE_E_HIP, "rope_stage_targets: a staging kernel failed");     // of a set left unfinished
    c->seg_n_total = 0;
    TargetSet &s = c->staged;
    s.n = 0;
    const size_t n = (size_t)c->fp.W * c->fp.H * (size_t)n_frames;
    if (s.grow(c->fp.W, c->fp.H, n_frames, t32 != nullptr, t32_tsweep != nullptr, true)) { (void)hipGetLastError(); return fail(ROPE_E_NOMEM, "rope_stage_targets: out of device memory"); }
    // the few bytes of flags first: a small (or pageable) source goes through the pinned block, which waits for the stream
    int rc = copy_h2d_on(c->copy_stream, c->h_copy2, c->stage_err, s.flags, link_flags, 8 * (size_t)n_frames);
    if (!rc) rc = copy_h2d_on(c->copy_stream, c->h_copy2, c->stage_err, s.tq, tq, n * sizeof(uint64_t));
    if (!rc && t32) rc = copy_h2d_on(c->copy_stream, c->h_copy2, c->stage_err, s.t32, t32, n * sizeof(float));
    if (!rc && t32_tsweep) rc = copy_h2d_on(c->copy_stream, c->h_copy2, c->stage_err, s.ts, t32_tsweep, n * sizeof(float));
    if (rc) return rc;
    s.has_t32 = (t32 != nullptr);
    s.has_ts = (t32_tsweep != nullptr);
    s.n = n_frames;
    return ROPE_OK;
}

// What a call that fills slots of the staged set ON THE DEVICE starts with, its arguments checked: a call with slot0 > 0 must go on
// with the set as it was started; the staged planes are written from here on, so a complete staging is withdrawn; slot0 == 0 sizes
// a new set of n_total frames.  `who` names the caller in the messages.
static int stage_slots_begin(rope_ctx *c, const char *who, int n_total, int slot0, bool ts)
{
    auto fail = [&](int code, const char *msg) { c->stage_err = std::string(who) + msg; return code; };
    const int W = c->fp.W, H = c->fp.H;
    if (slot0 > 0 && (c->seg_n_total != n_total || c->seg_ts != ts || c->staged.W != W || c->staged.H != H))
        return fail(ROPE_E_ARG, ": n_total, want_tsweep or the image size changed in mid-set (slot0 == 0 starts a set)");
    if (hipSetDevice(c->device) != hipSuccess) return fail(ROPE_E_HIP, ": hipSetDevice failed");
    c->staged.n = 0;                              // the staged planes are written from here on: complete again when every slot is filled
    if (slot0 != 0) return ROPE_OK;
    c->seg_n_total = 0;                           // a new set: sized here, once
    if (c->copy_stream && hipStreamSynchronize(c->copy_stream) != hipSuccess) return fail(ROPE_E_HIP, ": the upload stream failed");
    if (drain_stage_events(c)) return fail(ROPE_E_HIP, ": a staging kernel failed");   // of a set left unfinished
    if (c->staged.grow(W, H, n_total, true, ts, true) || c->s_counts.grow((size_t)n_total * 2 * ROPE_MAX_LINKS) != 0) {
        (void)hipGetLastError();
        return fail(ROPE_E_NOMEM, ": out of device memory");
    }
    c->meta_used = 0;
    c->seg_filled.assign((size_t)n_total, 0);
    c->seg_n_filled = 0;
    c->seg_ts = ts;
    c->seg_n_total = n_total;
    return ROPE_OK;
}

// ... and ends with, its kernels enqueued: the slots are marked, and the set is complete once every one of them has been filled
static void stage_slots_filled(rope_ctx *c, int n_total, int slot0, int n_frames, bool ts)
{
    for (int i = slot0; i < slot0 + n_frames; i++)
        if (!c->seg_filled[i]) { c->seg_filled[i] = 1; c->seg_n_filled++; }
    if (c->seg_n_filled == n_total) {
        c->staged.has_t32 = true;
        c->staged.has_ts = ts;
        c->staged.n = n_total;
    }
}

// The staged set filled on the DEVICE, slots slot0 .. slot0 + n_frames - 1 of n_total: the segmentation path's targets from instance
// masks that are in HBM already (rope_targets.hip: what rope_prepare_segmented computes per frame at f == 1).  The kernels go onto
// `stream`, the caller's, behind the work that produced the masks; the call does not wait for them — rope_commit_targets does.
extern "C" int rope_stage_targets_segmented(rope_ctx *c, int n_total, int slot0, int n_frames, const void *depth_dev, int depth_kind,
                                            const uint8_t *masks_dev, const int32_t *inst_first, const int32_t *link_of, int n_lookup_links,
                                            int want_tsweep, void *stream)
{
    if (!c) return ROPE_E_ARG;
    auto fail = [&](int code, const char *msg) { c->stage_err = msg; return code; };
    c->stage_err.clear();
    // the arguments first: a refused call changes nothing, neither a staging that waits for its commit nor a set half filled
    if (!c->have_camera || !c->have_robot) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: robot and camera must be set first");
    if (n_total < 1 || n_total > 65535 || n_frames < 1 || slot0 < 0 || slot0 > n_total || n_frames > n_total - slot0)
        return fail(ROPE_E_ARG, "rope_stage_targets_segmented: need 1 <= n_total <= 65535 and slots slot0 .. slot0 + n_frames - 1 inside it");
    if (depth_kind != 1 && depth_kind != 2) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: depth_kind is 1 (float32) or 2 (float64)");
    if (!depth_dev || !inst_first) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: depth_dev and inst_first are required");
    if (n_lookup_links < 0 || n_lookup_links > c->n_links) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: n_lookup_links outside 0 .. n_links");
    if (inst_first[0] < 0) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: inst_first not monotone");
    for (int i = 0; i < n_frames; i++)
        if (inst_first[i + 1] < inst_first[i]) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: inst_first not monotone");
    const int K = inst_first[n_frames];
    if (K > 0 && (!masks_dev || !link_of)) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: instances without masks_dev / link_of");
    for (int k = 0; k < K; k++)
        if (link_of[k] < -1 || link_of[k] >= c->n_links) return fail(ROPE_E_ARG, "rope_stage_targets_segmented: link_of outside -1 .. n_links - 1");
    const bool ts = want_tsweep != 0;
    if (int rc = stage_slots_begin(c, "rope_stage_targets_segmented", n_total, slot0, ts)) return rc;
    const int W = c->fp.W, H = c->fp.H;
    const size_t plane = (size_t)W * H;
    // this call's tables, appended: plane offsets | links present per frame | code per plane
    const size_t need = 2 * (size_t)n_frames + 1 + (size_t)K;
    if (c->meta_used + need > c->d_meta.cap()) {  // the kernels in flight read the old block: wait for them, then start a larger one
        if (drain_stage_events(c)) return fail(ROPE_E_HIP, "rope_stage_targets_segmented: a staging kernel failed");
        const size_t cap = std::max<size_t>(std::max<size_t>(2 * c->d_meta.cap(), need), 4096);
        c->meta_used = 0;
        c->d_meta.release();                      // the device block, allocated last, says how large the pair is
        if (c->h_meta.reset(cap) || c->d_meta.reset(cap)) {
            (void)hipGetLastError();
            return fail(ROPE_E_NOMEM, "rope_stage_targets_segmented: out of memory");
        }
    }
    int32_t *m = c->h_meta + c->meta_used;
    for (int i = 0; i <= n_frames; i++) m[i] = inst_first[i];
    for (int i = 0; i < n_frames; i++) {
        int present = 0;
        for (int k = inst_first[i]; k < inst_first[i + 1]; k++)
            if (link_of[k] >= 0) present |= 1 << link_of[k];
        m[n_frames + 1 + i] = present;
    }
    for (int k = 0; k < K; k++)
        m[2 * n_frames + 1 + k] = 0x200 | (link_of[k] >= 0 ? (1 << link_of[k]) | (link_of[k] < n_lookup_links ? 0x100 : 0) : 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t *meta_dev = c->d_meta + c->meta_used;
    if (hipMemcpyAsync(c->d_meta + c->meta_used, m, need * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(ROPE_E_HIP, "rope_stage_targets_segmented: hipMemcpyAsync failed");
    c->meta_used += need;
    const size_t o = plane * (size_t)slot0;
    hipEvent_t done = nullptr;
    if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) return fail(ROPE_E_HIP, "rope_stage_targets_segmented: no event");
    c->stage_events.push_back(done);              // recorded or not, the next wait gets rid of it
    if (launch_segmented_targets(st, H, W, n_frames, depth_dev, depth_kind, masks_dev, meta_dev, c->n_links, c->staged.tq + o, c->staged.t32 + o,
                                 ts ? c->staged.ts + o : nullptr, c->s_counts + (size_t)slot0 * 2 * ROPE_MAX_LINKS, c->staged.flags + slot0) != hipSuccess ||
        hipEventRecord(done, st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ROPE_E_HIP, "rope_stage_targets_segmented: the launch failed");
    }
    stage_slots_filled(c, n_total, slot0, n_frames, ts);
    return ROPE_OK;
}

// The same slots filled from full-size renders that are in HBM already (rope_synth.hip: what rope_prepare_synthetic computes per
// frame for the colour plane blue_of_id[ids] and float32 depth, the down-sampling included).  Slots, completion, commit, threading
// and refusals are those of rope_stage_targets_segmented.
extern "C" int rope_stage_targets_synthetic(rope_ctx *c, int n_total, int slot0, int n_frames, const float *depth_dev, const uint8_t *ids_dev,
                                            int H0, int W0, int f, const uint8_t *blue_of_id, const int32_t *link_blue, int n_links,
                                            int n_lookup_links, int want_tsweep, void *stream)
{
    if (!c) return ROPE_E_ARG;
    auto fail = [&](int code, const char *msg) { c->stage_err = msg; return code; };
    c->stage_err.clear();
    // the arguments first: a refused call changes nothing, neither a staging that waits for its commit nor a set half filled
    if (!c->have_camera || !c->have_robot) return fail(ROPE_E_ARG, "rope_stage_targets_synthetic: robot and camera must be set first");
    if (n_total < 1 || n_total > 65535 || n_frames < 1 || slot0 < 0 || slot0 > n_total || n_frames > n_total - slot0)
        return fail(ROPE_E_ARG, "rope_stage_targets_synthetic: need 1 <= n_total <= 65535 and slots slot0 .. slot0 + n_frames - 1 inside it");
    if (!depth_dev || !ids_dev || !blue_of_id || !link_blue) return fail(ROPE_E_ARG, "rope_stage_targets_synthetic: depth_dev, ids_dev, blue_of_id and link_blue are required");
    if (n_links < 1 || n_links > ROPE_MAX_LINKS || n_lookup_links < 0 || n_lookup_links > n_links)
        return fail(ROPE_E_ARG, "rope_stage_targets_synthetic: need 1 <= n_links <= 6 and n_lookup_links inside 0 .. n_links");
    if (H0 < 1 || W0 < 1 || f < 1 || (f > 1 && (f & 1)) || H0 % f || W0 % f || H0 / f != c->fp.H || W0 / f != c->fp.W)
        return fail(ROPE_E_ARG, "rope_stage_targets_synthetic: f is 1 or even, and H0 / f x W0 / f must be the image size of rope_set_camera");
    const bool ts = want_tsweep != 0;
    if (int rc = stage_slots_begin(c, "rope_stage_targets_synthetic", n_total, slot0, ts)) return rc;
    const size_t plane = (size_t)c->fp.W * c->fp.H, o = plane * (size_t)slot0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = nullptr;
    if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) return fail(ROPE_E_HIP, "rope_stage_targets_synthetic: no event");
    c->stage_events.push_back(done);              // recorded or not, the next wait gets rid of it
    if (launch_synthetic_targets(st, H0, W0, f, n_frames, depth_dev, ids_dev, blue_of_id, link_blue, n_links, n_lookup_links, c->staged.tq + o,
                                 c->staged.t32 + o, ts ? c->staged.ts + o : nullptr, c->s_counts + (size_t)slot0 * 2 * ROPE_MAX_LINKS,
                                 c->staged.flags + slot0) != hipSuccess ||
        hipEventRecord(done, st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ROPE_E_HIP, "rope_stage_targets_synthetic: the launch failed");
    }
    stage_slots_filled(c, n_total, slot0, n_frames, ts);
    return ROPE_OK;
}

// The resident set of targets back to the host, for tests: tq / t32 / t32_tsweep n_targets planes, flags n_targets x 8 bytes; any
// may be NULL.
extern "C" int rope_debug_targets(rope_ctx *c, uint64_t *tq, float *t32, float *t32_tsweep, uint8_t *flags)
{
    if (!c) return ROPE_E_ARG;
    const TargetSet &r = c->resident;
    if (c->n_targets() < 1) ARG_FAIL(c, "rope_debug_targets: no targets set (rope_set_targets / rope_commit_targets)");
    if ((t32 && !r.has_t32) || (t32_tsweep && !r.has_ts)) ARG_FAIL(c, "rope_debug_targets: the resident set has no such float32 planes");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->fp.W * c->fp.H * (size_t)r.n;
    int rc = ROPE_OK;
    if (tq) rc = copy_d2h_staged(c, tq, r.tq, n * sizeof(uint64_t));
    if (!rc && t32) rc = copy_d2h_staged(c, t32, r.t32, n * sizeof(float));
    if (!rc && t32_tsweep) rc = copy_d2h_staged(c, t32_tsweep, r.ts, n * sizeof(float));
    if (!rc && flags) rc = copy_d2h_staged(c, flags, r.flags, 8 * (size_t)r.n);
    return rc;
}

// How many targets are resident: what rope_predict_batch (rope_predict.cpp, written against the public ABI) holds n_frames to
extern "C" int rope_resident_targets(rope_ctx *c) { return c ? c->n_targets() : 0; }

// The staged set becomes the resident one (and the resident buffers the next staging space): waits for the upload and for the
// context's own stream, then swaps the sets whole — a buffer the staged set did not fill comes along unread (has_t32 / has_ts).
extern "C" int rope_commit_targets(rope_ctx *c)
{
    if (!c) return ROPE_E_ARG;
    if (c->staged.n < 1) { c->err = c->stage_err.empty() ? "rope_commit_targets: nothing staged (rope_stage_targets)" : c->stage_err; return ROPE_E_ARG; }
    if (c->staged.W != c->fp.W || c->staged.H != c->fp.H) { c->staged.n = 0; ARG_FAIL(c, "rope_commit_targets: the image size changed since rope_stage_targets"); }
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->copy_stream) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    if (drain_stage_events(c)) { c->staged.n = 0; c->seg_n_total = 0; c->err = "rope_commit_targets: a staging kernel failed"; return ROPE_E_HIP; }
    c->seg_n_total = 0;                           // the set is taken: a later rope_stage_targets_segmented starts at slot 0
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int n_frames = c->staged.n;
    c->resident.swap(c->staged);
    c->staged.n = c->resident.n = 0;              // what was resident, targets or frames, is gone
    c->resident_empty.invalidate();
    c->holds = rope_ctx::TARGETS;
    int rc = size_target_scratch(c, n_frames);
    if (rc) return rc;
    c->resident.n = n_frames;
    return ROPE_OK;
}

extern "C" int rope_eval_targets(rope_ctx *c, const double *cand, const int32_t *frame_of, int R, int n_render, int loss, const int32_t *crop,
                                 double *err_out)
{
    if (!c) return ROPE_E_ARG;
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "rope_eval_targets: robot and camera must be set first");
    const TargetSet &r = c->resident;
    if (c->n_targets() < 1) ARG_FAIL(c, "rope_eval_targets: no targets set (rope_set_targets)");
    if (!cand || !frame_of || !err_out || R < 1) ARG_FAIL(c, "rope_eval_targets: bad arguments");
    if (n_render < 1 || n_render > c->n_links) ARG_FAIL(c, "rope_eval_targets: n_render out of range");
    if (loss < 0 || loss > 3) ARG_FAIL(c, "rope_eval_targets: unknown loss");
    if (loss == ROPE_LOSS_LOOKUP && !r.has_t32) ARG_FAIL(c, "rope_eval_targets: this loss needs the targets' float32 planes");
    if (loss == ROPE_LOSS_TSWEEP && !r.plane32(loss)) ARG_FAIL(c, "rope_eval_targets: this loss needs float32 planes");
    for (int i = 0; i < R; i++)
        if (frame_of[i] < 0 || frame_of[i] >= r.n) ARG_FAIL(c, "rope_eval_targets: frame index outside the resident targets");
    FrameParams fp;
    double n_pix;
    int rc = loss_frame(c, "rope_eval_targets", loss, crop, fp, n_pix);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = ensure_totals(c, r, c->resident_empty, loss, fp);
    if (rc) return rc;
    for (int lo = 0; lo < R; lo += MAX_ROWS) {
        const int n = std::min(MAX_ROWS, R - lo);
        rc = upload_candidates(c, cand + 6 * (size_t)lo, n, true, frame_of + lo);
        if (rc) return rc;
        rc = enqueue_eval(c, n_render, loss, fp, n_pix, {r.tq, r.plane32(loss), nullptr, c->frame_of_dev}, EVAL_TARGETS);
        // the rows are scored against the frames' targets: nothing here is a result of the single-target calls
        c->cand_valid = c->results_valid = false;
        if (rc) return rc;
        if (!c->err_on_host) HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->d_err, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::memcpy(err_out + lo, c->err_on_host ? c->h_err.get() : c->h_stage.get(), (size_t)n * sizeof(double));
    }
    return ROPE_OK;
}

extern "C" int rope_lookup_score_targets(rope_ctx *c, int32_t *best_idx, double *best_score, double *scores_out)
{
    if (!c) return ROPE_E_ARG;
    if (c->table_C < 1) ARG_FAIL(c, "rope_lookup_score_targets: no table built");
    if (c->n_targets() < 1 || !c->resident.has_t32) ARG_FAIL(c, "rope_lookup_score_targets: needs targets with their float32 planes (rope_set_targets)");
    if (!best_idx) ARG_FAIL(c, "rope_lookup_score_targets: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    const FrameParams fp = table_frame(c);
    const size_t crop_px = table_crop_words(fp), N = (size_t)c->resident.n;     // crop rows padded to whole groups of four samples
    if (int rc = sync_grow(c, c->d_tg_t32c, N * crop_px)) return rc;
    if (int rc = sync_grow(c, c->d_tg_scores, N * c->table_C)) return rc;
    HIP_TRY(c, launch_table_score_frames(c->stream, fp, c->d_tcount, c->d_toff, c->d_tgoff, c->d_tgval, c->table_C, c->resident.t32, c->resident.n, c->d_tg_t32c, c->d_tg_ltotal,
                                         c->d_tg_scores, c->d_tg_best));
    std::vector<double> best(2 * N);
    HIP_TRY(c, hipMemcpyAsync(best.data(), c->d_tg_best, 2 * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (scores_out) HIP_TRY(c, hipMemcpyAsync(scores_out, c->d_tg_scores, N * c->table_C * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t f = 0; f < N; f++) {
        best_idx[f] = (int32_t)best[2 * f + 1];
        if (best_score) best_score[f] = best[2 * f];
    }
    return ROPE_OK;
}
