// rope_ctx.h — the context behind the C ABI and what the files that implement it share: rope_abi.hip (life cycle, robot, camera,
// single target, candidates, evaluation, render, table) and rope_abi_targets.hip (the sets of targets and the camera-pose frames).
// Host only, no translation unit of its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "rope_buffers.h"
#include "rope_fragstore.h"
#include "rope_geomcache.h"
#include "rope_kernels.h"
#include "rope_passplan.h"

using namespace rope;

// The target planes of n frames at one image size.  The context has three: `single` (n = 1; its link flags stay on the host, in
// rope_ctx::lf, which launch_finalize takes by value), `resident` (rope_set_targets / rope_commit_targets, or the camera-pose
// frames of rope_set_frames) and `staged` (the next resident set, filled while the resident one is in use).
struct TargetSet {
    DevBuf<uint64_t> tq;                    // packed planes
    DevBuf<float> t32, ts;                  // lookup planes; TensorSweep planes (the whole target depth as float32), when given
    DevBuf<LinkFlags> flags;                // per frame
    int n = 0, W = 0, H = 0;                // n 0: nothing set
    bool has_t32 = false, has_ts = false;   // a buffer may outlive its planes (swap): these say what the set holds, and gate every read

    // The float32 plane a loss reads: TensorSweep takes the whole target depth when it was given, everything else — and
    // TensorSweep without it — the lookup plane.
    const float *plane32(int loss) const { return (loss == ROPE_LOSS_TSWEEP && has_ts) ? ts.get() : (has_t32 ? t32.get() : nullptr); }
    // room for `frames` frames of W_ x H_, the set's image size from here on; contents are not carried over, and n / has_* are the
    // caller's to set once the planes are there
    int grow(int W_, int H_, int frames, bool want_t32, bool want_ts, bool want_flags)
    {
        const size_t px = (size_t)W_ * H_ * (size_t)frames;
        W = W_; H = H_;
        int e = tq.grow(px);
        if (!e && want_t32) e = t32.grow(px);
        if (!e && want_ts) e = ts.grow(px);
        if (!e && want_flags) e = flags.grow((size_t)frames);
        return e;
    }
    void swap(TargetSet &o)
    {
        tq.swap(o.tq); t32.swap(o.t32); ts.swap(o.ts); flags.swap(o.flags);
        std::swap(n, o.n); std::swap(W, o.W); std::swap(H, o.H); std::swap(has_t32, o.has_t32); std::swap(has_ts, o.has_ts);
    }
};

// "Nothing rendered": per loss the sums of a set's frames with nothing drawn, which a pass adds its render's deltas to.  Valid for
// the planes they were computed from — whoever changes a plane invalidates — and for one crop.
struct EmptyCache {
    DevBuf<uint64_t> totals, scratch;       // totals: per loss a block of frames x ROPE_SUM_WORDS; scratch: the per-tile sums they are added up from
    bool valid[5] = {};
    int crop[5][4] = {};

    int grow(size_t frames, size_t tiles)
    {
        const int e = totals.grow(5 * frames * ROPE_SUM_WORDS);
        return e ? e : scratch.grow(frames * tiles * ROPE_SUM_WORDS);
    }
    uint64_t *total(int loss) const { return totals + (size_t)loss * (totals.cap() / 5); }
    void invalidate() { for (bool &v : valid) v = false; }
    bool fresh(int loss, const FrameParams &fp) const
    {
        const int cr[4] = {fp.r0, fp.r1, fp.c0, fp.c1};
        return valid[loss] && std::memcmp(cr, crop[loss], sizeof cr) == 0;
    }
    void filled(int loss, const FrameParams &fp) { valid[loss] = true; crop[loss][0] = fp.r0; crop[loss][1] = fp.r1; crop[loss][2] = fp.c0; crop[loss][3] = fp.c1; }
};

// Every buffer the context owns is a DevBuf / PinnedBuf member (rope_buffers.h): the pointer and its size travel together, and
// what is not released earlier goes with the context.  Plain pointers below own nothing.
struct rope_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // robot
    bool have_robot = false;
    RobotParams rp{};
    DevBuf<uint32_t> d_header, d_tris;
    DevBuf<float> d_verts, d_aabb;
    DevBuf<double> d_joint_fixed, d_joint_axes;
    int n_links = 0, n_meshlets = 0;
    double reach = 0.0;                     // no point of any link, at any joint angles, is farther than this from the base frame's origin
    double h_PV[16] = {};                   // host copy of the camera matrix (the near-plane test below)
    bool clip_views = false;                // rope_eval_views: one of the call's cameras is close enough for near-plane clipping

    // camera
    bool have_camera = false;
    FrameParams fp{};
    DevBuf<double> d_PV;
    int n_tiles = 0;

    // the single target (rope_set_target; `ts`: rope_set_target_tsweep) and its link flags
    TargetSet single;
    LinkFlags lf{};
    EmptyCache single_empty;
    // What the evaluation calls score against besides it.  `resident` holds the targets of rope_set_targets / rope_commit_targets
    // or — in the same tq / t32 planes — the frames of the camera-pose path: setting one kind replaces the other, and `holds`
    // says which is there while resident.n > 0.  `staged`: rope_stage_targets* fill it beside an evaluation, rope_commit_targets
    // swaps it with `resident`.  One cache serves either kind; set and commit invalidate it.
    enum Holds { TARGETS, FRAMES };
    TargetSet resident, staged;
    Holds holds = TARGETS;
    EmptyCache resident_empty;
    int n_targets() const { return holds == TARGETS ? resident.n : 0; }
    int n_frames() const { return holds == FRAMES ? resident.n : 0; }
    // what only frames have: their joint vectors (n x 6) and, when given, their per-link planes
    std::vector<double> h_fq;
    DevBuf<uint64_t> d_ftl;
    bool frames_tl = false;

    // candidates + results: one group of per-candidate buffers, all sized for `cap` rows by ensure_capacity
    int C = 0, cap = 0;
    DevBuf<double> d_cand, d_err, d_best_err;
    PinnedBuf<double> h_stage;             // pinned staging: candidates up, errors + best down
    // small batches: the finalize kernel writes errors + best straight into mapped pinned host memory (no copy command)
    static constexpr int HOST_ERR_ROWS = 256;
    // lockstep batches (rope_eval_targets): a step's rows — 2 to 26 per frame, hundreds of frames — go up, and their errors come
    // back, through mapped host memory as well: a pass reads every row once and writes every error once, and the three copy
    // commands it would otherwise queue (rows, frame indices, errors: 20-30 us of stream time each between 100 us of kernels)
    // were a fifth of the device's time in a lockstep run
    static constexpr int TARGET_HOST_ROWS = 16384;
    PinnedBuf<double> h_err{true};         // mapped: the device writes through dev()
    // small batches: the candidates stay in mapped host memory and the FK kernel reads them from there — no copy command
    // in front of the first launch of a latency-bound chain
    PinnedBuf<double> h_cand{true};
    const double *cand_dev = nullptr;      // where the resident candidates are: d_cand or h_cand.dev()
    bool err_on_host = false;
    // rope_eval_views / rope_lookup_score reuse C and the per-candidate buffers for rows of their own: after them the
    // resident candidates (and the results of the last eval) are gone until rope_candidates_upload / the next eval
    bool cand_valid = false, results_valid = false;
    DevBuf<float> d_mvp;
    DevBuf<short4> d_bounds;
    DevBuf<uint32_t> d_mask_lo, d_mask_hi;
    int mask_words = 0;
    // shared upstream layers: candidates with bit-identical (q0, q1) have identical links 0..2
    int n_layers = 0;
    DevBuf<int32_t> d_layer_of, d_layer_rep;
    DevBuf<uint32_t> d_layers;             // keys
    DevBuf<uint64_t> d_layer_sums;
    // second level of sharing: layers with bit-identical q0 have identical links 0..1 ("parents")
    int n_parents = 0;
    DevBuf<int32_t> d_parent_of, d_parent_rep;   // layer -> parent; parent -> representative candidate
    DevBuf<uint32_t> d_parents;
    DevBuf<uint64_t> d_sums;
    DevBuf<int32_t> d_best_idx;
    int last_n_render = 0;
    // A fixed grid's geometry, kept from pass to pass: d_mvp, d_bounds, the masks, the queue weights and the layer key tiles (with
    // d_parents behind them) are functions of robot, camera, candidates, n_render and launch structure only — never of the target.
    // `geo` says which large layered EVAL_SINGLE pass built them; the next pass with the same key skips the geometry and layer
    // launches and only takes the layers' loss sums again (layer_sums_kernel).  Dropped at the choke points every writer of those
    // buffers goes through (enqueue_geometry, enqueue_layers, the grow paths, the robot / camera / strategy setters), set only when
    // a whole cacheable pass has been enqueued.  `shadow`: the last uploaded rows, so that an upload of the same rows keeps the epoch.
    GeometryCache geo;
    CandidateShadow shadow;
    uint64_t cand_epoch = 0, camera_epoch = 0, robot_epoch = 0;
    // The third state: once a pass has run on kept geometry, the context also keeps what the scoring launch would draw again bit for
    // bit — per row the 4-sample groups where the row's own links beat its layer, with their finished keys and the layer's
    // (rope_fragstore.h) — and later passes of the same key stream them against the target (fragment_score_kernel) instead of
    // launching score_queue_kernel and raster_queue_kernel<., SCORE>.  Built by the first hit (build_fragments, rope_abi.hip), chunk of
    // rows by chunk of rows through d_fscratch; belongs to the same GeometryKey; depends on neither loss nor target.  Dropped
    // wherever `geo` is dropped for good (drop_kept) and by every pass that is not a hit.
    FragmentStore frags;
    DevBuf<uint32_t> d_fscratch, d_fcount, d_fwhere;    // chunk's key tiles; groups per (row, tile); the store: where,
    DevBuf<uint4> d_ffin, d_fbase;                      // finished keys, base keys
    DevBuf<unsigned long long> d_foffs;                 // C x n_tiles + 1
    DevBuf<int32_t> d_frow;                             // 0, 1, 2, ...: the building launch's row -> candidate map, from any row on
    int frow_filled = 0;
    void drop_kept() { geo.drop(); frags.drop(); }

    // small batches: per-candidate tiles in global memory that split workgroups merge into
    DevBuf<int> d_touched;                 // MODE_SPLIT_GEO: per (candidate, tile) the number of the pass that last drew into it
    int pass_id = 0;
    bool mvp_valid = false;                // d_mvp holds the resident candidates' matrices (not after a pass that kept them in LDS)
    DevBuf<uint32_t> d_gtile;
    bool gtile_dirty = true;
    PassTunables tune;                     // the numbers the launch structure is chosen by (rope_passplan.h; rope_create reads the environment)
    int strategy = 0;                          // STRATEGY_* bits (rope_set_strategy): launch structure only, never a result
    // large batches: queue of the (candidate, tile) pairs with something to draw, worked off by a grid that just fills the chip
    DevBuf<uint32_t> d_qitems, d_tile_tris, d_tile_tris_lo;
    size_t q_segment = 0;
    bool q_weighted = false;
    DevBuf<int> d_qctr;                        // [0] pairs queued, [1] next pair to hand out; cleared by fk_mvp_kernel
    int n_cu = 256;

    // stored lookup table (cropped sqrt-depth of a pose grid)
    DevBuf<float> d_table;                     // dense rows while a table is built (released once it is packed)
    // the stored table (rope_lookup_build): per row d_tcount groups of four samples from d_toff on — d_tgoff: where in the crop,
    // d_tgval: the four values
    DevBuf<uint32_t> d_tcount, d_tgoff;
    DevBuf<unsigned long long> d_toff, d_tused;
    DevBuf<float4> d_tgval;
    DevBuf<uint64_t> d_ttotal;
    DevBuf<float> d_tc;                     // rope_lookup_score: the cropped target, rows padded to whole groups (table_crop_words)
    int table_C = 0, table_crop[4] = {0, 0, 0, 0};
    size_t table_groups = 0;                   // groups the stored table holds
    DevBuf<uint64_t> d_zero_total;
    // scores of the table's rows: buffers of their own (a grid may hold more rows than one candidate batch)
    DevBuf<uint64_t> d_tsums;
    DevBuf<double> d_terr;

    // camera-pose path (rope_eval_views): the resident frames scored under candidate views.
    // one pinned host block and its device twin per rope_eval_views call: candidates | view matrices | view index | frame index
    PinnedBuf<unsigned char> h_vstage;
    DevBuf<unsigned char> d_vstage;
    const double *dv_cand = nullptr, *dv_PV = nullptr;                  // into d_vstage (dv_PV: or d_PV)
    const int32_t *dv_view_of = nullptr, *dv_frame_of = nullptr;
    PinnedBuf<uint64_t> h_vsums;            // K x N x 23 sums, then N x 23 totals
    PinnedBuf<unsigned char> h_copy;        // staging of pageable host buffers on their way up (copy_h2d_staged)

    // rope_stage_targets / rope_commit_targets: the staged set is uploaded on a stream of its own while the resident set is in use
    hipStream_t copy_stream = nullptr;
    PinnedBuf<unsigned char> h_copy2;       // pinned block for pageable sources on the upload stream
    std::string stage_err;                  // rope_stage_targets may run beside an evaluation: its own message
    // rope_stage_targets_segmented: the staged set filled slot by slot by kernels on the CALLER's streams.  One event per call,
    // which rope_commit_targets waits for; the calls' small tables (plane offsets, link codes) go up through a page-locked block
    // that is only ever appended to while a set is being filled, so no call waits for the one before it.
    std::vector<hipEvent_t> stage_events;
    DevBuf<unsigned long long> s_counts;      // per staged frame: n_mask, n_depth per link
    PinnedBuf<int32_t> h_meta;
    DevBuf<int32_t> d_meta;                   // as large as h_meta
    size_t meta_used = 0;                     // int32 words
    std::vector<uint8_t> seg_filled;          // per slot of the set being filled
    int seg_n_total = 0, seg_n_filled = 0;    // seg_n_total 0: no set is being filled
    bool seg_ts = false;
    DevBuf<int32_t> d_frame_of;               // rows' frame indices: device copy / mapped host memory (small batches)
    PinnedBuf<int32_t> h_frame_of{true};
    const int32_t *frame_of_dev = nullptr;    // d_frame_of or h_frame_of.dev()
    // the stored lookup table against all targets
    DevBuf<float> d_tg_t32c;
    DevBuf<uint64_t> d_tg_ltotal;
    DevBuf<double> d_tg_scores, d_tg_best;

    // rope_coverage's plane
    DevBuf<uint8_t> d_cover;
    // the chunked render path (render_chunks): the output planes of one chunk of poses — depth and ids for rope_render_batch, ids,
    // label planes and boxes for rope_render_masks
    DevBuf<float> d_rdepth;
    DevBuf<uint8_t> d_rids, d_rmask;
    DevBuf<int32_t> d_rboxes;
};

void rope_range_push(const char *name);                  // roctx ranges (rope_abi.hip); also used by rope_predict.cpp (per stage)
void rope_range_pop();
void rope_pose_rotation(const double *pose, double R[3][3]);    // rope_hostprep.cpp: camera-to-world rotation of [x, y, z, a3, a4, a5]
struct RopeRange {
    explicit RopeRange(const char *name) { rope_range_push(name); }
    ~RopeRange() { rope_range_pop(); }
};

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = static_cast<hipError_t>(expr);                                                              \
        if (e_ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            return ROPE_E_HIP;                                                                 \
        }                                                                                      \
    } while (0)

#define ARG_FAIL(ctx, msg)      \
    do {                        \
        (ctx)->err = (msg);     \
        return ROPE_E_ARG;      \
    } while (0)

// Grow-or-keep for buffers that work in flight on the context's stream may still use: (buffer, elements) pairs; when one of
// them is too small the stream is waited for, once, and every one is grown.  Nothing happens, and nothing is waited for, otherwise.
inline bool any_short() { return false; }
template <typename B, typename... R> static bool any_short(const B &b, size_t n, const R &...r) { return n > b.cap() || any_short(r...); }
inline int grow_each() { return 0; }
template <typename B, typename... R> static int grow_each(B &b, size_t n, R &...r) { const int e = b.grow(n); return e ? e : grow_each(r...); }
template <typename... A> static int sync_grow(rope_ctx *c, A &&...a)
{
    if (!any_short(a...)) return ROPE_OK;
    c->drop_kept();                               // whichever buffer grows: a re-grown one holds nothing, and the key need not name them all
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, grow_each(a...));
    return ROPE_OK;
}

// ---- defined in rope_abi.hip, used by rope_abi_targets.hip as well

// One batch is at most MAX_ROWS candidates (the grid's y dimension).
static constexpr int MAX_ROWS = 65535;

// Host buffers handed over the C ABI are pageable; the runtime's own path for those is slow (measured 0.35 GB/s for
// freshly written numpy arrays).  Go through a pinned block instead: memcpy + asynchronous copy, chunk by chunk.
// copy_h2d_on: `stream` / `block` / `err` are the context's own stream, pinned block and message for copy_h2d_staged;
// rope_stage_targets, which may run beside an evaluation on another thread, passes the upload stream and a block and a message of its own
int copy_h2d_on(hipStream_t stream, PinnedBuf<unsigned char> &block, std::string &err, void *dst, const void *src, size_t bytes);
int copy_h2d_staged(rope_ctx *c, void *dst, const void *src, size_t bytes);
int copy_d2h_staged(rope_ctx *c, void *dst, const void *src, size_t bytes);   // returns with the data in dst

bool near_plane_in_reach(const rope_ctx *c, const double *PV);
int ensure_capacity(rope_ctx *c, int C);
// frame_of (rope_eval_targets): the frame every row is scored against; rows only share a layer inside one frame (a layer
// carries loss sums, and those belong to a target)
int upload_candidates(rope_ctx *c, const double *cand, int C, bool group, const int32_t *frame_of = nullptr);

// A crop {r0, r1, c0, c1} (inclusive) checked against the image and written into fp, its pixels into n_pix; refused as "<who>: crop outside the image"
int apply_crop(rope_ctx *c, const char *who, const int32_t *crop, FrameParams &fp, double &n_pix);
// the frame a loss is summed over: the camera's, and for ROPE_LOSS_LOOKUP the crop, which must be given ("<who>: lookup loss needs a crop")
int loss_frame(rope_ctx *c, const char *who, int loss, const int32_t *crop, FrameParams &fp, double &n_pix);
// the camera's frame cropped to the stored lookup table's
inline FrameParams table_frame(const rope_ctx *c)
{
    FrameParams fp = c->fp;
    fp.r0 = c->table_crop[0]; fp.r1 = c->table_crop[1]; fp.c0 = c->table_crop[2]; fp.c1 = c->table_crop[3];
    return fp;
}
// the "nothing rendered" totals of every frame of `s` for this loss and fp's crop, unless `cache` has them
int ensure_totals(rope_ctx *c, const TargetSet &s, EmptyCache &cache, int loss, const FrameParams &fp);

// What a pass scores its rows against: one frame's planes, or those of many frames and a frame index per row.
struct EvalPlanes {
    const uint64_t *tq;
    const float *t32;
    const uint64_t *tl;                     // per-link planes (ROPE_LOSS_CAMFULL), or nullptr
    const int32_t *frame_of;                // nullptr: every row against the one frame
};
// (EvalKind, who finalises: rope_passplan.h)
int enqueue_eval(rope_ctx *c, int n_render, int loss, const FrameParams &fp, double n_pix, const EvalPlanes &pl, EvalKind kind,
                 hipEvent_t *ev = nullptr /* 5 events */);
