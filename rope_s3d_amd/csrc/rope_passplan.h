// rope_passplan.h — which chain of kernels a pass runs, decided once and as a value: PassInputs (what the rules read) ->
// plan_pass() -> PassPlan (what rope_abi.hip then launches).  Every structure gives the same bits (rope_set_strategy's contract),
// so a wrong choice here only costs time; all the measured tuning of the launch structure lives in this file.  No HIP and no
// context here: tests/passplan_main.cpp builds this file alone, and tests/test_passplan_host.py holds it to tests/passplan_ref.py.
// Run-time state — whether the kept geometry or the kept fragments are there, buffer growth — stays with enqueue_eval.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/rope_s3d.h"

namespace rope {

// Who finalises: EVAL_SINGLE errors and their argmin against the single target's totals and flags; EVAL_TARGETS every row against its
// own frame's (no argmin: rows of many frames), up to TARGET_HOST_ROWS rows through mapped host memory; EVAL_VIEWS nobody — the rows
// are (view, frame) pairs with a view matrix of their own and no shared layers, and rope_eval_views takes the sums as they are.
enum EvalKind { EVAL_SINGLE, EVAL_TARGETS, EVAL_VIEWS };

// The border between a small batch and a large one.  Up to here: forward kinematics and boxes in one fused launch of one workgroup
// per candidate (fk_bounds_kernel), which takes no queue weights and leaves the queue counters alone.  Beyond: fk_mvp_kernel +
// bounds_kernel, the queues, and geometry worth keeping for the next pass.
constexpr int SMALL_BATCH_ROWS = 256;
// most rows of a batch whose raster workgroups may do their own forward kinematics (the clamp of geo_rows): d_touched holds this many
constexpr int OWN_GEOMETRY_MAX_ROWS = 256;
// the queues' grid is two workgroups per CU; weights are used while a workgroup gets at most this many busy pairs
constexpr int QUEUE_WG_PER_CU = 2, QUEUE_WEIGHTED_PAIRS_PER_WG = 256;

// MODE_SPLIT: busy workgroups aimed at per launch (one generation: 2 per CU), fewest / most per (tile, candidate), and the
// workgroups per launch of the scoring pass that follows.  Measured at 160x90, 640x360 and 640x480 (tools/r02_split_tune.sh).
struct PassTunables {
    int split_target = 512, split_min = 8, split_min_many = 3, split_cap = 64, score_target = 6144;
    int geo_rows = 48;                     // most rows of a small batch whose raster workgroups do their own forward kinematics and boxes
    int layer_min_wg = 64;                 // fewest busy workgroups of a shared-layer launch for it to pay in a small batch (layers_pay)
};

struct PassInputs {
    int C = 0, n_tiles = 0;
    int n_layers = 0, n_parents = 0;        // distinct (q0, q1) and distinct q0 among the rows (upload_candidates); n_layers == C: nothing shared
    int n_render = 0, loss = 0;
    EvalKind kind = EVAL_SINGLE;
    bool frame_index = false;               // the rows carry a frame index (EvalPlanes::frame_of)
    int strategy = 0;                       // ROPE_STRATEGY_* bits
    int n_cu = 256;
    bool q_weighted = false;                // the context's queue buffers have room for per-(candidate, tile) weights (ensure_capacity)
    bool clip = false;                      // the near-plane verdict for the pass's cameras (use_clip)
    bool skip = false;                      // profiling build: a phase-skipping flag is set (rope_debug_skip)
    PassTunables t;
};

enum Scoring { SCORE_GTILE, SCORE_QUEUE, SCORE_PLAIN };     // score_gtile_kernel after a split; the scoring queue; one workgroup per (tile, row)

struct PassPlan {
    bool layers = false;                    // links [0, n_shared) drawn once per layer
    int n_shared = 0;
    bool parents = false;                   // second sharing level: links 0-1 once per distinct q0, link 2 per layer
    int lo_first = 0;                       // first link the layer launch's weights count (bounds_kernel): 2 with parents
    bool layer_queue = false;               // the layers through the queue, else one workgroup per (layer, tile)
    bool weighted = false;                  // the queues hand out pairs by weight, else in candidate order
    int split = 1;                          // workgroups per (tile, candidate); 1: no split
    bool own_geometry = false;              // MODE_SPLIT_GEO: no geometry launch
    bool fused_geometry = false;            // fk_bounds_kernel, else fk_mvp_kernel + bounds_kernel
    Scoring scoring = SCORE_PLAIN;
    int slices = 1;                         // of score_gtile_kernel
    bool cache_scope = false;               // a pass the hit / miss counters count
    bool cacheable = false;                 // its geometry may be kept, and kept geometry may serve it
    bool fragment_scope = false;            // on a hit, the kept fragments may be built and may serve
    bool clip = false;
};

// about a third of a frame's tiles hold the robot (all of them when the frame is one or two tiles): the others' workgroups
// leave at once
inline int busy_tiles(int n_tiles) { return std::max(std::min(2, n_tiles), n_tiles / 3); }

// Layers pay off when many candidates share one upstream pose (lookup grids, sweeps of U).  upload_candidates sends the layer
// arrays up only then.
inline bool layers_wanted(int n_layers, int C) { return (int64_t)n_layers * 4 <= C; }
// the same rule one level up
inline bool parents_wanted(int n_parents, int n_layers) { return (int64_t)n_parents * 4 <= n_layers; }

// A small batch whose candidates share one or two upstream poses (a sweep of the third joint) would draw links 0-2 in a layer
// launch of a handful of workgroups — 59 000 triangles each, the rest of the chip idle (100 us at 160x90) — before the scoring
// launch: the split path draws all six links per candidate over many workgroups instead and is more than twice as fast there.
inline bool layers_pay(const PassInputs &in)
{
    return in.C > SMALL_BATCH_ROWS || (int64_t)in.n_layers * busy_tiles(in.n_tiles) >= in.t.layer_min_wg;
}

// The raster queue hands out the heaviest (candidate, tile) pairs first when a workgroup gets few enough pairs for the last ones
// to matter: with 40 pairs per workgroup (4096 candidates at 640x480) a 20 000-triangle pair that starts late kept its workgroup
// busy 180 us after the others had left, 7 % of the launch; with hundreds per workgroup (32 768 candidates at 1280x720) the tail is
// nothing and candidate order, which keeps a candidate's boxes in L2 for its tiles, is 1.5 % faster.
inline bool queue_weighted(const PassInputs &in)
{
    return in.q_weighted && in.C > SMALL_BATCH_ROWS &&          // a small batch: fk_bounds_kernel, no weights
           (int64_t)in.C * busy_tiles(in.n_tiles) <= (int64_t)QUEUE_WEIGHTED_PAIRS_PER_WG * QUEUE_WG_PER_CU * in.n_cu;
}

// The geometry and shared-layer launches of a batch with layers or without: all the render, coverage, table and debug entries,
// which score nothing, need of a plan.
inline PassPlan plan_geometry(const PassInputs &in, bool layers)
{
    PassPlan p;
    p.layers = layers;
    p.n_shared = layers ? std::min(3, in.n_render) : 0;
    p.weighted = queue_weighted(in);
    // the (layer, tile) pairs that have anything to draw, heaviest first, to a grid that just fills the chip: of the one-
    // workgroup-per-pair launch's 266 us the last 100 ran with a third of the chip (a 140 us pair that started at 150 us)
    p.layer_queue = p.weighted && !(in.strategy & ROPE_STRATEGY_NO_QUEUE);
    // Second level of sharing (links 0-1 once per distinct q0): pays when the layers are a launch of one workgroup per (layer, tile)
    // pair — not when they go through the weighted queue, which draws links 0-2 per layer faster than the extra launch of a
    // hundred busy workgroups plus the merge of every layer tile with its parent's (0.264 against 0.283 ms on the bench workload).
    p.parents = p.n_shared == 3 && parents_wanted(in.n_parents, in.n_layers) && !(in.strategy & ROPE_STRATEGY_NO_PARENTS) && !p.layer_queue;
    // weights of the shared links for the layer launch: with the second level in use it draws the last shared link only
    p.lo_first = p.parents ? 2 : 0;
    p.fused_geometry = in.C <= SMALL_BATCH_ROWS;
    p.clip = in.clip;
    return p;
}

inline PassPlan plan_pass(const PassInputs &in)
{
    const bool views = in.kind == EVAL_VIEWS;
    const PassTunables &t = in.t;
    PassPlan p = plan_geometry(in, !views && layers_wanted(in.n_layers, in.C) && layers_pay(in) && !(in.strategy & ROPE_STRATEGY_NO_LAYERS));
    // A large layered batch against the single target keeps its geometry for the next pass (rope_ctx::geo).  Every other pass
    // drops it: it either goes through enqueue_geometry or — the small batches that do their own — reuses the same buffers' rows.
    p.cache_scope = in.kind == EVAL_SINGLE && p.layers && in.C > SMALL_BATCH_ROWS && !in.frame_index;
    p.cacheable = p.cache_scope && !(in.strategy & ROPE_STRATEGY_NO_GEOMETRY_CACHE) && !in.skip;
    // Kept fragments (rope_ctx::frags): a hit may be scored from them, and builds them when they are not there yet.  Through the
    // queues only (the build is a queue launch).
    p.fragment_scope = p.cacheable && in.loss != ROPE_LOSS_CAMFULL && !(in.strategy & (ROPE_STRATEGY_NO_KEPT_FRAGMENTS | ROPE_STRATEGY_NO_QUEUE));
    // Few candidates (descent pairs, flips): one workgroup per (tile, candidate) would leave most of the chip idle,
    // so the meshlets of each tile are split over several workgroups that merge into a tile in global memory.
    if (!p.layers && !(in.strategy & ROPE_STRATEGY_NO_SPLIT)) {
        // Too few shares per busy tile make each workgroup's chain of meshlets long: a floor, lower once the
        // launch runs to several generations of workgroups anyway (every share pays for clearing and scanning its LDS tile).
        const int64_t pairs = (int64_t)in.C * busy_tiles(in.n_tiles);
        const int floor_ = pairs <= 256 ? t.split_min : t.split_min_many;
        p.split = std::max(std::min(t.split_cap, (int)(t.split_target / std::max<int64_t>(1, pairs))), std::min(floor_, t.split_cap));
        if (p.split < 2 || pairs > 4 * (int64_t)t.split_target) p.split = 1;       // enough (tile, candidate) pairs to fill the chip whole
    }
    // With the split, every workgroup can work out what it needs of the geometry itself — its candidate's six link matrices and
    // the screen boxes of its own share of the meshlets: the fk + boxes launch (10 us of a 60 us evaluation, most of it the launch)
    // goes.  (Not for the camera-pose path, whose rows name their own view matrices.)
    // Up to a few dozen rows: from 64 on, the launch saved is no more than what the matrices cost when every share of every row repeats them.
    // And on frames of a few tiles only (the Predictor's 160x90 is two): on a 25-tile frame two thirds of the workgroups belong to tiles
    // the robot does not reach — the masks of the separate launch let them leave at once, here each would do the matrices first.
    p.own_geometry = p.split > 1 && !views && in.C <= t.geo_rows && in.n_tiles <= 4 && !(in.strategy & ROPE_STRATEGY_SEPARATE_GEOMETRY);
    if (p.split > 1) {
        p.scoring = SCORE_GTILE;
        while (p.slices < 8 && (int64_t)in.C * in.n_tiles * p.slices * 2 <= t.score_target) p.slices *= 2;
    } else if (in.C > SMALL_BATCH_ROWS && !(in.strategy & ROPE_STRATEGY_NO_QUEUE)) {
        p.scoring = SCORE_QUEUE;            // fk_mvp_kernel ran (a large batch) and cleared the queue counters
    }
    return p;
}

}  // namespace rope
