// predict_table_main.cpp — rope_predict_batch's n_frames rule as a program of its own (no HIP, no Python), built under
// AddressSanitizer and UBSan by tests/test_stage_landscapes_host.py together with csrc/rope_predict.cpp and tests/native_shim.cpp.
// The shim's rope_lookup_score_targets writes one entry per RESIDENT target, as the library's does: a batch of fewer frames than
// that, let through, is a heap overrun of the stage machine's `best` — which the sanitiser stops — and a batch of more frames starts
// the surplus from row 0.  Both must come back as ROPE_E_ARG, naming both counts; the equal count runs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/rope_s3d.h"

extern "C" {
typedef int (*shim_table_cb)(int32_t *best_idx, int n);
typedef int (*shim_targets_cb)(const double *cand, const int32_t *frame_of, int R, int n_render, int loss, const int32_t *crop, double *err_out);
void shim_set_table_callbacks(shim_table_cb one, shim_table_cb targets);
void shim_set_targets_callback(shim_targets_cb cb);
void shim_set_resident(int n);
const char *shim_last_error();
}

namespace {

constexpr int RESIDENT = 4, GRID = 5;
int g_table_calls = 0;

// frame f's landscape: a bowl about (0.1 f, 0.2, 0.3 f, 0, 0, 0)
int answer(const double *cand, const int32_t *frame_of, int R, int, int, const int32_t *, double *err_out)
{
    for (int i = 0; i < R; i++) {
        const int f = frame_of[i];
        if (f < 0 || f >= RESIDENT) return ROPE_E_ARG;
        const double c[6] = {0.1 * f, 0.2, 0.3 * f, 0, 0, 0};
        double e = 0;
        for (int j = 0; j < 6; j++) e += (cand[6 * i + j] - c[j]) * (cand[6 * i + j] - c[j]);
        err_out[i] = e;
    }
    return ROPE_OK;
}

int table(int32_t *best_idx, int n)
{
    g_table_calls++;
    for (int f = 0; f < n; f++) best_idx[f] = (f + 1) % GRID;
    return ROPE_OK;
}

int fail(const char *what, int rc)
{
    std::printf("FAIL %s: rc %d, error '%s'\n", what, rc, shim_last_error());
    return 1;
}

}  // namespace

int main()
{
    const double limits[12] = {-3, 3, -1, 2.5, -2, 4, -3, 3, -2, 2, -6, 6}, cam[6] = {0, -1.5, 0.75, 0, 0, 0}, inc[6] = {.005, .005, .005, .005, .005, .005};
    double grid[GRID * 6];
    for (int r = 0; r < GRID; r++)
        for (int j = 0; j < 6; j++) grid[6 * r + j] = j < 3 ? 0.25 * r - 0.5 : 0.0;
    const int32_t crop[4] = {0, 1, 0, 1};
    rope_stage stages[3];
    std::memset(stages, 0, sizeof stages);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (rope_stage &s : stages) {
        for (double &r : s.init_rate) r = nan;
        s.to_render = 4; s.rate_reduction = 0.5; s.early_stop = 0.01; s.range = nan;
    }
    stages[0].kind = ROPE_STAGE_LOOKUP; stages[0].to_render = 6;
    stages[1].kind = ROPE_STAGE_SFLIP;
    stages[2].kind = ROPE_STAGE_DESCENT; stages[2].count = 4; stages[2].joints = 7;
    rope_predict_args a;
    std::memset(&a, 0, sizeof a);
    a.stages = stages; a.n_stages = 3; a.speculate = 3; a.limits = limits; a.camera_pose = cam; a.min_ang_inc = inc;
    a.lookup_angles = grid; a.n_lookup = GRID; a.lookup_crop = crop;
    rope_ctx *ctx = reinterpret_cast<rope_ctx *>(&a);          // any non-null context: the shim never looks inside
    shim_set_targets_callback(answer);
    shim_set_table_callbacks(nullptr, table);
    shim_set_resident(RESIDENT);
    for (int use_table = 1; use_table >= 0; use_table--) {
        a.use_table = use_table;
        for (int n_frames : {RESIDENT - 1, RESIDENT + 1}) {
            // buffers sized for what is asked: whatever the call writes beyond that, the sanitiser sees
            std::vector<double> out((size_t)n_frames * 6, -7.0), trace((size_t)n_frames * 3 * 6, -7.0);
            int64_t n = -1;
            const int calls = g_table_calls;
            const int rc = rope_predict_batch(ctx, &a, n_frames, out.data(), trace.data(), &n);
            if (rc != ROPE_E_ARG) return fail("a frame count other than the resident one must be refused", rc);
            char want_a[32], want_b[32];
            std::snprintf(want_a, sizeof want_a, "%d", n_frames);
            std::snprintf(want_b, sizeof want_b, "%d", RESIDENT);
            if (!std::strstr(shim_last_error(), want_a) || !std::strstr(shim_last_error(), want_b)) return fail("the message names both counts", rc);
            if (g_table_calls != calls || n != -1) return fail("a refused call runs nothing", rc);
            for (double v : out) if (v != -7.0) return fail("a refused call writes nothing", rc);
        }
        std::vector<double> out((size_t)RESIDENT * 6, -7.0), trace((size_t)RESIDENT * 3 * 6, -7.0);
        int64_t n = 0;
        const int rc = rope_predict_batch(ctx, &a, RESIDENT, out.data(), trace.data(), &n);
        if (rc != ROPE_OK) return fail("the resident count runs", rc);
        for (int f = 0; f < RESIDENT; f++) {
            if (use_table)                                       // Lookup took the table's row for THIS frame
                for (int j = 0; j < 6; j++)
                    if (trace[((size_t)f * 3 + 0) * 6 + j] != grid[6 * ((f + 1) % GRID) + j]) return fail("lookup row of a frame", f);
            for (int j = 0; j < 6; j++)
                if (!std::isfinite(out[(size_t)f * 6 + j]) || out[(size_t)f * 6 + j] != trace[((size_t)f * 3 + 2) * 6 + j]) return fail("angles of a frame", f);
        }
        if (n < RESIDENT * GRID) return fail("evaluations counted", (int)n);
    }
    // no targets resident at all
    shim_set_resident(0);
    std::vector<double> out(6);
    if (rope_predict_batch(ctx, &a, 1, out.data(), nullptr, nullptr) != ROPE_E_ARG) return fail("no resident targets", 0);
    std::printf("ok\n");
    return 0;
}
