// passplan_main.cpp — csrc/rope_passplan.h as a program of its own (no HIP, no context), built under AddressSanitizer and UBSan by
// tests/test_passplan_host.py.  stdin: rows of 20 integers, the fields of PassInputs in the order of tests/passplan_ref.py's INPUTS;
// stdout: per row one line of 15 integers, the fields of plan_pass()'s PassPlan in the order of its OUTPUTS.
#include <cstdio>

#include "../rope_s3d_amd/csrc/rope_passplan.h"

int main()
{
    using namespace rope;
    int v[20];
    long rows = 0;
    for (;;) {
        int got = 0;
        while (got < 20 && std::scanf("%d", &v[got]) == 1) got++;
        if (got == 0) break;
        if (got != 20) { std::fprintf(stderr, "row %ld: %d of 20 fields\n", rows, got); return 2; }
        PassInputs in;
        in.C = v[0]; in.n_tiles = v[1]; in.n_layers = v[2]; in.n_parents = v[3]; in.n_render = v[4]; in.loss = v[5];
        if (v[6] < 0 || v[6] > 2) { std::fprintf(stderr, "row %ld: kind %d\n", rows, v[6]); return 2; }
        in.kind = static_cast<EvalKind>(v[6]);
        in.frame_index = v[7] != 0; in.strategy = v[8]; in.n_cu = v[9]; in.q_weighted = v[10] != 0; in.clip = v[11] != 0; in.skip = v[12] != 0;
        in.t.split_target = v[13]; in.t.split_min = v[14]; in.t.split_min_many = v[15]; in.t.split_cap = v[16]; in.t.score_target = v[17];
        in.t.geo_rows = v[18]; in.t.layer_min_wg = v[19];
        const PassPlan p = plan_pass(in);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)p.layers, p.n_shared, (int)p.parents, p.lo_first, (int)p.layer_queue,
                    (int)p.weighted, p.split, (int)p.own_geometry, (int)p.fused_geometry, (int)p.scoring, p.slices, (int)p.cache_scope,
                    (int)p.cacheable, (int)p.fragment_scope, (int)p.clip);
        rows++;
    }
    return 0;
}
