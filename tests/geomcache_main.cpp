// The plain C++ half of the geometry cache (csrc/rope_geomcache.h) as a program of its own, built by tests/test_geomcache_host.py
// under AddressSanitizer and UBSan: the candidate shadow at its edges (rows held in heap blocks of exactly their size) and the
// record's key logic.  Prints "ok <n>" after n checks, or the first check that failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../rope_s3d_amd/csrc/rope_geomcache.h"

using namespace rope;

static int n_checks = 0;
#define CHECK(expr) do { n_checks++; if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); std::exit(1); } } while (0)

// C rows in a block of exactly 6 C doubles; row i, joint j = f(i, j)
static std::unique_ptr<double[]> rows_of(int C, double scale)
{
    std::unique_ptr<double[]> p(new double[6 * (size_t)C]);
    for (int i = 0; i < 6 * C; i++) p[i] = scale * (double)((i * 2654435761u) >> 20) - 1.0;
    return p;
}

static void shadow()
{
    CandidateShadow s;
    auto a = rows_of(320, 1e-3);
    CHECK(!s.same(a.get(), 320, true));                       // nothing kept yet
    s.keep(a.get(), 320, true);
    CHECK(s.same(a.get(), 320, true));
    auto copy = rows_of(320, 1e-3);                           // other memory, same bits
    CHECK(s.same(copy.get(), 320, true));
    CHECK(!s.same(a.get(), 320, false));                      // grouped differently
    CHECK(!s.same(a.get(), 319, true));                       // a prefix is another set
    CHECK(!s.same(nullptr, 320, true));
    // one angle changed in its last bit, in the last row's last joint and in the first row's first
    for (size_t at : {(size_t)6 * 320 - 1, (size_t)0}) {
        auto b = rows_of(320, 1e-3);
        uint64_t bits;
        std::memcpy(&bits, &b[at], 8);
        bits ^= 1;
        std::memcpy(&b[at], &bits, 8);
        CHECK(!s.same(b.get(), 320, true));
    }
    // -0.0 is not 0.0: the layers are grouped by bits
    auto z = rows_of(8, 0.0), nz = rows_of(8, 0.0);
    for (int i = 0; i < 48; i++) { z[i] = 0.0; nz[i] = 0.0; }
    nz[7] = -0.0;
    s.keep(z.get(), 8, true);
    CHECK(s.same(z.get(), 8, true) && !s.same(nz.get(), 8, true));
    // a larger set after a smaller one, and back: the comparison never reads past the shorter block
    auto big = rows_of(4096, 1e-4);
    CHECK(!s.same(big.get(), 4096, true));
    s.keep(big.get(), 4096, true);
    CHECK(s.same(big.get(), 4096, true) && !s.same(z.get(), 8, true));
    s.keep(z.get(), 1, false);                                // one row
    CHECK(s.same(z.get(), 1, false) && s.rows.size() == 6);
    s.drop();
    CHECK(!s.same(z.get(), 1, false));
    s.keep(z.get(), 1, false);
    CHECK(s.same(z.get(), 1, false));
}

struct Frame { int W, H, tiles_x, tiles_y, r0, r1, c0, c1; float a, b, c; };

static GeometryKey key_of(const Frame &f)
{
    GeometryKey k = GeometryKey::make();
    k.cand_epoch = 3; k.camera_epoch = 1; k.robot_epoch = 1;
    k.cap_layers = 64 * 4 * 12288; k.cap_layer_sums = 64 * 4 * 23; k.cap_bounds = 320 * 1450; k.cap_mvp = 320 * 96; k.q_segment = 320 * 32;
    k.C = 320; k.n_layers = 64; k.n_parents = 8; k.n_render = 6; k.n_shared = 3;
    k.strategy = 0; k.n_cu = 256;
    k.parents = 0; k.queue = 1; k.weighted = 1; k.clip = 0;
    CHECK(k.set_frame(&f, sizeof f));
    return k;
}

static void record()
{
    const Frame f = {160, 120, 2, 2, 0, 119, 0, 159, 1.0f, 2.0f, 3.0f};
    GeometryCache g;
    const GeometryKey k = key_of(f);
    CHECK(!g.holds(k));                                       // a fresh record holds nothing, whatever the key
    CHECK(!g.holds(GeometryKey::make()));
    g.filled(k);
    CHECK(g.holds(k) && g.holds(key_of(f)));                  // built again from the same values: equal bytes, padding included
    g.drop();
    CHECK(!g.holds(k));
    g.filled(k);
    // every member on its own makes another key
#define DIFFERS(stmt) do { GeometryKey o = key_of(f); stmt; CHECK(!g.holds(o)); } while (0)
    DIFFERS(o.cand_epoch++); DIFFERS(o.camera_epoch++); DIFFERS(o.robot_epoch++);
    DIFFERS(o.cap_layers *= 2); DIFFERS(o.cap_layer_sums *= 2); DIFFERS(o.cap_bounds *= 2); DIFFERS(o.cap_mvp *= 2); DIFFERS(o.q_segment = 0);
    DIFFERS(o.C++); DIFFERS(o.n_layers++); DIFFERS(o.n_parents++); DIFFERS(o.n_render = 3); DIFFERS(o.n_shared = 2);
    DIFFERS(o.strategy = 8); DIFFERS(o.n_cu = 304);
    DIFFERS(o.parents = 1); DIFFERS(o.queue = 0); DIFFERS(o.weighted = 0); DIFFERS(o.clip = 1);
#undef DIFFERS
    Frame crop = f;
    crop.c1 = 100;                                            // the crop rides in the frame
    CHECK(!g.holds(key_of(crop)));
    CHECK(g.holds(k));                                        // and none of that changed the record
    // a frame larger than the key's room is refused, not truncated
    unsigned char wide[sizeof(GeometryKey::frame) + 1] = {};
    GeometryKey o = key_of(f);
    CHECK(!o.set_frame(wide, sizeof wide));
    CHECK(o.set_frame(wide, sizeof(GeometryKey::frame)) && !g.holds(o));
    // a shorter frame after a longer one leaves no bytes of the longer behind
    GeometryKey p = key_of(f), q = GeometryKey::make();
    const int small = 7;
    CHECK(p.set_frame(&small, sizeof small));
    q = key_of(f);
    q.set_frame(&small, sizeof small);
    CHECK(p.equals(q));
    GeometryKey r = GeometryKey::make(), t = key_of(f);
    std::memcpy(&r, &t, sizeof r);
    r.set_frame(&small, sizeof small);
    CHECK(r.equals(p));
}

int main()
{
    shadow();
    record();
    std::printf("ok %d\n", n_checks);
    return 0;
}
