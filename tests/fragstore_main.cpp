// The plain C++ half of the kept fragments (csrc/rope_fragstore.h) as a program of its own, built by tests/test_fragstore_host.py
// under AddressSanitizer and UBSan: the chunk plan at its edges, the scan over heap blocks of exactly their size, the budget
// decision and the record's states.  Prints "ok <n>" after n checks, or the first check that failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../rope_s3d_amd/csrc/rope_fragstore.h"

using namespace rope;

static int n_checks = 0;
#define CHECK(expr) do { n_checks++; if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); std::exit(1); } } while (0)

static void chunks()
{
    // 320 rows of 4 tiles through a scratch of 64 layers x 4 tiles: five chunks of 64
    FragmentChunks p(320, 4, 256);
    CHECK(p.rows == 64 && p.chunks == 5);
    int covered = 0;
    for (int k = 0; k < p.chunks; k++) { CHECK(p.begin(k) == covered && p.count(k, 320) == 64); covered += p.count(k, 320); }
    CHECK(covered == 320 && p.count(p.chunks, 320) == 0);
    // a last chunk that is shorter; a scratch that is no multiple of a row
    FragmentChunks q(321, 4, 259);
    CHECK(q.rows == 64 && q.chunks == 6 && q.count(5, 321) == 1 && q.begin(5) == 320);
    // room for more than all rows: one chunk of exactly C; room for one row; for none
    FragmentChunks all(320, 4, 100000), one(320, 4, 7), none(320, 4, 3);
    CHECK(all.rows == 320 && all.chunks == 1 && all.count(0, 320) == 320);
    CHECK(one.rows == 1 && one.chunks == 320 && one.count(319, 320) == 1);
    CHECK(none.rows == 0 && none.chunks == 0);
    // the bench grids: 4096 rows x 25 tiles under 256 layers' worth of scratch; 32768 x 80 under 1024
    FragmentChunks b1(4096, 25, (size_t)256 * 25), b5(32768, 80, (size_t)1024 * 80);
    CHECK(b1.rows == 256 && b1.chunks == 16 && b5.rows == 1024 && b5.chunks == 32);
    // never more rows than a queue item can name; nonsense in, no plan out
    FragmentChunks wide(65535, 1, (size_t)1 << 20), bad(0, 4, 100), bad2(10, 0, 100);
    CHECK(wide.rows == 65535 && wide.chunks == 1 && bad.rows == 0 && bad2.rows == 0);
}

static void scan_and_budget()
{
    const size_t n = 320 * 4;
    std::unique_ptr<uint32_t[]> counts(new uint32_t[n]);
    std::unique_ptr<uint64_t[]> offs(new uint64_t[n + 1]);
    uint64_t want = 0, want_pairs = 0;
    for (size_t i = 0; i < n; i++) { counts[i] = (i % 3 == 0) ? 0u : (uint32_t)((i * 2654435761u) >> 22); want += counts[i]; want_pairs += counts[i] != 0; }
    uint64_t pairs = 0;
    CHECK(FragmentStore::scan(counts.get(), n, offs.get(), &pairs) == want && pairs == want_pairs);
    CHECK(offs[0] == 0 && offs[n] == want);
    for (size_t i = 0; i < n; i++) CHECK(offs[i + 1] - offs[i] == counts[i]);
    // nothing at all; one slot; counts whose sum passes 2^32
    uint64_t z[1];
    CHECK(FragmentStore::scan(nullptr, 0, z) == 0 && z[0] == 0);
    const uint32_t big[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 7u};
    uint64_t bo[4];
    CHECK(FragmentStore::scan(big, 3, bo) == 2 * 0xFFFFFFFFull + 7 && bo[2] == 2 * 0xFFFFFFFFull && bo[3] - bo[2] == 7);

    FragmentStore s;
    CHECK(s.budget == FRAGMENT_DEFAULT_BUDGET && FRAGMENT_DEFAULT_BUDGET == 858993459ull);
    CHECK(FragmentStore::bytes_for(0, 0) == 8 && FragmentStore::bytes_for(10, 4) == 360 + 40);
    s.budget = 400;
    CHECK(s.fits(10, 4) && !s.fits(11, 4) && !s.fits(10, 5));
    s.budget = 0;
    CHECK(!s.fits(0, 0));
    CHECK(fragment_tile(fragment_where(8191, 3071)) == 8191 && fragment_group(fragment_where(8191, 3071)) == 3071);
    CHECK(fragment_where(1, 0) == 4096 && fragment_where(0, 5) == 5);
}

static void record()
{
    GeometryKey k = GeometryKey::make(), other = GeometryKey::make();
    k.C = 320; k.cand_epoch = 3;
    other.C = 320; other.cand_epoch = 4;
    FragmentStore s;
    CHECK(!s.serves(k) && !s.refused(k) && !s.serves(GeometryKey::make()));      // a fresh record serves nothing, whatever the key
    s.built(k, 1000, 1280, 700);
    CHECK(s.serves(k) && !s.refused(k) && !s.serves(other));
    CHECK(s.builds == 1 && s.groups == 1000 && s.pairs == 700 && s.bytes == 36000 + 1281 * 8);
    s.passes_served += 2;
    s.drop();
    CHECK(!s.serves(k) && s.groups == 0 && s.bytes == 0 && s.pairs == 0 && s.builds == 1 && s.passes_served == 2);      // the counts stay
    s.decline(k);
    CHECK(s.refused(k) && !s.serves(k) && !s.refused(other) && s.bytes == 0 && s.builds == 1);
    s.drop();
    CHECK(!s.refused(k));
    s.built(k, 0, 1280, 0);                                                        // a grid that shows none of its own links: an empty store serves
    CHECK(s.serves(k) && s.groups == 0 && s.bytes == 1281 * 8 && s.builds == 2);
    s.decline(other);                                                              // declining one key lets go of the other's store
    CHECK(!s.serves(k) && s.refused(other));
    s.built(other, 5, 4, 2);
    CHECK(s.serves(other) && !s.refused(other));
}

int main()
{
    chunks();
    scan_and_budget();
    record();
    std::printf("ok %d\n", n_checks);
    return 0;
}
