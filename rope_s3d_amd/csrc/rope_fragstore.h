// rope_fragstore.h — the third thing a fixed grid keeps from pass to pass, as far as it is plain C++ (rope_geomcache.h has the first
// two): the record of the kept fragments — per row the 4-sample groups in which the row's own links beat its shared layer, with
// their finished keys and the layer's — the byte budget that decides whether a grid's fragments are kept at all, the plan by which
// the rows are drawn chunk by chunk into a bounded scratch, and the scan that turns per-(row, tile) counts into places in the one
// contiguous store.  No HIP here: tests/fragstore_main.cpp builds this file alone.  The buffers are rope_ctx.h, the policy rope_abi.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rope_geomcache.h"

namespace rope {

// One kept group: where it is (tile and 16-byte group inside the tile), the four finished keys min(own, base) and the four base
// keys — the layer's, or KEY_EMPTY where the layer does not reach the tile.  Three arrays side by side, 4 + 16 + 16 bytes a group.
constexpr uint64_t FRAGMENT_GROUP_BYTES = 36;
constexpr int FRAGMENT_GROUP_BITS = 12;                       // a tile has TILE_W * TILE_H / 4 = 3072 groups; the tile index sits above
static inline uint32_t fragment_where(uint32_t tile, uint32_t group) { return (tile << FRAGMENT_GROUP_BITS) | group; }
static inline uint32_t fragment_tile(uint32_t where) { return where >> FRAGMENT_GROUP_BITS; }
static inline uint32_t fragment_group(uint32_t where) { return where & ((1u << FRAGMENT_GROUP_BITS) - 1u); }

// The lookup table's budget (simulation/lookup.py: a tenth of an 8 GiB card), which the store replaces for the on-the-fly stage
constexpr uint64_t FRAGMENT_DEFAULT_BUDGET = ((uint64_t)8192 << 20) / 10;

// Rows per chunk of the building pass: as many whole rows (n_tiles key tiles each) as the scratch holds, at least one, at most C.
struct FragmentChunks {
    int rows = 0, chunks = 0;
    FragmentChunks(int C, int n_tiles, size_t scratch_tiles)
    {
        if (C < 1 || n_tiles < 1) return;
        size_t r = scratch_tiles / (size_t)n_tiles;
        if (r < 1) return;                                    // not one row fits: no plan
        if (r > (size_t)C) r = (size_t)C;
        if (r > 65535) r = 65535;                             // a queue item names its row in 16 bits
        rows = (int)r;
        chunks = (C + rows - 1) / rows;
    }
    int begin(int k) const { return k * rows; }
    int count(int k, int C) const { const int left = C - k * rows; return left < rows ? (left < 0 ? 0 : left) : rows; }
};

struct FragmentStore {
    bool valid = false, declined = false;                     // declined: the count pass of this key showed it would not fit
    GeometryKey key = GeometryKey::make();
    uint64_t budget = FRAGMENT_DEFAULT_BUDGET;
    uint64_t builds = 0, passes_served = 0;                   // since the context was created
    uint64_t groups = 0, bytes = 0, pairs = 0;                // of the store that is held (0: none); pairs: (row, tile) with a group

    // Geometry rebuilt, or about to be: nothing of it is good any more.  The buffers stay allocated for the next build.
    void drop() { valid = declined = false; groups = bytes = pairs = 0; }
    bool serves(const GeometryKey &k) const { return valid && key.equals(k); }
    bool refused(const GeometryKey &k) const { return declined && key.equals(k); }

    // bytes a store of `n_groups` groups over `n_slots` (row, tile) slots takes: the groups and the offsets (one more than slots)
    static uint64_t bytes_for(uint64_t n_groups, uint64_t n_slots) { return n_groups * FRAGMENT_GROUP_BYTES + (n_slots + 1) * sizeof(uint64_t); }
    bool fits(uint64_t n_groups, uint64_t n_slots) const { return bytes_for(n_groups, n_slots) <= budget; }

    // counts per (row, tile) slot, row-major -> offs[0 .. n]: where every slot's groups start, offs[n] = groups in all.  A row's list
    // is offs[row * n_tiles] .. offs[(row + 1) * n_tiles], ordered by tile.  Also counts the slots that hold anything.
    static uint64_t scan(const uint32_t *counts, size_t n, uint64_t *offs, uint64_t *n_pairs = nullptr)
    {
        uint64_t at = 0, p = 0;
        for (size_t i = 0; i < n; i++) { offs[i] = at; at += counts[i]; p += counts[i] != 0; }
        offs[n] = at;
        if (n_pairs) *n_pairs = p;
        return at;
    }
    void built(const GeometryKey &k, uint64_t n_groups, uint64_t n_slots, uint64_t n_pairs)
    {
        key = k; valid = true; declined = false;
        groups = n_groups; bytes = bytes_for(n_groups, n_slots); pairs = n_pairs;
        builds++;
    }
    void decline(const GeometryKey &k) { drop(); key = k; declined = true; }
};

}  // namespace rope
