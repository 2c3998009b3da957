// rope_geomcache.h — what a fixed grid keeps from pass to pass, as far as it is plain C++: the record that says which pass the
// context's geometry buffers (link matrices, screen boxes, tile masks, queue weights, layer key tiles) were built by, and the host
// copy of the last uploaded candidates that tells an upload of the same rows from a new one.  No HIP here: tests/geomcache_main.cpp
// builds this file alone.  The buffers themselves, and who drops the record, are rope_ctx.h / rope_abi.hip.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace rope {

// Everything the cached buffers are a function of.  Compared byte by byte: make() zeroes the padding.
struct GeometryKey {
    uint64_t cand_epoch, camera_epoch, robot_epoch;         // bumped by every upload of new rows, rope_set_camera, rope_set_robot[_mesh]
    uint64_t cap_layers, cap_layer_sums, cap_bounds, cap_mvp, q_segment;     // a re-grown buffer holds nothing
    int32_t C, n_layers, n_parents, n_render, n_shared;
    int32_t strategy, n_cu;
    uint8_t parents, queue, weighted, clip;                 // the launch structure the pass took
    uint32_t frame_bytes;
    unsigned char frame[64];                                // the pass's FrameParams (it carries the crop)

    static GeometryKey make() { GeometryKey k; std::memset(&k, 0, sizeof k); return k; }
    bool set_frame(const void *fp, size_t bytes)
    {
        if (bytes > sizeof frame) return false;
        std::memset(frame, 0, sizeof frame);
        std::memcpy(frame, fp, bytes);
        frame_bytes = (uint32_t)bytes;
        return true;
    }
    bool equals(const GeometryKey &o) const { return std::memcmp(this, &o, sizeof *this) == 0; }
};

struct GeometryCache {
    bool valid = false;
    GeometryKey key = GeometryKey::make();
    uint64_t hits = 0, misses = 0;

    void drop() { valid = false; }
    bool holds(const GeometryKey &k) const { return valid && key.equals(k); }
    void filled(const GeometryKey &k) { key = k; valid = true; }
};

// The rows of the last rope_candidates_upload, on the host.  A vector of its own: the pinned staging block is reused by downloads.
struct CandidateShadow {
    std::vector<double> rows;
    int C = 0;
    bool group = false, valid = false;

    void drop() { valid = false; }
    // the same rows, bit for bit (-0.0 is not 0.0: the grouping into layers goes by bits as well)
    bool same(const double *cand, int C_, bool group_) const
    {
        return valid && cand && C_ == C && group_ == group && rows.size() == 6 * (size_t)C_ &&
               std::memcmp(rows.data(), cand, rows.size() * sizeof(double)) == 0;
    }
    void keep(const double *cand, int C_, bool group_)
    {
        rows.assign(cand, cand + 6 * (size_t)C_);
        C = C_; group = group_; valid = true;
    }
};

}  // namespace rope
