// rope_abi.hip — host side of librope_hip.so: the context's life cycle, robot, camera, single target, candidates, launch sequencing
// (enqueue_*), results, render, coverage, the stored table and the debug entries.  The context itself: rope_ctx.h; the sets of
// targets and the camera-pose frames: rope_abi_targets.hip; the entries that are plain CPU code: rope_hostprep.cpp.
// Declarations and the reference call sites each entry point replaces: include/rope_s3d.h.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "rope_ctx.h"

// ---- roctx ranges (the reference times its stages with utils.Timer / FancyTimer, robotpose/utils.py:122-180).
// Named ranges around the phases of a pass and around every stage of the stage machine show up in `rocprofv3 --marker-trace`;
// the library is looked up at run time (librocprofiler-sdk-roctx, else the older libroctx64) and its absence costs two null checks.
namespace {
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        if (const char *e = std::getenv("ROPE_ROCTX")) if (e[0] == '0') return;
        for (const char *name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            if (void *h = dlopen(name, RTLD_LAZY | RTLD_LOCAL)) {
                push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
Roctx &roctx() { static Roctx r; return r; }
}  // namespace

void rope_range_push(const char *name) { if (roctx().push) (void)roctx().push(name); }
void rope_range_pop() { if (roctx().pop) (void)roctx().pop(); }

// what rope_buffers.h allocates with
int rope_dev_alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
int rope_dev_free(void *p) { return hipFree(p); }
int rope_pinned_free(void *p) { return hipHostFree(p); }
int rope_pinned_alloc(void **p, size_t bytes, void **dev_alias)
{
    hipError_t e = hipHostMalloc(p, bytes, dev_alias ? hipHostMallocMapped : hipHostMallocDefault);
    if (e != hipSuccess || !dev_alias) return e;
    e = hipHostGetDevicePointer(dev_alias, *p, 0);
    if (e != hipSuccess) { (void)hipHostFree(*p); *p = nullptr; }
    return e;
}

static thread_local std::string g_create_err;

extern "C" int rope_create(rope_ctx **out, int device)
{
    if (!out) return ROPE_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        g_create_err = "no usable HIP device";
        return ROPE_E_HIP;
    }
    rope_ctx *c = new (std::nothrow) rope_ctx();
    if (!c) return ROPE_E_NOMEM;
    c->device = device;
    PassTunables &t = c->tune;
    if (const char *e = std::getenv("ROPE_SPLIT_TARGET")) t.split_target = std::max(1, std::atoi(e));     // tuning aid
    if (const char *e = std::getenv("ROPE_STRATEGY")) c->strategy = std::atoi(e) & 255;                     // tuning aid: rope_set_strategy's bits
    if (const char *e = std::getenv("ROPE_SPLIT_CAP")) t.split_cap = std::max(1, std::min(64, std::atoi(e)));
    if (const char *e = std::getenv("ROPE_SPLIT_MIN")) t.split_min = std::max(1, std::min(64, std::atoi(e)));
    if (const char *e = std::getenv("ROPE_GEO_ROWS")) t.geo_rows = std::max(0, std::min(OWN_GEOMETRY_MAX_ROWS, std::atoi(e)));     // d_touched holds that many rows
    if (const char *e = std::getenv("ROPE_LAYER_MIN_WG")) t.layer_min_wg = std::max(0, std::atoi(e));
    if (const char *e = std::getenv("ROPE_SPLIT_MIN_MANY")) t.split_min_many = std::max(1, std::min(64, std::atoi(e)));
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        g_create_err = "hipSetDevice/hipStreamCreate failed";
        delete c;
        return ROPE_E_HIP;
    }
    if (c->h_err.reset(rope_ctx::TARGET_HOST_ROWS + 2) || c->h_cand.reset(6 * rope_ctx::TARGET_HOST_ROWS) ||
        c->h_frame_of.reset(rope_ctx::TARGET_HOST_ROWS) || c->d_best_idx.reset(1) || c->d_qctr.reset(2 * QUEUE_COUNTERS) ||
        c->d_best_err.reset(1) || c->d_PV.reset(16) || c->d_joint_fixed.reset(72) || c->d_joint_axes.reset(18)) {
        g_create_err = "hipMalloc failed";
        delete c;
        return ROPE_E_NOMEM;
    }
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu < 1) c->n_cu = 256;
    *out = c;
    return ROPE_OK;
}

// page-locked host memory (rope_host_alloc, or anything else registered with the runtime)?
static bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }     // pageable memory: an error by design
    return attr.type == hipMemoryTypeHost;
}

extern "C" void *rope_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

extern "C" void rope_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int copy_h2d_on(hipStream_t stream, PinnedBuf<unsigned char> &block, std::string &err, void *dst, const void *src, size_t bytes)
{
    constexpr size_t CHUNK = 8u << 20;
    auto failed = [&](hipError_t e, const char *what) { if (e != hipSuccess) err = std::string(what) + ": " + hipGetErrorString(e); return e != hipSuccess; };
    if (bytes >= (64u << 10) && is_pinned_host(src))       // already page-locked: one copy at the link's rate, no staging; the caller synchronises
        return failed(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync (host to device)") ? ROPE_E_HIP : ROPE_OK;
    if (failed(static_cast<hipError_t>(block.grow(2 * CHUNK)), "hipHostMalloc (copy block)")) return ROPE_E_HIP;   // two halves, alternating
    int half = 0;
    for (size_t off = 0; off < bytes; off += CHUNK, half ^= 1) {
        const size_t n = std::min(CHUNK, bytes - off);
        // the half about to be overwritten is free again
        if ((off >= 2 * CHUNK || off == 0) && failed(hipStreamSynchronize(stream), "hipStreamSynchronize (copy block)")) return ROPE_E_HIP;
        std::memcpy(block + half * CHUNK, static_cast<const unsigned char *>(src) + off, n);
        if (failed(hipMemcpyAsync(static_cast<unsigned char *>(dst) + off, block + half * CHUNK, n, hipMemcpyHostToDevice, stream), "hipMemcpyAsync (host to device)"))
            return ROPE_E_HIP;
    }
    return ROPE_OK;
}

int copy_h2d_staged(rope_ctx *c, void *dst, const void *src, size_t bytes)
{
    return copy_h2d_on(c->stream, c->h_copy, c->err, dst, src, bytes);
}

int copy_d2h_staged(rope_ctx *c, void *dst, const void *src, size_t bytes)
{
    constexpr size_t CHUNK = 8u << 20;
    HIP_TRY(c, c->h_copy.grow(2 * CHUNK));
    for (size_t off = 0; off < bytes; off += 2 * CHUNK) {
        const size_t n = std::min(2 * CHUNK, bytes - off);
        HIP_TRY(c, hipMemcpyAsync(c->h_copy, static_cast<const unsigned char *>(src) + off, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::memcpy(static_cast<unsigned char *>(dst) + off, c->h_copy, n);
    }
    return ROPE_OK;
}

extern "C" void rope_destroy(rope_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (hipEvent_t e : c->stage_events) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
    c->stage_events.clear();
    const hipStream_t stream = c->stream, copy_stream = c->copy_stream;
    delete c;                                     // every buffer goes with it: before the streams, as ever
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (stream) (void)hipStreamDestroy(stream);
}

#ifndef ROPE_BUILD_ID
#define ROPE_BUILD_ID "unknown"
#endif
extern "C" const char *rope_build_id(void) { return ROPE_BUILD_ID; }

extern "C" const char *rope_last_error(rope_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

// for the host-side stage machine (rope_predict.cpp), which sees the context only through the C ABI
void rope_set_error(rope_ctx *c, const std::string &msg) { if (c) c->err = msg; }

extern "C" int rope_set_robot(rope_ctx *c, const uint32_t *ml_header, int n_meshlets, const float *ml_verts,
                              int n_ml_verts, const uint32_t *ml_tris, int n_ml_tris, const int32_t *link_first,
                              int n_links, const double *joint_fixed, const double *joint_axes)
{
    if (!c) return ROPE_E_ARG;
    if (!ml_header || !ml_verts || !ml_tris || !link_first || !joint_fixed || !joint_axes) ARG_FAIL(c, "rope_set_robot: null pointer");
    if (n_links < 1 || n_links > ROPE_MAX_LINKS) ARG_FAIL(c, "rope_set_robot: n_links must be 1..6");
    if (n_meshlets < 1 || n_meshlets > MAX_MESHLETS) ARG_FAIL(c, "rope_set_robot: meshlet count out of range");
    if (link_first[0] != 0 || link_first[n_links] != n_meshlets) ARG_FAIL(c, "rope_set_robot: link_first does not span the meshlets");
    // validate every meshlet against the pools so that no kernel can index out of bounds
    std::vector<float> aabb(8 * (size_t)n_meshlets, 0.0f);
    for (int l = 0; l < n_links; l++) {
        if (link_first[l + 1] < link_first[l]) ARG_FAIL(c, "rope_set_robot: link_first not monotone");
        for (int m = link_first[l]; m < link_first[l + 1]; m++) {
            const uint32_t *h = ml_header + 8 * (size_t)m;
            uint32_t v0 = h[4], t0 = h[5], nv = h[6] & 0xFFFF, nt = h[6] >> 16;
            if (h[7] != (uint32_t)l) ARG_FAIL(c, "rope_set_robot: meshlet link id mismatch");
            if (nv < 1 || nv > MESHLET_MAX_VERTS || (size_t)v0 + nv > (size_t)n_ml_verts) ARG_FAIL(c, "rope_set_robot: meshlet vertex range");
            if (nt < 1 || nt > MESHLET_MAX_TRIS || (size_t)t0 + nt > (size_t)n_ml_tris) ARG_FAIL(c, "rope_set_robot: meshlet triangle range");
            for (uint32_t t = 0; t < nt; t++) {
                uint32_t p = ml_tris[t0 + t];
                if ((p & 0xFF) >= nv || ((p >> 8) & 0xFF) >= nv || ((p >> 16) & 0xFF) >= nv) ARG_FAIL(c, "rope_set_robot: triangle index outside its meshlet");
            }
            double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
            for (uint32_t v = 0; v < nv; v++)
                for (int k = 0; k < 3; k++) {
                    double x = ml_verts[3 * (size_t)(v0 + v) + k];
                    if (!std::isfinite(x)) ARG_FAIL(c, "rope_set_robot: non-finite vertex");
                    lo[k] = std::min(lo[k], x);
                    hi[k] = std::max(hi[k], x);
                }
            for (int k = 0; k < 3; k++) {
                // box centre and half extent, rounded outwards
                float ctr = (float)(0.5 * (lo[k] + hi[k]));
                float ext = (float)(std::max(hi[k] - (double)ctr, (double)ctr - lo[k]) * (1.0 + 1e-6) + 1e-7);
                aabb[8 * (size_t)m + k] = ctr;
                aabb[8 * (size_t)m + 4 + k] = ext;
            }
        }
    }
    // how far from the base origin a vertex can get: joints rotate, so a link's points stay within the sum of the joint
    // offsets up to it plus the link's own extent about its origin — whatever the joint angles
    double reach = 0.0, chain = 0.0;
    for (int l = 0; l < n_links; l++) {
        if (l > 0) chain += std::sqrt(joint_fixed[12 * (l - 1) + 3] * joint_fixed[12 * (l - 1) + 3] + joint_fixed[12 * (l - 1) + 7] * joint_fixed[12 * (l - 1) + 7] +
                                      joint_fixed[12 * (l - 1) + 11] * joint_fixed[12 * (l - 1) + 11]);
        double r = 0.0;
        for (int m = link_first[l]; m < link_first[l + 1]; m++) {
            double far2 = 0.0;
            for (int k = 0; k < 3; k++) {
                const double a = std::fabs((double)aabb[8 * (size_t)m + k]) + (double)aabb[8 * (size_t)m + 4 + k];
                far2 += a * a;
            }
            r = std::max(r, std::sqrt(far2));
        }
        reach = std::max(reach, chain + r);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    c->drop_kept();                               // boxes, masks, weights and layer tiles are this robot's no longer
    c->shadow.drop();
    c->robot_epoch++;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, c->d_header.reset(8 * (size_t)n_meshlets));
    HIP_TRY(c, c->d_verts.reset(3 * (size_t)n_ml_verts));
    HIP_TRY(c, c->d_tris.reset((size_t)n_ml_tris));
    HIP_TRY(c, c->d_aabb.reset(8 * (size_t)n_meshlets));
    HIP_TRY(c, hipMemcpyAsync(c->d_aabb, aabb.data(), 32 * (size_t)n_meshlets, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_header, ml_header, 32 * (size_t)n_meshlets, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_verts, ml_verts, 12 * (size_t)n_ml_verts, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_tris, ml_tris, 4 * (size_t)n_ml_tris, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_joint_fixed, joint_fixed, 72 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_joint_axes, joint_axes, 18 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // Every copy and fill of this library goes through the context's OWN stream and is waited for there: the stream is a
    // non-blocking one, which the null stream's operations are not ordered with, and whether a null-stream hipMemset / hipMemcpy
    // has finished when it returns is the runtime's business (round 3: a first small batch on a fresh context sometimes scored
    // against stamps that a late hipMemset of their array had wiped)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->rp.ml_header = c->d_header;
    c->rp.ml_verts = c->d_verts;
    c->rp.ml_tris = c->d_tris;
    for (int l = 0; l <= ROPE_MAX_LINKS; l++) c->rp.link_first[l] = link_first[l < n_links ? l : n_links];
    c->rp.ml_aabb = c->d_aabb;
    c->rp.n_meshlets = n_meshlets;
    c->cap = 0;                                   // per-candidate buffers depend on the meshlet count
    c->C = 0;
    c->table_C = 0;
    c->n_links = n_links;
    c->n_meshlets = n_meshlets;
    c->reach = reach;
    c->have_robot = true;
    return ROPE_OK;
}

extern "C" int rope_set_camera(rope_ctx *c, const double *PV, int W, int H, double znear, double zfar)
{
    if (!c) return ROPE_E_ARG;
    if (!PV) ARG_FAIL(c, "rope_set_camera: null PV");
    if (W < 1 || H < 1 || W > 8192 || H > 8192) ARG_FAIL(c, "rope_set_camera: image size out of range");
    if (!(znear > 0.0) || !(zfar > znear)) ARG_FAIL(c, "rope_set_camera: need 0 < znear < zfar");
    HIP_TRY(c, hipSetDevice(c->device));
    c->drop_kept();                               // whatever the values: the matrices are not compared
    c->camera_epoch++;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const bool resized = !c->have_camera || W != c->fp.W || H != c->fp.H;
    // the new geometry in locals: the context keeps describing the old image until every buffer of the new one exists
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + TILE_H - 1) / TILE_H, n_tiles = tiles_x * tiles_y;
    if ((n_tiles + 31) / 32 > MAX_MASK_WORDS) ARG_FAIL(c, "rope_set_camera: too many tiles");
    if (resized) {
        // a failed allocation below must not leave old-sized (or freed) buffers behind a camera that looks usable:
        // the context has no camera, no target and no frames until this call has gone through
        c->have_camera = false;
        c->single.n = c->resident.n = 0;
        c->single.has_ts = false;
        c->staged.n = 0;                          // a staged set of the old size is not committed
        c->C = 0;
        c->cand_valid = c->results_valid = false;
        HIP_TRY(c, c->single.grow(W, H, 1, true, true, false));
        HIP_TRY(c, c->d_cover.reset((size_t)W * H));
        HIP_TRY(c, c->single_empty.grow(1, (size_t)n_tiles));
        c->single_empty.invalidate();
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_PV, PV, 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(c->h_PV, PV, sizeof c->h_PV);
    c->fp.W = W; c->fp.H = H;
    c->fp.tiles_x = tiles_x;
    c->fp.tiles_y = tiles_y;
    c->fp.r0 = 0; c->fp.r1 = H - 1; c->fp.c0 = 0; c->fp.c1 = W - 1;
    c->fp.c_num = (float)(2.0 * znear * zfar);
    c->fp.c_sum = (float)(zfar + znear);
    c->fp.c_dif = (float)(zfar - znear);
    // per-candidate buffers are sized by the tile count (mask words; the queue's weights, one per tile)
    if (n_tiles != c->n_tiles) { c->mask_words = (n_tiles + 31) / 32; c->cap = 0; c->C = 0; c->cand_valid = c->results_valid = false; }
    c->n_tiles = n_tiles;
    c->table_C = 0;                               // a stored lookup table belongs to one camera
    c->have_camera = true;
    return ROPE_OK;
}

extern "C" int rope_set_target(rope_ctx *c, const uint64_t *tq, const float *t32, const uint8_t *link_flags)
{
    if (!c) return ROPE_E_ARG;
    if (!c->have_camera) ARG_FAIL(c, "rope_set_target: call rope_set_camera first");
    if (!tq || !link_flags) ARG_FAIL(c, "rope_set_target: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    size_t n = (size_t)c->fp.W * c->fp.H;
    int rc = copy_h2d_staged(c, c->single.tq, tq, n * sizeof(uint64_t));
    if (rc) return rc;
    if (t32) { rc = copy_h2d_staged(c, c->single.t32, t32, n * sizeof(float)); if (rc) return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->single.has_t32 = (t32 != nullptr);
    c->single.has_ts = false;
    std::memcpy(c->lf.f, link_flags, 8);
    c->single.n = 1;
    c->single_empty.invalidate();
    return ROPE_OK;
}

extern "C" int rope_set_target_tsweep(rope_ctx *c, const float *t32_full)
{
    if (!c) return ROPE_E_ARG;
    if (c->single.n < 1) ARG_FAIL(c, "rope_set_target_tsweep: call rope_set_target first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (t32_full) {
        const int rc = copy_h2d_staged(c, c->single.ts, t32_full, (size_t)c->fp.W * c->fp.H * sizeof(float));
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->single.has_ts = (t32_full != nullptr);
    c->single_empty.valid[ROPE_LOSS_TSWEEP] = false;    // that loss's "nothing rendered" sums belong to the other plane
    return ROPE_OK;
}


// Can a vertex of the robot get behind the near plane of camera PV (P·V, row-major doubles)?  z + w is affine in the world
// position; over the ball of radius `reach` about the base origin it is at least its value at the origin minus |gradient|
// times the radius.  Conservative with a centimetre to spare: "no" means the kernels without the clipping code draw every
// triangle exactly as the clipping ones would.
bool near_plane_in_reach(const rope_ctx *c, const double *PV)
{
    const double g[3] = {PV[8] + PV[12], PV[9] + PV[13], PV[10] + PV[14]}, h = PV[11] + PV[15];
    const double gn = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    return !(h - gn * (c->reach + 0.01) > 0.0);                  // NaN counts as "in reach"
}

// the raster kernels that can clip, for this context's camera (or, on the camera-pose path, the current call's cameras)
static bool use_clip(const rope_ctx *c, bool views = false)
{
    if (c->strategy & STRATEGY_CLIP_KERNELS) return true;
    return views ? c->clip_views : near_plane_in_reach(c, c->h_PV);
}

int ensure_capacity(rope_ctx *c, int C)
{
    if (C <= c->cap) return ROPE_OK;
    c->drop_kept();                               // every per-candidate buffer is allocated anew
    c->shadow.drop();
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int cap = C < 64 ? 64 : C;
    HIP_TRY(c, c->d_cand.reset(6 * (size_t)cap));
    HIP_TRY(c, c->d_err.reset((size_t)cap + 2));              // errors, then best error and best index
    HIP_TRY(c, c->h_stage.reset((size_t)cap * 6 + 2));
    HIP_TRY(c, c->d_mvp.reset((size_t)cap * ROPE_MAX_LINKS * 16));
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "candidates: robot and camera must be set first");
    HIP_TRY(c, c->d_bounds.reset((size_t)cap * c->n_meshlets));
    HIP_TRY(c, c->d_mask_lo.reset((size_t)cap * c->mask_words));
    HIP_TRY(c, c->d_mask_hi.reset((size_t)cap * c->mask_words));
    HIP_TRY(c, c->d_layer_of.reset((size_t)cap));
    HIP_TRY(c, c->d_sums.reset((size_t)cap * ROPE_SUM_WORDS));
    // raster queue: QUEUE_CLASSES segments (pairs by weight, heaviest first) and the per-(candidate, tile) weights, when the frame
    // has few enough tiles for the weights and the segments stay small; otherwise one segment, pairs in candidate order
    const size_t seg = (size_t)cap * c->mask_words * 32;
    c->q_weighted = c->n_tiles <= QUEUE_WEIGHT_TILES && 2 * seg * QUEUE_CLASSES * sizeof(uint32_t) <= ((size_t)512 << 20);
    c->q_segment = c->q_weighted ? seg : 0;
    HIP_TRY(c, c->d_qitems.reset(c->q_weighted ? 2 * seg * QUEUE_CLASSES : seg));      // weighted: the scoring queue, then the layer queue
    c->d_tile_tris.release();
    c->d_tile_tris_lo.release();
    if (c->q_weighted) {
        HIP_TRY(c, c->d_tile_tris.reset((size_t)cap * c->n_tiles));
        HIP_TRY(c, c->d_tile_tris_lo.reset((size_t)cap * c->n_tiles));
    }
    c->cap = cap;
    return ROPE_OK;
}

extern "C" int rope_candidates_upload(rope_ctx *c, const double *cand, int C)
{
    if (!c) return ROPE_E_ARG;
    return upload_candidates(c, cand, C, true);
}

int upload_candidates(rope_ctx *c, const double *cand, int C, bool group, const int32_t *frame_of)
{
    if (!cand || C < 1 || C > 65535) ARG_FAIL(c, "rope_candidates_upload: need 1 <= C <= 65535");
    // The rows that are resident already (a fixed grid scored against frame after frame through rope_eval): nothing to check, copy,
    // sort or upload, and the candidate epoch — with it the geometry a pass may have kept — stands.  Only while the last upload
    // still describes the context: the camera-pose and render entries take the rows away (cand_valid), a new capacity drops the shadow.
    if (!frame_of && c->cand_valid && c->C == C && c->shadow.same(cand, C, group)) {
        c->results_valid = false;
        return ROPE_OK;
    }
    c->shadow.drop();
    c->drop_kept();
    c->cand_epoch++;
    for (size_t i = 0; i < 6 * (size_t)C; i++)
        if (!std::isfinite(cand[i]) || std::fabs(cand[i]) > 1.0e4) ARG_FAIL(c, "rope_candidates_upload: joint angle not finite or |q| > 1e4 rad");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_capacity(c, C);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // the staging buffer may still feed an earlier copy
    if (C <= (frame_of ? rope_ctx::TARGET_HOST_ROWS : rope_ctx::HOST_ERR_ROWS)) {            // nothing is in flight (synchronised above): the kernels of the next pass read it in place
        std::memcpy(c->h_cand, cand, 6 * (size_t)C * sizeof(double));
        c->cand_dev = c->h_cand.dev();
        if (frame_of) { std::memcpy(c->h_frame_of, frame_of, (size_t)C * sizeof(int32_t)); c->frame_of_dev = c->h_frame_of.dev(); }
    } else {
        std::memcpy(c->h_stage, cand, 6 * (size_t)C * sizeof(double));
        HIP_TRY(c, hipMemcpyAsync(c->d_cand, c->h_stage, 6 * (size_t)C * sizeof(double), hipMemcpyHostToDevice, c->stream));
        c->cand_dev = c->d_cand;
        if (frame_of) {
            rc = sync_grow(c, c->d_frame_of, (size_t)std::max(C, 1024));
            if (rc) return rc;
            // pageable source: the copy has read it when the call returns
            HIP_TRY(c, hipMemcpyAsync(c->d_frame_of, frame_of, (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            c->frame_of_dev = c->d_frame_of;
        }
    }
    if (!frame_of) c->frame_of_dev = nullptr;
    // group candidates whose first two joint angles are bit-identical: their base_link, link_1_s and
    // link_2_l transforms are the same bits, so those links are rasterised once per group (a "layer")
    c->n_layers = C;                               // "no sharing" unless the grouping below finds some
    if (group && C >= 8) {
        struct Key { uint64_t a, b; int idx, frame; };
        std::vector<Key> keys((size_t)C);
        for (int i = 0; i < C; i++) {
            std::memcpy(&keys[i].a, &cand[6 * (size_t)i], 8);
            std::memcpy(&keys[i].b, &cand[6 * (size_t)i + 1], 8);
            keys[i].idx = i;
            keys[i].frame = frame_of ? frame_of[i] : 0;
        }
        std::sort(keys.begin(), keys.end(), [](const Key &x, const Key &y) {
            return x.frame != y.frame ? x.frame < y.frame : (x.a != y.a ? x.a < y.a : (x.b != y.b ? x.b < y.b : x.idx < y.idx));
        });
        std::vector<int32_t> layer_of((size_t)C), layer_rep, parent_of, parent_rep;
        for (int i = 0; i < C; i++) {
            const bool new_frame = i == 0 || keys[i].frame != keys[i - 1].frame;
            if (new_frame || keys[i].a != keys[i - 1].a || keys[i].b != keys[i - 1].b) {
                layer_rep.push_back(keys[i].idx);
                // layers come out sorted by q0: a new q0 opens a new parent, represented by this layer's own candidate
                if (new_frame || keys[i].a != keys[i - 1].a) parent_rep.push_back(keys[i].idx);
                parent_of.push_back((int32_t)parent_rep.size() - 1);
            }
            layer_of[keys[i].idx] = (int32_t)layer_rep.size() - 1;
        }
        c->n_layers = (int)layer_rep.size();
        c->n_parents = (int)parent_rep.size();
        if (layers_wanted(c->n_layers, C)) {        // only then are the arrays read
            rc = sync_grow(c, c->d_layer_rep, (size_t)c->n_layers);
            if (rc) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->d_layer_of, layer_of.data(), (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(c->d_layer_rep, layer_rep.data(), layer_rep.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            if (parents_wanted(c->n_parents, c->n_layers)) {
                rc = sync_grow(c, c->d_parent_of, (size_t)c->n_layers, c->d_parent_rep, (size_t)c->n_layers);
                if (rc) return rc;
                HIP_TRY(c, hipMemcpyAsync(c->d_parent_of, parent_of.data(), parent_of.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
                HIP_TRY(c, hipMemcpyAsync(c->d_parent_rep, parent_rep.data(), parent_rep.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            }
            HIP_TRY(c, hipStreamSynchronize(c->stream));   // layer_of / layer_rep are stack-local
        }
    }
    c->C = C;
    c->cand_valid = true;
    c->results_valid = false;
    if (!frame_of) c->shadow.keep(cand, C, group);
    return ROPE_OK;
}

int apply_crop(rope_ctx *c, const char *who, const int32_t *crop, FrameParams &fp, double &n_pix)
{
    if (crop[0] < 0 || crop[1] >= fp.H || crop[0] > crop[1] || crop[2] < 0 || crop[3] >= fp.W || crop[2] > crop[3])
        ARG_FAIL(c, std::string(who) + ": crop outside the image");
    fp.r0 = crop[0]; fp.r1 = crop[1]; fp.c0 = crop[2]; fp.c1 = crop[3];
    n_pix = (double)(crop[1] - crop[0] + 1) * (double)(crop[3] - crop[2] + 1);
    return ROPE_OK;
}

int loss_frame(rope_ctx *c, const char *who, int loss, const int32_t *crop, FrameParams &fp, double &n_pix)
{
    fp = c->fp;
    n_pix = (double)fp.W * fp.H;
    if (loss != ROPE_LOSS_LOOKUP) return ROPE_OK;
    if (!crop) ARG_FAIL(c, std::string(who) + ": lookup loss needs a crop");
    return apply_crop(c, who, crop, fp, n_pix);
}

static int check_eval_args(rope_ctx *c, int n_render, int loss, const int32_t *crop, FrameParams &fp, double &n_pix)
{
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "eval: robot and camera must be set first");
    if (c->C < 1 || !c->cand_valid) ARG_FAIL(c, "eval: no candidates resident (upload them again after rope_eval_views)");
    if (n_render < 1 || n_render > c->n_links) ARG_FAIL(c, "eval: n_render out of range");
    if (loss < 0 || loss > 3) ARG_FAIL(c, "eval: unknown loss");
    if (c->single.n < 1) ARG_FAIL(c, "eval: no target set");
    if (loss == ROPE_LOSS_LOOKUP && !c->single.has_t32) ARG_FAIL(c, "eval: this loss needs the float32 target plane");
    if (loss == ROPE_LOSS_TSWEEP && !c->single.plane32(loss)) ARG_FAIL(c, "eval: this loss needs a float32 target plane");
    return loss_frame(c, "eval", loss, crop, fp, n_pix);
}

int ensure_totals(rope_ctx *c, const TargetSet &s, EmptyCache &cache, int loss, const FrameParams &fp)
{
    if (cache.fresh(loss, fp)) return ROPE_OK;
    HIP_TRY(c, launch_empty(loss, c->stream, fp, s.tq, s.plane32(loss), nullptr, cache.scratch, cache.total(loss), s.n));
    cache.filled(loss, fp);
    return ROPE_OK;
}

// What the rules of rope_passplan.h read, taken from the context once per pass.  `clip`: use_clip() for the pass's cameras.  The
// render, coverage, table and debug entries, which only take the geometry part of a plan, say EVAL_SINGLE.
static PassInputs pass_inputs(const rope_ctx *c, int n_render, int loss, const FrameParams &fp, EvalKind kind, bool frame_index, bool clip)
{
    PassInputs in;
    in.C = c->C; in.n_tiles = c->n_tiles; in.n_layers = c->n_layers; in.n_parents = c->n_parents;
    in.n_render = n_render; in.loss = loss; in.kind = kind; in.frame_index = frame_index;
    in.strategy = c->strategy; in.n_cu = c->n_cu; in.q_weighted = c->q_weighted;
    in.clip = clip; in.skip = ROPE_SKIP(fp, ~0);
    in.t = c->tune;
    return in;
}

static int ensure_layers(rope_ctx *c)
{
    size_t need = (size_t)c->n_layers * c->n_tiles * (TILE_W * TILE_H);
    // (a re-grown buffer drops the kept geometry: sync_grow)
    return sync_grow(c, c->d_layers, need, c->d_layer_sums, (size_t)c->n_layers * c->n_tiles * ROPE_SUM_WORDS);
}

// The shared links of every layer into c->d_layers (+ their loss sums when `la` carries targets and layer_sums).
// Two levels when many layers share their first joint angle: links 0-1 once per distinct q0, then link 2 per layer
// merged with its parent's tile.
static int enqueue_layers(rope_ctx *c, const PassPlan &plan, RasterArgs la, int loss, const FrameParams &fp)
{
    c->drop_kept();                               // every writer of the layer tiles comes through here
    la.cand_of_row = c->d_layer_rep; la.layers = c->d_layers;
    if (plan.parents) {
        const size_t need = (size_t)c->n_parents * c->n_tiles * (TILE_W * TILE_H);
        if (int rc = sync_grow(c, c->d_parents, need)) return rc;
        RasterArgs pa = la;
        pa.l_begin = 0; pa.l_end = 2; pa.cand_of_row = c->d_parent_rep; pa.layers = c->d_parents; pa.layer_sums = nullptr;
        HIP_TRY(c, launch_raster(MODE_LAYER, loss, c->n_parents, c->stream, fp, c->rp, pa, plan.clip));
        la.l_begin = 2; la.l_end = 3; la.base_layers = c->d_parents; la.base_of_row = c->d_parent_of; la.base_rep = c->d_parent_rep;
    } else {
        la.l_begin = 0; la.l_end = plan.n_shared;
    }
    if (plan.layer_queue) {
        HIP_TRY(c, launch_layer_queue(loss, c->n_layers, QUEUE_WG_PER_CU * c->n_cu, c->stream, fp, c->rp, la, c->d_qitems + QUEUE_CLASSES * c->q_segment,
                                      c->q_segment, c->d_qctr + QUEUE_COUNTERS, c->d_tile_tris_lo, plan.clip));
        return ROPE_OK;
    }
    HIP_TRY(c, launch_raster(MODE_LAYER, loss, c->n_layers, c->stream, fp, c->rp, la, plan.clip));
    return ROPE_OK;
}

static RasterArgs base_args(rope_ctx *c, int n_render)
{
    RasterArgs a{};
    a.l_begin = 0; a.l_end = n_render; a.n_render = n_render;
    a.mvp = c->d_mvp; a.bounds = c->d_bounds;
    a.mask_lo = c->d_mask_lo; a.mask_hi = c->d_mask_hi; a.mask_words = c->mask_words;
    return a;
}

// the queues' per-(candidate, tile) weights, when the plan uses them
static uint32_t *queue_weights(const rope_ctx *c, const PassPlan &plan) { return plan.weighted ? c->d_tile_tris.get() : nullptr; }

// What the buffers a large layered pass leaves behind depend on (GeometryKey): candidates, camera and robot by their epochs, the
// pass's frame and n_render, and everything that decides which launches write them — the second sharing level, the queues and
// their weights, the clipping kernels: copied from the plan the pass's launches run by — plus the capacities of the
// buffers themselves.  The loss is not part of it: the one thing of these launches that depends on loss or target, the layers'
// sums, is taken anew by every pass.
static GeometryKey geometry_key(const rope_ctx *c, const PassPlan &plan, int n_render, const FrameParams &fp)
{
    static_assert(sizeof(FrameParams) <= sizeof(GeometryKey::frame), "GeometryKey::frame holds a FrameParams");
    GeometryKey k = GeometryKey::make();
    k.cand_epoch = c->cand_epoch; k.camera_epoch = c->camera_epoch; k.robot_epoch = c->robot_epoch;
    k.cap_layers = c->d_layers.cap(); k.cap_layer_sums = c->d_layer_sums.cap(); k.cap_bounds = c->d_bounds.cap(); k.cap_mvp = c->d_mvp.cap();
    k.q_segment = c->q_segment;
    k.C = c->C; k.n_layers = c->n_layers; k.n_parents = c->n_parents; k.n_render = n_render; k.n_shared = plan.n_shared;
    k.strategy = c->strategy; k.n_cu = c->n_cu;
    k.parents = plan.parents; k.queue = plan.scoring == SCORE_QUEUE; k.weighted = plan.weighted; k.clip = plan.clip;
    k.set_frame(&fp, sizeof fp);
    return k;
}

// forward kinematics + link matrices + screen boxes + tile masks (+ cleared sums) of the resident candidates
static int enqueue_geometry(rope_ctx *c, const PassPlan &plan, int n_render, const FrameParams &fp, bool views)
{
    c->drop_kept();                               // every writer of d_mvp, d_bounds, the masks and the weights comes through here
    const double *PV = views ? c->dv_PV : c->d_PV, *cand = views ? c->dv_cand : c->cand_dev;
    const int32_t *view_of = views ? c->dv_view_of : nullptr;
    const int n_shared = plan.n_shared;
    if (plan.fused_geometry) {                      // one fused launch, one workgroup per candidate
        HIP_TRY(c, launch_fk_bounds(c->stream, cand, c->C, fp, c->rp, n_render, n_shared, c->d_joint_fixed, c->d_joint_axes, PV,
                                    view_of, c->d_mvp, c->d_bounds, c->d_sums, c->d_mask_lo, c->d_mask_hi, c->mask_words));
        return ROPE_OK;
    }
    HIP_TRY(c, launch_fk(c->stream, cand, c->C, n_render, c->d_joint_fixed, c->d_joint_axes, PV, view_of, c->d_mvp, c->d_sums,
                         c->d_mask_lo, c->d_mask_hi, c->mask_words, c->d_qctr, queue_weights(c, plan), c->d_tile_tris_lo, c->n_tiles));
    HIP_TRY(c, launch_bounds(c->stream, c->C, fp, c->rp, n_render, n_shared, c->d_mvp, c->d_bounds, c->d_mask_lo, c->d_mask_hi, c->mask_words,
                             n_shared > 0 ? c->d_layer_of : nullptr, n_shared > 0 ? c->d_layer_rep : nullptr, queue_weights(c, plan), c->d_tile_tris_lo, plan.lo_first));
    return ROPE_OK;
}

// One chunk of rows' own links into c->d_fscratch: the MODE_LAYER queue launch with a RasterArgs of its own — the row -> candidate map
// is the identity from row0 on, "mask_lo" is the candidates' mask_hi (the tiles their own links reach), the weights are the own
// links', and there is neither a parent level nor sums.  It runs on the layer queue's counters and segment, which a hit pass leaves idle.
static int draw_own_links(rope_ctx *c, const PassPlan &plan, const RasterArgs &a, int loss, const FrameParams &fp, int row0, int rows)
{
    RasterArgs la = base_args(c, a.n_render);
    la.l_begin = a.l_begin; la.l_end = a.n_render;
    la.cand_of_row = c->d_frow + row0;
    la.mask_lo = c->d_mask_hi;
    la.layers = c->d_fscratch;
    int *counters = c->d_qctr + QUEUE_COUNTERS;
    HIP_TRY(c, hipMemsetAsync(counters, 0, QUEUE_COUNTERS * sizeof(int), c->stream));
    const bool weighted = plan.weighted;
    HIP_TRY(c, launch_layer_queue(loss, rows, QUEUE_WG_PER_CU * c->n_cu, c->stream, fp, c->rp, la, weighted ? c->d_qitems + QUEUE_CLASSES * c->q_segment : c->d_qitems.get(),
                                  weighted ? c->q_segment : 0, counters, queue_weights(c, plan), plan.clip));
    return ROPE_OK;
}

// The kept fragments of the grid whose geometry the context holds, built inside the first pass that hits it: the rows' own links
// drawn chunk by chunk (draw_own_links) and counted, the counts scanned on the host — here the stream is waited for; the one pass
// that builds pays that — and, when the store fits the budget, drawn once more and written to their places.  Two draws instead of
// one so that nothing is allocated before its size is known.  The scratch and the counts are released at the end, kept or declined.  `a`: the pass's scoring arguments (masks, layers, l_begin).
// Leaves c->frags serving `key`, or declined for it; the queue counters and sums the pass's own scoring launch needs are untouched.
static int build_fragments(rope_ctx *c, const PassPlan &pass, const GeometryKey &key, const RasterArgs &a, int loss, const FrameParams &fp)
{
    RopeRange r("rope:fragments-build");
    const int n_tiles = c->n_tiles, C = c->C;
    const size_t tile_px = (size_t)TILE_W * TILE_H, n_slots = (size_t)C * n_tiles;
    const FragmentChunks plan(C, n_tiles, std::min(n_slots, c->d_layers.cap() / tile_px));      // a scratch no larger than the layer buffer
    if (!plan.rows) { c->frags.decline(key); return ROPE_OK; }
    if (int rc = sync_grow(c, c->d_fscratch, (size_t)plan.rows * n_tiles * tile_px, c->d_fcount, n_slots, c->d_foffs, n_slots + 1, c->d_frow, (size_t)C)) return rc;
    if (c->frow_filled < C) {                       // (a re-grown d_frow is larger than what was filled)
        std::vector<int32_t> id((size_t)C);
        for (int i = 0; i < C; i++) id[i] = i;
        HIP_TRY(c, hipMemcpyAsync(c->d_frow, id.data(), id.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->frow_filled = C;
    }
    HIP_TRY(c, hipMemsetAsync(c->d_fcount, 0, n_slots * sizeof(uint32_t), c->stream));
    for (int k = 0; k < plan.chunks; k++) {
        if (int rc = draw_own_links(c, pass, a, loss, fp, plan.begin(k), plan.count(k, C))) return rc;
        HIP_TRY(c, launch_fragment_count(c->stream, a, c->d_fscratch, plan.begin(k), plan.count(k, C), n_tiles, c->d_fcount));
    }
    std::vector<uint32_t> counts(n_slots);
    std::vector<uint64_t> offs(n_slots + 1);
    HIP_TRY(c, hipMemcpyAsync(counts.data(), c->d_fcount, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t n_pairs = 0;
    const uint64_t n_groups = FragmentStore::scan(counts.data(), n_slots, offs.data(), &n_pairs);
    if (!c->frags.fits(n_groups, n_slots)) {
        // over the budget: nothing is kept, and the building pass's own buffers — the scratch is as large as the layer buffer — go too
        c->d_fscratch.release(); c->d_fcount.release(); c->d_foffs.release();       // the stream is idle
        c->frags.decline(key);
        return ROPE_OK;
    }
    const size_t room = (size_t)std::max<uint64_t>(n_groups, 1);
    HIP_TRY(c, grow_each(c->d_fwhere, room, c->d_ffin, room, c->d_fbase, room));       // the stream is idle
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets go up as they are");
    HIP_TRY(c, hipMemcpyAsync(c->d_foffs, offs.data(), (n_slots + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                                         // offs is local
    for (int k = 0; k < plan.chunks; k++) {
        if (int rc = draw_own_links(c, pass, a, loss, fp, plan.begin(k), plan.count(k, C))) return rc;
        HIP_TRY(c, launch_fragment_fill(c->stream, a, c->d_fscratch, plan.begin(k), plan.count(k, C), n_tiles, c->d_foffs, c->d_fwhere, c->d_ffin, c->d_fbase));
    }
    // the scratch and the counts are the build's alone: let them go, which means one more wait in the pass that waits anyway
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->d_fscratch.release(); c->d_fcount.release();
    c->frags.built(key, n_groups, n_slots, n_pairs);
    return ROPE_OK;
}

int enqueue_eval(rope_ctx *c, int n_render, int loss, const FrameParams &fp, double n_pix, const EvalPlanes &pl, EvalKind kind, hipEvent_t *ev)
{
    const bool views = kind == EVAL_VIEWS, targets = kind == EVAL_TARGETS;
    // which launches the pass consists of: decided here, once (rope_passplan.h); below, only the plan and what the context holds
    const PassPlan plan = plan_pass(pass_inputs(c, n_render, loss, fp, kind, pl.frame_of != nullptr, use_clip(c, views)));
    const bool layers = plan.layers, geo = plan.own_geometry;
    const int n_shared = plan.n_shared, split = plan.split;
    if (layers) { int rc = ensure_layers(c); if (rc) return rc; }
    // A cacheable pass keeps its geometry for the next one (rope_ctx::geo); every other pass drops it.
    const bool cacheable = plan.cacheable;
    GeometryKey key = GeometryKey::make();
    if (cacheable) key = geometry_key(c, plan, n_render, fp);
    const bool hit = cacheable && c->geo.holds(key);
    c->geo.drop();                                  // a pass that fails half way leaves nothing behind; set again at the end
    if (plan.cache_scope) (hit ? c->geo.hits : c->geo.misses)++;
    // Kept fragments (rope_ctx::frags): a hit may be scored from them, and builds them when they are not there yet; any other pass
    // is about to write the geometry they were taken from.
    if (!hit) c->frags.drop();
    const bool frag_scope = hit && plan.fragment_scope;
    const bool served_now = frag_scope && c->frags.serves(key);       // a later hit: the scorer writes every row's sums whole, nothing to clear
    if (ev) HIP_TRY(c, hipEventRecord(ev[0], c->stream));
    if (served_now) { }
    else if (hit) HIP_TRY(c, launch_clear_pass(c->stream, c->d_sums, c->C, c->d_qctr));      // what is left of fk_mvp_kernel: cleared sums and queue counters
    else if (!geo) { RopeRange r("rope:fk+bounds"); int rc = enqueue_geometry(c, plan, n_render, fp, views); if (rc) return rc; }
    c->mvp_valid = !geo;
    if (ev) HIP_TRY(c, hipEventRecord(ev[1], c->stream));
    RasterArgs a = base_args(c, n_render);
    if (split > 1) {
        const size_t need = (size_t)c->C * c->n_tiles * (TILE_W * TILE_H);
        if (need > c->d_gtile.cap()) {
            if (int rc = sync_grow(c, c->d_gtile, need)) return rc;
            c->gtile_dirty = true;
        }
        // the scoring kernel hands the buffer back "empty"; clear it only when new, after a failed pass, or when a
        // profiling flag may have skipped that kernel's work
        if (c->gtile_dirty || ROPE_SKIP(fp, ~0)) HIP_TRY(c, hipMemsetAsync(c->d_gtile, 0xFF, c->d_gtile.cap() * sizeof(uint32_t), c->stream));
        c->gtile_dirty = true;
        RasterArgs sa = a;
        sa.split = split; sa.gtile = c->d_gtile;
        if (geo) {
            if ((size_t)c->C * c->n_tiles > c->d_touched.cap()) {      // C <= geo_rows <= OWN_GEOMETRY_MAX_ROWS: room for any such batch at once
                if (int rc = sync_grow(c, c->d_touched, (size_t)OWN_GEOMETRY_MAX_ROWS * c->n_tiles)) return rc;
                HIP_TRY(c, hipMemsetAsync(c->d_touched, 0, (size_t)OWN_GEOMETRY_MAX_ROWS * c->n_tiles * sizeof(int), c->stream));     // ordered with the kernels that stamp it
            }
            sa.cand_q = c->cand_dev; sa.joint_fixed = c->d_joint_fixed; sa.joint_axes = c->d_joint_axes; sa.PV = c->d_PV;
            sa.sums = c->d_sums;
            sa.touched = c->d_touched;
            if (c->pass_id == 0x7FFFFFFF) {                 // the stamp wraps after 2^31 passes: start over on a clean array
                HIP_TRY(c, hipMemsetAsync(c->d_touched, 0, c->d_touched.cap() * sizeof(int), c->stream));
                c->pass_id = 0;
            }
            sa.pass_id = ++c->pass_id;
            a.touched = sa.touched; a.pass_id = sa.pass_id;
        }
        HIP_TRY(c, launch_raster(geo ? MODE_SPLIT_GEO : MODE_SPLIT, loss, c->C, c->stream, fp, c->rp, sa, plan.clip));
        a.gtile = c->d_gtile;
    }
    if (layers) {
        RasterArgs la = a;
        la.layer_sums = c->d_layer_sums; la.tq = pl.tq; la.t32 = pl.t32; la.frame_of = pl.frame_of;
        if (hit) {
            // the key tiles are the last pass's; their loss sums against this pass's target are all the layer launch would add
            RopeRange r("rope:layer-sums");
            la.cand_of_row = c->d_layer_rep; la.layers = c->d_layers;
            HIP_TRY(c, launch_layer_sums(loss, c->n_layers, c->stream, fp, la));
        } else { RopeRange r("rope:shared-layers"); int rc = enqueue_layers(c, plan, la, loss, fp); if (rc) return rc; }
        a.l_begin = n_shared; a.layer_of = c->d_layer_of; a.layer_rep = c->d_layer_rep; a.layers = c->d_layers; a.layer_sums = c->d_layer_sums;
    }
    a.tq = pl.tq; a.t32 = pl.t32; a.tl = pl.tl; a.frame_of = pl.frame_of; a.sums = c->d_sums;
    if (ev) HIP_TRY(c, hipEventRecord(ev[2], c->stream));
    {
        RopeRange r("rope:raster+score");
        bool served = false;
        if (frag_scope) {
            // first hit: build the store, inside this pass (and this interval of rope_profile_eval); when the count shows it would
            // not fit the budget it is declined for this key and the pass, like every later one, runs as before
            if (!served_now && !c->frags.refused(key)) { int rc = build_fragments(c, plan, key, a, loss, fp); if (rc) return rc; }
            if (c->frags.serves(key)) {
                HIP_TRY(c, launch_fragment_score(loss, c->C, c->stream, fp, a, c->d_foffs, c->d_fwhere, c->d_ffin, c->d_fbase));
                c->frags.passes_served++;
                served = true;
            }
        }
        if (served) { }
        else if (plan.scoring == SCORE_GTILE) {
            HIP_TRY(c, launch_score_gtile(loss, c->C, plan.slices, c->stream, fp, a));
            c->gtile_dirty = ROPE_SKIP(fp, ~0);
        } else if (plan.scoring == SCORE_QUEUE) {
            // two 12-wave workgroups fit a CU
            HIP_TRY(c, launch_raster_queue(loss, c->C, QUEUE_WG_PER_CU * c->n_cu, c->stream, fp, c->rp, a, c->d_qitems, plan.weighted ? c->q_segment : 0, c->d_qctr,
                                           queue_weights(c, plan), plan.clip));
        } else {
            HIP_TRY(c, launch_raster(MODE_SCORE, loss, c->C, c->stream, fp, c->rp, a, plan.clip));
        }
    }
    if (ev) HIP_TRY(c, hipEventRecord(ev[3], c->stream));
    RopeRange fin("rope:finalize");
    if (views) return ROPE_OK;                     // per-(view, frame) sums are finalised by the caller
    c->err_on_host = c->C <= (targets ? rope_ctx::TARGET_HOST_ROWS : rope_ctx::HOST_ERR_ROWS);
    if (targets)                                   // every row against its own frame's totals and link flags; no argmin (rows of many frames)
        HIP_TRY(c, launch_finalize_frames(c->stream, c->d_sums, c->resident_empty.total(loss), pl.frame_of, c->resident.flags, c->C, loss, n_render, n_pix,
                                          c->err_on_host ? c->h_err.dev() : c->d_err.get()));
    else
        HIP_TRY(c, launch_finalize(c->stream, c->d_sums, c->single_empty.total(loss), c->C, loss, n_render, n_pix, c->lf,
                                   c->err_on_host ? c->h_err.dev() : c->d_err.get()));
    if (ev) HIP_TRY(c, hipEventRecord(ev[4], c->stream));
    c->last_n_render = n_render;
    c->results_valid = true;
    if (cacheable) c->geo.filled(key);              // every launch of the pass is in the stream
    return ROPE_OK;
}

static EvalPlanes single_planes(const rope_ctx *c, int loss) { return {c->single.tq, c->single.plane32(loss), nullptr, nullptr}; }

extern "C" int rope_eval_resident(rope_ctx *c, int n_render, int loss, const int32_t *crop)
{
    if (!c) return ROPE_E_ARG;
    FrameParams fp; double n_pix;
    int rc = check_eval_args(c, n_render, loss, crop, fp, n_pix);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = ensure_totals(c, c->single, c->single_empty, loss, fp);
    if (rc) return rc;
    return enqueue_eval(c, n_render, loss, fp, n_pix, single_planes(c, loss), EVAL_SINGLE);
}

extern "C" int rope_sync(rope_ctx *c)
{
    if (!c) return ROPE_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ROPE_OK;
}

extern "C" int rope_results_download(rope_ctx *c, double *err_out, uint64_t *sums_out, int32_t *best_idx, double *best_err)
{
    if (!c) return ROPE_E_ARG;
    if (c->C < 1 || !c->results_valid) ARG_FAIL(c, "rope_results_download: nothing evaluated (results do not survive rope_eval_views / rope_lookup_score / a new upload)");
    HIP_TRY(c, hipSetDevice(c->device));
    // one copy brings the errors, the best error and the best index (pinned staging)
    const double *res = c->err_on_host ? c->h_err.get() : c->h_stage.get();
    if (!c->err_on_host) HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->d_err, ((size_t)c->C + 2) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (sums_out) HIP_TRY(c, hipMemcpyAsync(sums_out, c->d_sums, (size_t)c->C * ROPE_SUM_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (err_out) std::memcpy(err_out, res, (size_t)c->C * sizeof(double));
    if (best_err) *best_err = res[c->C];
    if (best_idx) *best_idx = (int32_t)res[c->C + 1];
    return ROPE_OK;
}

extern "C" int rope_eval(rope_ctx *c, const double *cand, int C, int n_render, int loss, const int32_t *crop,
                         double *err_out, uint64_t *sums_out, int32_t *best_idx, double *best_err)
{
    if (!c) return ROPE_E_ARG;
    if (C <= MAX_ROWS) {
        int rc = rope_candidates_upload(c, cand, C);
        if (rc) return rc;
        rc = rope_eval_resident(c, n_render, loss, crop);
        if (rc) return rc;
        return rope_results_download(c, err_out, sums_out, best_idx, best_err);
    }
    // larger sets (lookup grids up to 200 divisions per joint, lookup.py:50): batch after batch, the argmin merged by the
    // rule of finalize_argmin_kernel — first index of the smallest error, a NaN never beats a number
    if (!cand) ARG_FAIL(c, "rope_eval: null candidates");
    int32_t best = -1;
    double be = 0.0;
    for (int lo = 0; lo < C; lo += MAX_ROWS) {
        const int n = std::min(MAX_ROWS, C - lo);
        int rc = rope_candidates_upload(c, cand + 6 * (size_t)lo, n);
        if (rc) return rc;
        rc = rope_eval_resident(c, n_render, loss, crop);
        if (rc) return rc;
        int32_t bi = 0;
        double e = 0.0;
        rc = rope_results_download(c, err_out ? err_out + lo : nullptr, sums_out ? sums_out + (size_t)lo * ROPE_SUM_WORDS : nullptr, &bi, &e);
        if (rc) return rc;
        if (best < 0 || e < be || (be != be && e == e)) { best = lo + bi; be = e; }
    }
    if (best_idx) *best_idx = best;
    if (best_err) *best_err = be;
    return ROPE_OK;
}

static int raster_only(rope_ctx *c, const double *cand, int C, int n_render, int mode)
{
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "render: robot and camera must be set first");
    if (n_render < 1 || n_render > c->n_links) ARG_FAIL(c, "render: n_render out of range");
    int rc = rope_candidates_upload(c, cand, C);
    if (rc) return rc;
    const PassPlan plan = plan_geometry(pass_inputs(c, n_render, ROPE_LOSS_DEPTH, c->fp, EVAL_SINGLE, false, use_clip(c)), false);
    rc = enqueue_geometry(c, plan, n_render, c->fp, false);
    if (rc) return rc;
    RasterArgs a = base_args(c, n_render);
    a.cover = c->d_cover;
    HIP_TRY(c, launch_raster(mode, ROPE_LOSS_DEPTH, c->C, c->stream, c->fp, c->rp, a, plan.clip));
    c->last_n_render = n_render;
    return ROPE_OK;
}

// device -> host for the render planes: one copy straight into page-locked memory, else through the staging block
static int copy_d2h_out(rope_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes >= (64u << 10) && is_pinned_host(dst)) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return ROPE_OK;
    }
    return copy_d2h_staged(c, dst, src, bytes);
}

// device bytes of output planes one chunk of rope_render_batch may hold
static constexpr size_t RENDER_BATCH_BUDGET = (size_t)256 << 20;

// What an entry of the chunked render path asks for.  A chunk's planes: depth -> d_rdepth (cleared to 0), ids -> d_rids (to 0xFF),
// labels -> d_rmask and d_rboxes (the boxes to 0xFF).
struct RenderAsk {
    const char *entry;                  // the entry's name, for the messages
    const int32_t *crop;                // rows and columns to draw, or nullptr: the whole frame
    bool depth, ids, labels;
    const uint8_t *lut;                 // a 256-byte id -> label table that rides in the staging block, or nullptr
};

// rope_render_batch, rope_render_batch_device and rope_render_masks: N poses drawn chunk by chunk into the planes the entry asks
// for.  own_checks() -> a message or nullptr: the entry's own arguments, checked where they always were (n_render is known good);
// after(lo, n, px, lut_dev) -> code: what follows the raster launch of poses lo .. lo + n - 1 and takes the results away.
template <typename Checks, typename After>
static int render_chunks(rope_ctx *c, const RenderAsk &ask, const double *q, const double *PV, int N, int n_render, Checks own_checks, After after)
{
#define RC_FAIL(msg) do { c->err = std::string(ask.entry) + ": " msg; return ROPE_E_ARG; } while (0)
    if (N < 1) RC_FAIL("need N >= 1");
    if (!ask.depth && !ask.ids && !ask.labels) RC_FAIL("no output (depth and ids both null)");
    if (!c->have_robot || !c->have_camera) RC_FAIL("robot and camera must be set first");
    if (n_render < 1 || n_render > c->n_links) RC_FAIL("n_render out of range");
    FrameParams fp = c->fp;
    double n_pix = (double)fp.W * fp.H;
    if (ask.crop)
        if (int rc = apply_crop(c, ask.entry, ask.crop, fp, n_pix)) return rc;
    if (const char *msg = own_checks()) ARG_FAIL(c, msg);
    for (size_t i = 0; i < 6 * (size_t)N; i++)
        if (!std::isfinite(q[i]) || std::fabs(q[i]) > 1.0e4) RC_FAIL("joint angle not finite or |q| > 1e4 rad");
    bool clip = use_clip(c);
    if (PV) {
        for (size_t i = 0; i < 16 * (size_t)N; i++)
            if (!std::isfinite(PV[i])) RC_FAIL("non-finite view matrix");
        clip = c->strategy & STRATEGY_CLIP_KERNELS;                // the call's cameras decide, not the context's
        for (int i = 0; i < N && !clip; i++) clip = near_plane_in_reach(c, PV + 16 * (size_t)i);
    }
#undef RC_FAIL
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t px = (size_t)n_pix;
    const size_t per_pose = px * ((ask.depth ? sizeof(float) : 0) + (ask.ids ? 1 : 0) + (ask.labels ? 1 : 0));
    const int chunk = (int)std::min<size_t>({(size_t)N, (size_t)MAX_ROWS, std::max<size_t>(1, RENDER_BATCH_BUDGET / per_pose)});
    int rc = ensure_capacity(c, chunk);
    if (rc) return rc;
    if (ask.depth && (rc = sync_grow(c, c->d_rdepth, (size_t)chunk * px))) return rc;
    if (ask.ids && (rc = sync_grow(c, c->d_rids, (size_t)chunk * px))) return rc;
    if (ask.labels && ((rc = sync_grow(c, c->d_rmask, (size_t)chunk * px)) || (rc = sync_grow(c, c->d_rboxes, (size_t)chunk * 32)))) return rc;
    // the rows of a chunk go up in one block, as rope_eval_views sends its own: joint vectors | view matrices | view index | the table
    const size_t off_pv = 6 * (size_t)chunk * sizeof(double), off_vo = off_pv + (PV ? 16 * (size_t)chunk * sizeof(double) : 0),
                 end_vo = off_vo + (PV ? (size_t)chunk * sizeof(int32_t) : 0), off_lut = (end_vo + 15) & ~(size_t)15,
                 bytes = ask.lut ? off_lut + 256 : end_vo;
    rc = sync_grow(c, c->h_vstage, bytes, c->d_vstage, bytes);
    if (rc) return rc;
    // the per-candidate buffers hold render rows from here on (rope_eval_views does the same)
    c->cand_valid = c->results_valid = false;
    c->cand_dev = nullptr;
    c->mvp_valid = false;
    for (int lo = 0; lo < N; lo += chunk) {
        const int n = std::min(chunk, N - lo);
        HIP_TRY(c, hipStreamSynchronize(c->stream));         // the block may still feed the previous chunk's copy
        std::memcpy(c->h_vstage, q + 6 * (size_t)lo, 6 * (size_t)n * sizeof(double));
        if (PV) {
            std::memcpy(c->h_vstage + off_pv, PV + 16 * (size_t)lo, 16 * (size_t)n * sizeof(double));
            int32_t *vo = reinterpret_cast<int32_t *>(c->h_vstage + off_vo);
            for (int i = 0; i < n; i++) vo[i] = i;
        }
        if (ask.lut) std::memcpy(c->h_vstage + off_lut, ask.lut, 256);
        HIP_TRY(c, hipMemcpyAsync(c->d_vstage, c->h_vstage, bytes, hipMemcpyHostToDevice, c->stream));
        c->dv_cand = reinterpret_cast<const double *>(c->d_vstage.get());
        c->dv_PV = PV ? reinterpret_cast<const double *>(c->d_vstage + off_pv) : c->d_PV.get();
        c->dv_view_of = PV ? reinterpret_cast<const int32_t *>(c->d_vstage + off_vo) : nullptr;
        c->C = n;
        c->n_layers = n;                                      // nothing shared: every row draws all its links
        rc = enqueue_geometry(c, plan_geometry(pass_inputs(c, n_render, ROPE_LOSS_DEPTH, fp, EVAL_SINGLE, false, clip), false), n_render, fp, true);
        if (rc) return rc;
        if (ask.depth) HIP_TRY(c, hipMemsetAsync(c->d_rdepth, 0, (size_t)n * px * sizeof(float), c->stream));
        if (ask.ids) HIP_TRY(c, hipMemsetAsync(c->d_rids, 0xFF, (size_t)n * px, c->stream));
        if (ask.labels) HIP_TRY(c, hipMemsetAsync(c->d_rboxes, 0xFF, (size_t)n * 32 * sizeof(int32_t), c->stream));
        RasterArgs a = base_args(c, n_render);
        a.depth_out = ask.depth ? c->d_rdepth.get() : nullptr;
        a.ids_out = ask.ids ? c->d_rids.get() : nullptr;
        HIP_TRY(c, launch_raster(MODE_DUMP, ROPE_LOSS_DEPTH, n, c->stream, fp, c->rp, a, clip));
        rc = after(lo, n, px, ask.lut ? c->d_vstage + off_lut : nullptr);
        if (rc) return rc;
    }
    c->C = 0;
    c->last_n_render = n_render;
    return ROPE_OK;
}

// rope_render_batch and rope_render_batch_device: `to_device` says where depth and ids point, and so how a chunk's planes leave
static int render_batch(rope_ctx *c, const double *q, const double *PV, int N, int n_render, const int32_t *crop, float *depth, uint8_t *ids,
                        bool to_device)
{
    const RenderAsk ask{to_device ? "rope_render_batch_device" : "rope_render_batch", crop, depth != nullptr, ids != nullptr, false, nullptr};
    if (!q) ARG_FAIL(c, std::string(ask.entry) + ": null joint vectors");
    const int rc = render_chunks(c, ask, q, PV, N, n_render, [] { return (const char *)nullptr; }, [&](int lo, int n, size_t px, const uint8_t *) -> int {
        if (to_device) {                                      // in stream order: the next chunk's clearing comes after these copies
            if (depth) HIP_TRY(c, hipMemcpyAsync(depth + (size_t)lo * px, c->d_rdepth, (size_t)n * px * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            if (ids) HIP_TRY(c, hipMemcpyAsync(ids + (size_t)lo * px, c->d_rids, (size_t)n * px, hipMemcpyDeviceToDevice, c->stream));
            return ROPE_OK;
        }
        int rc = ROPE_OK;
        if (depth) rc = copy_d2h_out(c, depth + (size_t)lo * px, c->d_rdepth, (size_t)n * px * sizeof(float));
        if (!rc && ids) rc = copy_d2h_out(c, ids + (size_t)lo * px, c->d_rids, (size_t)n * px);
        return rc;
    });
    if (!rc && to_device) HIP_TRY(c, hipStreamSynchronize(c->stream));      // the planes are the caller's, on any stream, when the call returns
    return rc;
}

extern "C" int rope_render_batch(rope_ctx *c, const double *q, const double *PV, int N, int n_render, const int32_t *crop,
                                 float *depth, uint8_t *ids)
{
    if (!c) return ROPE_E_ARG;
    return render_batch(c, q, PV, N, n_render, crop, depth, ids, false);
}

// The whole frame of N poses into the CALLER's device memory: rope_render_batch with another destination for the copy-out
extern "C" int rope_render_batch_device(rope_ctx *c, const double *q, const double *PV, int N, int n_render, float *depth_dev, uint8_t *ids_dev)
{
    if (!c) return ROPE_E_ARG;
    return render_batch(c, q, PV, N, n_render, nullptr, depth_dev, ids_dev, true);
}

// rope_render_batch's chunks, each drawn into id planes only and then turned into label planes on the device (rope_masks.hip):
// the host gets one byte per pixel with the labels' dilation done, and each label's box
extern "C" int rope_render_masks(rope_ctx *c, const double *q, const double *PV, int N, int n_render,
                                 const uint8_t *label_of_link, int pad, uint8_t *masks, int32_t *boxes)
{
    if (!c) return ROPE_E_ARG;
    if (!q || !label_of_link || !masks) ARG_FAIL(c, "rope_render_masks: null pointer");
    uint8_t lut[256] = {};                                      // link id -> label bits; background (255) and the rest -> none
    auto own_checks = [&]() -> const char * {
        if (pad < 1 || pad > ROPE_MASK_MAX_PAD) return "rope_render_masks: pad must be 1..64";
        for (int l = 0; l < n_render; l++) {
            if (label_of_link[l] == 255) continue;
            if (label_of_link[l] > 7) return "rope_render_masks: label bit must be 0..7 or 255";
            lut[l] = (uint8_t)(1u << label_of_link[l]);
        }
        return nullptr;
    };
    const RenderAsk ask{"rope_render_masks", nullptr, false, true, true, lut};
    return render_chunks(c, ask, q, PV, N, n_render, own_checks, [&](int lo, int n, size_t px, const uint8_t *lut_dev) -> int {
        HIP_TRY(c, launch_masks(c->stream, c->d_rids, n, c->fp.H, c->fp.W, lut_dev, pad, c->d_rmask, c->d_rboxes));
        int rc = copy_d2h_out(c, masks + (size_t)lo * px, c->d_rmask, (size_t)n * px);
        if (!rc && boxes) rc = copy_d2h_out(c, boxes + (size_t)lo * 32, c->d_rboxes, (size_t)n * 32 * sizeof(int32_t));
        return rc;
    });
}

extern "C" int rope_render(rope_ctx *c, const double *q, int n_render, float *depth, uint8_t *ids)
{
    if (!c) return ROPE_E_ARG;
    if (!q || !depth || !ids) ARG_FAIL(c, "rope_render: null pointer");
    if (!c->have_camera) ARG_FAIL(c, "rope_render: camera not set");
    return rope_render_batch(c, q, nullptr, 1, n_render, nullptr, depth, ids);
}

extern "C" int rope_coverage(rope_ctx *c, const double *cand, int C, int n_render, uint8_t *cover)
{
    if (!c) return ROPE_E_ARG;
    if (!cand || !cover) ARG_FAIL(c, "rope_coverage: null pointer");
    if (!c->have_camera) ARG_FAIL(c, "rope_coverage: camera not set");
    HIP_TRY(c, hipSetDevice(c->device));
    size_t n = (size_t)c->fp.W * c->fp.H;
    HIP_TRY(c, hipMemsetAsync(c->d_cover, 0, n, c->stream));
    int rc = raster_only(c, cand, C, n_render, MODE_COVER);
    if (rc) return rc;
    return copy_d2h_staged(c, cover, c->d_cover, n);
}

extern "C" int rope_lookup_build(rope_ctx *c, const double *cand, int C, int n_render, const int32_t *crop)
{
    if (!c) return ROPE_E_ARG;
    if (!cand || !crop) ARG_FAIL(c, "rope_lookup_build: null pointer");
    if (C < 1) ARG_FAIL(c, "rope_lookup_build: empty grid");
    if (!c->have_robot || !c->have_camera) ARG_FAIL(c, "rope_lookup_build: robot and camera must be set first");
    if (n_render < 1 || n_render > c->n_links) ARG_FAIL(c, "rope_lookup_build: n_render out of range");
    FrameParams fp = c->fp;
    double n_pix;
    if (int rc = apply_crop(c, "rope_lookup_build", crop, fp, n_pix)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->table_C = 0;
    const size_t px = (size_t)n_pix, need = px * (size_t)C;
    if (int rc = sync_grow(c, c->d_table, need)) return rc;
    if (int rc = sync_grow(c, c->d_tsums, (size_t)C * ROPE_SUM_WORDS, c->d_terr, (size_t)C + 2)) return rc;
    if (!c->d_zero_total) {
        HIP_TRY(c, c->d_zero_total.grow(ROPE_SUM_WORDS));
        HIP_TRY(c, hipMemsetAsync(c->d_zero_total, 0, ROPE_SUM_WORDS * sizeof(uint64_t), c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(c->d_table, 0, need * sizeof(float), c->stream));
    // the reference allows 200 divisions per joint (lookup.py:50, constants.py:30): more rows than one batch holds, so the
    // grid is rendered batch after batch into its rows of the table
    for (int lo = 0; lo < C; lo += MAX_ROWS) {
        const int n = std::min(MAX_ROWS, C - lo);
        int rc = rope_candidates_upload(c, cand + 6 * (size_t)lo, n);
        if (rc) return rc;
        // (a table is built once: shared layers whenever the rows share, whatever the strategy says about scoring passes)
        const PassPlan plan = plan_geometry(pass_inputs(c, n_render, ROPE_LOSS_LOOKUP, fp, EVAL_SINGLE, false, use_clip(c)), layers_wanted(c->n_layers, c->C));
        const bool layers = plan.layers;
        const int n_shared = plan.n_shared;
        if (layers) { rc = ensure_layers(c); if (rc) return rc; }
        rc = enqueue_geometry(c, plan, n_render, fp, false);
        if (rc) return rc;
        RasterArgs a = base_args(c, n_render);
        if (layers) {
            // layer pass without loss sums (layer_sums == nullptr): no target is needed to build a table
            rc = enqueue_layers(c, plan, a, ROPE_LOSS_DEPTH, c->fp);
            if (rc) return rc;
            a.l_begin = n_shared; a.layer_of = c->d_layer_of; a.layer_rep = c->d_layer_rep; a.layers = c->d_layers;
        }
        a.table = c->d_table + (size_t)lo * px;
        HIP_TRY(c, launch_raster(MODE_TABLE, ROPE_LOSS_LOOKUP, c->C, c->stream, fp, c->rp, a, plan.clip));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    // keep of every row only the groups of samples that hold something (the crop is the box of all poses together, and a pose
    // fills a fraction of its own box), then let the dense rows go: this is what the per-frame pass reads
    HIP_TRY(c, c->d_tcount.grow((size_t)C));
    HIP_TRY(c, c->d_toff.grow((size_t)C));
    HIP_TRY(c, c->d_tused.grow(1));
    HIP_TRY(c, c->d_ttotal.grow(ROPE_SUM_WORDS));
    const int cw = crop[3] - crop[2] + 1, ch = crop[1] - crop[0] + 1;
    unsigned long long used = 0;
    hipError_t e = hipMemsetAsync(c->d_tused, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = launch_table_count(c->stream, cw, ch, c->d_table, C, c->d_tcount, c->d_toff, c->d_tused);
    if (e == hipSuccess) e = hipMemcpyAsync(&used, c->d_tused, sizeof(used), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    c->d_tgoff.release();
    c->d_tgval.release();
    if (e == hipSuccess) e = static_cast<hipError_t>(c->d_tgoff.reset(std::max<size_t>(used, 1)));
    if (e == hipSuccess) e = static_cast<hipError_t>(c->d_tgval.reset(std::max<size_t>(used, 1)));
    if (e == hipSuccess) e = launch_table_fill(c->stream, cw, ch, c->d_table, C, c->d_toff, c->d_tgoff, c->d_tgval);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    c->d_table.release();
    HIP_TRY(c, e);
    c->table_groups = used;
    c->table_C = C;
    std::memcpy(c->table_crop, crop, 4 * sizeof(int32_t));
    return ROPE_OK;
}

extern "C" int rope_lookup_score(rope_ctx *c, double *scores_out, int32_t *best_idx, double *best_score)
{
    if (!c) return ROPE_E_ARG;
    if (c->table_C < 1) ARG_FAIL(c, "rope_lookup_score: no table built");
    if (c->single.n < 1 || !c->single.has_t32) ARG_FAIL(c, "rope_lookup_score: needs a target with the float32 plane");
    HIP_TRY(c, hipSetDevice(c->device));
    const FrameParams fp = table_frame(c);
    const double n_pix = (double)(fp.r1 - fp.r0 + 1) * (double)(fp.c1 - fp.c0 + 1);
    const size_t words = table_crop_words(fp);
    if (int rc = sync_grow(c, c->d_tc, words)) return rc;
    HIP_TRY(c, launch_table_score(c->stream, fp, c->d_tcount, c->d_toff, c->d_tgoff, c->d_tgval, c->table_C, c->single.t32, c->d_tc,
                                  c->d_ttotal, c->d_tsums));
    HIP_TRY(c, launch_finalize(c->stream, c->d_tsums, c->d_zero_total, c->table_C, ROPE_LOSS_LOOKUP, ROPE_MAX_LINKS, n_pix, c->lf, c->d_terr));
    if (scores_out) HIP_TRY(c, hipMemcpyAsync(scores_out, c->d_terr, (size_t)c->table_C * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    double tail[2];
    HIP_TRY(c, hipMemcpyAsync(tail, c->d_terr + c->table_C, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (best_score) *best_score = tail[0];
    if (best_idx) *best_idx = (int32_t)tail[1];
    return ROPE_OK;
}


// Depth holes in place on N float32 planes that are in HBM (rope_synth.hip), on the caller's stream; no context, the current device.
extern "C" int rope_depth_holes(float *depth_dev, int N, int H, int W, uint32_t frame0, uint64_t seed, const uint32_t *T, const int32_t *d,
                                int n_d, int connection, void *stream)
{
    if (!depth_dev || N < 1 || N > 65535 || H < 1 || W < 1 || n_d < 0 || n_d > ROPE_HOLE_MAX_DILATIONS || (n_d > 0 && (!T || !d)) ||
        connection < 1 || connection > ROPE_HOLE_MAX_WINDOW || (uint64_t)H * (uint64_t)W > 0xFFFFFFFFull || (H + 63) / 64 > 65535)
        return ROPE_E_ARG;
    for (int j = 0; j < n_d; j++)
        if (d[j] < 1 || d[j] > ROPE_HOLE_MAX_WINDOW) return ROPE_E_ARG;
    if (launch_depth_holes(static_cast<hipStream_t>(stream), depth_dev, N, H, W, frame0, seed, T, d, n_d, connection) != hipSuccess) {
        (void)hipGetLastError();
        return ROPE_E_HIP;
    }
    return ROPE_OK;
}


extern "C" int rope_debug_mvp(rope_ctx *c, float *mvp_out, int C, int n_render)
{
    if (!c) return ROPE_E_ARG;
    if (!mvp_out || C < 1 || C > c->C || n_render < 1 || n_render > ROPE_MAX_LINKS) ARG_FAIL(c, "rope_debug_mvp: bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->mvp_valid) {
        // the last pass worked the matrices out inside its raster workgroups: form them the way any other pass does
        if (!c->cand_valid) ARG_FAIL(c, "rope_debug_mvp: no resident candidates");
        const int rc = enqueue_geometry(c, plan_geometry(pass_inputs(c, n_render, ROPE_LOSS_DEPTH, c->fp, EVAL_SINGLE, false, use_clip(c)), false), n_render, c->fp, false);
        if (rc) return rc;
        c->results_valid = false;                     // that launch cleared the sums
        c->mvp_valid = true;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < C; i++)
        HIP_TRY(c, hipMemcpy(mvp_out + (size_t)i * n_render * 16, c->d_mvp + (size_t)i * ROPE_MAX_LINKS * 16,
                             (size_t)n_render * 16 * sizeof(float), hipMemcpyDeviceToHost));
    return ROPE_OK;
}

extern "C" int rope_set_strategy(rope_ctx *c, int flags)
{
    if (!c) return ROPE_E_ARG;
    if (flags & ~(STRATEGY_NO_LAYERS | STRATEGY_NO_SPLIT | STRATEGY_NO_PARENTS | STRATEGY_NO_QUEUE | STRATEGY_CLIP_KERNELS | STRATEGY_SEPARATE_GEOMETRY |
                  STRATEGY_NO_GEOMETRY_CACHE | STRATEGY_NO_KEPT_FRAGMENTS)) ARG_FAIL(c, "rope_set_strategy: unknown flag");
    c->drop_kept();
    c->strategy = flags;
    return ROPE_OK;
}

extern "C" int rope_geometry_cache_stats(rope_ctx *c, uint64_t *hits, uint64_t *misses)
{
    if (!c) return ROPE_E_ARG;
    if (hits) *hits = c->geo.hits;
    if (misses) *misses = c->geo.misses;
    return ROPE_OK;
}

extern "C" int rope_fragment_store_stats(rope_ctx *c, uint64_t *builds, uint64_t *passes_served, uint64_t *bytes, uint64_t *groups)
{
    if (!c) return ROPE_E_ARG;
    if (builds) *builds = c->frags.builds;
    if (passes_served) *passes_served = c->frags.passes_served;
    if (bytes) *bytes = c->frags.bytes;
    if (groups) *groups = c->frags.groups;
    return ROPE_OK;
}

extern "C" int rope_fragment_store_pairs(rope_ctx *c, uint64_t *pairs)
{
    if (!c || !pairs) return ROPE_E_ARG;
    *pairs = c->frags.pairs;
    return ROPE_OK;
}

extern "C" int rope_set_fragment_budget(rope_ctx *c, uint64_t bytes)
{
    if (!c) return ROPE_E_ARG;
    c->frags.drop();                                // what is held was admitted under the old budget, and a refusal was one of it too
    c->frags.budget = bytes;
    return ROPE_OK;
}

#ifdef ROPE_PROFILE
namespace rope { hipError_t read_clock_stamps(unsigned long long *out); hipError_t read_bounds_violations(unsigned int *out); }

// Profiling build: how many indices into the raster kernels' shared arrays / queue segments were out of range since the library
// was loaded (ROPE_CHECK_INDEX in rope_kernels.hip: the raster code, which is why it and its counter stay in that one file)
extern "C" int rope_debug_bounds(rope_ctx *c, int *violations)
{
    if (!c || !violations) return ROPE_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned int v = 0;
    HIP_TRY(c, read_bounds_violations(&v));
    *violations = (int)v;
    return ROPE_OK;
}

// Profiling build: the shader clock (GHz) during the last scoring launch of a large batch — median over its workgroups of
// delta s_memtime / delta s_memrealtime (100 MHz); ghz[1] = the launch's length by the same stamps in ms (first start to last end)
extern "C" int rope_debug_clock(rope_ctx *c, double *ghz)
{
    if (!c || !ghz) return ROPE_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> st(4 * 1024);
    HIP_TRY(c, read_clock_stamps(st.data()));
    std::vector<double> f;
    unsigned long long r_lo = ~0ull, r_hi = 0;
    const int n = std::min(1024, 2 * c->n_cu);
    for (int i = 0; i < n; i++) {
        const unsigned long long t0 = st[4 * i], r0 = st[4 * i + 1], t1 = st[4 * i + 2], r1 = st[4 * i + 3];
        if (r1 > r0 + 100 && t1 > t0) f.push_back((double)(t1 - t0) / ((double)(r1 - r0) * 10.0));       // workgroups that ran for more than a microsecond
        if (r1 > r0) { r_lo = std::min(r_lo, r0); r_hi = std::max(r_hi, r1); }
    }
    if (f.empty()) ARG_FAIL(c, "rope_debug_clock: no stamps (run a batch of more than 256 rows first)");
    std::sort(f.begin(), f.end());
    ghz[0] = f[f.size() / 2];
    ghz[1] = (double)(r_hi - r_lo) * 1.0e-5;
    return ROPE_OK;
}

extern "C" int rope_debug_skip(rope_ctx *c, int mask)
{
    if (!c) return ROPE_E_ARG;
    c->fp.debug = mask;
    return ROPE_OK;
}
#endif

extern "C" int rope_profile_eval(rope_ctx *c, int n_render, int loss, const int32_t *crop, int reps, float *ms)
{
    if (!c) return ROPE_E_ARG;
    if (!ms || reps < 1) ARG_FAIL(c, "rope_profile_eval: bad arguments");
    FrameParams fp; double n_pix;
    int rc = check_eval_args(c, n_render, loss, crop, fp, n_pix);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = ensure_totals(c, c->single, c->single_empty, loss, fp);
    if (rc) return rc;
    std::vector<hipEvent_t> ev(5 * (size_t)reps);
    for (auto &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int r = 0; r < reps; r++) {
        rc = enqueue_eval(c, n_render, loss, fp, n_pix, single_planes(c, loss), EVAL_SINGLE, &ev[5 * (size_t)r]);
        if (rc) break;
    }
    if (!rc) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        double acc[4] = {0, 0, 0, 0};
        for (int r = 0; r < reps; r++) {
            float t;
            for (int k = 0; k < 4; k++) {
                HIP_TRY(c, hipEventElapsedTime(&t, ev[5 * (size_t)r + k], ev[5 * (size_t)r + k + 1]));
                acc[k] += t;
            }
        }
        float total;
        HIP_TRY(c, hipEventElapsedTime(&total, ev[0], ev[5 * (size_t)reps - 1]));
        for (int k = 0; k < 4; k++) ms[k] = (float)(acc[k] / reps);
        ms[4] = total / (float)reps;
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    return rc;
}
