/*
 * rope_s3d.h — C ABI of the MI355X render-and-compare pose engine (librope_hip.so).
 *
 * The reference (OSU-AIMS/RoPE-S3D) is pure Python; the calls it makes on this path
 * go to pyrender/OpenGL, Klampt, TensorFlow and numpy.  Each entry point below names
 * the reference call site(s) it stands in for.  Conventions: plain pointers and
 * sizes, caller-owned host buffers, return 0 on success or a negative ROPE_E_* code
 * (text via rope_last_error), no exceptions cross the boundary, one context per
 * GPU, a context is not thread-safe (the reference's Predictor is not re-entrant
 * either: one GL context and mutable target state, predict.py:127-148).
 */
#ifndef ROPE_S3D_H
#define ROPE_S3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rope_ctx rope_ctx;

enum {
    ROPE_OK = 0,
    ROPE_E_ARG = -1,      /* bad argument / wrong call order */
    ROPE_E_HIP = -2,      /* a HIP runtime call failed */
    ROPE_E_NOMEM = -3
};

/* Loss kinds (what is reduced over the pixels of one candidate render). */
enum {
    ROPE_LOSS_DEPTH = 0,  /* last term of Predictor._error only: mean(D[D!=0])*std(D)   predict.py:503-507 */
    ROPE_LOSS_FULL = 1,   /* whole Predictor._error                                      predict.py:475-509 */
    ROPE_LOSS_LOOKUP = 2, /* Lookup stage score mean|T-sqrt(D)|*std over the crop        predict.py:165-171 */
    ROPE_LOSS_TSWEEP = 3, /* TensorSweep score  mean|sqrt(T)-sqrt(D)| * -std, full frame predict.py:363-369 */
    ROPE_LOSS_CAMFULL = 4 /* CameraPredictor._error sums (rope_eval_views only)  camera_pose_prediction.py:933-970 */
};

#define ROPE_MAX_LINKS 6          /* link_6_t is never rendered: render_utils.py:31-32 */
#define ROPE_SUM_WORDS 23         /* uint64 words of integer sums per candidate */

/* Lifetime.  `device` is the HIP device ordinal. */
int rope_create(rope_ctx **out, int device);
void rope_destroy(rope_ctx *ctx);
const char *rope_last_error(rope_ctx *ctx);

/* Identity of the sources this library was built from (first 16 hex digits of their SHA-256, rope_s3d_amd/build.py:source_hash):
 * committed profiles carry the same string, so a benchmark can tell whether their counters belong to the build it is timing. */
const char *rope_build_id(void);

/* Robot geometry + kinematic chain, uploaded once.
 * Replaces MeshLoader.load + pyrender.Mesh.from_trimesh (render_utils.py:22-41) and
 * klampt.WorldModel(urdf) (kinematics.py:23-33).
 *   ml_header   n_meshlets x 8 uint32: centre xyz + radius (float bits), first vertex,
 *               first triangle, n_verts | n_tris<<16, link id
 *   ml_verts    n_ml_verts x 3 float32 (meshlet-local copies of link-frame vertices)
 *   ml_tris     n_ml_tris uint32, three 8-bit local indices each
 *   link_first  n_links+1 meshlet offsets
 *   joint_fixed 6 x 12 doubles, row-major 3x4 parent-link -> joint frame (<origin>)
 *   joint_axes  6 x 3 doubles, unit rotation axes (<axis>) */
int rope_set_robot(rope_ctx *ctx, const uint32_t *ml_header, int n_meshlets, const float *ml_verts,
                   int n_ml_verts, const uint32_t *ml_tris, int n_ml_tris, const int32_t *link_first,
                   int n_links, const double *joint_fixed, const double *joint_axes);

/* The same from plain meshes: partitions every link into meshlets on the host (rope_partition_mesh), builds the
 * arrays above and calls rope_set_robot — everything MeshLoader.load + from_trimesh leave to pyrender
 * (render_utils.py:22-41), for hosts that are not Python.
 *   verts    V x 3 float32, welded link meshes concatenated (link frame, metres)
 *   faces    T x 3 int32, vertex indices LOCAL to the triangle's link
 *   vtx_off / tri_off   n_links+1 offsets of every link into verts / faces */
int rope_set_robot_mesh(rope_ctx *ctx, const float *verts, const int32_t *faces, const int32_t *vtx_off, const int32_t *tri_off,
                        int n_links, const double *joint_fixed, const double *joint_axes);

/* One mesh -> surface patches of <= max_tris (<= 128) triangles over <= max_verts (<= 64) vertices.  Host only: no
 * context, no GPU.  tri_order receives the n_tris triangle ids grouped by patch, meshlet_first (n_tris+1 entries
 * available) the offsets of the patches into it; returns the number of patches or ROPE_E_ARG.  Any partition renders
 * the same image; this one keeps patches compact on the surface (small screen boxes). */
int rope_partition_mesh(const float *verts, int n_verts, const int32_t *faces, int n_tris, int max_tris, int max_verts,
                        int32_t *tri_order, int32_t *meshlet_first);

/* Host only (no context): camera pose + pinhole intrinsics -> the matrix P·V rope_set_camera takes (16 doubles, row-major).
 * Replaces Renderer.setCameraPose's pose convention (render.py:107-111: roll = a4 + pi/2, pitch = a3, yaw = a5; makePose /
 * angToPoseArr, render_utils.py:56-108: R = Rz(yaw)·Ry(pitch)·Rx(roll), camera looking along -Z with +Y up, V = pose^-1) and
 * Intrinsics.pyrender_camera (projection.py:161-169: pyrender 0.1.45's IntrinsicsCamera projection).
 *   pose  [x, y, z, a3, a4, a5]: position in metres, the three angles in radians, as the reference's camera_pose arrays */
int rope_camera_matrix(const double *pose, double fx, double fy, double cx, double cy, int W, int H, double znear, double zfar, double *PV);

/* Host only (no context): the Lookup stage's pose grid (RobotLookupCreator / RobotLookupManager, lookup.py:39-66): divisions[j] >= 1
 * samples of joint j between its limits (6 x 2 doubles), np.linspace's values, joint 0 varying fastest; divisions[j] <= 0: joint j
 * is not part of the grid (angle 0).  Returns the number of rows; writes rows x 6 doubles to `out` when it is not NULL and
 * `capacity` rows fit (else ROPE_E_ARG). */
int64_t rope_lookup_grid(const double *limits, const int32_t *divisions, double *out, int64_t capacity);

/* Host only (no context): the divisions (rope_lookup_grid's convention) of the pose grid Crop renders to find the image bounds of the
 * first num_links links (2..6) of the robot at an image of n_pixels pixels (robotpose/crop.py:114-146; constants.py:19-23).  With
 * rope_lookup_grid and rope_coverage this replaces Crop._create (crop.py:50-96): bounds = box of the covered pixels, padded by 10. */
int rope_crop_divisions(int64_t n_pixels, int num_links, int32_t *divisions);

/* Camera: PV = P·V (4x4 row-major doubles), image size and clip planes.
 * Replaces Renderer.setCameraPose (render.py:107-111) + Intrinsics.pyrender_camera
 * (projection.py:161-169) + pyrender.OffscreenRenderer(W,H) (render.py:60). */
int rope_set_camera(rope_ctx *ctx, const double *PV, int W, int H, double znear, double zfar);

/* Target of the current frame.
 * Replaces the cached state of Predictor._load_target/_loadSynthetic (predict.py:397-413,445-469).
 *   tq         H x W uint64: bits 0..38 target depth in Q32 metres, bits 40..47 link mask bits
 *   t32        H x W float32 plane for ROPE_LOSS_LOOKUP (lookup target) / ROPE_LOSS_TSWEEP
 *              (full target); may be NULL when those losses are not used
 *   link_flags 8 bytes: bit0 link present in the target, bit1 ">5 % of mask has depth" (predict.py:495) */
int rope_set_target(rope_ctx *ctx, const uint64_t *tq, const float *t32, const uint8_t *link_flags);

/* The float32 plane ROPE_LOSS_TSWEEP reads, when it is not the lookup plane: TensorSweep compares against the WHOLE target depth
 * (predict.py:358-363, `self._tgt_depth`), the Lookup stage against the depth under the lookup links (predict.py:165-169).  Call after
 * rope_set_target (which forgets it); NULL goes back to the one plane. */
int rope_set_target_tsweep(rope_ctx *ctx, const float *t32_full);

/* Host only (no context): the packing rope_set_target expects.  depth n float64 metres (NaN, inf and values <= 0 count
 * as "no depth"), mask_bits n bytes (bit l = link l's mask) or NULL -> out n uint64: Q32 depth, round half even,
 * clipped to 2^39-1, mask bits at 40..47. */
int rope_pack_target(const double *depth, const uint8_t *mask_bits, int64_t n, uint64_t *out);

/* Host only (no context): cv2.resize(img, (W/f, H/f)) with INTER_LINEAR for an even integer factor f — the frame
 * down-sampling of Predictor._downsample (predict.py:378-381); four taps per output sample, OpenCV's fixed-point
 * rounding for uint8.  kind 0 uint8, 1 float32, 2 float64; `channels` interleaved; rows `row_stride` bytes apart;
 * dst is dense (H/f x W/f x channels). */
int rope_downsample_even(const void *src, int H, int W, int channels, int64_t row_stride, int f, int kind, void *dst);

/* Host only (no context): one frame of the synthetic path, camera arrays in, target planes out, in one pass: the down-sampling
 * of Predictor._downsample (predict.py:378-381, as rope_downsample_even), the link masks read off channel 0 of the colour render
 * and the lookup depth of _loadSynthetic (predict.py:445-469), the per-link flags and the packing of _load_target (predict.py:397-413).
 *   color  H0 x W0 x 3 uint8 (BGR, only channel 0 is read), rows color_stride bytes apart
 *   depth  H0 x W0 float32 (depth_kind 1) or float64 (2) metres, rows depth_stride bytes apart
 *   f      down-sampling factor: 1 or even;  link_blue: n_links channel-0 values (DEFAULT_RENDER_COLORS, constants.py:65-91), the first
 *          n_lookup_links of them the links of the lookup depth
 *   out    tq, lookup_f32 (H0/f x W0/f), flags (8 bytes) as rope_set_target takes them; tgt_depth float64 or NULL */
int rope_prepare_synthetic(const uint8_t *color, int64_t color_stride, const void *depth, int depth_kind, int64_t depth_stride, int H0, int W0,
                           int f, const int32_t *link_blue, int n_links, int n_lookup_links, uint64_t *tq, float *lookup_f32, double *tgt_depth,
                           uint8_t *flags);

/* Page-locked host memory for the planes handed to rope_set_target / rope_set_targets / rope_set_frames: copies out of it go to the
 * device in one transfer at the link's rate, instead of chunk by chunk through the library's own staging block (what pageable
 * memory needs).  Optional — any host pointer is accepted everywhere.  NULL when the allocation fails. */
void *rope_host_alloc(size_t bytes);
void rope_host_free(void *p);

/* Host only (no context): one frame of the SEGMENTATION path, segmenter output in, target planes out: the merge of a class's
 * instances (_reorganize_by_link, predict.py:383-395), the body mask erode7(dilate8(sum of the masks)) applied to the depth — over
 * all detected classes for the target, over the lookup links for the lookup depth (predict.py:419-438; cv2's box kernels with their
 * default anchors) — the depth's down-sampling (predict.py:378-381), the flags and the packing of _load_target (predict.py:397-413).
 *   depth    H0 x W0 float32 (kind 1) / float64 (kind 2), rows depth_stride bytes apart;  f: 1 or even
 *   masks    (H0/f) x (W0/f) x K bytes, non-zero = inside instance k (the segmenter's `masks`);  link_of: K link indices
 *            (class id - 1), -1 for an instance that is none of the rendered links (it still widens the body mask)
 *   out      tq, lookup_f32, flags as rope_set_target takes them; tgt_depth float64 (the masked depth) or NULL */
int rope_prepare_segmented(const void *depth, int depth_kind, int64_t depth_stride, int H0, int W0, int f, const uint8_t *masks, int K,
                           const int32_t *link_of, int n_links, int n_lookup_links, uint64_t *tq, float *lookup_f32, double *tgt_depth,
                           uint8_t *flags);

/* Candidate joint vectors (C x 6 doubles) into HBM; they stay resident until replaced.
 * The context keeps a host copy of the rows it was last given: an upload of the same C rows, bit for bit, while they are still
 * resident copies, sorts and uploads nothing, and whatever rope_eval_resident kept of the last pass (below) stays good.  This is
 * what a fixed grid scored through rope_eval against frame after frame comes to. */
int rope_candidates_upload(rope_ctx *ctx, const double *cand, int C);

/* FK + raster of the first n_render links + loss reduction + argmin for the resident
 * candidates, enqueued on the context's stream (no host sync).
 * Replaces, per candidate, render_at_pos + _error (predict.py:159-161,475-509) and, for the
 * lookup loss, the TF reduction over the pre-rendered table (predict.py:167-171).
 *   crop   r0,r1,c0,c1 inclusive image rows/cols; required for ROPE_LOSS_LOOKUP, else NULL
 * Kept from pass to pass: a batch of more than 256 rows that shares upstream layers leaves its link matrices, screen boxes, tile
 * masks, queue weights and layer key tiles in the context — none depends on the target — and the next such pass with the same
 * candidates, camera, robot, n_render, crop and strategy runs without the forward-kinematics, box and shared-layer launches: it
 * only takes the layers' loss sums against the current target again (any loss; rope_set_target between the passes is the
 * point).  Results are the same bits.  Dropped by: an upload of other rows, rope_set_camera (same values included),
 * rope_set_robot[_mesh], rope_set_strategy, another n_render or crop, and every other entry that uses the per-candidate
 * buffers (small batches, rope_eval_targets, rope_eval_views, the render entries, rope_coverage, rope_lookup_build,
 * rope_debug_mvp).  ROPE_STRATEGY_NO_GEOMETRY_CACHE turns it off; rope_geometry_cache_stats counts.
 * Kept fragments: the first pass that runs on kept geometry also stores, per row, the 4-sample groups in which the row's own links
 * (3 .. n_render - 1) beat its shared layer, with their finished keys and the layer's — a function of the same geometry, of neither
 * loss nor target — and every later pass of that grid scores by streaming them against the target instead of drawing the own links
 * again.  The same bits again.  The store goes wherever the kept geometry goes, is built only if it fits rope_set_fragment_budget,
 * and only for passes that go through the queues; ROPE_STRATEGY_NO_KEPT_FRAGMENTS turns it off; rope_fragment_store_stats counts.
 * The pass that builds waits for the stream (it sizes the store on the host); no other pass does. */
int rope_eval_resident(rope_ctx *ctx, int n_render, int loss, const int32_t *crop);

int rope_sync(rope_ctx *ctx);

/* Results of the last rope_eval_resident.  Any pointer may be NULL.
 *   err_out  C doubles; sums_out C x ROPE_SUM_WORDS uint64; best_idx/best_err = first argmin */
int rope_results_download(rope_ctx *ctx, double *err_out, uint64_t *sums_out, int32_t *best_idx, double *best_err);

/* upload + eval + sync + download in one call (host buffers in, host buffers out). */
int rope_eval(rope_ctx *ctx, const double *cand, int C, int n_render, int loss, const int32_t *crop,
              double *err_out, uint64_t *sums_out, int32_t *best_idx, double *best_err);

/* Stored lookup table.  rope_lookup_build renders the pose grid once (first n_render links) and keeps the
 * cropped sqrt-depth images in HBM (C x crop_h x crop_w float32); rope_lookup_score streams the table against
 * the current target's float32 plane and returns the lookup score of every row and the first argmin.
 * Replaces RobotLookupCreator.run / RobotLookupManager.get (lookup.py:69-106,184-283), tf.pow(depth, 0.5)
 * (predict.py:117) and the TF reduction + argmin per frame (predict.py:167-171).  Scores are bit-identical to
 * rope_eval with ROPE_LOSS_LOOKUP on the same grid and crop. */
int rope_lookup_build(rope_ctx *ctx, const double *cand, int C, int n_render, const int32_t *crop);
int rope_lookup_score(rope_ctx *ctx, double *scores_out, int32_t *best_idx, double *best_score);

/* One pose to images.  Replaces Renderer.setJointAngles + Renderer.render (render.py:88-98).
 *   depth H x W float32 metres (0 = empty), ids H x W uint8 link id (255 = background)
 * rope_render_batch with N = 1, PV = NULL and crop = NULL. */
int rope_render(rope_ctx *ctx, const double *q, int n_render, float *depth, uint8_t *ids);

/* N poses to images in one device batch.  Replaces N x (Renderer.setJointAngles [+ setCameraPose] + render)
 * (render.py:88-111) and the render loops of DatasetRenderer.render_at / RobotLookupCreator._generate_depth_array
 * (render.py:175-183, lookup.py:69-86).
 *   q      N x 6 joint vectors
 *   PV     N x 16 row-major P·V per pose (rope_camera_matrix), or NULL = the camera of rope_set_camera
 *   crop   {r0, r1, c0, c1} inclusive, or NULL = whole frame; planes are (r1-r0+1) x (c1-c0+1)
 *   depth  N planes float32 metres (0 = empty) or NULL;  ids  N planes uint8 (255 = background) or NULL
 * Image size, znear / zfar and the context's own camera are those of rope_set_camera, which this call leaves as they are.
 * Rows go to the device in chunks (at most 65 535 poses, output planes within a fixed device budget), each chunk's planes
 * copied out before the next one is drawn.  Like rope_eval_views it uses the per-candidate buffers: resident candidates and
 * the results of the last evaluation are gone afterwards. */
int rope_render_batch(rope_ctx *ctx, const double *q, const double *PV, int N, int n_render, const int32_t *crop,
                      float *depth, uint8_t *ids);

/* rope_render_batch for the whole frame with the N planes written to the CALLER's device memory (float32 depth, uint8 ids; one of
 * them may be NULL) instead of host memory: a synthetic run's frames stay on the GPU.  Chunks, limits and the effect on the
 * per-candidate buffers as rope_render_batch; only the destination of the copy-out differs.  The planes are complete when the call
 * returns. */
int rope_render_batch_device(rope_ctx *ctx, const double *q, const double *PV, int N, int n_render, float *depth_dev, uint8_t *ids_dev);

/* N poses to per-pixel label bit planes.  Replaces, per frame of AutomaticAnnotator.run, Renderer.render + Annotator._mask_color
 * for every label (annotation.py:117-127,163-176): bit b of masks[p][y][x] is set when any pixel of label b lies within the
 * pad x pad window anchored at (pad/2, pad/2) around (x, y), which is cv2.dilate(mask_b, ones((pad, pad))).
 *   q, PV, N, n_render   as rope_render_batch (PV NULL = the context's camera); whole frame only
 *   label_of_link        n_render entries: the bit (0..7) that a pixel drawn by link l sets, or 255 = none
 *   pad                  1..64 (1 = no dilation)
 *   masks                N planes H x W uint8
 *   boxes                N x 8 x 4 int32 {r0, r1, c0, c1} inclusive per (pose, bit), all -1 when the bit is empty; or NULL
 * Chunks, cameras and the per-candidate buffers as rope_render_batch; only the masks and boxes leave the device. */
int rope_render_masks(rope_ctx *ctx, const double *q, const double *PV, int N, int n_render,
                      const uint8_t *label_of_link, int pad, uint8_t *masks, int32_t *boxes);

/* Borders of one label of a mask plane, as cv2.findContours(mask_b, cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE) of OpenCV 4.5.1
 * gives them to Annotator._get_contour (annotation.py:77-86,125-127).  Host only, needs no context, thread-safe.
 *   mask        H x W uint8; the label is bit `bit` (0..7) of each byte; the plane has a frame of zero pixels around it
 *   box         {r0, r1, c0, c1} inclusive enclosing every set pixel of the bit (rope_render_masks' boxes), all -1 = empty;
 *               or NULL = the whole plane
 *   min_points  contours of fewer points are left out (the reference keeps those of at least 20); 0 keeps all
 *   points      out: (x, y) int32 pairs, capacity points_cap pairs
 *   starts      out: n_contours + 1 offsets into points (in pairs), capacity starts_cap
 * Outer and hole borders (Suzuki-Abe, 8-connected foreground) in the order the raster scan finds them; each keeps its start
 * point and every point where the chain direction changes.  *n_points and *n_contours get the sizes (also when the buffers
 * are too small: then nothing is written and ROPE_E_NOMEM is returned). */
int rope_trace_contours(const uint8_t *mask, int H, int W, int bit, const int32_t *box, int min_points, int32_t *points,
                        int points_cap, int32_t *starts, int starts_cap, int *n_points, int *n_contours);

/* OR over candidates of "pixel covered" (H x W uint8 0/1).  Replaces the depth-sum loop
 * of Crop._create (crop.py:60-81). */
int rope_coverage(rope_ctx *ctx, const double *cand, int C, int n_render, uint8_t *cover);

/* Camera-pose path: N frames (a known joint vector + target planes each) scored under K candidate cameras.
 * Replaces do_renders_at_pose + _error of ModellessCameraPredictor / CameraPredictor
 * (camera_pose_prediction.py:116-124,389-427,656-664,933-970): K x N renders and reductions in one batch.
 *   q            N x 6 joint vectors (robot_poses)
 *   tq           N planes H x W uint64, bits 0..38 target depth in Q32 metres
 *   t32          N planes H x W float32 target depth (ROPE_LOSS_TSWEEP: |sqrt(T)-sqrt(D)|), or NULL
 *   link_planes  N x 6 planes H x W uint64 (ROPE_LOSS_CAMFULL): bit 40 = link mask, bits 0..38 = mask * depth in
 *                Q32 metres (_masked_targets / _target_masks, camera_pose_prediction.py:919-931), or NULL
 * rope_eval_views: PV = K matrices P·V (row-major doubles); sums_out = K x N x ROPE_SUM_WORDS exact integer sums,
 * candidate order view-major.  Words: ROPE_LOSS_DEPTH / ROPE_LOSS_TSWEEP as rope_results_download;
 * ROPE_LOSS_CAMFULL: [0] #(D!=0), [1] sum |T-D| (Q32), [2] sum floor(sqrt|T-D| * 2^32), per link l at 5+3l:
 * #(M_l != R_l), #(d_l != 0), sum floor(sqrt(d_l) * 2^32).  The float epilogue stays with the caller. */
int rope_set_frames(rope_ctx *ctx, int n_frames, const double *q, const uint64_t *tq, const float *t32,
                    const uint64_t *link_planes);
int rope_eval_views(rope_ctx *ctx, const double *PV, int K, int n_render, int loss, uint64_t *sums_out);

/* The whole per-frame stage machine on the host, driving device batches through the calls above.
 * Replaces the stage loop of Predictor.run (predict.py:144-375) for the stages of the reference's 'SL' and 'SLU'
 * lists (stages.py:128-178); the target must have been set with rope_set_target (full loss masks + lookup plane).
 * Decisions follow the reference operation for operation, quirks included (SFlip's aliasing and its comparison
 * outside the endpoint loop, ISweep's stale base error, Descent's error history of the last joint only); the
 * not-a-knot cubic of interp1d(kind='cubic') (predict.py:310) is solved directly.  TensorSweep (in neither list, but a stage the
 * reference defines) is ROPE_STAGE_TSWEEP. */
enum {
    ROPE_STAGE_LOOKUP = 0,   /* stages.py:16-24   predict.py:165-171 */
    ROPE_STAGE_DESCENT = 1,  /* stages.py:92-119  predict.py:173-230 */
    ROPE_STAGE_SFLIP = 2,    /* stages.py:30-41   predict.py:232-281 */
    ROPE_STAGE_ISWEEP = 3,   /* stages.py:50-69   predict.py:283-338 */
    ROPE_STAGE_TSWEEP = 4    /* stages.py:71-90   predict.py:340-373: `count` divisions over `joints`, `range` as InterpolativeSweep; scored
                                with ROPE_LOSS_TSWEEP against the plane of rope_set_target_tsweep (the *- sign kept: the largest mean*std wins) */
};

typedef struct rope_stage {
    int32_t kind;
    int32_t to_render;        /* links drawn: 4 or 6 (Lookup: LOOKUP_NUM_RENDERED) */
    int32_t count;            /* Descent: iterations; InterpolativeSweep: divisions (>= 4) */
    uint32_t joints;          /* bit j set: joint j (S=0 .. T=5) takes part */
    double init_rate[6];      /* Descent: starting step per joint, NaN = keep the running step (None) */
    double rate_reduction;    /* Descent */
    double early_stop;        /* Descent */
    double range;             /* InterpolativeSweep: rad about the current angle, NaN = the whole joint range */
} rope_stage;

typedef void (*rope_eval_hook)(void *user, int32_t stage, int32_t n_render, const double *rows, int32_t n_rows);

typedef struct rope_predict_args {
    const rope_stage *stages;
    int32_t n_stages;
    int32_t speculate;            /* Descent: joints whose under/over pairs go out as one batch, 1..3 (1 = the
                                     reference's two renders at a time; the decisions are the same either way) */
    const double *limits;         /* 6 x 2 joint limits (URDFReader.joint_limits) */
    const double *camera_pose;    /* 6: x y z + the three angles, as Predictor.camera_pose (SFlip's axis, predict.py:245) */
    const double *min_ang_inc;    /* 6 (Predictor.min_ang_inc) */
    const double *lookup_angles;  /* n_lookup x 6 pose grid (lookup.py:56-66 order) */
    int32_t n_lookup;
    int32_t use_table;            /* 1: score the table of rope_lookup_build; 0: render and score the grid now */
    const int32_t *lookup_crop;   /* r0,r1,c0,c1 when use_table == 0 */
    double *lookup_angles_live;   /* NULL (default): every frame starts from the grid row itself and frames are independent.
                                     Non-NULL: the reference's table aliasing, opt-in — an n_lookup x 6 copy of the grid that the
                                     caller keeps from frame to frame.  The Lookup stage takes its row from HERE (scores still
                                     come from the grid / the stored table), and while the current angles are still that row —
                                     until an SFlip or a sweep rebinds them — Descent's steps are written back into it, as
                                     `angles = self.lookup_angles[argmin]` (a numpy view, predict.py:171) followed by
                                     `angles[idx] += rate` (predict.py:212-215) does in the reference.  Results then depend on
                                     the order of the frames: one context, frames in sequence. */
    rope_eval_hook on_eval;       /* NULL: nothing.  Else called after every scored batch of a stage (not the Lookup grid) with the
                                     stage's index, its links drawn and the rows in the order they were scored (a viewer shows the
                                     poses the stages looked at).  Must not call back into the context.  rope_predict only. */
    void *on_eval_user;           /* handed to on_eval as `user` */
} rope_predict_args;

/*   angles_out  6 doubles
 *   trace_out   n_stages x 6 doubles, the angles after every stage; may be NULL
 *   n_evals     candidate poses rendered and scored (lookup rows included); may be NULL */
int rope_predict(rope_ctx *ctx, const rope_predict_args *args, double *angles_out, double *trace_out, int64_t *n_evals);

/* ---- Many frames at once.  The reference predicts a dataset frame by frame (predict_dataset.py:43-44), each frame a chain of ~25
 * dependent render batches of 2-26 poses (predict.py:173-338).  Frames are independent (fresh state per frame, predict.py:144-148),
 * so B of them can walk the stage list in lockstep: every step then is ONE device batch holding the rows of all B frames, each row
 * scored against its own frame's target.
 *
 * rope_set_targets: the targets of n_frames frames, resident until replaced (they share buffers with rope_set_frames: one or the other).
 *   tq          n_frames planes H x W uint64 (as rope_set_target)
 *   t32         n_frames planes H x W float32 (lookup planes) or NULL
 *   t32_tsweep  n_frames planes H x W float32 for ROPE_LOSS_TSWEEP (rope_set_target_tsweep) or NULL
 *   link_flags  n_frames x 8 bytes (as rope_set_target)
 * rope_eval_targets: R candidate rows, row i scored against frame frame_of[i]'s target -> err_out[i]; loss DEPTH / FULL / LOOKUP
 *   (crop required) / TSWEEP.  Every error has the bits rope_eval gives with that frame as the single target.
 * rope_lookup_score_targets: the stored table of rope_lookup_build against every resident target in one pass: per frame the first
 *   argmin row and (optionally) its score; scores_out: n_frames x table rows or NULL.  Same bits as rope_lookup_score per frame. */
int rope_set_targets(rope_ctx *ctx, int n_frames, const uint64_t *tq, const float *t32, const float *t32_tsweep, const uint8_t *link_flags);
int rope_eval_targets(rope_ctx *ctx, const double *cand, const int32_t *frame_of, int R, int n_render, int loss, const int32_t *crop,
                      double *err_out);
int rope_lookup_score_targets(rope_ctx *ctx, int32_t *best_idx, double *best_score, double *scores_out);

/* The next set of targets on its way up while the resident set is being predicted (a dataset in groups of frames: the upload of
 * group k+1 hidden behind the stages of group k).  The context holds two sets of target planes.
 * rope_stage_targets: arguments as rope_set_targets, into the set NOT in use, on a stream of its own; returns when the copies are
 *   enqueued (sources from rope_host_alloc; pageable sources are copied through a pinned block and the call returns when the last
 *   chunk is enqueued).  May be called from another thread than the one evaluating on this context.  The host buffers belong to
 *   the copy until rope_commit_targets returns.
 * rope_commit_targets: waits for the upload and for the context's work, then makes the staged set the resident one (as if
 *   rope_set_targets had been called with it).  ROPE_E_ARG when nothing is staged or the image size changed in between. */
int rope_stage_targets(rope_ctx *ctx, int n_frames, const uint64_t *tq, const float *t32, const float *t32_tsweep, const uint8_t *link_flags);
int rope_commit_targets(rope_ctx *ctx);

/* The staged set filled ON THE DEVICE from instance masks that are there already (a segmenter on the same GPU): per frame what
 * rope_prepare_segmented computes at f == 1 — the merge of a link's instances, both body masks erode7(dilate8(.)), the masked depth,
 * the packing and the flags — by kernels enqueued on `stream`, the caller's (for example the one the segmenter ran on), with no
 * host synchronisation in the call.  Down-sampling stays with the caller (rope_downsample_even).
 *   n_total, slot0, n_frames   the staged set holds n_total frames; this call fills slots slot0 .. slot0 + n_frames - 1.  The call
 *                with slot0 == 0 starts and sizes a set; the others must name the same n_total and want_tsweep.  The set is
 *                complete, and rope_commit_targets takes it, once every slot has been filled.
 *   depth_dev    n_frames planes H x W (the image size of rope_set_camera), float32 (depth_kind 1) or float64 (2), DEVICE
 *   masks_dev    K_total = inst_first[n_frames] planes H x W of bytes, non-zero = inside the instance (a torch.bool tensor
 *                (K, H, W)), DEVICE; may be NULL when K_total == 0
 *   inst_first   n_frames + 1 offsets into the planes: frame i owns planes inst_first[i] .. inst_first[i + 1] - 1, HOST
 *   link_of      K_total link indices, -1 for an instance that is none of the rendered links (it still widens the body), HOST
 *   n_lookup_links  links 0 .. n_lookup_links - 1 make up the lookup plane's body;  want_tsweep: also the TensorSweep plane
 * rope_commit_targets waits for every stream such a call used since the last commit before it swaps the sets.  Like
 * rope_stage_targets the call touches nothing the evaluation calls use and may run on another thread.  ROPE_E_ARG for a null
 * pointer where instances exist, slots outside the set, a non-monotone inst_first, link_of outside -1 .. n_links - 1,
 * n_lookup_links outside 0 .. n_links, an unknown depth_kind, or a changed n_total in mid-set.  A refused call changes nothing:
 * a staging that waits for its commit still does, a set half filled can be continued.  A call that goes through writes the staged
 * planes, so it withdraws any staging that was complete (also one of rope_stage_targets): rope_commit_targets answers ROPE_E_ARG
 * until every slot of the set has been filled. */
int rope_stage_targets_segmented(rope_ctx *ctx, int n_total, int slot0, int n_frames, const void *depth_dev, int depth_kind,
                                 const uint8_t *masks_dev, const int32_t *inst_first, const int32_t *link_of, int n_lookup_links,
                                 int want_tsweep, void *stream);

/* The staged set filled on the device from full-size RENDERS that are there already (rope_render_batch_device): per frame what
 * rope_prepare_synthetic writes for the colour plane blue_of_id[ids] and float32 depth (kind 1) — the four-tap down-sampling by f
 * (OpenCV's fixed-point rounding for the colour, float32 for the depth; f = 1 passes through), the masks blue == link_blue[l], the
 * lookup depth over the first n_lookup_links links, the packing, the flags and, when asked, the TensorSweep plane.
 *   depth_dev, ids_dev   n_frames planes H0 x W0, float32 metres and uint8 link ids, DEVICE
 *   f                    1 or even; H0 / f x W0 / f must be the image size of rope_set_camera, else ROPE_E_ARG
 *   blue_of_id           256 bytes: channel 0 of the colour an id is drawn in (Renderer's table; 255 = background), HOST
 *   link_blue            n_links (<= 6) channel-0 values, as rope_prepare_synthetic takes them, HOST
 * Slots (n_total, slot0, n_frames), completion, rope_commit_targets, threading and refusals are those of
 * rope_stage_targets_segmented; the two calls fill the same staged set. */
int rope_stage_targets_synthetic(rope_ctx *ctx, int n_total, int slot0, int n_frames, const float *depth_dev, const uint8_t *ids_dev,
                                 int H0, int W0, int f, const uint8_t *blue_of_id, const int32_t *link_blue, int n_links,
                                 int n_lookup_links, int want_tsweep, void *stream);

/* Depth holes of synthetic frames (NoiseMaker.holes, noise.py:12-24) on the device, by an integer contract.
 * The reference thresholds eight Gaussian fields per frame, dilates them by 3, 6, .. and closes their union with a 20 x 20 box;
 * of each field only one bit per pixel matters, and that bit is drawn directly: the same distribution, another stream (the
 * reference's is unseeded).
 * rope_hole_thresholds: host only.  Dilation j has size d = 3 (j + 1) < max_size; its bit is set with probability
 *   p = erfc((1 - thresh_factor / d) / (sigma sqrt 2)), and T_out[j] = floor(p 2^32) (0xFFFFFFFF when p reaches 1).  *n gets the
 *   number of dilations (at most 10, d at most 32); T_out may be NULL.
 * rope_depth_holes: in place on N float32 planes H x W in DEVICE memory, on `stream`; needs no context, runs on the current device.
 *   Seed bit of pixel i = y W + x of plane m for dilation j: word (j & 3) of Philox4x32-10 with key (seed low 32, seed high 32)
 *   and counter (i, frame0 + m, j >> 2, 0), compared as word < T[j].  hole = close_connection(OR_j dilate_d[j](seed_j)) with
 *   cv2's box windows (anchor k / 2, borders ignored); depth becomes 0 where hole is set.  T, d: n_d values each, HOST;
 *   d[j] and connection 1 .. 32. */
int rope_hole_thresholds(double sigma, double thresh_factor, int max_size, uint32_t *T_out, int *n);
int rope_depth_holes(float *depth_dev, int N, int H, int W, uint32_t frame0, uint64_t seed, const uint32_t *T, const int32_t *d, int n_d,
                     int connection, void *stream);

/* The resident set of targets (rope_set_targets / rope_commit_targets) back to the host, for tests: n_frames planes each and
 * n_frames x 8 flag bytes; any pointer may be NULL. */
int rope_debug_targets(rope_ctx *ctx, uint64_t *tq, float *t32, float *t32_tsweep, uint8_t *flags);

/* The number of resident targets (rope_set_targets / rope_commit_targets); 0 when there are none — nothing set yet, a single
 * target (rope_set_target) only, or the planes taken by rope_set_frames — and for a NULL context. */
int rope_resident_targets(rope_ctx *ctx);

/* rope_predict for the n_frames resident targets of rope_set_targets, in lockstep: the same stage list, limits and camera for all of
 * them (args as rope_predict; lookup_angles_live must be NULL — the table aliasing makes frames depend on their order — and so must
 * on_eval).  n_frames must EQUAL the number of resident targets (rope_resident_targets): frame f is resident target f, and any other
 * count, smaller or larger, is refused with ROPE_E_ARG before anything runs.  A frame
 * that leaves a Descent stage early simply contributes no rows to the later batches of that stage.  Every frame's angles and trace
 * are those of rope_predict on that frame alone.
 *   angles_out  n_frames x 6;  trace_out  n_frames x n_stages x 6 or NULL;  n_evals  total poses rendered and scored, or NULL */
int rope_predict_batch(rope_ctx *ctx, const rope_predict_args *args, int n_frames, double *angles_out, double *trace_out, int64_t *n_evals);

/* Device-side per-candidate link matrices of the last eval (C x n_render x 16 float32), for tests. */
int rope_debug_mvp(rope_ctx *ctx, float *mvp_out, int C, int n_render);

/* Time `reps` back-to-back rope_eval_resident passes with HIP events on the context's
 * stream; ms[0] = FK + bounds kernels (a pass on kept geometry: the clearing launch), ms[1] = shared-layer raster launch (on kept
 * geometry: the layer-sums kernel; 0 when layers are not in use),
 * ms[2] = raster+score launch — on kept fragments: the streaming scorer, and in the pass that builds the store the build as well
 * (it is recorded with the scorer, not in a slot of its own) —, ms[3] = finalize+argmin, ms[4] = whole pass (averages per pass,
 * milliseconds). */
int rope_profile_eval(rope_ctx *ctx, int n_render, int loss, const int32_t *crop, int reps, float *ms);

/* Execution strategy: how a batch is laid out over launches.  Every value gives bit-identical results (the depth test is
 * a minimum and the sums are exact integers); the equivalence tests and the "unshared" bench figure use it.
 *   1  do not share links 0-2 between candidates with equal (q0, q1): six links drawn per candidate
 *   2  do not split the meshlets of a tile over several workgroups for small batches
 *   4  no second level of sharing (links 0-1 per distinct q0)
 *   8  large batches as one workgroup per (tile, candidate) pair instead of a queue of the pairs that have work
 *  16  always the raster kernels that can clip triangles at the near plane (by default only when the camera is within the
 *      robot's reach of it: they are several per cent slower, and without a triangle at the plane they draw the same image)
 *  32  small batches: forward kinematics and screen boxes as a launch of their own instead of inside the split raster's workgroups
 *  64  large batches: keep no geometry from pass to pass (rope_eval_resident) — every pass builds all of it, as the first one does
 *      (and keeps no fragments either)
 * 128  large batches: keep no fragments — a pass on kept geometry draws every row's own links again */
enum { ROPE_STRATEGY_NO_LAYERS = 1, ROPE_STRATEGY_NO_SPLIT = 2, ROPE_STRATEGY_NO_PARENTS = 4, ROPE_STRATEGY_NO_QUEUE = 8, ROPE_STRATEGY_CLIP_KERNELS = 16,
       ROPE_STRATEGY_SEPARATE_GEOMETRY = 32, ROPE_STRATEGY_NO_GEOMETRY_CACHE = 64, ROPE_STRATEGY_NO_KEPT_FRAGMENTS = 128 };
int rope_set_strategy(rope_ctx *ctx, int flags);

/* Passes of rope_eval_resident that could keep geometry (more than 256 rows, shared layers, the single target) since the context
 * was created: how many ran on what the pass before them left (hits) and how many built it (misses; with
 * ROPE_STRATEGY_NO_GEOMETRY_CACHE all of them).  Either pointer may be NULL. */
int rope_geometry_cache_stats(rope_ctx *ctx, uint64_t *hits, uint64_t *misses);

/* The kept fragments (rope_eval_resident): stores built and passes scored from one since the context was created; bytes and 4-sample
 * groups of the store held now (0: none — not built yet, dropped, or refused by the budget).  Any pointer may be NULL. */
int rope_fragment_store_stats(rope_ctx *ctx, uint64_t *builds, uint64_t *passes_served, uint64_t *bytes, uint64_t *groups);
/* (row, tile) pairs of the store held now in which any group is kept (0: no store). */
int rope_fragment_store_pairs(rope_ctx *ctx, uint64_t *pairs);
/* Most bytes a fragment store may take; a grid whose count comes to more keeps none and is scored as without the store.  Default: the
 * lookup table's budget, a tenth of 8 GiB.  Drops the store held (the next pass on kept geometry counts again). */
int rope_set_fragment_budget(rope_ctx *ctx, uint64_t bytes);

/* ---- Segmentation stage (robotpose/prediction/predict.py:94-98,416: the Matterport Mask R-CNN in front of the engine).
 * The convolutions are library calls from PyTorch-ROCm (rope_s3d_amd/maskrcnn.py); the two box-shaped steps between them
 * are kernels of this library.  No context: plain device pointers and the HIP stream to launch on (hipStream_t, NULL = default).
 *
 * rope_seg_nms: greedy non-maximum suppression (tf.image.non_max_suppression, as the ProposalLayer and
 * refine_detections_graph of mrcnn/model.py call it) of n_sets independent sets of n boxes each.
 *   boxes    n_sets x n x 4 float32 (y1, x1, y2, x2), each set sorted by DESCENDING score; 16-byte aligned
 *   groups   n_sets x n int32 or NULL: boxes only suppress boxes of the same group (per-class NMS)
 *   valid    n_sets x n bytes or NULL: 0 = padding (never kept, never suppressing)
 *   limit    at most this many boxes kept per set (the best ones)
 *   scratch  n_sets x n x ceil(n / 64) uint64 of device memory
 *   keep     n_sets x n bytes out: 1 = kept (in the order of `boxes`)
 *
 * rope_seg_roi_align: PyramidROIAlign — the pyramid level by box area, then tf.image.crop_and_resize (bilinear,
 * pool x pool samples spanning the box, corners included, 0 outside the map).
 *   rows_bf16       the pyramid levels P2..P5 of all frames as one table of channel rows (bfloat16, `channels` per
 *                   feature pixel), level l starting at row level_off[l], frames back to back inside a level
 *   boxes           n_boxes x 4 float32 normalised (y1, x1, y2, x2); 16-byte aligned;  frame: n_boxes int32 batch entry
 *   level_hw        4 x (H, W) int32;  level_off 4 int64
 *   inv_level_unit  1 / (224 / image_size) as float32;  t: `pool` float32 sample positions in [0, 1] (device)
 *   out_bf16        n_boxes x pool x pool x channels bfloat16 */
/* rope_seg_bias_act: what follows a convolution, in place and in one pass: y <- [relu](bf16(bf16(y + bias[channel]) [+ residual])),
 * with the roundings separate tensor operations would make.
 *   y_bf16    n bfloat16 (n a multiple of 8), NCHW (`inner` = H*W, a multiple of 8) or channels-last (`inner` = 1, channels a
 *             multiple of 8);  bias_bf16: `channels` bfloat16;  residual_bf16: n bfloat16 in y's layout, or NULL;  relu: 0 / 1 */
int rope_seg_bias_act(void *y_bf16, const void *bias_bf16, const void *residual_bf16, int64_t n, int channels, int64_t inner, int relu,
                      void *stream);
int rope_seg_nms(const float *boxes, const int32_t *groups, const uint8_t *valid, int n_sets, int n, float iou_thr, int limit,
                 uint64_t *scratch, uint8_t *keep, void *stream);
int rope_seg_roi_align(const void *rows_bf16, const float *boxes, const int32_t *frame, const int32_t *level_hw,
                       const int64_t *level_off, int n_boxes, int channels, int pool, float inv_level_unit, const float *t,
                       void *out_bf16, void *stream);

/* ---- Segmentation training (rope_s3d_amd/training.py: Matterport's training graph, mrcnn/model.py).  Same conventions as the
 * rope_seg_* calls above.  Random choices are per-element keys from the caller: a kernel keeps the smallest (key, index) pairs.
 *
 * rope_seg_rpn_targets: build_rpn_targets of n_frames frames (float64, pixel coordinates).
 *   anchors     n_anchors x 4 float64 (y1, x1, y2, x2), n_anchors < 131 072;  gt_boxes: n_frames x gt_stride x 4 float64
 *   gt_count    n_frames int32 (<= gt_stride <= 100);  keys: n_frames x n_anchors uint32
 *   anchor_max  n_frames x n_anchors float64, anchor_arg n_frames x n_anchors int32 (out: best IoU and its GT);  gt_max: scratch
 *   match       n_frames x n_anchors int32 out: 1 positive, -1 negative, 0 neutral (at most 128 positives, 256 in all)
 *   bbox        n_frames x 256 x 4 float64 out: the positives' deltas / RPN_BBOX_STD_DEV in anchor order, zero rows after
 *
 * rope_seg_roi_targets: DetectionTargetLayer of n_frames frames (float32, normalised coordinates).
 *   proposals   n_frames x prop_stride x 4 (prop_stride <= 2048), prop_count valid rows each;  keys: n_frames x prop_stride uint32
 *   gt_boxes    n_frames x gt_stride x 4;  gt_class, gt_count int32;  gt_masks n_frames x gt_stride x mask_h x mask_w bytes (0/1)
 *   inv_positive_ratio  float32(1 / ROI_POSITIVE_RATIO)
 *   out, 200 rows per frame (positives by key, negatives by key, zero rows): rois x 4, class_ids, deltas x 4 / BBOX_STD_DEV,
 *   masks 28 x 28 (round(crop_and_resize) of the matched GT mask over the roi)
 *
 * rope_seg_roi_align_float / rope_seg_roi_align_backward: rope_seg_roi_align on float32 rows (no bfloat16 roundings) and its
 * transpose: grad_out (n_boxes x pool x pool x channels) times each sample's four bilinear weights, added into grad_rows (the
 * row table's shape, zeroed by the caller) with global float atomics. */
int rope_seg_rpn_targets(const double *anchors, int n_anchors, const double *gt_boxes, const int32_t *gt_count, int gt_stride,
                         int n_frames, const uint32_t *keys, double *anchor_max, int32_t *anchor_arg, uint64_t *gt_max, int32_t *match,
                         double *bbox, void *stream);
int rope_seg_roi_targets(const float *proposals, const int32_t *prop_count, int prop_stride, const float *gt_boxes, const int32_t *gt_class,
                         const int32_t *gt_count, int gt_stride, const uint8_t *gt_masks, int mask_h, int mask_w, int n_frames,
                         const uint32_t *keys, float inv_positive_ratio, float *rois, int32_t *class_ids, float *deltas, float *masks,
                         void *stream);
int rope_seg_roi_align_float(const float *rows, const float *boxes, const int32_t *frame, const int32_t *level_hw, const int64_t *level_off,
                           int n_boxes, int channels, int pool, float inv_level_unit, const float *t, float *out, void *stream);
int rope_seg_roi_align_backward(const float *grad_out, const float *boxes, const int32_t *frame, const int32_t *level_hw,
                                const int64_t *level_off, int n_boxes, int channels, int pool, float inv_level_unit, const float *t,
                                float *grad_rows, void *stream);

/* ---- Segmentation evaluation (rope_s3d_amd/evaluation.py, evaluate.py).  Same conventions as the rope_seg_* calls above: no
 * context, plain device pointers, the HIP stream to launch on, ROPE_E_ARG for arguments it refuses.
 *
 * rope_seg_mask_overlaps: how far the instance planes of a detector overlap the ground-truth labels of their frames, as exact
 * pixel counts (csrc/rope_eval.hip), by kernels enqueued on `stream` with no host synchronisation in the call.
 *   pred_dev      K_total = inst_first[n_frames] planes H x W of bytes, non-zero = inside the instance (any non-zero value; a
 *                 torch.bool tensor (K, H, W), as rope_stage_targets_segmented takes it), DEVICE; may be NULL when K_total == 0
 *   inst_first    n_frames + 1 offsets into the planes: frame i owns planes inst_first[i] .. inst_first[i + 1] - 1, HOST
 *   gt_bits_dev   n_frames planes H x W of bytes, bit b set where the pixel belongs to ground-truth label b (what
 *                 rope_render_masks writes: up to 8 labels, which may overlap), DEVICE
 *   inter_dev     K_total x 8 uint32 out: [k][b] = pixels where plane k is non-zero and bit b of its frame's plane is set
 *   area_pred_dev K_total uint32 out: non-zero pixels of plane k;  area_gt_dev: n_frames x 8 uint32 out: pixels of frame i with bit b
 * The outputs are DEVICE memory of the caller's and are written completely (the caller need not clear them); the counts are exact
 * integers, the same from run to run.  n_frames == 0 and K_total == 0 succeed (area_gt_dev is filled all the same).  ROPE_E_ARG for
 * a null pointer where planes exist, n_frames < 0, H < 1, W < 1, H W >= 2^32, or an inst_first that does not start at 0 or
 * decreases; a refused call enqueues nothing. */
int rope_seg_mask_overlaps(const uint8_t *pred_dev, const int32_t *inst_first, int n_frames, const uint8_t *gt_bits_dev, int H, int W,
                           uint32_t *inter_dev, uint32_t *area_pred_dev, uint32_t *area_gt_dev, void *stream);

/* ---- Dataset verification (rope_s3d_amd/data/verification.py, verify.py).  Same conventions: no context, plain device pointers,
 * the HIP stream to launch on, nothing synchronised in the call.
 *
 * rope_frame_agreement: how far every recorded frame agrees with the render at its recorded pose (csrc/rope_verify.hip).  It
 * replaces verification.py:58-67 and :222, where the reference renders each frame, blends the render over the photograph and leaves
 * the judgement to a person: here the render's depth is compared with the recorded depth pixel by pixel, in integers.
 *   render_depth_dev  n_frames planes H x W float32 metres: the renders (rope_render_batch_device), DEVICE, 4-byte aligned.  The
 *                     depth of a rendered pixel is finite and in [0, 128) (the renderer's far plane is at 100 m); other values
 *                     count as the nearer end of that range, NaN as 0
 *   render_ids_dev    n_frames planes H x W of link ids, 255 = background, DEVICE, any alignment
 *   frame_depth_dev   n_frames planes H x W float32 metres: the recorded depth maps, DEVICE, 4-byte aligned
 *   n_links           1 .. ROPE_MAX_LINKS: ids below it are links
 *   tol_m             finite, >= 0: how far apart two depths may lie and still agree
 *   sums_dev          n_frames x ROPE_AGREE_WORDS uint64 out, DEVICE, 8-byte aligned; zeroed by the call itself
 * With q(x) = floor(x 2^32), R, id, T a pixel of the three planes: T is VALID when finite and 0 < T < 128; the pixel is RENDERED when
 * id < n_links; BOTH = rendered and valid; CLOSE = both and |q(R) - q(T)| <= q(tol_m); FRONT = both and q(T) < q(R) - q(tol_m)
 * (something stands before the robot).  Per frame:
 *   [0] valid pixels   [1] rendered pixels   [2] sum over both of |q(R) - q(T)|
 *   [3] pixels with n_links <= id < 255 (counted nowhere else)   [4 + 4 l .. 7 + 4 l] link l: rendered, both, close, front
 * All sums are exact integers, the same from run to run.  ROPE_E_ARG, with nothing enqueued, for n_frames < 1, H < 1, W < 1,
 * H W > 2^24 (word 2 holds 2^39 a pixel), n_links outside 1 .. ROPE_MAX_LINKS, a tol_m that is negative or not finite, a null or
 * misaligned pointer.  ROPE_E_HIP when the runtime refuses the memset or the launch (a grid of n_frames x up to 2 048 workgroups:
 * far beyond any set that fits the device); sums_dev may then have been zeroed already. */
#define ROPE_AGREE_WORDS 28
int rope_frame_agreement(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames, int H,
                         int W, int n_links, float tol_m, uint64_t *sums_dev, void *stream);

/* ---- Conditioning of raw depth frames (rope_s3d_amd/prediction/conditioning.py, csrc/rope_feed.hip).  Same conventions: no context,
 * plain device pointers, the HIP stream to launch on, nothing synchronised in the call, no state that the caller does not own.
 * They stand in for what the reference's LiveCamera asks of pyrealsense2 for every frame (feed.py:32-99: decimation, spatial and
 * temporal filters, rs.align to the colour stream).  The arithmetic below is this project's definition, restated from memory of
 * librealsense's filters and not checked against them; tests/feed_ref.py is its plain reference.
 * All depth planes are uint16 in raw sensor units, 0 = no data, (n_frames, h, w) contiguous, DEVICE.  One stack of planes holds
 * at most 2^31 - 1 elements.  Every call returns ROPE_E_ARG, with nothing enqueued and nothing written, for a null pointer, a size
 * below 1 or a parameter outside the range given; ROPE_E_HIP when the runtime refuses a launch.
 *
 * rope_depth_decimated_shape (host only): the shape rope_depth_decimate writes for H x W planes and k in 2 .. 8:
 *   h = ((H / k) / 4) * 4, w = ((W / k) / 4) * 4 in integer division; ROPE_E_ARG when either is 0.
 * rope_depth_decimate: out (n_frames, h, w); pixel (r, c) from the k x k patch at (r k, c k) of the frame, rows and columns beyond
 *   h k and w k dropped.  With m non-zero values in the patch: k 2 or 3: the value at index (m - 1) / 2 of those values sorted
 *   ascending (the lower median); k >= 4: floor(sum / m); 0 when m == 0.
 *
 * rope_depth_spatial, in place: `iterations` (1 .. 5) times a horizontal sweep of every row, then a vertical sweep of every column.
 *   A sweep of a line x[0 .. L) is a forward pass i = 1 .. L - 1, then a backward pass i = L - 2 .. 0.  A pass takes a = x[previous i]
 *   as already updated in this pass and b = x[i]; if a != 0, b != 0 and 1 <= |b - a| <= delta then
 *   x[i] = (uint16)(float(b) * alpha + float(a) * (1.0f - alpha) + 0.5f), float32 with each of the five operations rounded on its
 *   own, then truncated; otherwise x[i] stays.  Zeros are never written over and never start a chain; a line of length 1 is left
 *   alone.  alpha float32 in (0, 1], delta 1 .. 65535, n_frames at most 65535.
 *
 * rope_depth_temporal, in place; the n_frames of a call are consecutive in time.  last_dev (uint16, h x w) and history_dev (uint8,
 *   h x w) are the caller's state, zeroed by the caller to reset.  Per pixel and frame, c the incoming value and p = last:
 *     c != 0, p != 0, |c - p| <= delta:  f = (uint16)(alpha * float(c) + (1.0f - alpha) * float(p) + 0.5f); the frame and last get f
 *     c != 0 otherwise:                  last = c, the frame keeps c
 *     c == 0:                            the frame gets p when p != 0 and the persistence rule holds on history as it stood before
 *                                        this frame, else stays 0; last is unchanged
 *   and in every case history = (history << 1) | (c != 0) afterwards (bit 0 = the newest frame).  The rule for persistence 0 .. 8
 *   is a (need, window) pair: 0 never, 1 (8, 8), 2 (2, 3), 3 (2, 4), 4 (2, 8), 5 (1, 2), 6 (1, 5), 7 (1, 8), 8 always; it holds when
 *   popcount(history & ((1 << window) - 1)) >= need.  One call with n frames gives what n calls with one frame each give, state
 *   included.  alpha float32 in (0, 1], delta 1 .. 65535.
 *
 * rope_depth_align: depth planes (n_frames, h, w) seen from the colour sensor: out_dev (n_frames, Hc, Wc), 0 where nothing lands.
 *   depth_intrin, color_intrin   {fx, fy, cx, cy}, 4 doubles each, HOST, no distortion terms
 *   extrin                       row-major 3x3 R followed by t, 12 doubles, HOST: depth to colour, metres
 *   scratch_dev                  n_frames x Hc x Wc uint32, DEVICE, 4-byte aligned; filled by the call itself
 *   Every pixel (x, y) with z != 0 contributes; Z = double(z) * depth_scale.  Its corners (x - 0.5, y - 0.5) and (x + 0.5, y + 0.5)
 *   each go, in double and in this order of operations, through  P = ((u - cx) / fx * Z, (v - cy) / fy * Z, Z);
 *   P' = R P + t, each row as ((R0 X + R1 Y) + R2 Z) + t;  the pixel is skipped when either corner has Z' <= 0;
 *   (u', v') = (X' / Z' * fx + cx, Y' / Z' * fy + cy) with the colour sensor's terms.  x0 = floor(u0' + 0.5), likewise y0, x1, y1, then
 *   ordered; the pixel is skipped when any of the four lies outside the colour image or the footprint is larger than
 *   ROPE_ALIGN_MAX_FOOTPRINT colour pixels either way (with sane sensors it is 3 x 3).  Every colour pixel of [x0 .. x1] x [y0 .. y1]
 *   takes the minimum z of all its contributors: an integer atomic minimum on scratch_dev, narrowed to out_dev by a second pass, so
 *   the result does not depend on the order of the atomics.  depth_scale finite and > 0, all terms finite, depth fx, fy non-zero. */
#define ROPE_ALIGN_MAX_FOOTPRINT 16
int rope_depth_decimated_shape(int H, int W, int k, int *h, int *w);
int rope_depth_decimate(const uint16_t *raw_dev, int n_frames, int H, int W, int k, uint16_t *out_dev, void *stream);
int rope_depth_spatial(uint16_t *planes_dev, int n_frames, int h, int w, float alpha, int delta, int iterations, void *stream);
int rope_depth_temporal(uint16_t *planes_dev, int n_frames, int h, int w, float alpha, int delta, int persistence, uint16_t *last_dev,
                        uint8_t *history_dev, void *stream);
int rope_depth_align(const uint16_t *planes_dev, int n_frames, int h, int w, const double *depth_intrin, const double *color_intrin,
                     const double *extrin, double depth_scale, int Hc, int Wc, uint32_t *scratch_dev, uint16_t *out_dev, void *stream);

/* ---- Photo-like synthetic frames (rope_s3d_amd/simulation/shading.py, csrc/rope_shade.hip).  Same conventions: no context, plain
 * device pointers, the HIP stream to launch on, nothing synchronised, allocated or copied in the call.  This is the project's own
 * picture of the robot, not the reference's (pyrender's shader): one directional light, a Lambert surface whose normals come from
 * the rendered depth, a colour per link, a background and sensor noise.  tests/shade_ref.py restates the text below in numpy.
 *
 * rope_shade_frames: N renders to N pictures.
 *   depth_dev, ids_dev   N planes H x W: float32 metres (4-byte aligned) and link ids, as rope_render_batch_device writes them, DEVICE
 *   n_links              1 .. ROPE_MAX_LINKS: a pixel is ROBOT iff id < n_links; 255 and every other id are background
 *   fx, fy, cx, cy       the camera's terms as float32
 *   params               N records, HOST (they travel as kernel arguments); light is the direction the light TRAVELS in camera axes
 *                        (x right, y down, z forward), of unit length as the host rounded it: the kernel does not renormalise
 *   bg_dev               n_bg planes H x W x 3 bytes, DEVICE, any alignment; may be NULL when every bg_index is -1
 *   frame0, seed         as in rope_depth_holes: plane m draws the noise of frame frame0 + m of the 64-bit seed
 *   bgr_dev              N planes H x W x 3 bytes out, DEVICE, any alignment
 *   depth_out_dev        NULL, or N planes H x W float32 out (4-byte aligned): depth where the pixel is robot, bg_depth elsewhere.
 *                        It may be depth_dev itself.
 * Everything below is float32 with ONE correctly rounded IEEE operation per written operation (no fused multiply-add; / and sqrt
 * are the correctly rounded ones), in the order written; z = depth[y][x], id = ids[y][x], rec = params[m].
 *   1. P(x, y) = (kx(x) * z, ky(y) * z, z) with kx(x) = ((float)x - cx) / fx and ky(y) = ((float)y - cy) / fy.
 *   2. dX = P(x + 1, y) - P(x, y) if x + 1 < W and ids[y][x + 1] == id; else P(x, y) - P(x - 1, y) if x > 0 and ids[y][x - 1] == id;
 *      else (0, 0, 0).  dY likewise along y (y + 1 first).  Differences never cross an id boundary or the image edge.
 *   3. n = dX x dY: n.x = dX.y * dY.z - dX.z * dY.y, n.y = dX.z * dY.x - dX.x * dY.z, n.z = dX.x * dY.y - dX.y * dY.x (each a product
 *      minus a product).  nn = (n.x * n.x + n.y * n.y) + n.z * n.z;  dot = (n.x * L.x + n.y * L.y) + n.z * L.z.
 *      lam = 1 if nn == 0, else (dot > 0 ? dot : 0) / sqrt(nn).  dX x dY points away from the camera and so does L, so a surface that
 *      faces a head-on light has dot > 0.  A NaN depth in the neighbourhood makes nn NaN, which is not == 0: lam is then NaN, and
 *      the pixel comes out 0 in step 5 (this is why the test is nn == 0 and not nn > 0).
 *   4. s = ambient + (1 - ambient) * lam;  shade = s > 1 ? 1 : s  (a NaN stays).
 *   5. channel c (0 blue, 1 green, 2 red) of a robot pixel: v = rint(((float)albedo[id][c] * shade) * gain[c]), ties to even.
 *   6. of a background pixel: v = (float)bg_dev[bg_index][y][x][c], or (float)bg_colour[c] when bg_index is -1.
 *   7. noise: with noise_q == 0 it is 0 and nothing is drawn.  Otherwise the four words of Philox4x32-10 with rope_depth_holes' key
 *      (seed low 32, seed high 32) and counter (y W + x, frame0 + m, 0, 1) — the last word keeps this stream apart from the holes' —
 *      and for channel c, with b0..b3 the bytes of word c:  noise = ((b0 + b1 + b2 + b3 - 510) * noise_q) >> 10, an arithmetic shift
 *      of a 32-bit integer (floor).
 *   8. t = v + (float)noise;  byte = t > 0 ? (t < 255 ? t : 255) : 0, so a NaN gives 0; t is a whole number, the conversion exact.
 * ROPE_E_ARG, with nothing enqueued, for N < 0, a null depth_dev, ids_dev, bgr_dev or params where N > 0, H or W < 1, H W >= 2^31,
 * n_bg < 0, n_links outside 1 .. ROPE_MAX_LINKS, a noise_q outside 0 .. ROPE_SHADE_MAX_NOISE_Q, a bg_index outside -1 .. n_bg - 1 or
 * one >= 0 with bg_dev NULL, a depth_dev or depth_out_dev that is not 4-byte aligned.  N == 0 succeeds.  ROPE_E_HIP when the runtime
 * refuses a launch. */
#define ROPE_SHADE_MAX_NOISE_Q 1023
typedef struct rope_shade_params {
    float light[3];                         /* L */
    float ambient;
    float gain[3];
    float bg_depth;                         /* metres; 0 = leave the background empty */
    int32_t noise_q;                        /* 0 .. ROPE_SHADE_MAX_NOISE_Q; the noise spans -+ (510 noise_q) >> 10 levels */
    int32_t bg_index;                       /* -1 = bg_colour */
    uint8_t albedo[ROPE_MAX_LINKS][3];      /* BGR per link; rows from n_links on are not read */
    uint8_t bg_colour[3];
    uint8_t reserved[3];                    /* to 64 bytes */
} rope_shade_params;
int rope_shade_frames(const float *depth_dev, const uint8_t *ids_dev, int N, int H, int W, int n_links, float fx, float fy, float cx, float cy,
                      const rope_shade_params *params, const uint8_t *bg_dev, int n_bg, uint32_t frame0, uint64_t seed, uint8_t *bgr_dev,
                      float *depth_out_dev, void *stream);

/* ---- Pose refinement (rope_s3d_amd/prediction/refinement.py, csrc/rope_refine.hip).  Same conventions: no context, plain device
 * pointers, the HIP stream to launch on, nothing synchronised, allocated or copied in the call.  The reference has nothing like it:
 * its answer is the last lattice point of a search.  tests/refine_ref.py restates the text below in numpy.
 *
 * rope_pose_normal_equations: per frame, the Gauss-Newton normal equations of the depth residual between the render at a pose and
 * the frame, with respect to the joint angles.
 *   render_depth_dev, render_ids_dev   n_frames planes H x W: float32 metres (4-byte aligned) and link ids (255 = background), as
 *                        rope_render_batch_device writes them at the pose, DEVICE
 *   frame_depth_dev      n_frames planes H x W float32 metres: the frames, DEVICE, 4-byte aligned
 *   n_links              1 .. ROPE_MAX_LINKS: ids below it are links
 *   fx, fy, cx, cy       the camera's terms as float32, as rope_shade_frames takes them; finite, fx and fy not 0
 *   joints_dev           n_frames x n_joints x 6 doubles, DEVICE, 8-byte aligned: per joint its unit axis a and a point o on the axis,
 *                        at the frame's pose, in the camera axes of P below (x right, y down, z forward, metres)
 *   n_joints             1 .. 6.  Link l is moved by the joints j < l; link 0 is the base and moves with none
 *   clip_m               finite, > 0: the truncation of the residual, metres
 *   out_dev              n_frames x ROPE_NEQ_WORDS doubles out, DEVICE, 8-byte aligned; written completely
 *   work_dev             rope_pose_normal_workspace(n_frames, H, W) bytes of scratch, DEVICE, 8-byte aligned
 * Everything is float64 with ONE correctly rounded IEEE operation per written operation, in the order written; R, T, fx .. cy and
 * clip_m are widened first.  z = R[y][x], id = ids[y][x], T = depth[y][x]; dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; u x v has the
 * components u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x.
 *   1. P(x, y) = (kx(x) z, ky(y) z, z) with kx(x) = (x - cx) / fx, ky(y) = (y - cy) / fy: rope_shade_frames' points, in float64.
 *   2. dX = P(x + 1, y) - P(x, y) if x + 1 < W and ids[y][x + 1] == id; else P(x, y) - P(x - 1, y) if x > 0 and ids[y][x - 1] == id;
 *      else 0.  dY likewise along y.  n = dX x dY.  The pixel has NO NORMAL when a component of n is not finite or all three are 0.
 *   3. RENDERED: id < n_links.  VALID: T finite and 0 < T < 128 (compared as float32).  BOTH: rendered and valid.  r = z - T.
 *      MOVING: 1 <= id <= n_joints.
 *   4. INLIER: both, moving, |r| <= clip, a normal, and with nn = dot(n, n), nP = dot(n, P), PP = dot(P, P):
 *      nP nP >= 0.01 (nn PP) and nP != 0 — the surface is seen at more than 0.1 of head-on (a design constant, not a measurement).
 *   5. For an inlier on link l = id and joint j < min(l, n_joints), a and o the joint's:
 *      J_j = (z dot(n, a x (P - o))) / nP;  J_j = 0 for every other j < 6.  (Exact for a plane turning about the axis: the
 *      normal's own rotation cancels at first order.)
 * Per frame:  [0] BOTH pixels   [1] sum over both of (r r <= clip clip ? r r : clip clip) (a NaN residual counts as the clip)
 *   [2] inliers   [3] sum over inliers of r r   [4 + j] sum of J_j r   [10 ..30] sum of J_j J_i for j <= i, row by row
 *   (00 01 .. 05 11 12 .. 55)   [31] 0.  The counts are doubles too (exact: at most 2^24).
 * Determinism is part of the contract: no floating-point atomic is used; a workgroup covers pixels that depend on H W alone and
 * adds them in a fixed order, its one partial goes to work_dev, and a second kernel adds a frame's partials in index order.  The
 * same planes give the same bytes from run to run, and whether the frames come in one call or in several.  The ORDER of the
 * summation is not part of the contract: a restatement that adds in another order differs by at most the rounding of a sum of
 * that many terms.
 * ROPE_E_ARG, with nothing enqueued, for n_frames < 1, H < 1, W < 1, H W > 2^24, 2^24 workgroups or more (n_frames x
 * ceil(H W / 2048)), n_links outside 1 .. ROPE_MAX_LINKS, n_joints outside 1 .. 6, a clip_m that is not finite or not positive,
 * camera terms that are not finite or a zero fx or fy, a null or misaligned pointer.  ROPE_E_HIP when the runtime refuses a launch.
 * rope_pose_normal_workspace (host only): the bytes of work_dev for such a call; 0 for a shape the call refuses. */
#define ROPE_NEQ_WORDS 32
int rope_pose_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames, int H,
                               int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev, int n_joints, float clip_m,
                               double *out_dev, double *work_dev, void *stream);
size_t rope_pose_normal_workspace(int n_frames, int H, int W);

/* rope_camera_normal_equations: the same normal equations with respect to the CAMERA pose (prediction/refinement.py,
 * CameraPoseRefiner; tests/camera_refine_ref.py restates the text below in numpy).  Every argument but two is
 * rope_pose_normal_equations', work_dev has rope_pose_normal_workspace(n_frames, H, W) bytes, and the text above holds word for word
 * — the arithmetic rule, steps 1 and 2, RENDERED, VALID, BOTH and r of step 3, the 32 words, determinism — with these changes:
 *   twists_dev           n_frames x n_cols x 6 doubles, DEVICE, 8-byte aligned, in place of joints_dev: per column k its angular
 *                        part w_k (3) and its linear part v_k (3), in the camera axes of P (x right, y down, z forward; rad and
 *                        metres per unit of the column).  Per frame, as the joints are: one call may hold several trial cameras
 *   n_cols               1 .. 6, in place of n_joints
 *   3'. MOVING: id < n_links — every drawn link moves with every column, the base (link 0) too.
 *   4'. INLIER: both, |r| <= clip, a normal, and the same test on nP nP >= 0.01 (nn PP), nP != 0.
 *   5'. For an inlier and a column k < n_cols, a point of the surface has the velocity u = w_k x P + v_k per unit of the column, the
 *      sum taken component by component after the cross product:
 *        c = w_k x P;   u = (c.x + v_k.x, c.y + v_k.y, c.z + v_k.z);   J_k = (z dot(n, u)) / nP;
 *      J_k = 0 for n_cols <= k < 6.  (The depth along the pixel's ray changes by that much: exact for a plane under the twist, the
 *      normal's own rotation cancels at first order as in 5.)
 * Words [4 + k] and every [10 .. 30] entry with a column >= n_cols are exactly 0.
 * ROPE_E_ARG as above with n_cols in place of n_joints and twists_dev in place of joints_dev; out_dev is left untouched. */
int rope_camera_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames, int H,
                                 int W, int n_links, float fx, float fy, float cx, float cy, const double *twists_dev, int n_cols, float clip_m,
                                 double *out_dev, double *work_dev, void *stream);

/* rope_bundle_normal_equations: the normal equations with respect to the joint angles AND the camera pose in ONE system of twelve
 * column slots (csrc/rope_bundle.hip; prediction/refinement.py, BundleRefiner; tests/bundle_ref.py restates the text below in
 * numpy).  The planes, n_links, fx .. cy, clip_m, out_dev, the stream, the arithmetic rule, steps 1 and 2, RENDERED, VALID, BOTH
 * and r of step 3 and the text on determinism are rope_pose_normal_equations'; what differs:
 *   joints_dev, n_joints n_frames x n_joints x 6 doubles as rope_pose_normal_equations takes them; n_joints 0 .. 6
 *   twists_dev, n_cols   n_frames x n_cols x 6 doubles as rope_camera_normal_equations takes them; n_cols 0 .. 6
 *                        n_joints + n_cols >= 1.  A pointer whose count is 0 is not read and may be null
 *   out_dev              n_frames x ROPE_BNEQ_WORDS doubles; written completely
 *   work_dev             rope_bundle_normal_workspace(n_frames, H, W) bytes, DEVICE, 8-byte aligned
 *   Slots.  Slot c = j (0 .. 5) is joint j: J_c is step 5's J_j, so link l moves with the joints j < min(l, n_joints) and the base
 *     with none.  Slot c = 6 + k (0 .. 5) is camera column k: J_c is step 5''s J_k.  J_c = 0 for a joint slot >= n_joints and for a
 *     camera slot >= 6 + n_cols.
 *   INLIER is rule 4': both, |r| <= clip, a normal, the test on nP — EVERY drawn link counts, the base too.  A base pixel has zero
 *     joint entries and camera entries that are not: that is what tells joint 0 from a camera orbiting about joint 0's axis.
 * Per frame:  [0] BOTH pixels   [1] the truncated cost sum   [2] inliers   [3] sum over inliers of r r   [4 + c] sum of J_c r, c < 12
 *   [16 .. 93] sum of J_a J_b for a <= b, row by row over the twelve slots (0.0 0.1 .. 0.11 1.1 .. 11.11: 78 words)   [94], [95] 0.
 *   Every entry with a slot that is 0 by the rule above is exactly 0.  On the same planes [0] .. [3] and the camera block are
 *   rope_camera_normal_equations' sums and the joint block is rope_pose_normal_equations' (a base pixel adds zeros to it), each up
 *   to the order of the summation.
 * ROPE_E_ARG, with nothing enqueued and out_dev untouched, for every case of rope_pose_normal_equations but its n_joints rule, and
 * for n_joints or n_cols outside 0 .. 6, both 0, a null or misaligned joints_dev with n_joints > 0, a null or misaligned twists_dev
 * with n_cols > 0.  rope_bundle_normal_workspace (host only): the bytes of work_dev; 0 for a shape the call refuses. */
#define ROPE_BNEQ_WORDS 96
int rope_bundle_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames, int H,
                                 int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev, int n_joints,
                                 const double *twists_dev, int n_cols, float clip_m, double *out_dev, double *work_dev, void *stream);
size_t rope_bundle_normal_workspace(int n_frames, int H, int W);

/* ---- Robust weights for the depth term of the bundle polish (csrc/rope_robust.hip; prediction/refinement.py,
 * BundleRefiner(robust=...); tests/robust_ref.py restates the text below in numpy).  rope_bundle_normal_equations counts a residual
 * fully up to clip_m and not at all beyond it; here the residuals are weighted by a Huber or Tukey rule at a scale below the
 * truncation, and the scale comes from a histogram of the residuals.  Same conventions: no context, plain device pointers, the HIP
 * stream to launch on, nothing synchronised or allocated in the call, no floating-point atomics.
 *
 * rope_residual_histogram: per frame, the counts of |r| over the BOTH pixels of rope_pose_normal_equations' step 3.
 *   render_depth_dev, render_ids_dev, frame_depth_dev, n_frames, H, W, n_links, clip_m   as rope_bundle_normal_equations takes them
 *   hist_dev             n_frames x ROPE_RESID_WORDS uint32 out, DEVICE, 4-byte aligned; written completely (the call zeroes it)
 * With r = (double)R - (double)T and inv = 256.0 / (double)clip_m, one float64 division:
 *   [b], b < 256   the BOTH pixels with |r| <= clip in bin b = min(255, (int)(fabs(r) * inv)): 256 bins of clip / 256 metres
 *   [256]          the BOTH pixels that are not |r| <= clip (a NaN residual counts here)
 *   [257]          the pixels that are not BOTH.  A frame's words add up to H W.
 * Every addition is an integer addition (a workgroup counts in LDS, then adds its non-empty bins to the frame's words), so the words
 * depend neither on the order of anything nor on how the frames are cut into calls.
 * ROPE_E_ARG, with nothing enqueued and hist_dev untouched, for the shapes, n_links, clip_m and plane pointers
 * rope_pose_normal_equations refuses, and for a null or misaligned hist_dev.  ROPE_E_HIP when the runtime refuses the fill or the launch.
 *
 * rope_bundle_normal_equations_robust: rope_bundle_normal_equations with a weight per inlier.  Every argument it shares with that call
 * means the same, the words have the same layout and slots, work_dev has rope_bundle_normal_workspace_robust(n_frames, H, W) bytes
 * (the same number), and the text on the arithmetic rule, steps 1 .. 5', determinism and the refusals holds; what differs:
 *   kind                 ROPE_ROBUST_HUBER or ROPE_ROBUST_TUKEY
 *   scale_m              finite, 0 < scale_m <= clip_m (compared as float32): the scale k of the weights, metres
 * With k = (double)scale_m, r2 = r r and u = r2 / (k k), for a BOTH pixel:
 *                        HUBER                                          TUKEY
 *   within (rule 4')     fabs(r) <= clip                                fabs(r) <= k
 *   weight w             1.0 if fabs(r) <= k, else k / fabs(r)          (1.0 - u) (1.0 - u)
 *   cost share           r2 if fabs(r) <= k;                            ((k k) / 3.0) (1.0 - ((1.0 - u) (1.0 - u)) (1.0 - u)) within;
 *                        (2.0 k) fabs(r) - k k up to clip;              (k k) / 3.0 beyond, or for a NaN
 *                        (2.0 k) clip - k k beyond, or for a NaN
 * INLIER: both, within, a normal, the test on nP.  An inlier's row v = (J_0 .. J_11, r) of rope_bundle_normal_equations becomes
 * v' = s v with s = sqrt(w), one multiplication an entry, and the sums are taken over v' as that call takes them over v:
 * Per frame:  [0] BOTH pixels   [1] the sum of the cost shares   [2] inliers   [3] sum of w r r   [4 + c] sum of w J_c r
 *   [16 .. 93] sum of w J_a J_b   [94], [95] 0 — each product (s x)(s y), and added in rope_bundle_normal_equations' order.
 * HUBER with scale_m == clip_m gives the BYTES of rope_bundle_normal_equations on any planes: every w is 1.0, sqrt(1.0) is 1.0, and
 * (2 k) clip - k k is clip clip exactly.  The costs of two calls compare only at the same kind and scale.
 * ROPE_E_ARG, with nothing enqueued and out_dev untouched, for every case of rope_bundle_normal_equations, a kind that is neither, and
 * a scale_m that is not finite, not positive or above clip_m. */
#define ROPE_RESID_WORDS 258
#define ROPE_ROBUST_HUBER 1
#define ROPE_ROBUST_TUKEY 2
int rope_residual_histogram(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames, int H,
                            int W, int n_links, float clip_m, uint32_t *hist_dev, void *stream);
int rope_bundle_normal_equations_robust(const float *render_depth_dev, const uint8_t *render_ids_dev, const float *frame_depth_dev, int n_frames,
                                        int H, int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev, int n_joints,
                                        const double *twists_dev, int n_cols, float clip_m, int kind, float scale_m, double *out_dev,
                                        double *work_dev, void *stream);
size_t rope_bundle_normal_workspace_robust(int n_frames, int H, int W);

/* ---- The silhouette term (csrc/rope_silhouette.hip; prediction/refinement.py, BundleRefiner(silhouette=...);
 * tests/silhouette_ref.py restates the text below in numpy).  Depth along a ray barely changes when the robot slides across the
 * image; its outline does, and needs no depth at all.  Same conventions as above: no context, plain device pointers, the HIP stream
 * to launch on, nothing synchronised, allocated or copied in the call, no floating-point atomics.
 *
 * rope_mask_distance: the truncated signed SQUARED distance of every pixel to the boundary of its mask, in exact integers.
 *   mask_dev             N planes H x W uint8, DEVICE: non-zero = robot
 *   radius               R, 1 .. ROPE_SIL_MAX_RADIUS
 *   sd2_dev              N planes H x W int32 out, DEVICE, 4-byte aligned; written completely
 * For a pixel p, in(p) = mask[p] != 0:  m = the least dx dx + dy dy over the pixels q INSIDE THE IMAGE with |dx| <= R, |dy| <= R and
 * in(q) != in(p).  Without such a q, or with m > R R:  m = R R + 1 (FAR).  sd2[p] = -m when in(p), else +m; never 0.  The image edge
 * is not a boundary: a mask that fills the plane, or is empty, is FAR everywhere.
 * ROPE_E_ARG, with nothing enqueued, for N < 0, H or W < 1, H W >= 2^31, a radius out of range, and with N > 0 a null mask_dev or
 * sd2_dev or a misaligned sd2_dev.  N == 0 succeeds.  ROPE_E_HIP when the runtime refuses a launch.
 *
 * rope_silhouette_normal_equations: per frame, the Gauss-Newton normal equations of the distance between the render's OUTLINE and
 * the mask's boundary, over the twelve column slots of rope_bundle_normal_equations and in its ROPE_BNEQ_WORDS layout, so that the
 * same host solve takes either or a weighted sum of both.  The term is ONE-DIRECTIONAL: it measures the render's outline against
 * the mask; a part of the mask that no outline of the render comes near pulls nothing.
 *   render_depth_dev, render_ids_dev, n_frames, H, W, n_links, fx .. cy, joints_dev, n_joints (0 .. 6), twists_dev, n_cols (0 .. 6),
 *   the twelve slots, out_dev and the stream are rope_bundle_normal_equations'; what differs:
 *   sd2_dev              n_frames planes H x W int32 as rope_mask_distance writes them for the frames' masks, DEVICE, 4-byte aligned,
 *                        in place of frame_depth_dev
 *   radius               R, 1 .. ROPE_SIL_MAX_RADIUS, in place of clip_m: the truncation the field was made with
 *   work_dev             rope_silhouette_normal_workspace(n_frames, H, W) bytes, DEVICE, 8-byte aligned
 * Everything is float64 with ONE correctly rounded IEEE operation per written operation, in the order written; R[y][x] and fx .. cy
 * are widened first.  id = ids[y][x]; u x v as above.
 *   1. phi(q) = s (sqrt((double)m) - 0.5) with m = |sd2[q]| and s = -1 for sd2[q] < 0, else +1: the signed distance in pixels to the
 *      boundary, which lies midway between an inside pixel and its outside neighbour.  A FAR pixel, |sd2[q]| > R R, uses m = R R + 1.
 *   2. RENDERED: id < n_links.  CONTOUR: rendered, and at least one of the 4-neighbours INSIDE THE IMAGE is not rendered: a robot cut
 *      by the frame's edge has no contour there.  NEAR: |sd2[p]| <= R R.  INLIER: contour and near.
 *   3. e = phi(p) + 0.5: a contour pixel's centre sits half a pixel inside the render's outline, so a render that matches its mask
 *      has e = 0 on every contour pixel.
 *   4. gx = (phi(x + 1, y) - phi(x - 1, y)) / 2 when both neighbours are in the image; phi(x + 1, y) - phi(x, y) or
 *      phi(x, y) - phi(x - 1, y) with the one that is; 0 when W == 1.  gy likewise along y.
 *   5. P = (kx z, ky z, z), z = R[y][x], kx = (x - cx) / fx, ky = (y - cy) / fy: step 1 of rope_pose_normal_equations.
 *   6. Joint slot j < min(id, n_joints): u = a x (P - o).  Camera slot 6 + k, k < n_cols: c = w_k x P, u = (c.x + v_k.x, c.y + v_k.y,
 *      c.z + v_k.z), as in 5' above.
 *   7. vx = (fx (u.x - kx u.z)) / z;  vy = (fy (u.y - ky u.z)) / z;  J_c = gx vx + gy vy: what e changes by per unit of the column,
 *      the image velocity of the surface point along the field's gradient.  J_c = 0, exactly, for every other slot.
 * Per frame:  [0] contour pixels   [1] sum over contour pixels of e e (a FAR pixel adds its clamped phi: the sum is truncated by
 *   construction)   [2] inliers   [3] sum over inliers of e e   [4 + c] sum of J_c e   [16 .. 93] sum of J_a J_b, laid out as the
 *   bundle's   [94], [95] 0.
 * Determinism is rope_pose_normal_equations': a workgroup covers pixels that depend on H W alone, one partial a workgroup in
 * work_dev, a second kernel adds a frame's partials in index order; the same bytes from run to run and however the frames are cut
 * into calls.  The order of the summation is not part of the contract.
 * ROPE_E_ARG, with nothing enqueued and out_dev untouched, for every case of rope_bundle_normal_equations with sd2_dev in place of
 * frame_depth_dev, and for a radius out of range in place of its clip_m rule.  rope_silhouette_normal_workspace (host only): the
 * bytes of work_dev; 0 for a shape the call refuses. */
#define ROPE_SIL_MAX_RADIUS 16
int rope_mask_distance(const uint8_t *mask_dev, int N, int H, int W, int radius, int32_t *sd2_dev, void *stream);
int rope_silhouette_normal_equations(const float *render_depth_dev, const uint8_t *render_ids_dev, const int32_t *sd2_dev, int n_frames, int H,
                                     int W, int n_links, float fx, float fy, float cx, float cy, const double *joints_dev, int n_joints,
                                     const double *twists_dev, int n_cols, int radius, double *out_dev, double *work_dev, void *stream);
size_t rope_silhouette_normal_workspace(int n_frames, int H, int W);

/* ---- The silhouette term's second direction, mask -> render (csrc/rope_silhouette_reverse.hip; prediction/refinement.py,
 * BundleRefiner(silhouette=..., both_ways=True); tests/silhouette_reverse_ref.py restates the text below in numpy).  The term above
 * walks the RENDER's contour against a field of the mask; a part of the mask that no outline of the render comes near pulls
 * nothing there.  Here the MASK's contour is walked against a field of the render, which moves, so the field is made every round:
 * one int16 a pixel.  Same conventions as above; the words of the two directions are in the same units and slots, and add.
 *
 * rope_render_nearest: for every pixel the nearest pixel of the other state of a render's coverage, in exact integers.
 *   render_ids_dev       N planes H x W uint8, DEVICE: rope_render_batch_device's ids; rendered(p) = ids[p] < n_links
 *   n_links              1 .. 255
 *   radius               R, 1 .. ROPE_SIL_MAX_RADIUS
 *   near_dev             N planes H x W int16 out, DEVICE, 2-byte aligned; written completely
 * For a pixel p: over the pixels u INSIDE THE IMAGE with |dx| <= R, |dy| <= R (u = p + (dx, dy)) and rendered(u) != rendered(p), the
 * one with the least dx dx + dy dy; among several at that distance the FIRST IN RASTER ORDER, the smallest y, then the smallest x.
 * near[p] = (dy + 16) 33 + (dx + 16), 0 .. ROPE_SIL_NEAREST_MAX.  Without such a u, or with a least distance > R R: near[p] = -1
 * (FAR).  The image edge is not a boundary.  What follows from it: sd(p) = -(dx dx + dy dy) when rendered(p), else +(dx dx + dy dy),
 * and -(R R + 1) / +(R R + 1) for FAR — bit for bit what rope_mask_distance writes for the mask ids < n_links at the same radius.
 * ROPE_E_ARG, with nothing enqueued, for every case of rope_mask_distance (near_dev in place of sd2_dev, misaligned: odd), and for
 * n_links outside 1 .. 255.  N == 0 succeeds.  ROPE_E_HIP when the runtime refuses a launch.
 *
 * rope_silhouette_normal_equations_reverse: per frame, the normal equations of the distance between the MASK's outline and the
 * render's boundary, in the layout and slots of rope_silhouette_normal_equations.
 *   mask_dev             n_frames planes H x W uint8, DEVICE: non-zero = robot
 *   near_dev             n_frames planes H x W int16 as rope_render_nearest writes them for render_ids_dev at this n_links and
 *                        radius, DEVICE, 2-byte aligned.  A value it never writes there — out of range, or one whose anchor is
 *                        outside the image or not rendered — is read as FAR
 *   everything else      rope_silhouette_normal_equations'
 * sd(q) as above from near[q] and ids[q]; phi(q) is step 1 above on sd(q).  Every operation float64, one IEEE operation each.
 *   1'. CONTOUR: mask[p] != 0 and at least one of the 4-neighbours INSIDE THE IMAGE has mask == 0.  NEAR: |sd(p)| <= R R.  INLIER: both.
 *   2'. e = phi(p) + 0.5: step 3 mirrored — a mask contour pixel's centre sits half a pixel inside the MASK's outline, so a mask that
 *       is the render's coverage has e = 0 on every contour pixel.
 *   3'. gx, gy: step 4 on this phi.
 *   4'. The ANCHOR c, the rendered pixel whose surface point carries the boundary that p sees, with u = p + (dx, dy) of near[p]:
 *       p not rendered: c = u.  p rendered: c = u moved ONE pixel towards p along x when |dx| >= |dy|, else along y.  c is inside the
 *       image, rendered, and strictly nearer to p than u.
 *   5'. z = R[c], kx = (c.x - cx) / fx, ky = (c.y - cy) / fy, P = (kx z, ky z, z), id = ids[c]; u_c of a column as in step 6 with
 *       this id and P; vx, vy as in step 7 with kx, ky, z of c; J_c = -(gx vx + gy vy): it is the boundary that moves and not the
 *       pixel, d phi(p) / d theta = -grad phi(p) . (the image velocity of c).  J_c = 0, exactly, for every other slot.
 * Per frame: [0] contour pixels of the mask  [1] their sum of e e  [2] inliers  [3] their sum of e e  [4 + c] sum of J_c e
 *   [16 .. 93] sum of J_a J_b  [94], [95] 0.  Determinism, the workspace (rope_silhouette_normal_workspace) and ROPE_E_ARG are
 * rope_silhouette_normal_equations', with mask_dev and near_dev in place of sd2_dev (null; near_dev odd). */
#define ROPE_SIL_NEAREST_MAX 1088
int rope_render_nearest(const uint8_t *render_ids_dev, int N, int H, int W, int n_links, int radius, int16_t *near_dev, void *stream);
int rope_silhouette_normal_equations_reverse(const uint8_t *mask_dev, const int16_t *near_dev, const float *render_depth_dev,
                                             const uint8_t *render_ids_dev, int n_frames, int H, int W, int n_links, float fx, float fy,
                                             float cx, float cy, const double *joints_dev, int n_joints, const double *twists_dev,
                                             int n_cols, int radius, double *out_dev, double *work_dev, void *stream);

/* ---- The polish, natively (csrc/rope_polish.hip; prediction/refinement.py, PoseRefiner(native=True); tests/polish_ref.py restates
 * the text below with plain loops over Python floats).  What rope_pose_normal_equations leaves to its caller — the joint axes of a
 * pose, the Levenberg step, the formal variances, and the loop around them — for a host that is not Python.
 * Every float64 operation written below is ONE correctly rounded IEEE operation in the order written; nothing is fused.
 * A frame's words w are rope_pose_normal_equations': A[i][j] = A[j][i] = w[10 + 6 i - i (i - 1) / 2 + (j - i)] for i <= j, g[j] = w[4 + j].
 * idx: the joints j with bit j of active_mask set and A[j][j] > 0, ascending; p = |idx|.
 * THE ELIMINATION of a p x p system M x = b:  for k = 0 .. p - 1: the pivot row is k, replaced by each r = k + 1 .. p - 1 in turn
 * whose |M[r][k]| is greater than the greatest so far (the FIRST row with the largest magnitude; a NaN is never greater); a pivot
 * M[r][k] that is 0 or not finite makes the system SINGULAR; rows k and r are swapped; for i > k: f = M[i][k] / M[k][k], for c > k
 * ascending M[i][c] = M[i][c] - f M[k][c], and b[i] = b[i] - f b[k].  Then for i = p - 1 .. 0: s = b[i]; for c = i + 1 .. p - 1
 * ascending s = s - M[i][c] x[c]; x[i] = s / M[i][i].
 *
 * rope_joint_axes: per frame the six joints' unit axis and a point on it in camera axes: n_frames x 6 x 6 doubles in joints_dev, the
 * layout rope_pose_normal_equations takes.  One thread per frame.
 *   ctx                  a context with its robot set (rope_set_robot / rope_set_robot_mesh): the chain is the context's joint_fixed
 *                        and joint_axes and the renderer's own code (csrc/rope_fk.h): T = identity; for joint j = 0 .. 5:
 *                        T = T (F_j Rot(a_j, q_j)), the transform of link j + 1, with the device's deterministic sine and cosine
 *   q_dev                n_frames x 6 doubles, DEVICE, 8-byte aligned
 *   Rwc, tc              9 and 3 HOST doubles, finite: X_c = Rwc (X_w - tc), camera axes x right, y down, z forward
 *   joints_dev           n_frames x 36 doubles out, DEVICE, 8-byte aligned
 * With dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, after link j + 1's T:  a_w = (dot(T row r rotation part, a_j)) r = 0 .. 2;
 * o = (T[r][3] - tc[r]);  axis[r] = dot(Rwc row r, a_w);  point[r] = dot(Rwc row r, o).
 * It differs from the numpy mirror (refinement.joint_axes_camera) by the device's sine against libm's (<= 1 ulp) and the order of
 * the 3 x 3 products.  ROPE_E_ARG, with nothing enqueued, without a robot, for n_frames < 1, a null or misaligned pointer, an Rwc or
 * tc that is not finite.
 *
 * rope_levenberg_step: per frame refinement.levenberg_step and the clip to the limits.  One thread per frame.
 *   words_dev            n_frames x ROPE_NEQ_WORDS doubles, DEVICE, 8-byte aligned
 *   q_dev, lam_dev       n_frames x 6 and n_frames doubles, DEVICE, 8-byte aligned: the angles and each frame's damping (a negative
 *                        or NaN damping is the caller's business)
 *   active_mask          0 .. 63: bit j set = joint j is refined
 *   limits               12 HOST doubles lo_0 hi_0 .. lo_5 hi_5, finite, lo <= hi
 *   trial_dev            n_frames x 6 doubles out, DEVICE, 8-byte aligned; written completely
 * M = A[idx][idx] with the diagonal M[k][k] = A_kk + lam A_kk; b = -g[idx]; x by the elimination.  d[idx[k]] = x[k], every other d[j] = 0;
 * d = 0 for all six joints when p = 0, when the system is singular or when any x is not finite.
 * v = q[j] + d[j];  v = lo_j if v < lo_j;  v = hi_j if v > hi_j;  trial[j] = v.
 *
 * rope_formal_variance: per frame the SQUARE of refinement.formal_sigma (the caller takes the root: how a device rounds a float64
 * square root never enters).  One thread per frame.
 *   words_dev, active_mask   as above;   var_dev   n_frames x 6 doubles out, DEVICE, 8-byte aligned; written completely
 * var[j] = NaN for a joint outside active_mask.  Every active joint gets +inf when p = 0, when w[2] < p + 1, when the block is
 * singular, or when any variance is not finite or is negative.  Otherwise var[idx[k]] = (w[3] / (w[2] - p)) x_k[k], x_k solving
 * A[idx][idx] x = e_k by the elimination (no damping), and an active joint outside idx keeps +inf.
 * The systems of a workgroup lie in LDS (64 frames x 42 or 48 doubles); no kernel of the file uses scratch
 * (tests/test_polish_resources.py).
 * Both: ROPE_E_ARG, with nothing enqueued and the output untouched, for n_frames < 1, a null or misaligned pointer, an active_mask
 * outside 0 .. 63, and for the step limits that are null, not finite or have lo > hi.  ROPE_E_HIP when the runtime refuses the launch.
 *
 * rope_refine_poses: PoseRefiner.refine's loop.  Robot and camera are set on the context; n = min(n_links, 6) links are drawn.
 *   q                    n_frames x 6 HOST doubles: the poses to polish (finite, |q| <= 1e4)
 *   frame_depth_dev      n_frames planes H x W float32 metres, H x W the camera's (rope_set_camera), DEVICE, 4-byte aligned
 *   camera_pose6         [x, y, z, a3, a4, a5] as rope_camera_matrix takes it.  With R its camera-to-world rotation (the same host
 *                        code, libm's sine and cosine): Rwc row 0 = column 0 of R, rows 1 and 2 = the NEGATED columns 1 and 2 of R
 *                        (diag(1, -1, -1) R^T), tc = (x, y, z)
 *   fx, fy, cx, cy, clip_m   rope_pose_normal_equations';   active_mask, limits   rope_levenberg_step's
 *   iterations           >= 0: rounds at most;   damping   finite, >= 0: every frame's lam at the start
 *   work_dev             rope_refine_workspace(ctx, n_frames) bytes, DEVICE, 8-byte aligned
 *   angles_out, var_out  n_frames x 6 HOST doubles;  cost_before, cost_after, inliers_out  n_frames HOST doubles;  steps_out n_frames
 *                        int32;  words_out  n_frames x ROPE_NEQ_WORDS HOST doubles, the final systems, or NULL
 * equations(a): rope_render_batch_device at the angles a (whole frame, n links), rope_joint_axes at a, rope_pose_normal_equations
 * with n_links = n and n_joints = 6.  cost(w) = w[0] > 0 ? w[1] / w[0] : +inf.
 *   words = equations(q); cost = cost_before = cost(words); lam = damping; steps = 0.  `iterations` times: trial =
 *   rope_levenberg_step; w_t = equations(trial); per frame, if cost(w_t) < cost (strictly): q = trial, words = w_t, cost = cost(w_t),
 *   steps += 1; else lam = lam 10.  Then var = rope_formal_variance(words), inliers = words[2], cost_after = cost.
 * Systems, angles, damping, costs and step counts stay on the device between the rounds.  The raster path takes HOST rows, so each
 * round brings its n_frames x 6 trial angles down once and waits for them; nothing else crosses.  The call runs on the context's
 * stream and is complete when it returns.  Like rope_render_batch_device it uses the per-candidate buffers: resident candidates and
 * the results of the last evaluation do not survive it.  The same inputs give the same bytes, in one call or with the frames cut
 * into several.  ROPE_E_ARG, with nothing enqueued and no output written, for whatever its parts refuse, robot or camera not set,
 * iterations < 0, a damping that is negative or not finite, n_frames above 65535.
 * rope_refine_workspace (host only): the bytes of work_dev — the renders (5 bytes a pixel), rope_pose_normal_workspace, and some
 * 900 bytes a frame of state; 0 without a camera or for a batch the call refuses. */
int rope_joint_axes(rope_ctx *ctx, const double *q_dev, int n_frames, const double *Rwc, const double *tc, double *joints_dev, void *stream);
int rope_levenberg_step(const double *words_dev, const double *q_dev, const double *lam_dev, int n_frames, int active_mask, const double *limits,
                        double *trial_dev, void *stream);
int rope_formal_variance(const double *words_dev, int n_frames, int active_mask, double *var_dev, void *stream);
int rope_refine_poses(rope_ctx *ctx, const double *q, const float *frame_depth_dev, int n_frames, const double *camera_pose6, float fx, float fy,
                      float cx, float cy, int active_mask, const double *limits, float clip_m, int iterations, double damping, void *work_dev,
                      double *angles_out, double *var_out, double *cost_before, double *cost_after, int32_t *steps_out, double *inliers_out,
                      double *words_out);
size_t rope_refine_workspace(rope_ctx *ctx, int n_frames);

/* ---- The camera polish and the bundle polish, natively (csrc/rope_bundle_polish.hip; prediction/refinement.py,
 * BundleRefiner(native=True); tests/bundle_polish_ref.py restates the text below with plain loops over Python floats).  What
 * rope_bundle_normal_equations leaves to its caller: the twists of a camera pose, the pool over the frames, the Levenberg step of
 * the block-arrow system ('frame' mode) and of the pooled twelve columns ('offset' mode), their formal variances and the loop.
 * Every float64 operation written below is ONE correctly rounded IEEE operation in the order written; nothing is fused.
 * Words w (a frame's, or the pooled ones) are rope_bundle_normal_equations': A[i][j] = A[j][i] = w[16 + 12 i - i (i - 1) / 2 + (j - i)]
 * for i <= j over the twelve slots, g[c] = w[4 + c]; slots 0 .. 5 the joints, 6 .. 11 the camera.
 * THE ELIMINATION is rope_levenberg_step's rule for p <= 12 rows and SEVERAL right-hand sides b_0 .. b_(m-1): the pivot search and
 * the row swap as written there, the swap taking every right-hand side along; for i > k: f = M[i][k] / M[k][k], for c > k ascending
 * M[i][c] = M[i][c] - f M[k][c], then for every right-hand side in ascending order b[i] = b[i] - f b[k].  The back substitution
 * runs per right-hand side, in ascending order, as written there.  A system is NOT FINITE when any x of any right-hand side is not.
 * A sum "from the first product" over an ascending index is s = t_0; s = s + t_1; ...; an empty one is 0.0.
 * kc: the camera slots 6 + k with bit k of camera_mask set and a positive POOLED diagonal, ascending; nk = |kc|.
 * idx_f: the joints j with bit j of joint_mask set and a positive diagonal in frame f's OWN words, ascending; p_f = |idx_f|.
 *
 * rope_camera_twists (host only): pose6 [x, y, z, a3, a4, a5] -> Rwc9 and tc3 as rope_refine_poses derives them (R =
 *   rope_camera_matrix's camera-to-world rotation, libm's sine and cosine; Rwc row 0 = column 0 of R, rows 1 and 2 the NEGATED columns
 *   1 and 2; tc = (x, y, z)) and twists36, six rows (w, v) as rope_camera_normal_equations takes them (refinement.camera_twists):
 *   row k < 3: w = 0, v[r] = -Rwc[r][k].  Row 3 + k: v = 0, w[r] = -((Rwc[r][0] a.x + Rwc[r][1] a.y) + Rwc[r][2] a.z) with the axis
 *   a = (-sy, cy, 0) for a3, (cy cp, sy cp, -sp) for a4, (0, 0, 1) for a5; cy, sy = cos, sin of a5, cp, sp = cos, sin of a3 (libm).
 *   ROPE_E_ARG for a null pointer or a pose that is not finite; nothing is written then.
 *
 * rope_bundle_pool: pooled[k] = ((0.0 + w_0[k]) + w_1[k]) + ... over the frames in order, k < 96; one thread a word.  Bit-equal to
 *   refinement.pool_bundle.  words_dev n_frames x 96 and pooled_dev 96 doubles, DEVICE, 8-byte aligned.
 *
 * rope_bundle_schur_step: refinement.schur_step, then pose + dc and the clip of q + dq to the limits.
 *   words_dev, pooled_dev   as above (pooled_dev = rope_bundle_pool of words_dev)
 *   q_dev, pose_dev, lam_dev   n_frames x 6, 6 and 1 doubles, DEVICE, 8-byte aligned: the angles, the camera pose, ONE damping
 *   joint_mask, camera_mask    0 .. 63 each;   limits   12 HOST doubles as rope_levenberg_step takes them
 *   work_dev             rope_bundle_schur_workspace(n_frames) bytes, DEVICE, 8-byte aligned (88 doubles a frame and 48)
 *   trial_q_dev, trial_pose_dev   n_frames x 6 and 6 doubles out, DEVICE, 8-byte aligned; written completely
 *   1. Per frame with p_f > 0: D = A[idx][idx] with the diagonal a + lam a; right-hand sides the nk columns B[r][a] = A[idx[r]][kc[a]]
 *      and then g[idx]; X = D^-1 [B | g] by the elimination.  The frame is OUT when p_f = 0, D is singular or X is not finite.
 *   2. Per frame that is in: P[a][b] = sum over r ascending from the first product of B[r][a] X[r][b], b over the nk columns and g.
 *   3. S[a][b] = C[a][b] (C = pooled A[kc][kc]), the diagonal c + lam c; rhs[a] = pooled g[kc[a]].  Then for the frames that are in,
 *      in ascending order, S[a][b] = S[a][b] - P_f[a][b] and rhs[a] = rhs[a] - P_f[a][g].
 *   4. d solves S d = -rhs by the elimination; d = 0 when nk = 0, S is singular or d is not finite.  dc[kc[a] - 6] = d[a], else 0.
 *   5. Frame in: dq[idx[r]] = -(X[r][g] + s), s the sum over a ascending from the first product of X[r][a] d[a]; every other dq is 0.
 *   6. trial_pose[k] = pose[k] + dc[k];  trial_q = q + dq clipped as rope_levenberg_step clips.
 *   The per-frame work is one kernel (a frame a thread, the 6 x 13 system in LDS), steps 3 and 4 one workgroup (a thread an entry of
 *   S and rhs over the frames in order, then one thread solves), steps 5 and 6 per frame again.
 *
 * rope_bundle_schur_variance: the SQUARE of refinement.schur_sigma (the caller takes the root).
 *   var_q_dev, var_pose_dev   n_frames x 6 and 6 doubles out, DEVICE, 8-byte aligned; written completely; work_dev as above
 *   NaN for an unknown whose mask bit is clear; every other unknown is +inf unless given below.  p = nk + sum of p_f.
 *   Nothing more when p = 0 or pooled[2] < p + 1.  s2 = pooled[3] / (pooled[2] - p).
 *   Per frame with p_f > 0: X = A[idx][idx]^-1 [B | I] (no damping); OUT when singular or not finite.  Y = the B part, Ainv the I part;
 *   P[a][b] as above over the nk columns.  S0 = C less the P of the frames that are in, in ascending order.  cov = S0^-1 [I] by the
 *   elimination; when nk > 0 and S0 is singular or cov not finite, nothing more.  var_pose[kc[a] - 6] = s2 cov[a][a] when ALL of them
 *   are finite and not negative.  Frame in: t_a = sum over b from the first product of cov[a][b] Y[r][b]; u = sum over a from the first
 *   product of Y[r][a] t_a; var_q[idx[r]] = s2 (Ainv[r][r] + u) when all of the frame's are finite and not negative.
 *
 * rope_bundle_columns_step: refinement.bundle_columns_step over slot_mask (0 .. 4095, bit c = slot c) and what follows it.
 *   idx = the slots of slot_mask with a positive pooled diagonal; M = A[idx][idx], the diagonal a + lam a; b = -g[idx]; x by the
 *   elimination; d[idx[k]] = x[k], d = 0 altogether when idx is empty, M singular or x not finite.
 *   trial_pose[k] = pose[k] + d[6 + k];  trial_off[j] = off[j] + d[j];  trial_q[f][j] = q0[f][j] + trial_off[j], clipped.
 *   pose_dev, off_dev 6 doubles, q0_dev n_frames x 6, outputs likewise; the 12 x 13 system lies in LDS and one thread solves it.
 * rope_bundle_columns_variance: the SQUARE of refinement.bundle_columns_sigma -> 12 doubles: NaN outside slot_mask; +inf when idx is
 *   empty, pooled[2] < p + 1, A[idx][idx] is singular, A^-1 (right-hand sides I) not finite, or any variance not finite or negative;
 *   else var[idx[k]] = (pooled[3] / (pooled[2] - p)) x_k[k], and a slot of slot_mask outside idx keeps +inf.
 * All of the above: ROPE_E_ARG, with nothing enqueued and the outputs untouched, for n_frames < 1, a null or misaligned pointer, a
 * mask out of range, limits that are null, not finite or have lo > hi.  ROPE_E_HIP when the runtime refuses a launch.  Nothing is
 * synchronised.  No kernel of the file uses scratch (tests/test_bundle_polish_resources.py).
 *
 * rope_refine_bundle: BundleRefiner.refine's depth loop.  Robot and camera are set on the context; n = min(n_links, 6) links.
 *   mode                 ROPE_BUNDLE_FRAME or ROPE_BUNDLE_OFFSET
 *   camera_pose6, q      6 and n_frames x 6 HOST doubles: the start (finite, |q| <= 1e4)
 *   frame_depth_dev      n_frames planes H x W float32 metres, H x W the camera's, DEVICE, 4-byte aligned
 *   fx, fy, cx, cy, znear, zfar   rope_camera_matrix's, as doubles; znear and zfar those of rope_set_camera.  The equations take
 *                        fx .. cy rounded to float32
 *   joint_mask, camera_mask   0 .. 63, not both 0.  joint_mask 0 is the camera polish alone
 *   limits, clip_m, iterations, damping   rope_refine_poses';  ONE damping for the whole system
 *   work_dev             rope_refine_bundle_workspace(ctx, n_frames) bytes, DEVICE, 8-byte aligned
 *   pose_out, offsets_out, var_pose_out   6 HOST doubles each;  angles_out, frame_cost_out  n_frames x 6 and n_frames;
 *   var_joints_out       FRAME: n_frames x 6 (the angles'); OFFSET: 6 (the offsets');  costs_out  3: cost before, after, pooled inliers;
 *   steps_out            1 int32;  words_out  n_frames x 96 HOST doubles, the final systems, or NULL
 * equations(pose, a): rope_camera_twists(pose); a render of the rows a, every row under P V = rope_camera_matrix(pose, fx .. zfar)
 *   (rope_render_batch_device; the context's own camera is not moved); rope_joint_axes at a when joint_mask != 0 (n_joints 6, else 0);
 *   the twists for every frame when camera_mask != 0 (n_cols 6, else 0); rope_bundle_normal_equations; rope_bundle_pool.
 *   cost(pooled) = pooled[0] > 0 ? pooled[1] / pooled[0] : +inf.
 *   words, pooled = equations(pose, q); cost = cost_before; lam = damping; off = 0; q0 = q.  `iterations` times: the trial by
 *   rope_bundle_schur_step (FRAME; off stays) or rope_bundle_columns_step with slot_mask = joint_mask | camera_mask << 6 (OFFSET);
 *   the equations there; a kernel keeps the trial when its pooled cost is strictly smaller (words, pooled, q, off, pose, cost,
 *   steps += 1), else lam = lam 10.  Then the variances, frame_cost[f] = cost(words_f), offsets = off (NaN in FRAME).
 * Between rounds only the trial pose and the trial angles come down (the raster path takes HOST rows); one copy at the end brings
 * the results.  The call runs on the context's stream, is complete when it returns, uses the per-candidate buffers as
 * rope_render_batch_device does, and gives the same bytes for the same inputs.  The silhouette term is not part of it.
 * ROPE_E_ARG, with nothing enqueued and no output written, for whatever its parts refuse, robot or camera not set, a mode that is
 * neither, both masks 0, iterations < 0, a damping that is negative or not finite, n_frames above 65535.
 * rope_refine_bundle_workspace (host only): the bytes of work_dev; 0 without a camera or for a batch the call refuses. */
#define ROPE_BUNDLE_FRAME 0
#define ROPE_BUNDLE_OFFSET 1
int rope_camera_twists(const double *pose6, double *Rwc9, double *tc3, double *twists36);
int rope_bundle_pool(const double *words_dev, int n_frames, double *pooled_dev, void *stream);
size_t rope_bundle_schur_workspace(int n_frames);
int rope_bundle_schur_step(const double *words_dev, const double *pooled_dev, const double *q_dev, const double *pose_dev, const double *lam_dev,
                           int n_frames, int joint_mask, int camera_mask, const double *limits, void *work_dev, double *trial_q_dev,
                           double *trial_pose_dev, void *stream);
int rope_bundle_schur_variance(const double *words_dev, const double *pooled_dev, int n_frames, int joint_mask, int camera_mask, void *work_dev,
                               double *var_q_dev, double *var_pose_dev, void *stream);
int rope_bundle_columns_step(const double *pooled_dev, const double *lam_dev, int slot_mask, const double *pose_dev, const double *off_dev,
                             const double *q0_dev, int n_frames, const double *limits, double *trial_pose_dev, double *trial_off_dev,
                             double *trial_q_dev, void *stream);
int rope_bundle_columns_variance(const double *pooled_dev, int slot_mask, double *var_dev, void *stream);
int rope_refine_bundle(rope_ctx *ctx, int mode, const double *camera_pose6, const double *q, const float *frame_depth_dev, int n_frames, double fx,
                       double fy, double cx, double cy, double znear, double zfar, int joint_mask, int camera_mask, const double *limits,
                       float clip_m, int iterations, double damping, void *work_dev, double *pose_out, double *angles_out, double *offsets_out,
                       double *var_pose_out, double *var_joints_out, double *costs_out, int32_t *steps_out, double *frame_cost_out,
                       double *words_out);
size_t rope_refine_bundle_workspace(rope_ctx *ctx, int n_frames);

/* Phase-skipping switches for kernel ablations (rope_debug_skip) exist only in the profiling build of the library
 * (librope_hip_profile.so, `python tools/build_variants.py profile`, -DROPE_PROFILE); this library does not export them. */

#ifdef __cplusplus
}
#endif
#endif
