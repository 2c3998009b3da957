// rope_train.hip — the steps of a Mask R-CNN training step that are not library convolutions, for gfx950: the RPN targets
// (build_rpn_targets), the detection targets (DetectionTargetLayer) and a float32 pyramid RoIAlign with its backward pass.
// The host side is rope_s3d_amd/training.py, which also holds the host restatements every kernel here is tested against;
// these entry points take plain device pointers and a HIP stream (include/rope_s3d.h).
//
// Reference: the Matterport Mask R-CNN that PixelLib 0.5.6 trains (train.py:29-57 of the reference):
//   mrcnn/model.py build_rpn_targets      numpy float64, pixel coordinates
//   mrcnn/model.py DetectionTargetLayer   TF float32, normalised coordinates
//   mrcnn/model.py PyramidROIAlign        tf.image.crop_and_resize (bilinear)
// Random choices (np.random.choice, tf.random_shuffle) are replaced by per-element keys from one seeded host generator: a
// kernel keeps the elements with the smallest (key, index) pairs.  The file is built with -ffp-contract=off:
// one IEEE operation per written step, in the order of the host restatement.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rope_s3d.h"

namespace {

constexpr int RPN_THREADS = 256;
constexpr int SELECT_THREADS = 1024;
constexpr int RPN_POS_MAX = 128, RPN_ANCHORS_PER_IMAGE = 256;   // RPN_TRAIN_ANCHORS_PER_IMAGE and half of it
constexpr int ANCHOR_BITS = 17;                                   // anchors per frame < 2^17 (65 472 at 512)
constexpr int ROI_THREADS = 256;
constexpr int ROI_MAX = 2048, ROI_BITS = 11;                      // proposals per frame (POST_NMS_ROIS_TRAINING = 2000)
constexpr int TRAIN_ROIS = 200, ROI_POS_MAX = 66;                 // TRAIN_ROIS_PER_IMAGE, int(200 * 0.33)
constexpr int MASK = 28;                                          // MASK_SHAPE
constexpr int GT_MAX = 100;                                       // MAX_GT_INSTANCES

// ------------------------------------------------------------ RPN targets -----
// utils.compute_iou(gt, anchors, gt_area, anchor_areas): the operation order of the numpy restatement
__device__ __forceinline__ double iou64(const double *g, const double ga, const double *a)
{
    const double y1 = fmax(g[0], a[0]), y2 = fmin(g[2], a[2]);
    const double x1 = fmax(g[1], a[1]), x2 = fmin(g[3], a[3]);
    const double inter = fmax(x2 - x1, 0.0) * fmax(y2 - y1, 0.0);
    const double aa = (a[2] - a[0]) * (a[3] - a[1]);
    return inter / ((ga + aa) - inter);
}

// pass 1: every anchor's best GT (first maximum, np.argmax) and every GT's best IoU over the anchors (atomic max of the bit
// pattern: IoUs are >= 0, where the order of doubles is that of their bits)
__global__ void __launch_bounds__(RPN_THREADS)
rpn_iou_kernel(const double *__restrict__ anchors, int n_anchors, const double *__restrict__ gt, const int32_t *__restrict__ gt_count,
               int gt_stride, double *__restrict__ anchor_max, int32_t *__restrict__ anchor_arg, unsigned long long *__restrict__ gt_max)
{
    __shared__ double s_gt[GT_MAX][4];
    __shared__ double s_area[GT_MAX];
    __shared__ unsigned long long s_max[GT_MAX];
    const int f = blockIdx.y, tid = threadIdx.x, a = blockIdx.x * RPN_THREADS + tid;
    const int G = gt_count[f];
    for (int g = tid; g < G; g += RPN_THREADS) {
        for (int c = 0; c < 4; c++) s_gt[g][c] = gt[((size_t)f * gt_stride + g) * 4 + c];
        s_area[g] = (s_gt[g][2] - s_gt[g][0]) * (s_gt[g][3] - s_gt[g][1]);
        s_max[g] = 0ull;
    }
    __syncthreads();
    if (a < n_anchors) {
        double box[4];
        for (int c = 0; c < 4; c++) box[c] = anchors[(size_t)a * 4 + c];
        double best = 0.0;
        int arg = 0;
        for (int g = 0; g < G; g++) {
            const double v = iou64(s_gt[g], s_area[g], box);
            if (g == 0 || v > best) { best = v; arg = g; }
            atomicMax(&s_max[g], (unsigned long long)__double_as_longlong(v));
        }
        anchor_max[(size_t)f * n_anchors + a] = best;        // no GT: 0, every anchor a negative
        anchor_arg[(size_t)f * n_anchors + a] = arg;
    }
    __syncthreads();
    for (int g = tid; g < G; g += RPN_THREADS) atomicMax(&gt_max[(size_t)f * gt_stride + g], s_max[g]);
}

// pass 2: the three-step rule — negative below 0.3, then every anchor at a GT's maximum (ties included), then >= 0.7
__global__ void __launch_bounds__(RPN_THREADS)
rpn_label_kernel(const double *__restrict__ anchors, int n_anchors, const double *__restrict__ gt, const int32_t *__restrict__ gt_count,
                 int gt_stride, const double *__restrict__ anchor_max, const unsigned long long *__restrict__ gt_max,
                 int32_t *__restrict__ match)
{
    __shared__ double s_gt[GT_MAX][4];
    __shared__ double s_area[GT_MAX];
    __shared__ double s_max[GT_MAX];
    const int f = blockIdx.y, tid = threadIdx.x, a = blockIdx.x * RPN_THREADS + tid;
    const int G = gt_count[f];
    for (int g = tid; g < G; g += RPN_THREADS) {
        for (int c = 0; c < 4; c++) s_gt[g][c] = gt[((size_t)f * gt_stride + g) * 4 + c];
        s_area[g] = (s_gt[g][2] - s_gt[g][0]) * (s_gt[g][3] - s_gt[g][1]);
        s_max[g] = __longlong_as_double((long long)gt_max[(size_t)f * gt_stride + g]);
    }
    __syncthreads();
    if (a >= n_anchors) return;
    const double m = anchor_max[(size_t)f * n_anchors + a];
    int lab = m < 0.3 ? -1 : 0;
    double box[4];
    for (int c = 0; c < 4; c++) box[c] = anchors[(size_t)a * 4 + c];
    for (int g = 0; g < G; g++)
        if (iou64(s_gt[g], s_area[g], box) == s_max[g]) lab = 1;
    if (m >= 0.7) lab = 1;
    match[(size_t)f * n_anchors + a] = lab;
}

__device__ __forceinline__ int block_sum(int v, int *s_cnt)
{
    __syncthreads();
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    if (v) atomicAdd(s_cnt, v);
    __syncthreads();
    return *s_cnt;
}

// Keep the `keep` elements labelled `lab` with the smallest (key, index); the others of that label become 0 (neutral).
// The keep-th smallest composite key is found by bisection over its 49 bits (one block-wide count per step).
__device__ void keep_smallest(int32_t *match, const uint32_t *keys, int n, int lab, int total, int keep, int *s_cnt)
{
    if (total <= keep) return;
    unsigned long long lo = 0, hi = (1ull << (32 + ANCHOR_BITS)) - 1ull;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        int c = 0;
        for (int a = threadIdx.x; a < n; a += SELECT_THREADS)
            c += (match[a] == lab && (((unsigned long long)keys[a] << ANCHOR_BITS) | (unsigned)a) <= mid) ? 1 : 0;
        if (block_sum(c, s_cnt) >= keep) hi = mid; else lo = mid + 1;
    }
    __syncthreads();
    for (int a = threadIdx.x; a < n; a += SELECT_THREADS)
        if (match[a] == lab && (((unsigned long long)keys[a] << ANCHOR_BITS) | (unsigned)a) > lo) match[a] = 0;
    __syncthreads();
}

// pass 3, one workgroup per frame: the balanced subsample, then the deltas of the positives packed in anchor order
__global__ void __launch_bounds__(SELECT_THREADS)
rpn_select_kernel(const double *__restrict__ anchors, int n_anchors, const double *__restrict__ gt, int gt_stride,
                  const uint32_t *__restrict__ keys, const int32_t *__restrict__ anchor_arg, int32_t *__restrict__ match_all,
                  double *__restrict__ bbox_all)
{
    __shared__ int s_cnt;
    __shared__ int s_wave[SELECT_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t *const match = match_all + (size_t)f * n_anchors;
    const uint32_t *const key = keys + (size_t)f * n_anchors;
    double *const bbox = bbox_all + (size_t)f * RPN_ANCHORS_PER_IMAGE * 4;
    int p = 0, q = 0;
    for (int a = tid; a < n_anchors; a += SELECT_THREADS) { p += match[a] == 1; q += match[a] == -1; }
    const int n_pos = block_sum(p, &s_cnt);
    const int n_neg = block_sum(q, &s_cnt);
    keep_smallest(match, key, n_anchors, 1, n_pos, RPN_POS_MAX, &s_cnt);
    const int kept_pos = n_pos < RPN_POS_MAX ? n_pos : RPN_POS_MAX;
    keep_smallest(match, key, n_anchors, -1, n_neg, RPN_ANCHORS_PER_IMAGE - kept_pos, &s_cnt);
    for (int i = tid; i < RPN_ANCHORS_PER_IMAGE * 4; i += SELECT_THREADS) bbox[i] = 0.0;
    __syncthreads();
    // positives in anchor order: rank = positives before it (wave ballots, then the waves' counts)
    int base = 0;
    for (int a0 = 0; a0 < n_anchors; a0 += SELECT_THREADS) {
        const int a = a0 + tid;
        const bool pos = a < n_anchors && match[a] == 1;
        const unsigned long long bal = __ballot(pos);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = base, chunk = 0;
        for (int w = 0; w < SELECT_THREADS / 64; w++) { if (w < wave) before += s_wave[w]; chunk += s_wave[w]; }
        before += __popcll(bal & ((1ull << lane) - 1ull));
        if (pos) {
            const double *an = anchors + (size_t)a * 4;
            const double *g = gt + ((size_t)f * gt_stride + anchor_arg[(size_t)f * n_anchors + a]) * 4;
            const double gh = g[2] - g[0], gw = g[3] - g[1];
            const double gcy = g[0] + 0.5 * gh, gcx = g[1] + 0.5 * gw;
            const double ah = an[2] - an[0], aw = an[3] - an[1];
            const double acy = an[0] + 0.5 * ah, acx = an[1] + 0.5 * aw;
            double *row = bbox + (size_t)before * 4;
            row[0] = ((gcy - acy) / ah) / 0.1;                 // / RPN_BBOX_STD_DEV
            row[1] = ((gcx - acx) / aw) / 0.1;
            row[2] = log(gh / ah) / 0.2;
            row[3] = log(gw / aw) / 0.2;
        }
        base += chunk;
        __syncthreads();
    }
}

// ---------------------------------------------------------- detection targets -----
// utils.overlaps_graph(proposals, gt_boxes): float32, the order of the graph
__device__ __forceinline__ float iou32(const float4 b1, const float4 b2)
{
    const float y1 = fmaxf(b1.x, b2.x), x1 = fmaxf(b1.y, b2.y), y2 = fminf(b1.z, b2.z), x2 = fminf(b1.w, b2.w);
    const float inter = fmaxf(x2 - x1, 0.0f) * fmaxf(y2 - y1, 0.0f);
    const float a1 = (b1.z - b1.x) * (b1.w - b1.y), a2 = (b2.z - b2.x) * (b2.w - b2.y);
    return inter / ((a1 + a2) - inter);
}

// One workgroup per frame.  rois / deltas / classes / masks: TRAIN_ROIS rows per frame, positives first (by key), then the
// negatives (by key), then zero rows.
__global__ void __launch_bounds__(ROI_THREADS)
roi_targets_kernel(const float4 *__restrict__ proposals, const int32_t *__restrict__ prop_count, int prop_stride,
                   const float4 *__restrict__ gt, const int32_t *__restrict__ gt_class, const int32_t *__restrict__ gt_count, int gt_stride,
                   const uint8_t *__restrict__ gt_masks, int mask_h, int mask_w, const uint32_t *__restrict__ keys, float inv_ratio,
                   float4 *__restrict__ rois, int32_t *__restrict__ cls, float4 *__restrict__ deltas, float *__restrict__ masks)
{
    __shared__ float4 s_gt[GT_MAX];
    __shared__ unsigned long long s_key[ROI_MAX];
    __shared__ int8_t s_flag[ROI_MAX];
    __shared__ uint8_t s_arg[ROI_MAX];
    __shared__ int16_t s_prop[TRAIN_ROIS];
    __shared__ int s_cnt;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int R = prop_count[f], G = gt_count[f];
    const float4 *const prop = proposals + (size_t)f * prop_stride;
    for (int g = tid; g < G; g += ROI_THREADS) s_gt[g] = gt[(size_t)f * gt_stride + g];
    for (int r = tid; r < TRAIN_ROIS; r += ROI_THREADS) s_prop[r] = -1;
    __syncthreads();
    int p = 0, q = 0;
    for (int i = tid; i < R; i += ROI_THREADS) {
        const float4 b = prop[i];
        float best = -__builtin_inff();                    // reduce_max over no GT
        int arg = 0;
        for (int g = 0; g < G; g++) {
            const float v = iou32(b, s_gt[g]);
            if (v > best) { best = v; arg = g; }           // tf.argmax: the first maximum
        }
        const int8_t fl = best >= 0.5f ? 1 : (best < 0.5f ? 2 : 0);
        s_flag[i] = fl; s_arg[i] = (uint8_t)arg;
        s_key[i] = ((unsigned long long)keys[(size_t)f * prop_stride + i] << ROI_BITS) | (unsigned)i;
        p += fl == 1; q += fl == 2;
    }
    const int n_pos = block_sum(p, &s_cnt);
    const int n_neg = block_sum(q, &s_cnt);
    const int P = n_pos < ROI_POS_MAX ? n_pos : ROI_POS_MAX;
    const int Nq = (int)(inv_ratio * (float)P) - P;        // tf.cast(r * tf.cast(positive_count, float32), int32) - positive_count
    const int N = n_neg < Nq ? n_neg : Nq;
    for (int i = tid; i < R; i += ROI_THREADS) {
        const int fl = s_flag[i];
        if (!fl) continue;
        const unsigned long long k = s_key[i];
        int rank = 0;
        for (int j = 0; j < R; j++) rank += (s_flag[j] == fl && s_key[j] < k);
        if (fl == 1 && rank < P) s_prop[rank] = (int16_t)i;
        if (fl == 2 && rank < N) s_prop[P + rank] = (int16_t)i;
    }
    __syncthreads();
    const size_t ro = (size_t)f * TRAIN_ROIS;
    for (int r = tid; r < TRAIN_ROIS; r += ROI_THREADS) {
        const int i = s_prop[r];
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        int c = 0;
        if (r < P) {                                       // box_refinement_graph(positive_rois, roi_gt_boxes) / BBOX_STD_DEV
            const float4 b = prop[i], g = s_gt[s_arg[i]];
            const float h = b.z - b.x, w = b.w - b.y;
            const float cy = b.x + 0.5f * h, cx = b.y + 0.5f * w;
            const float gh = g.z - g.x, gw = g.w - g.y;
            const float gcy = g.x + 0.5f * gh, gcx = g.y + 0.5f * gw;
            // the log in float64, rounded to float32: the same bits as the host restatement's
            d = make_float4(((gcy - cy) / h) / 0.1f, ((gcx - cx) / w) / 0.1f, (float)log((double)(gh / h)) / 0.2f,
                            (float)log((double)(gw / w)) / 0.2f);
            c = gt_class[(size_t)f * gt_stride + s_arg[i]];
        }
        rois[ro + r] = i >= 0 ? prop[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        deltas[ro + r] = d;
        cls[ro + r] = c;
    }
    // mask targets: round(crop_and_resize(gt mask, positive roi, 28 x 28)), zero rows after the positives
    const float hm1 = (float)(mask_h - 1), wm1 = (float)(mask_w - 1);
    for (int e = tid; e < TRAIN_ROIS * MASK * MASK; e += ROI_THREADS) {
        const int r = e / (MASK * MASK), y = (e / MASK) % MASK, x = e % MASK;
        float v = 0.0f;
        if (r < P) {
            const int i = s_prop[r];
            const float4 b = prop[i];
            const uint8_t *m = gt_masks + ((size_t)f * gt_stride + s_arg[i]) * mask_h * mask_w;
            const float hs = ((b.z - b.x) * hm1) / (float)(MASK - 1), ws = ((b.w - b.y) * wm1) / (float)(MASK - 1);
            const float in_y = b.x * hm1 + (float)y * hs, in_x = b.y * wm1 + (float)x * ws;
            if (in_y >= 0.0f && in_y <= hm1 && in_x >= 0.0f && in_x <= wm1) {
                const int t = (int)floorf(in_y), bo = (int)ceilf(in_y), l = (int)floorf(in_x), rr = (int)ceilf(in_x);
                const float yl = in_y - (float)t, xl = in_x - (float)l;
                const float tl = m[t * mask_w + l], tr = m[t * mask_w + rr], bl = m[bo * mask_w + l], br = m[bo * mask_w + rr];
                const float top = tl + (tr - tl) * xl, bot = bl + (br - bl) * xl;
                v = rintf(top + (bot - top) * yl);          // tf.round: half to even
            }
        }
        masks[(ro + r) * MASK * MASK + y * MASK + x] = v;
    }
}

// ------------------------------------------------------------ RoIAlign f32 -----
struct Levels { int H[4], W[4]; long long off[4]; };

struct Sample {
    long long r00, r10, r01, r11;                        // table rows of the four corners
    float omwy, wy, omwx, wx, inside;
};

// maskrcnn.py::_roi_align's float32 steps for sample (py, px) of box k: level, position, corners, weights
__device__ __forceinline__ Sample sample_at(const float4 b, int frame, const Levels &lv, float inv_level_unit, float ty, float tx)
{
    const float h = b.z - b.x, w = b.w - b.y;
    const float lf = fminf(fmaxf(rintf(4.0f + log2f(sqrtf(fmaxf(h * w, 1e-12f)) * inv_level_unit)), 2.0f), 5.0f);
    const int li = (int)lf - 2;
    const int Hf = lv.H[li], Wf = lv.W[li];
    const long long base = lv.off[li] + (long long)frame * ((long long)Hf * Wf);
    const float hm = (float)(Hf - 1), wm = (float)(Wf - 1);
    const float ys = (b.x + ty * (b.z - b.x)) * hm, xs = (b.y + tx * (b.w - b.y)) * wm;
    const float y0 = floorf(ys), x0 = floorf(xs);
    Sample s;
    s.wy = ys - y0; s.omwy = 1.0f - s.wy;
    s.wx = xs - x0; s.omwx = 1.0f - s.wx;
    s.inside = (ys >= 0.0f && ys <= hm && xs >= 0.0f && xs <= wm) ? 1.0f : 0.0f;
    const long long y0i = (long long)y0, x0i = (long long)x0;
    const long long y0c = min(max(y0i, 0ll), (long long)(Hf - 1)), y1c = min(max(y0i + 1, 0ll), (long long)(Hf - 1));
    const long long x0c = min(max(x0i, 0ll), (long long)(Wf - 1)), x1c = min(max(x0i + 1, 0ll), (long long)(Wf - 1));
    s.r00 = base + y0c * Wf + x0c; s.r10 = base + y1c * Wf + x0c;
    s.r01 = base + y0c * Wf + x1c; s.r11 = base + y1c * Wf + x1c;
    return s;
}

// One workgroup per (box, sample row), one wave per sample, lanes over channels (256 contiguous bytes per wave-instruction).
// out: K x pool x pool x C float32.
__global__ void __launch_bounds__(256)
roi_align_f32_kernel(const float *__restrict__ rows, const float4 *__restrict__ boxes, const int32_t *__restrict__ frame, Levels lv,
                     int channels, int pool, float inv_level_unit, const float *__restrict__ t, float *__restrict__ out)
{
    const int k = blockIdx.x, py = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float4 b = boxes[k];
    for (int px = wave; px < pool; px += 4) {
        const Sample s = sample_at(b, frame[k], lv, inv_level_unit, t[py], t[px]);
        float *o = out + (((size_t)k * pool + py) * pool + px) * channels;
        for (int c = lane; c < channels; c += 64) {
            const float g00 = rows[s.r00 * channels + c], g10 = rows[s.r10 * channels + c];
            const float g01 = rows[s.r01 * channels + c], g11 = rows[s.r11 * channels + c];
            // (g00 (1 - wy) + g10 wy) (1 - wx) + (g01 (1 - wy) + g11 wy) wx, then x inside
            const float left = (g00 * s.omwy + g10 * s.wy) * s.omwx;
            const float right = (g01 * s.omwy + g11 * s.wy) * s.wx;
            o[c] = (left + right) * s.inside;
        }
    }
}

// The transpose: every sample's gradient row, times its four bilinear weights, added into the grad-rows table with global
// float atomics (no-return global_atomic_add_f32).  Samples outside the map add nothing.
__global__ void __launch_bounds__(256)
roi_align_f32_bwd_kernel(const float *__restrict__ grad_out, const float4 *__restrict__ boxes, const int32_t *__restrict__ frame, Levels lv,
                         int channels, int pool, float inv_level_unit, const float *__restrict__ t, float *__restrict__ grad_rows)
{
    const int k = blockIdx.x, py = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float4 b = boxes[k];
    for (int px = wave; px < pool; px += 4) {
        const Sample s = sample_at(b, frame[k], lv, inv_level_unit, t[py], t[px]);
        if (s.inside == 0.0f) continue;
        const float *go = grad_out + (((size_t)k * pool + py) * pool + px) * channels;
        for (int c = lane; c < channels; c += 64) {
            const float g = go[c];
            const float gl = g * s.omwx, gr = g * s.wx;
            unsafeAtomicAdd(grad_rows + s.r00 * channels + c, gl * s.omwy);
            unsafeAtomicAdd(grad_rows + s.r10 * channels + c, gl * s.wy);
            unsafeAtomicAdd(grad_rows + s.r01 * channels + c, gr * s.omwy);
            unsafeAtomicAdd(grad_rows + s.r11 * channels + c, gr * s.wy);
        }
    }
}

int read_levels(const int32_t *level_hw, const int64_t *level_off, Levels &lv)
{
    for (int l = 0; l < 4; l++) {
        lv.H[l] = level_hw[2 * l]; lv.W[l] = level_hw[2 * l + 1]; lv.off[l] = level_off[l];
        if (lv.H[l] < 1 || lv.W[l] < 1 || lv.off[l] < 0) return ROPE_E_ARG;
    }
    return ROPE_OK;
}

}  // namespace

extern "C" int rope_seg_rpn_targets(const double *anchors, int n_anchors, const double *gt_boxes, const int32_t *gt_count, int gt_stride,
                                    int n_frames, const uint32_t *keys, double *anchor_max, int32_t *anchor_arg, uint64_t *gt_max,
                                    int32_t *match, double *bbox, void *stream)
{
    if (!anchors || !gt_boxes || !gt_count || !keys || !anchor_max || !anchor_arg || !gt_max || !match || !bbox) return ROPE_E_ARG;
    if (n_anchors < 1 || n_anchors >= (1 << ANCHOR_BITS) || n_frames < 1 || gt_stride < 1 || gt_stride > GT_MAX) return ROPE_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(gt_max, 0, (size_t)n_frames * gt_stride * sizeof(uint64_t), st) != hipSuccess) return ROPE_E_HIP;
    const dim3 grid((n_anchors + RPN_THREADS - 1) / RPN_THREADS, n_frames);
    hipLaunchKernelGGL(rpn_iou_kernel, grid, dim3(RPN_THREADS), 0, st, anchors, n_anchors, gt_boxes, gt_count, gt_stride, anchor_max,
                       anchor_arg, reinterpret_cast<unsigned long long *>(gt_max));
    hipLaunchKernelGGL(rpn_label_kernel, grid, dim3(RPN_THREADS), 0, st, anchors, n_anchors, gt_boxes, gt_count, gt_stride, anchor_max,
                       reinterpret_cast<const unsigned long long *>(gt_max), match);
    hipLaunchKernelGGL(rpn_select_kernel, dim3(n_frames), dim3(SELECT_THREADS), 0, st, anchors, n_anchors, gt_boxes, gt_stride, keys,
                       anchor_arg, match, bbox);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" int rope_seg_roi_targets(const float *proposals, const int32_t *prop_count, int prop_stride, const float *gt_boxes,
                                    const int32_t *gt_class, const int32_t *gt_count, int gt_stride, const uint8_t *gt_masks, int mask_h,
                                    int mask_w, int n_frames, const uint32_t *keys, float inv_positive_ratio, float *rois, int32_t *class_ids,
                                    float *deltas, float *masks, void *stream)
{
    if (!proposals || !prop_count || !gt_boxes || !gt_class || !gt_count || !gt_masks || !keys || !rois || !class_ids || !deltas || !masks)
        return ROPE_E_ARG;
    if (n_frames < 1 || prop_stride < 1 || prop_stride > ROI_MAX || gt_stride < 1 || gt_stride > GT_MAX || mask_h < 2 || mask_w < 2)
        return ROPE_E_ARG;
    hipLaunchKernelGGL(roi_targets_kernel, dim3(n_frames), dim3(ROI_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(proposals), prop_count, prop_stride, reinterpret_cast<const float4 *>(gt_boxes), gt_class,
                       gt_count, gt_stride, gt_masks, mask_h, mask_w, keys, inv_positive_ratio, reinterpret_cast<float4 *>(rois), class_ids,
                       reinterpret_cast<float4 *>(deltas), masks);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" int rope_seg_roi_align_float(const float *rows, const float *boxes, const int32_t *frame, const int32_t *level_hw,
                                      const int64_t *level_off, int n_boxes, int channels, int pool, float inv_level_unit, const float *t,
                                      float *out, void *stream)
{
    if (!rows || !boxes || !frame || !level_hw || !level_off || !t || !out || n_boxes < 1 || pool < 1 || channels < 1) return ROPE_E_ARG;
    Levels lv;
    if (read_levels(level_hw, level_off, lv) != ROPE_OK) return ROPE_E_ARG;
    hipLaunchKernelGGL(roi_align_f32_kernel, dim3(n_boxes, pool), dim3(256), 0, (hipStream_t)stream, rows,
                       reinterpret_cast<const float4 *>(boxes), frame, lv, channels, pool, inv_level_unit, t, out);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}

extern "C" int rope_seg_roi_align_backward(const float *grad_out, const float *boxes, const int32_t *frame, const int32_t *level_hw,
                                           const int64_t *level_off, int n_boxes, int channels, int pool, float inv_level_unit,
                                           const float *t, float *grad_rows, void *stream)
{
    if (!grad_out || !boxes || !frame || !level_hw || !level_off || !t || !grad_rows || n_boxes < 1 || pool < 1 || channels < 1)
        return ROPE_E_ARG;
    Levels lv;
    if (read_levels(level_hw, level_off, lv) != ROPE_OK) return ROPE_E_ARG;
    hipLaunchKernelGGL(roi_align_f32_bwd_kernel, dim3(n_boxes, pool), dim3(256), 0, (hipStream_t)stream, grad_out,
                       reinterpret_cast<const float4 *>(boxes), frame, lv, channels, pool, inv_level_unit, t, grad_rows);
    return hipGetLastError() == hipSuccess ? ROPE_OK : ROPE_E_HIP;
}
