// The FCOS criterion, forward only (fcos_utils/fcos.py:523-570 the matching, :44-178 the six terms, fcos_utils/utils.py the
// GIoU loss, det_utils.py:233-264 encode_single, torchvision's sigmoid_focal_loss), on the head tensors as the detector leaves
// them (cls_lr, reg_ctr, ext per level, NHWC).  Built with -ffp-contract=off: the matching is compared bit for bit with the
// reference's chain of float32 torch ops, and tests/fcos_loss_ref.py states the terms one rounding per operation.
//
//   fcos_loss_kernel         grid = ceil(P / 1024) chunks x n images (the chunking of fcos_candidates_count_kernel).  The image's
//                            <= 64 scaled ground-truth rows sit in LDS; a point loops over them in index order (the first index
//                            wins a tie), then adds its share of the six terms.  Wave sums by __shfl_xor, the 16 waves through LDS
//                            in wave order, ONE store of the chunk's seven partial sums (six terms, the foreground count) widened
//                            to double.
//   fcos_loss_reduce_kernel  one workgroup: per image the chunk partials in chunk order -> terms, fg; then the images in image
//                            order -> the six dict values over max(1, foreground).
// No atomics, no inter-workgroup waiting, a fixed order: two runs give the same bytes, and image i of a batch gives the bytes of
// that image launched alone.
#include "hn_common.h"
#include "fcos_points.h"

#pragma clang fp contract(off)

namespace {

using hn_fcos::LevelTable;

constexpr int kChunk = 1024;
constexpr int kSums = 8;   // six terms, the foreground count, one pad: 64 bytes per chunk

struct ExtLevels {
  const float* p[HN_FCOS_MAX_LEVELS];   // all null: no ext heads
};

struct GtTables {
  const float* boxes;    // [n][G][4], scaled to the canvas
  const int32_t* labels; // [n][G]
  const float* info;     // [n][G][5] = (contactstate, handside, mag, dx, dy)
  const int32_t* count;  // [n]
  int G;
};

// alpha_t * softplus(z) * sigmoid(z)^2 with z = -x on the target column and x elsewhere: torchvision's
// ce * (1 - p_t)^2 * alpha_t (alpha 0.25, gamma 2) without the cancellation in 1 - p_t
__device__ __forceinline__ float focal_term(float x, bool hit) {
  const float z = hit ? -x : x;
  const float e = expf(-fabsf(z));
  const float sp = fmaxf(z, 0.f) + log1pf(e);
  const float den = 1.f + e;
  const float sig = z >= 0.f ? 1.f / den : e / den;
  return (sp * (sig * sig)) * (hit ? 0.25f : 0.75f);
}

__device__ __forceinline__ float focal_row(const float* x, int cols, int target) {
  float acc = focal_term(x[0], target == 0);
  for (int c = 1; c < cols; ++c) acc = acc + focal_term(x[c], target == c);
  return acc;
}

__global__ __launch_bounds__(1024) void fcos_loss_kernel(const LevelTable lt, const ExtLevels ex, const GtTables gt,
                                                         int num_classes, float radius, double* __restrict__ partial,
                                                         int32_t* __restrict__ matched) {
  __shared__ float g_box[HN_FCOS_MAX_GT][4];
  __shared__ float g_ctr[HN_FCOS_MAX_GT][2];
  __shared__ float g_key[HN_FCOS_MAX_GT];
  __shared__ float g_info[HN_FCOS_MAX_GT][5];
  __shared__ int g_label[HN_FCOS_MAX_GT];
  __shared__ float wave_sums[16][kSums];
  const int img = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = lt.start[lt.num_levels];
  const int G = gt.G;
  const int count = min(max(gt.count[img], 0), G);
  if (tid < count) {
    const float* b = gt.boxes + ((long)img * G + tid) * 4;
    const float x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
    g_box[tid][0] = x0; g_box[tid][1] = y0; g_box[tid][2] = x1; g_box[tid][3] = y1;
    g_ctr[tid][0] = (x0 + x1) / 2.f;
    g_ctr[tid][1] = (y0 + y1) / 2.f;
    g_key[tid] = 1e8f - (y0 - x0) * (y1 - y0);   // fcos.py:563-564: not the box area; float32, one ulp at 1e8 is 8
    g_label[tid] = gt.labels[(long)img * G + tid];
    const float* f = gt.info + ((long)img * G + tid) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) g_info[tid][k] = f[k];
  }
  __syncthreads();

  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int fg = 0;
  const int i = chunk * kChunk + tid;
  if (i < P) {
    const int lv = hn_fcos::point_level(lt, i);
    const int q = i - lt.start[lv];
    const long row = (long)img * (lt.h[lv] * lt.w[lv]) + q;
    const hn_fcos::PointAnchor a = hn_fcos::point_anchor(lt, lv, q);
    // ---- matching (fcos.py:531-568) ----
    const float size = a.bw;
    const float reach = radius * size;
    const float lower = lv == 0 ? 0.f : size * 4.f;
    const float upper = lv == lt.num_levels - 1 ? INFINITY : size * 8.f;
    float best = -INFINITY;
    int m = -1;
    for (int g = 0; g < count; ++g) {
      const float l = a.cx - g_box[g][0], t = a.cy - g_box[g][1], r = g_box[g][2] - a.cx, b = g_box[g][3] - a.cy;
      const float off = fmaxf(fabsf(a.cx - g_ctr[g][0]), fabsf(a.cy - g_ctr[g][1]));
      const float near = fminf(fminf(l, t), fminf(r, b)), far = fmaxf(fmaxf(l, t), fmaxf(r, b));
      const bool hit = off < reach && near > 0.f && far > lower && far < upper;
      const float val = hit ? g_key[g] : 0.f;
      if (val > best) {   // the first index wins a tie (torch.max)
        best = val;
        m = g;
      }
    }
    if (best < 1e-5f) m = -1;
    if (matched) matched[(long)img * P + i] = m;
    fg = m >= 0 ? 1 : 0;
    // ---- per-point targets: -1 = no column ----
    const int m0 = max(m, 0);
    const int cls_t = m >= 0 ? g_label[m] : -1;
    const int side_t = m >= 0 ? (int)g_info[m][1] : -1;
    const int contact_t = m >= 0 ? (int)g_info[m][0] : -1;
    // ---- focal terms ----
    const float* pc = lt.cls_lr[lv] + row * (num_classes + 2);
    v[0] = focal_row(pc, num_classes, cls_t);
    v[3] = focal_row(pc + num_classes, 2, side_t);
    const float* pr = lt.reg_ctr[lv] + row * 5;
    if (m >= 0) {
      // GIoU loss of the decoded box against the matched box (fcos_utils/utils.py, eps 1e-7)
      const float bx0 = g_box[m][0], by0 = g_box[m][1], bx1 = g_box[m][2], by1 = g_box[m][3];
      const float x1 = a.cx - pr[0] * a.bw, y1 = a.cy - pr[1] * a.bh;
      const float x2 = a.cx + pr[2] * a.bw, y2 = a.cy + pr[3] * a.bh;
      const float iw = fmaxf(fminf(x2, bx1) - fmaxf(x1, bx0), 0.f);
      const float ih = fmaxf(fminf(y2, by1) - fmaxf(y1, by0), 0.f);
      const float inter = iw * ih;
      const float uni = ((x2 - x1) * (y2 - y1) + (bx1 - bx0) * (by1 - by0)) - inter;
      const float iou = inter / (uni + 1e-7f);
      const float area_c = (fmaxf(x2, bx1) - fminf(x1, bx0)) * (fmaxf(y2, by1) - fminf(y1, by0));
      const float miou = iou - (area_c - uni) / (area_c + 1e-7f);
      v[1] = 1.f - miou;
      // centre-ness: BCE with logits against sqrt(|min(l, r) / max(l, r) * min(t, b) / max(t, b)|) of encode_single
      const float el = (a.cx - bx0) / a.bw, et = (a.cy - by0) / a.bh;
      const float er = (bx1 - a.cx) / a.bw, eb = (by1 - a.cy) / a.bh;
      const float tgt = sqrtf(fabsf((fminf(el, er) / fmaxf(el, er)) * (fminf(et, eb) / fmaxf(et, eb))));
      const float z = pr[4];
      v[2] = (fmaxf(z, 0.f) - z * tgt) + log1pf(expf(-fabsf(z)));
    }
    if (ex.p[0]) {
      const float* e = ex.p[lv] + row * 8;
      v[4] = focal_row(e + 3, 5, contact_t);
      // a background point carries the row of ground truth 0 (matched.clip(min=0)); an image without boxes zeros
      float pred[3];
      hn_fcos::ext_dxdymag(e, pred);
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float d = pred[k] - (count > 0 ? g_info[m0][2 + k] : 0.f);
        acc = k == 0 ? d * d : acc + d * d;
      }
      v[5] = acc;
    }
  }
  // ---- chunk sums: wave butterfly, then the waves in order ----
  float fgf = (float)fg;   // <= 1024: exact
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = v[k] + __shfl_xor(v[k], o);
    fgf = fgf + __shfl_xor(fgf, o);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) wave_sums[wave][k] = v[k];
    wave_sums[wave][6] = fgf;
    wave_sums[wave][7] = 0.f;
  }
  __syncthreads();
  if (tid < kSums) {
    float tot = 0.f;
    for (int k = 0; k < 16; ++k) tot = tot + wave_sums[k][tid];
    partial[((long)img * chunks + chunk) * kSums + tid] = (double)tot;
  }
}

// partial [n][chunks][8] -> image_sums [n][8] (double, in the workspace), terms [n][6], fg [n], losses [6]
__global__ __launch_bounds__(256) void fcos_loss_reduce_kernel(const double* __restrict__ partial,
                                                               double* __restrict__ image_sums, int n, int chunks,
                                                               int total_points, float* __restrict__ terms,
                                                               int32_t* __restrict__ fg, float* __restrict__ losses) {
  __shared__ double batch[kSums];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < n * kSums; idx += blockDim.x) {
    const int img = idx / kSums, k = idx - img * kSums;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s = s + partial[((long)img * chunks + c) * kSums + k];
    image_sums[idx] = s;
    if (k < 6) terms[img * 6 + k] = (float)s;
    if (k == 6) fg[img] = (int32_t)s;
  }
  __syncthreads();   // one workgroup: image_sums was written by this workgroup's threads
  if (tid < kSums) {
    double s = 0.0;
    for (int img = 0; img < n; ++img) s = s + image_sums[img * kSums + tid];
    batch[tid] = s;
  }
  __syncthreads();
  if (tid < 6) {
    const double div = batch[6] > 1.0 ? batch[6] : 1.0;   // max(1, num_foreground)
    double s = batch[tid];
    if (tid == 3) s = s * 2e-2;
    if (tid == 4) s = s * 1e-2;
    if (tid == 5) s = 10.0 * (s / ((double)n * (double)total_points * 3.0));   // mse_loss's mean over ALL elements, times 10
    losses[tid] = (float)(s / div);
  }
}

}  // namespace

extern "C" int64_t hn_fcos_loss_ws_bytes(int n, int total_points) {
  if (n <= 0 || total_points <= 0) return 0;
  const int64_t chunks = (total_points + kChunk - 1) / kChunk;
  return (int64_t)n * (chunks + 1) * kSums * 8;
}

extern "C" int hn_fcos_loss_f32(const hn_fcos_levels* lv, const float* const* ext, int n, int num_classes,
                                const float* gt_boxes, const int32_t* gt_labels, const float* gt_info,
                                const int32_t* gt_count, int G, float radius, float* terms, int32_t* fg, float* losses,
                                int32_t* matched, void* ws, int64_t ws_bytes, void* stream) {
  HN_CHECK_ARG(lv && gt_boxes && gt_labels && gt_info && gt_count && terms && fg && losses && ws,
               "hn_fcos_loss_f32: null pointer");
  HN_CHECK_ARG((uintptr_t)ws % 8 == 0, "hn_fcos_loss_f32: unaligned workspace");
  HN_CHECK_ARG(G >= 1 && G <= HN_FCOS_MAX_GT, "G = %d outside 1..%d", G, HN_FCOS_MAX_GT);
  HN_CHECK_ARG(num_classes >= 1 && num_classes <= 8, "num_classes = %d outside 1..8", num_classes);
  HN_CHECK_ARG(n > 0 && n <= 65535, "bad image count");
  HN_CHECK_ARG(radius > 0.f, "bad radius");
  LevelTable lt;
  if (const int rc = hn_fcos::level_table_fill(lv, lt)) return rc;
  ExtLevels ex;
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l) {
    ex.p[l] = ext && l < lv->num_levels ? ext[l] : nullptr;
    if (ext && l < lv->num_levels) HN_CHECK_ARG(ext[l], "null ext level %d", l);
  }
  const int P = lt.start[lv->num_levels], chunks = (P + kChunk - 1) / kChunk;
  HN_CHECK_ARG(ws_bytes >= hn_fcos_loss_ws_bytes(n, P), "workspace too small: %lld < %lld bytes", (long long)ws_bytes,
               (long long)hn_fcos_loss_ws_bytes(n, P));
  HN_CHECK_ARG((long)n * P < ((long)1 << 31), "too many points");
  GtTables gt = {gt_boxes, gt_labels, gt_info, gt_count, G};
  double* partial = (double*)ws;
  double* image_sums = partial + (long)n * chunks * kSums;
  hipLaunchKernelGGL(fcos_loss_kernel, dim3(chunks, n), dim3(kChunk), 0, (hipStream_t)stream, lt, ex, gt, num_classes,
                     radius, partial, matched);
  HN_CHECK_LAUNCH("fcos_loss_kernel");
  hipLaunchKernelGGL(fcos_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partial,
                     image_sums, n, chunks, P, terms, fg, losses);
  HN_CHECK_LAUNCH("fcos_loss_reduce_kernel");
  return HN_OK;
}
