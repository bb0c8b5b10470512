// The FCOS criterion, forward and backward at the heads (fcos_utils/fcos.py:523-570 the matching, :44-178 the six terms, fcos_utils/utils.py the
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
//   fcos_loss_grad_kernel    the backward at the heads (tests/fcos_loss_grad_ref.py): the first kernel's grid
//                            and ground truth in LDS, after the two launches above on the same stream.  Each workgroup adds the
//                            forward's fg[n] (integers: exact in any order) into the batch-wide divisor and forms the six
//                            coefficients from the upstream weights on the device; a point repeats its matching and writes its
//                            C + 2, 5 and 8 gradient values from closed forms, zeros included: every element once, no memset.
// The matching, the per-point targets and the focal / GIoU / centre-ness / dxdy arithmetic are __device__ functions both sweeps call.
// No atomics, no inter-workgroup waiting, a fixed order: two runs give the same bytes, and image i of a batch gives the forward
// bytes of that image launched alone.
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

// The image's ground truth in LDS (filled by the first `count` threads)
struct GtShared {
  float box[HN_FCOS_MAX_GT][4];
  float ctr[HN_FCOS_MAX_GT][2];
  float key[HN_FCOS_MAX_GT];
  float info[HN_FCOS_MAX_GT][5];
  int label[HN_FCOS_MAX_GT];
};

// rows [0, count) of image img -> s; returns count.  The caller synchronises.
__device__ __forceinline__ int gt_load(GtShared& s, const GtTables& gt, int img, int tid) {
  const int G = gt.G;
  const int count = min(max(gt.count[img], 0), G);
  if (tid < count) {
    const float* b = gt.boxes + ((long)img * G + tid) * 4;
    const float x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
    s.box[tid][0] = x0; s.box[tid][1] = y0; s.box[tid][2] = x1; s.box[tid][3] = y1;
    s.ctr[tid][0] = (x0 + x1) / 2.f;
    s.ctr[tid][1] = (y0 + y1) / 2.f;
    s.key[tid] = 1e8f - (y0 - x0) * (y1 - y0);   // fcos.py:563-564: not the box area; float32, one ulp at 1e8 is 8
    s.label[tid] = gt.labels[(long)img * G + tid];
    const float* f = gt.info + ((long)img * G + tid) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) s.info[tid][k] = f[k];
  }
  return count;
}

// the matching (fcos.py:531-568): the point's ground-truth row, -1 for background
__device__ __forceinline__ int match_point(const GtShared& s, int count, const hn_fcos::PointAnchor& a, int lv, int num_levels,
                                           float radius) {
  const float size = a.bw;
  const float reach = radius * size;
  const float lower = lv == 0 ? 0.f : size * 4.f;
  const float upper = lv == num_levels - 1 ? INFINITY : size * 8.f;
  float best = -INFINITY;
  int m = -1;
  for (int g = 0; g < count; ++g) {
    const float l = a.cx - s.box[g][0], t = a.cy - s.box[g][1], r = s.box[g][2] - a.cx, b = s.box[g][3] - a.cy;
    const float off = fmaxf(fabsf(a.cx - s.ctr[g][0]), fabsf(a.cy - s.ctr[g][1]));
    const float near = fminf(fminf(l, t), fminf(r, b)), far = fmaxf(fmaxf(l, t), fmaxf(r, b));
    const bool hit = off < reach && near > 0.f && far > lower && far < upper;
    const float val = hit ? s.key[g] : 0.f;
    if (val > best) {   // the first index wins a tie (torch.max)
      best = val;
      m = g;
    }
  }
  return best < 1e-5f ? -1 : m;
}

// per-point targets: -1 = no column; m0 = the row a background point's dxdy target is read from
struct PointTargets {
  int cls_t, side_t, contact_t, m0;
};
__device__ __forceinline__ PointTargets point_targets(const GtShared& s, int m) {
  PointTargets t;
  t.m0 = max(m, 0);
  t.cls_t = m >= 0 ? s.label[m] : -1;
  t.side_t = m >= 0 ? (int)s.info[m][1] : -1;
  t.contact_t = m >= 0 ? (int)s.info[m][0] : -1;
  return t;
}

// softplus(z), sigmoid(z) and 1 - sigmoid(z) of z = -x on the target column and x elsewhere, none of them through a cancellation
struct FocalParts {
  float sp, sig, oms;
};
__device__ __forceinline__ FocalParts focal_parts(float x, bool hit) {
  const float z = hit ? -x : x;
  const float e = expf(-fabsf(z));
  const float den = 1.f + e;
  FocalParts p;
  p.sp = fmaxf(z, 0.f) + log1pf(e);
  p.sig = z >= 0.f ? 1.f / den : e / den;
  p.oms = z >= 0.f ? e / den : 1.f / den;
  return p;
}

// alpha_t * softplus(z) * sigmoid(z)^2: torchvision's ce * (1 - p_t)^2 * alpha_t (alpha 0.25, gamma 2) without the cancellation
// in 1 - p_t
__device__ __forceinline__ float focal_term(float x, bool hit) {
  const FocalParts p = focal_parts(x, hit);
  return (p.sp * (p.sig * p.sig)) * (hit ? 0.25f : 0.75f);
}

__device__ __forceinline__ float focal_row(const float* x, int cols, int target) {
  float acc = focal_term(x[0], target == 0);
  for (int c = 1; c < cols; ++c) acc = acc + focal_term(x[c], target == c);
  return acc;
}

// d/dx of coef * focal_term: alpha_t sigma^2 (sigma + 2 sp (1 - sigma)) in z, the sign flipped on the target column
__device__ __forceinline__ float focal_grad(float x, bool hit, float coef) {
  const FocalParts p = focal_parts(x, hit);
  const float inner = p.sig + 2.f * (p.sp * p.oms);
  const float d = (((p.sig * p.sig) * inner) * (hit ? 0.25f : 0.75f)) * coef;
  return hit ? -d : d;
}

// The decoded box against the matched box (fcos_utils/utils.py): the pieces the GIoU loss and its derivative share
struct GiouParts {
  float x1, y1, x2, y2;    // the decoded box
  float wk, hk;            // the intersection's sides before any clamp
  float inter, uni;
  float pw, ph, cw, ch;    // the decoded and the enclosing box's sides
  float area_c;
};
__device__ __forceinline__ GiouParts giou_parts(const hn_fcos::PointAnchor& a, const float* pr, const float* box) {
  const float bx0 = box[0], by0 = box[1], bx1 = box[2], by1 = box[3];
  GiouParts g;
  g.x1 = a.cx - pr[0] * a.bw; g.y1 = a.cy - pr[1] * a.bh;
  g.x2 = a.cx + pr[2] * a.bw; g.y2 = a.cy + pr[3] * a.bh;
  g.wk = fminf(g.x2, bx1) - fmaxf(g.x1, bx0);
  g.hk = fminf(g.y2, by1) - fmaxf(g.y1, by0);
  g.inter = fmaxf(g.wk, 0.f) * fmaxf(g.hk, 0.f);
  g.pw = g.x2 - g.x1; g.ph = g.y2 - g.y1;
  g.uni = (g.pw * g.ph + (bx1 - bx0) * (by1 - by0)) - g.inter;
  g.cw = fmaxf(g.x2, bx1) - fminf(g.x1, bx0);
  g.ch = fmaxf(g.y2, by1) - fminf(g.y1, by0);
  g.area_c = g.cw * g.ch;
  return g;
}

// centre-ness target: sqrt(|min(l, r) / max(l, r) * min(t, b) / max(t, b)|) of encode_single
__device__ __forceinline__ float ctrness_target(const hn_fcos::PointAnchor& a, const float* box) {
  const float el = (a.cx - box[0]) / a.bw, et = (a.cy - box[1]) / a.bh;
  const float er = (box[2] - a.cx) / a.bw, eb = (box[3] - a.cy) / a.bh;
  return sqrtf(fabsf((fminf(el, er) / fmaxf(el, er)) * (fminf(et, eb) / fmaxf(et, eb))));
}

__global__ __launch_bounds__(1024) void fcos_loss_kernel(const LevelTable lt, const ExtLevels ex, const GtTables gt,
                                                         int num_classes, float radius, double* __restrict__ partial,
                                                         int32_t* __restrict__ matched) {
  __shared__ GtShared gs;
  __shared__ float wave_sums[16][kSums];
  const int img = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = lt.start[lt.num_levels];
  const int count = gt_load(gs, gt, img, tid);
  __syncthreads();

  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int fg = 0;
  const int i = chunk * kChunk + tid;
  if (i < P) {
    const int lv = hn_fcos::point_level(lt, i);
    const int q = i - lt.start[lv];
    const long row = (long)img * (lt.h[lv] * lt.w[lv]) + q;
    const hn_fcos::PointAnchor a = hn_fcos::point_anchor(lt, lv, q);
    const int m = match_point(gs, count, a, lv, lt.num_levels, radius);
    if (matched) matched[(long)img * P + i] = m;
    fg = m >= 0 ? 1 : 0;
    const PointTargets t = point_targets(gs, m);
    // ---- focal terms ----
    const float* pc = lt.cls_lr[lv] + row * (num_classes + 2);
    v[0] = focal_row(pc, num_classes, t.cls_t);
    v[3] = focal_row(pc + num_classes, 2, t.side_t);
    const float* pr = lt.reg_ctr[lv] + row * 5;
    if (m >= 0) {
      // GIoU loss of the decoded box against the matched box (fcos_utils/utils.py, eps 1e-7)
      const GiouParts g = giou_parts(a, pr, gs.box[m]);
      const float iou = g.inter / (g.uni + 1e-7f);
      const float miou = iou - (g.area_c - g.uni) / (g.area_c + 1e-7f);
      v[1] = 1.f - miou;
      // centre-ness: BCE with logits against the target of encode_single
      const float tgt = ctrness_target(a, gs.box[m]);
      const float z = pr[4];
      v[2] = (fmaxf(z, 0.f) - z * tgt) + log1pf(expf(-fabsf(z)));
    }
    if (ex.p[0]) {
      const float* e = ex.p[lv] + row * 8;
      v[4] = focal_row(e + 3, 5, t.contact_t);
      // a background point carries the row of ground truth 0 (matched.clip(min=0)); an image without boxes zeros
      float pred[3];
      hn_fcos::ext_dxdymag(e, pred);
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float d = pred[k] - (count > 0 ? gs.info[t.m0][2 + k] : 0.f);
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

// what the backward adds to the sweep's arguments: the per-level gradient tensors, the layouts of the heads
struct GradLevels {
  float* cls_lr[HN_FCOS_MAX_LEVELS];
  float* reg_ctr[HN_FCOS_MAX_LEVELS];
  float* ext[HN_FCOS_MAX_LEVELS];   // all null: no ext heads
};

// [a > b] as torch.max / torch.min of two tensors hand the gradient on: 1, 1/2 on a tie, 0
__device__ __forceinline__ float tie_sel(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }

// d/dr of c1 * GIoU loss for one edge: side = the intersection's other side under the reference's mask, other / enc = the decoded
// and the enclosing box's other sides, s_in / s_out = the edge's share of the intersection's and the enclosing box's edge
__device__ __forceinline__ float giou_edge_grad(float k_i, float k_p, float k_c, float side, float s_in, float other, float enc,
                                                float s_out, float sc) {
  return (((k_i * (side * s_in)) + k_p * other) + k_c * (enc * s_out)) * sc;
}

__global__ __launch_bounds__(1024) void fcos_loss_grad_kernel(const LevelTable lt, const ExtLevels ex, const GtTables gt,
                                                              int num_classes, float radius, int n,
                                                              const int32_t* __restrict__ fg_image,
                                                              const float* __restrict__ upstream, const GradLevels out) {
  __shared__ GtShared gs;
  __shared__ int wave_fg[16];
  __shared__ float coef[6];
  const int img = blockIdx.y, chunk = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = lt.start[lt.num_levels];
  const int count = gt_load(gs, gt, img, tid);
  // ---- the batch-wide divisor: the forward's fg[n], integers ----
  int part = 0;
  for (int k = tid; k < n; k += kChunk) part += fg_image[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) wave_fg[wave] = part;
  __syncthreads();
  if (tid < 6) {
    int total = 0;
    for (int k = 0; k < 16; ++k) total += wave_fg[k];
    const double div = total > 1 ? (double)total : 1.0;   // max(1, num_foreground)
    const double w = upstream ? (double)upstream[tid] : 1.0;
    double c = w / div;
    if (tid == 3) c = (w * 2e-2) / div;
    if (tid == 4) c = (w * 1e-2) / div;
    if (tid == 5) c = (w * 20.0) / ((((double)n * (double)P) * 3.0) * div);   // d/dpred of 10 * mean over ALL elements of the squares
    coef[tid] = (float)c;
  }
  __syncthreads();

  const int i = chunk * kChunk + tid;
  if (i >= P) return;
  const int lv = hn_fcos::point_level(lt, i);
  const int q = i - lt.start[lv];
  const long row = (long)img * (lt.h[lv] * lt.w[lv]) + q;
  const hn_fcos::PointAnchor a = hn_fcos::point_anchor(lt, lv, q);
  const int m = match_point(gs, count, a, lv, lt.num_levels, radius);
  const PointTargets t = point_targets(gs, m);
  // ---- focal columns ----
  const int cols = num_classes + 2;
  const float* pc = lt.cls_lr[lv] + row * cols;
  float* dc = out.cls_lr[lv] + row * cols;
  for (int c = 0; c < num_classes; ++c) dc[c] = focal_grad(pc[c], t.cls_t == c, coef[0]);
#pragma unroll
  for (int c = 0; c < 2; ++c) dc[num_classes + c] = focal_grad(pc[num_classes + c], t.side_t == c, coef[3]);
  // ---- GIoU and centre-ness: foreground only, zeros elsewhere ----
  const float* pr = lt.reg_ctr[lv] + row * 5;
  float* dr = out.reg_ctr[lv] + row * 5;
  float gr[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (m >= 0) {
    const float* box = gs.box[m];
    const GiouParts g = giou_parts(a, pr, box);
    const float uu = g.uni + 1e-7f, ace = g.area_c + 1e-7f;
    const float ru = 1.f / uu, ra = 1.f / ace;
    const float qq = (g.inter / uu) / uu;
    const float k_i = (ra - ru) - qq, k_p = qq - ra, k_c = (uu * ra) * ra;
    const bool overlap = g.wk > 0.f && g.hk > 0.f;   // the reference's mask: strict
    const float ihm = overlap ? g.hk : 0.f, iwm = overlap ? g.wk : 0.f;
    const float scx = a.bw * coef[1], scy = a.bh * coef[1];
    gr[0] = giou_edge_grad(k_i, k_p, k_c, ihm, tie_sel(g.x1, box[0]), g.ph, g.ch, tie_sel(box[0], g.x1), scx);
    gr[1] = giou_edge_grad(k_i, k_p, k_c, iwm, tie_sel(g.y1, box[1]), g.pw, g.cw, tie_sel(box[1], g.y1), scy);
    gr[2] = giou_edge_grad(k_i, k_p, k_c, ihm, tie_sel(box[2], g.x2), g.ph, g.ch, tie_sel(g.x2, box[2]), scx);
    gr[3] = giou_edge_grad(k_i, k_p, k_c, iwm, tie_sel(box[3], g.y2), g.pw, g.cw, tie_sel(g.y2, box[3]), scy);
    const float tgt = ctrness_target(a, box);
    const float z = pr[4];
    const float e = expf(-fabsf(z));
    const float den = 1.f + e;
    const float sig = z >= 0.f ? 1.f / den : e / den;
    gr[4] = (sig - tgt) * coef[2];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) dr[k] = gr[k];
  // ---- ext: the dxdy regression on EVERY point, then the contact columns ----
  if (ex.p[0]) {
    const float* e = ex.p[lv] + row * 8;
    const float dx = e[1], dy = e[2];
    const float nrm = sqrtf(dx * dx + dy * dy);
    const float den = fmaxf(nrm, 1e-12f);
    const float u0 = dx / den, u1 = dy / den;
    const float pred[3] = {e[0], 0.1f * u0, 0.1f * u1};
    float gk[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) gk[k] = (pred[k] - (count > 0 ? gs.info[t.m0][2 + k] : 0.f)) * coef[5];
    // below the clamp the norm passes no gradient (clamp_min): the Jacobian is 0.1 / 1e-12 on the diagonal, a kept quirk
    const float dot = nrm < 1e-12f ? 0.f : gk[1] * u0 + gk[2] * u1;
    const float rden = 0.1f / den;
    float4 lo, hi;
    lo.x = gk[0];
    lo.y = (gk[1] - u0 * dot) * rden;
    lo.z = (gk[2] - u1 * dot) * rden;
    lo.w = focal_grad(e[3], t.contact_t == 0, coef[4]);
    hi.x = focal_grad(e[4], t.contact_t == 1, coef[4]);
    hi.y = focal_grad(e[5], t.contact_t == 2, coef[4]);
    hi.z = focal_grad(e[6], t.contact_t == 3, coef[4]);
    hi.w = focal_grad(e[7], t.contact_t == 4, coef[4]);
    float4* de = reinterpret_cast<float4*>(out.ext[lv] + row * 8);   // 32-byte rows of a 16-byte aligned tensor
    de[0] = lo;
    de[1] = hi;
  }
}

}  // namespace

extern "C" int64_t hn_fcos_loss_ws_bytes(int n, int total_points) {
  if (n <= 0 || total_points <= 0) return 0;
  const int64_t chunks = (total_points + kChunk - 1) / kChunk;
  return (int64_t)n * (chunks + 1) * kSums * 8;
}

namespace {

// the checked arguments of the forward's two launches
struct LossPlan {
  LevelTable lt;
  ExtLevels ex;
  GtTables gt;
  int P, chunks;
  double* partial;
  double* image_sums;
};

// every refusal of hn_fcos_loss_f32 (and the shared ones of hn_fcos_loss_grad_f32); nothing is launched here
int loss_plan_fill(const hn_fcos_levels* lv, const float* const* ext, int n, int num_classes, const float* gt_boxes,
                   const int32_t* gt_labels, const float* gt_info, const int32_t* gt_count, int G, float radius, float* terms,
                   int32_t* fg, float* losses, void* ws, int64_t ws_bytes, LossPlan& p) {
  HN_CHECK_ARG(lv && gt_boxes && gt_labels && gt_info && gt_count && terms && fg && losses && ws,
               "hn_fcos_loss_f32: null pointer");
  HN_CHECK_ARG((uintptr_t)ws % 8 == 0, "hn_fcos_loss_f32: unaligned workspace");
  HN_CHECK_ARG(G >= 1 && G <= HN_FCOS_MAX_GT, "G = %d outside 1..%d", G, HN_FCOS_MAX_GT);
  HN_CHECK_ARG(num_classes >= 1 && num_classes <= 8, "num_classes = %d outside 1..8", num_classes);
  HN_CHECK_ARG(n > 0 && n <= 65535, "bad image count");
  HN_CHECK_ARG(radius > 0.f, "bad radius");
  if (const int rc = hn_fcos::level_table_fill(lv, p.lt)) return rc;
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l) {
    p.ex.p[l] = ext && l < lv->num_levels ? ext[l] : nullptr;
    if (ext && l < lv->num_levels) HN_CHECK_ARG(ext[l], "null ext level %d", l);
  }
  p.P = p.lt.start[lv->num_levels];
  p.chunks = (p.P + kChunk - 1) / kChunk;
  HN_CHECK_ARG(ws_bytes >= hn_fcos_loss_ws_bytes(n, p.P), "workspace too small: %lld < %lld bytes", (long long)ws_bytes,
               (long long)hn_fcos_loss_ws_bytes(n, p.P));
  HN_CHECK_ARG((long)n * p.P < ((long)1 << 31), "too many points");
  p.gt = {gt_boxes, gt_labels, gt_info, gt_count, G};
  p.partial = (double*)ws;
  p.image_sums = p.partial + (long)n * p.chunks * kSums;
  return HN_OK;
}

int loss_launch(const LossPlan& p, int n, int num_classes, float radius, float* terms, int32_t* fg, float* losses,
                int32_t* matched, void* stream) {
  hipLaunchKernelGGL(fcos_loss_kernel, dim3(p.chunks, n), dim3(kChunk), 0, (hipStream_t)stream, p.lt, p.ex, p.gt, num_classes,
                     radius, p.partial, matched);
  HN_CHECK_LAUNCH("fcos_loss_kernel");
  hipLaunchKernelGGL(fcos_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)p.partial,
                     p.image_sums, n, p.chunks, p.P, terms, fg, losses);
  HN_CHECK_LAUNCH("fcos_loss_reduce_kernel");
  return HN_OK;
}

}  // namespace

extern "C" int hn_fcos_loss_f32(const hn_fcos_levels* lv, const float* const* ext, int n, int num_classes,
                                const float* gt_boxes, const int32_t* gt_labels, const float* gt_info,
                                const int32_t* gt_count, int G, float radius, float* terms, int32_t* fg, float* losses,
                                int32_t* matched, void* ws, int64_t ws_bytes, void* stream) {
  LossPlan p;
  if (const int rc = loss_plan_fill(lv, ext, n, num_classes, gt_boxes, gt_labels, gt_info, gt_count, G, radius, terms, fg, losses,
                                    ws, ws_bytes, p))
    return rc;
  return loss_launch(p, n, num_classes, radius, terms, fg, losses, matched, stream);
}

extern "C" int hn_fcos_loss_grad_f32(const hn_fcos_levels* lv, const float* const* ext, int n, int num_classes,
                                     const float* gt_boxes, const int32_t* gt_labels, const float* gt_info,
                                     const int32_t* gt_count, int G, float radius, float* terms, int32_t* fg, float* losses,
                                     int32_t* matched, void* ws, int64_t ws_bytes, const float* upstream,
                                     float* const* d_cls_lr, float* const* d_reg_ctr, float* const* d_ext, void* stream) {
  LossPlan p;
  if (const int rc = loss_plan_fill(lv, ext, n, num_classes, gt_boxes, gt_labels, gt_info, gt_count, G, radius, terms, fg, losses,
                                    ws, ws_bytes, p))
    return rc;
  HN_CHECK_ARG(d_cls_lr && d_reg_ctr, "hn_fcos_loss_grad_f32: null pointer");
  HN_CHECK_ARG((ext != nullptr) == (d_ext != nullptr), "hn_fcos_loss_grad_f32: d_ext goes with ext");
  HN_CHECK_ARG((uintptr_t)upstream % 4 == 0, "hn_fcos_loss_grad_f32: unaligned upstream");
  GradLevels out;
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l) {
    const bool used = l < lv->num_levels;
    out.cls_lr[l] = used ? d_cls_lr[l] : nullptr;
    out.reg_ctr[l] = used ? d_reg_ctr[l] : nullptr;
    out.ext[l] = used && d_ext ? d_ext[l] : nullptr;
    if (used) HN_CHECK_ARG(out.cls_lr[l] && out.reg_ctr[l] && (!d_ext || out.ext[l]), "null gradient level %d", l);
    if (used && d_ext) HN_CHECK_ARG((uintptr_t)out.ext[l] % 16 == 0, "hn_fcos_loss_grad_f32: d_ext level %d must be 16-byte aligned", l);
  }
  if (const int rc = loss_launch(p, n, num_classes, radius, terms, fg, losses, matched, stream)) return rc;
  hipLaunchKernelGGL(fcos_loss_grad_kernel, dim3(p.chunks, n), dim3(kChunk), 0, (hipStream_t)stream, p.lt, p.ex, p.gt,
                     num_classes, radius, n, (const int32_t*)fg, upstream, out);
  HN_CHECK_LAUNCH("fcos_loss_grad_kernel");
  return HN_OK;
}
