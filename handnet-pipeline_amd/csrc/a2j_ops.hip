// HBM-bound helpers of the A2J / ResNet path: 3x3/2 max pooling, depth -> NHWC packing, the softmax-weighted anchor
// aggregation (a2j/anchor.py:57-82) with its criterion (anchor.py:99-153) and the criterion's backward -- three kernels over
// ONE head sweep (AggMap, joint_max, sums<NQ>, joint_totals<NQ> below) --, the joint conversion, the lifter's input, the
// all-gather records and the stem image.
#include "hn_common.h"

#include <float.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// one thread = one output pixel x 4 channels; consecutive threads walk channels first,
// so a wave reads/writes contiguous 16-B pieces (coalesced NHWC).
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           int n, int h, int w, int c4, int oh, int ow) {
  const long total = (long)n * oh * ow * c4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c4);
    long pix = i / c4;
    const int x_ = (int)(pix % ow);
    pix /= ow;
    const int y_ = (int)(pix % oh);
    const int img = (int)(pix / oh);
    f32x4 m = {-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = y_ * 2 - 1 + dy;
      if ((unsigned)iy >= (unsigned)h) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int ix = x_ * 2 - 1 + dx;
        if ((unsigned)ix >= (unsigned)w) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((long)img * h + iy) * w + ix) * c4 * 4 + cc * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = hn::max_nan(m[e], v[e]);
      }
    }
    *reinterpret_cast<f32x4*>(y + i * 4) = m;
  }
}

__global__ __launch_bounds__(256) void pack_depth_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                         long npix, int c4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix * c4; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / c4;
    const int cc = (int)(i - pix * c4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (cc == 0) v[0] = src[pix];
    *reinterpret_cast<f32x4*>(dst + i * 4) = v;
  }
}

// crop-(u,v,d) of one joint -> image (u,v,d) and / or camera xyz in millimetres (a2j/a2j.py:17-34 convert_joints +
// datasets3d/a2jdataset.py:31-38 uvd2xyz).  ONE function for the stand-alone kernel and the aggregation's epilogue: the two are
// bit-identical by construction.  (Every operation is a single rounding in the reference's order; nothing here can contract
// into an fma: each product feeds a division.)
struct ConvertSpec {
  const long long* box;   // [n,4] padded crop boxes (x1,y1,x2,y2), or nullptr: no conversion (unless box_f32)
  const float* box_f32;   // [n,4] the DATASET's float boxes (the evaluation caller, a2j/a2j.py:339-346; a2jdataset.py:293): used instead
  const float* sample_paras;   // [n,4] per-sample (fx, fy, cx, cy) on the device (a2jdataset.py:279,293): used instead of fx..cy
  float crop_w, crop_h;
  int has_paras;          // camera intrinsics given: xyz_mm is written
  float fx, fy, cx, cy;
  int clamp_kp;           // clamp the crop-(u,v,d) to [0, crop_w] first (ros_demo.py:283 clamps all three to [0, 176])
  int clamp_h, clamp_w;   // > 0: clamp box x1,y1 to [0, clamp_h] and x2,y2 to [0, clamp_w] first (ros_demo.py:279-280, as written there)
  float* image_uvd;       // [n,J,3] or nullptr
  float* xyz_mm;          // [n,J,3] or nullptr
  const int* mirror;      // [n] or nullptr: rows with mirror != 0 come from a crop mirrored along its width (a left hand on its
                          // way through the right-handed network): the aggregation un-mirrors u = crop_w - u first of all
};

__device__ __forceinline__ void convert_one(const ConvertSpec& cs, int img, long joint_row, float ku, float kv, float kd) {
  float x0, y0, x1, y1;
  if (cs.box_f32) {
    x0 = cs.box_f32[img * 4 + 0], y0 = cs.box_f32[img * 4 + 1], x1 = cs.box_f32[img * 4 + 2], y1 = cs.box_f32[img * 4 + 3];
  } else {
    x0 = (float)cs.box[img * 4 + 0], y0 = (float)cs.box[img * 4 + 1], x1 = (float)cs.box[img * 4 + 2], y1 = (float)cs.box[img * 4 + 3];
  }
  if (cs.clamp_h > 0) {
    x0 = fminf(fmaxf(x0, 0.f), (float)cs.clamp_h);
    y0 = fminf(fmaxf(y0, 0.f), (float)cs.clamp_h);
    x1 = fminf(fmaxf(x1, 0.f), (float)cs.clamp_w);
    y1 = fminf(fmaxf(y1, 0.f), (float)cs.clamp_w);
  }
  if (cs.clamp_kp) {   // torch.clamp keeps NaN; fminf / fmaxf would drop it
    ku = ku != ku ? ku : fminf(fmaxf(ku, 0.f), cs.crop_w);
    kv = kv != kv ? kv : fminf(fmaxf(kv, 0.f), cs.crop_w);
    kd = kd != kd ? kd : fminf(fmaxf(kd, 0.f), cs.crop_w);
  }
  const float u = ku * (x1 - x0) / cs.crop_w + x0;
  const float v = kv * (y1 - y0) / cs.crop_h + y0;
  if (cs.image_uvd) {
    float* o = cs.image_uvd + joint_row * 3;
    o[0] = u;
    o[1] = v;
    o[2] = kd;
  }
  if (cs.xyz_mm && cs.has_paras) {
    float* o = cs.xyz_mm + joint_row * 3;
    float fx = cs.fx, fy = cs.fy, cx = cs.cx, cy = cs.cy;
    if (cs.sample_paras) fx = cs.sample_paras[img * 4 + 0], fy = cs.sample_paras[img * 4 + 1], cx = cs.sample_paras[img * 4 + 2], cy = cs.sample_paras[img * 4 + 3];
    o[0] = (u - cx) * kd / fx * 1000.f;
    o[1] = (v - cy) * kd / fy * 1000.f;
    o[2] = kd * 1000.f;
  }
}

constexpr int kAnchorsPerCell = 16;
constexpr int kMaxGroups = 9;   // (round 4: 3 -> 9 cell groups: on an 11 x 11 map a thread owns 14 cells = ONE batch of loads per pass
                                // instead of three, 18 -> ~11 us at one crop; the group count fixes the summation order, so it is the
                                // same for every batch size)
constexpr int kJointSplit = 3;

// what the loss form (hn_a2j_aggregate_loss_f32; DESIGN.md section 9o, tests/loss_ref.py) adds to the kernel's arguments
struct LossSpec {
  const float* gt;   // [n,J,3] ground truth in crop (coord0, coord1, depth), the coordinates of the output row
  float* terms;      // [n,J,8]: (La_h, La_w, Lr_h, Lr_w, d, (gt - out)^2 x 3)
};
constexpr int kLossTerms = 8;

// a2j/anchor.py:125-129,135-139: where(diff <= 1, 0.5 * diff^2, diff - 0.5); a NaN takes the second branch and stays NaN
__device__ __forceinline__ float smooth_l1(float a) {
#pragma clang fp contract(off)
  return a <= 1.f ? 0.5f * (a * a) : a - 0.5f;
}

// the criterion's terms of one joint (a2j/anchor.py:123-150), one rounding per operation: e0, e1 = sum w anchor; (ku, kv, kd) =
// the keypoint the caller gets.  The depth term is the plain |difference| (the smooth-L1 with knee 3 of lines 145-149 is never used)
__device__ __forceinline__ void loss_terms_one(const LossSpec& ls, long joint_row, float e0, float e1, float ku, float kv, float kd) {
#pragma clang fp contract(off)
  const float* g = ls.gt + joint_row * 3;
  const float g0 = g[0], g1 = g[1], g2 = g[2];
  const float du = g0 - ku, dv = g1 - kv, dd = g2 - kd;
  f32x4* o = reinterpret_cast<f32x4*>(ls.terms + joint_row * kLossTerms);
  const f32x4 lo = {smooth_l1(fabsf(g0 - e0)), smooth_l1(fabsf(g1 - e1)), smooth_l1(fabsf(du)), smooth_l1(fabsf(dv))};
  const f32x4 hi = {fabsf(dd), du * du, dv * dv, dd * dd};
  o[0] = lo;
  o[1] = hi;
}

// ---------------------------------------------------------------------------------------
// The head sweep of a2j_aggregate_kernel, a2j_loss_aggregate_kernel and a2j_loss_grad_kernel, written once.
// kJointSplit workgroups per crop, each owning a contiguous range of joints (the joints are independent; one workgroup
// per crop was 28 us of the batch-1 frame on one CU).  Thread (g, a, jl): anchor-in-cell a, joint j = j0 + jl; the G
// thread groups take the cells p = g, g+G, ... (a single group walked all fh*fw cells with two dependent loads each: 60 us
// of pure latency per launch).
// joint_max: per-joint max of the logits (exact, order independent).
// sums<NQ>: e = exp(x - max); partial sums of e, e*(anchor+offset), e*depth (and, NQ == 6, e*anchor) per (group, anchor, joint),
// then combined through LDS in a fixed order (group-major here, anchor order in joint_totals<NQ>): bitwise reproducible,
// independent of the joint split, and the same bytes in all three kernels.
// Both cell loops fetch kBatch (14: three rounds for the 41 cells a thread owns on an 11 x 11 map) cells' operands before they use
// any (same operations in the same order): written as load -> use per cell, each of the 2 x 41 iterations waited for its own L2
// round trip -- 27 us per launch.
// ---------------------------------------------------------------------------------------
constexpr int kBatch = 14;

struct AggMap {
  int k, j0, jn;      // crop; first joint and joints of this workgroup (the last one may have fewer, or none)
  int AJ, AW;         // channels per cell in memory; thread slots per cell group
  int g, cl, a, jl;   // cell group, slot in it = (anchor, joint of the workgroup)
  int c;              // channel in memory
  int cells;
  bool active;
  const float *cls, *reg, *dep;   // the crop's slices of the heads
  __device__ __forceinline__ AggMap(const float* cls_, const float* reg_, const float* dep_, int fh, int fw, int J, int Jw, int G) {
    k = blockIdx.x;
    j0 = blockIdx.y * Jw;
    jn = min(Jw, J - j0);
    AJ = kAnchorsPerCell * J;
    AW = kAnchorsPerCell * Jw;
    g = threadIdx.x / AW, cl = threadIdx.x - g * AW;
    a = cl / Jw, jl = cl - a * Jw;
    c = a * J + j0 + jl;
    cells = fh * fw;
    active = g < G && jl < jn;
    cls = cls_ + (long)k * cells * AJ;
    dep = dep_ + (long)k * cells * AJ;
    reg = reg_ + (long)k * cells * AJ * 2;
  }
  // this thread's element of cell p in the crop's slice of cls / dep.  (p >= 0 and AJ > 0, said with unsigned operands: ONE
  // 32 x 32 -> 64 bit multiply.  The signed 64-bit product is two, and the second one's addend pair has a don't-care half that
  // the register allocator once put on the destination of a load in flight: the first sweep then waited out a third of its
  // loads one by one)
  __device__ __forceinline__ long at(int p) const { return (long)((unsigned long)(unsigned)p * (unsigned)AJ) + c; }
};

// A row with valid != 1 (uniform per workgroup): 0 = no crop (zeros; the loss's reduction leaves the row out), 2 = non-finite
// crop (NaN, as the reference's network returns for it: every cell of the 11 x 11 maps sees every pixel of the crop).  The
// workgroup's joints of every [n,J,3] output given and of the [n,J,8] terms; nullptr: not an output of the caller.
__device__ __forceinline__ float row_fill(int valid_k) { return valid_k == 0 ? 0.f : __builtin_nanf(""); }
__device__ __forceinline__ void fill_row(const AggMap& m, int J, float fill, float* uvd, float* image_uvd, float* xyz_mm, float* terms) {
  const long row = (long)m.k * J + m.j0;
  if ((int)threadIdx.x < m.jn * 3) {
    if (uvd) uvd[row * 3 + threadIdx.x] = fill;
    if (image_uvd) image_uvd[row * 3 + threadIdx.x] = fill;
    if (xyz_mm) xyz_mm[row * 3 + threadIdx.x] = fill;
  }
  if (terms && (int)threadIdx.x < m.jn * kLossTerms) terms[row * kLossTerms + threadIdx.x] = fill;
}

// the maximum of this thread's joint over all cells and anchors; lds: AW * G floats, free again on return
__device__ __forceinline__ float joint_max(const AggMap& m, int Jw, int G, float* lds) {
  float mx = -FLT_MAX;
  if (m.active)
    for (int pb = m.g; pb < m.cells; pb += kBatch * G) {
      float v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        v[u] = p < m.cells ? m.cls[m.at(p)] : -FLT_MAX;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) mx = fmaxf(mx, v[u]);
    }
  if (m.g < G) lds[m.g * m.AW + m.cl] = mx;
  __syncthreads();
  if ((int)threadIdx.x < m.AW) {   // (group 0's threads: slot cl = threadIdx.x) maximum over the groups, then over the anchors below
    float mm = lds[threadIdx.x];
    for (int gg = 1; gg < G; ++gg) mm = fmaxf(mm, lds[gg * m.AW + threadIdx.x]);
    lds[threadIdx.x] = mm;
  }
  __syncthreads();
  float mj = -FLT_MAX;
  if (m.active)
    for (int aa = 0; aa < kAnchorsPerCell; ++aa) mj = fmaxf(mj, lds[aa * Jw + m.jl]);
  __syncthreads();
  return mj;
}

// the NQ sums of every (anchor, joint) slot over all cells: on return plane q of lds ([NQ][AW], group 0's) holds them, summed
// over the groups 0 .. G-1 in that order; lds: [G][NQ][AW] floats
template <int NQ>
__device__ __forceinline__ void sums(const AggMap& m, float mj, int fw, int stride, int G, float* lds) {
  static_assert(NQ == 4 || NQ == 6, "s, s0, s1, sd and, for the criterion, sa0, sa1");
  const int AW = m.AW, cl = m.cl;
  if (m.active) {
    float s = 0.f, s0 = 0.f, s1 = 0.f, sd = 0.f;
    [[maybe_unused]] float sa0 = 0.f, sa1 = 0.f;   // e * anchor
    const float p0 = 2.f + 4.f * (float)(m.a >> 2), p1 = 2.f + 4.f * (float)(m.a & 3);
    for (int pb = m.g; pb < m.cells; pb += kBatch * G) {
      float vc[kBatch], vd[kBatch];
      float2 vr[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        const long q = m.at(p < m.cells ? p : m.g);   // (clamped: the tail batch's extra cells are not used)
        vc[u] = m.cls[q];
        vr[u] = *reinterpret_cast<const float2*>(m.reg + q * 2);
        vd[u] = m.dep[q];
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        if (p < m.cells) {
          const int hh = p / fw, ww = p - hh * fw;
          const float e = expf(vc[u] - mj);
          const float a0 = (float)(hh * stride) + p0, a1 = (float)(ww * stride) + p1;
          s += e;
          s0 += e * (a0 + vr[u].x);
          s1 += e * (a1 + vr[u].y);
          sd += e * vd[u];
          if constexpr (NQ == 6) {
            sa0 += e * a0;
            sa1 += e * a1;
          }
        }
      }
    }
    float* o = lds + (long)m.g * NQ * AW;
    o[cl] = s;
    o[AW + cl] = s0;
    o[2 * AW + cl] = s1;
    o[3 * AW + cl] = sd;
    if constexpr (NQ == 6) {
      o[4 * AW + cl] = sa0;
      o[5 * AW + cl] = sa1;
    }
  }
  __syncthreads();
  // fixed-order combination in two steps: thread (quantity q, anchor a, joint jl) of the first NQ * AW sums its slot over the
  // groups 0 .. G-1, then joint_totals sums the 16 anchors of a joint (G + 16 dependent additions instead of 16 G)
  for (int s4 = threadIdx.x; s4 < NQ * AW; s4 += blockDim.x) {
    float acc = lds[s4];
    for (int gg = 1; gg < G; ++gg) acc += lds[(long)gg * NQ * AW + s4];
    lds[s4] = acc;   // (group 0's slot: only this thread reads or writes it here)
  }
  __syncthreads();
}

// joint jj's totals over its 16 anchors, in anchor order: t[q] of plane q
template <int NQ>
struct JointTotals {
  float t[NQ];
};
template <int NQ>
__device__ __forceinline__ JointTotals<NQ> joint_totals(const float* lds, int AW, int Jw, int jj) {
  JointTotals<NQ> r;
#pragma unroll
  for (int q = 0; q < NQ; ++q) r.t[q] = 0.f;
  for (int aa = 0; aa < kAnchorsPerCell; ++aa) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) r.t[q] += lds[q * AW + aa * Jw + jj];
  }
  return r;
}

// The aggregation (NQ == 4) and, with the criterion's terms behind the same sweep (NQ == 6; hn_a2j_aggregate_loss_f32, DESIGN.md
// section 9o), the loss form: two more running sums (e * anchor) and six LDS planes per group instead of four.
template <int NQ>
__device__ __forceinline__ void aggregate_row(const float* __restrict__ cls, const float* __restrict__ reg,
                                              const float* __restrict__ dep, const int* __restrict__ valid, int fh, int fw, int J,
                                              int Jw, int stride, int G, float* __restrict__ out, const ConvertSpec& cs,
                                              const LossSpec& ls, float* lds) {
  constexpr bool kLoss = NQ == 6;
  const AggMap m(cls, reg, dep, fh, fw, J, Jw, G);
  if (m.jn <= 0) return;
  if (valid && valid[m.k] != 1) {
    const bool convert = cs.box || cs.box_f32;
    fill_row(m, J, row_fill(valid[m.k]), out, convert ? cs.image_uvd : nullptr, convert && cs.has_paras ? cs.xyz_mm : nullptr,
             kLoss ? ls.terms : nullptr);
    return;
  }
  const float mj = joint_max(m, Jw, G, lds);
  sums<NQ>(m, mj, fw, stride, G, lds);
  if ((int)threadIdx.x < m.jn) {
    const int jj = threadIdx.x;
    const JointTotals<NQ> tt = joint_totals<NQ>(lds, m.AW, Jw, jj);
    const long joint_row = (long)m.k * J + m.j0 + jj;
    const float t = tt.t[0];
    float* o = out + joint_row * 3;
    float ku = tt.t[1] / t;
    const float kv = tt.t[2] / t, kd = tt.t[3] / t;
    if constexpr (!kLoss)   // (the loss form's entry takes no mirror flags: gt is in the coordinates of the crop as cut)
      if (cs.mirror && cs.mirror[m.k]) ku = cs.crop_w - ku;   // (one fp32 subtraction, before anything else sees the value)
    o[0] = ku;
    o[1] = kv;
    o[2] = kd;
    // convert_joints + uvd2xyz in the aggregation's epilogue (what every caller does next: ros_demo.py:289,
    // 329-330, a2j/a2j.py:341-348) -- from the registers that hold the joint, no second launch
    if (cs.box || cs.box_f32) convert_one(cs, m.k, joint_row, ku, kv, kd);
    if constexpr (kLoss) loss_terms_one(ls, joint_row, tt.t[4] / t, tt.t[5] / t, ku, kv, kd);
  }
}

// (two kernels and not one template's instantiations: each has a name of its own in the build's resource record)
__global__ __launch_bounds__(1024) void a2j_aggregate_kernel(const float* __restrict__ cls, const float* __restrict__ reg,
                                                             const float* __restrict__ dep, const int* __restrict__ valid, int fh,
                                                             int fw, int J, int Jw, int stride, int G, float* __restrict__ out,
                                                             const ConvertSpec cs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [G][4][A*Jw]
  aggregate_row<4>(cls, reg, dep, valid, fh, fw, J, Jw, stride, G, out, cs, LossSpec{}, lds);
}

__global__ __launch_bounds__(1024) void a2j_loss_aggregate_kernel(const float* __restrict__ cls, const float* __restrict__ reg,
                                                                  const float* __restrict__ dep, const int* __restrict__ valid,
                                                                  int fh, int fw, int J, int Jw, int stride, int G,
                                                                  float* __restrict__ out, const ConvertSpec cs, const LossSpec ls) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [G][6][A*Jw]
  aggregate_row<6>(cls, reg, dep, valid, fh, fw, J, Jw, stride, G, out, cs, ls, lds);
}

// what the criterion's backward (hn_a2j_loss_grad_f32; DESIGN.md section 9r, tests/loss_grad_ref.py) adds to the kernel's arguments
struct GradSpec {
  const float* gt;         // [n,J,3]
  const float* upstream;   // device (wa, wr): the weights of classification and regression in the differentiated scalar; nullptr: (1, 1)
  float spatial_factor, reg_loss_factor;
  float* d_cls;            // [n,fh,fw,16 J]
  float* d_reg;            // [n,fh,fw,16 J,2]
  float* d_dep;            // [n,fh,fw,16 J]
  float* uvd;              // [n,J,3] or nullptr: the loss entry's keypoints
  float* terms;            // [n,J,8] or nullptr: the loss entry's terms
};
constexpr int kGradJoint = 12;   // per-joint values of the third sweep: mj, t, Ea x 2, Er x 2, Ed, ga x 2, gr x 2, gd

// the derivative of smooth_l1(|x|) in x (C1: the knee needs no guard); a NaN stays NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clip1(float x) { return x != x ? x : fminf(fmaxf(x, -1.f), 1.f); }
// the derivative of |x|: sign(0) = 0 as torch's, a NaN stays NaN
__device__ __forceinline__ float sign1(float x) { return x > 0.f ? 1.f : x < 0.f ? -1.f : x; }

// The criterion's backward in the aggregation's sweep: a2j_loss_aggregate_kernel's grid, AggMap, joint_max, sums<6> and
// joint_totals<6> (so the divided uvd and the eight terms are the loss entry's bytes), then
//   the thread that owns a joint: n = rows with valid != 0 (counted here, per workgroup), the coefficients
//     ga_c = wa / n / (2J) clip(Ea_c - g_c),  gr_c = wr R sf / n / (2J) clip(Er_c - g_c),  gd = wr R / n / J sign(Ed - g_d)
//     and t, Ea, Er, Ed into LDS (mj is there since the first phase);
//   a third sweep over the workgroup's own cells: e = expf(cls - mj) (the same expression), w = e / t,
//     d_reg = w gr_c,  d_dep = w gd,  d_cls = w (sum_c ga_c (anchor_c - Ea_c) + sum_c gr_c (anchor_c + reg_c - Er_c) + gd (dep - Ed)).
// Every gradient element is written by exactly one thread (the one that summed it): no atomics, no second launch.  Rows with
// valid == 0 get zero gradients, rows with valid == 2 NaN.  Dynamic LDS: [G][6][AW] floats + kGradJoint * Jw.
__global__ __launch_bounds__(1024) void a2j_loss_grad_kernel(const float* __restrict__ cls, const float* __restrict__ reg,
                                                             const float* __restrict__ dep, const int* __restrict__ valid, int fh,
                                                             int fw, int J, int Jw, int stride, int G, const GradSpec gs) {
  constexpr int NQ = 6;
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [G][NQ][A*Jw], then [kGradJoint][Jw]
  __shared__ int wave_rows[16];
  const AggMap m(cls, reg, dep, fh, fw, J, Jw, G);
  if (m.jn <= 0) return;
  const int k = m.k, j0 = m.j0, jn = m.jn, AJ = m.AJ, AW = m.AW, g = m.g, a = m.a, jl = m.jl, c = m.c, cells = m.cells;
  const bool active = m.active;
  if (valid && valid[k] != 1) {  // the row's slice of the gradients (and of the forward outputs) is 0 or NaN
    const float fill = row_fill(valid[k]);
    if (active)
      for (int p = g; p < cells; p += G) {
        const long q = ((long)k * cells + p) * AJ + c;
        gs.d_cls[q] = fill;
        *reinterpret_cast<float2*>(gs.d_reg + q * 2) = make_float2(fill, fill);
        gs.d_dep[q] = fill;
      }
    fill_row(m, J, fill, gs.uvd, nullptr, nullptr, gs.terms);
    return;
  }
  {  // rows that count in the batch means: this thread's share, then its wave's (read behind the barriers below)
    int rows = 0;
    if (valid)
      for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) rows += valid[i] != 0 ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o);
    if ((threadIdx.x & 63) == 0) wave_rows[threadIdx.x >> 6] = rows;
  }
  const float *clsk = m.cls, *depk = m.dep, *regk = m.reg;

  const float mj = joint_max(m, Jw, G, lds);
  float* jv = lds + (long)G * NQ * AW;   // [kGradJoint][Jw]: behind the planes
  if ((int)threadIdx.x < jn) jv[threadIdx.x] = mj;   // (thread jl = group 0, anchor 0 of its joint; read in the third sweep)
  sums<NQ>(m, mj, fw, stride, G, lds);
  if ((int)threadIdx.x < jn) {
    const int jj = threadIdx.x;
    const JointTotals<NQ> tt = joint_totals<NQ>(lds, AW, Jw, jj);
    const long joint_row = (long)k * J + j0 + jj;
    const float t = tt.t[0];
    const float ku = tt.t[1] / t, kv = tt.t[2] / t, kd = tt.t[3] / t;
    const float e0 = tt.t[4] / t, e1 = tt.t[5] / t;
    if (gs.uvd) {
      float* o = gs.uvd + joint_row * 3;
      o[0] = ku;
      o[1] = kv;
      o[2] = kd;
    }
    if (gs.terms) loss_terms_one(LossSpec{gs.gt, gs.terms}, joint_row, e0, e1, ku, kv, kd);
    {
#pragma clang fp contract(off)
      int rows = (int)gridDim.x;
      if (valid) {
        rows = 0;
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) rows += wave_rows[wv];
      }
      const float wa = gs.upstream ? gs.upstream[0] : 1.f, wr = gs.upstream ? gs.upstream[1] : 1.f;
      const float n = (float)rows, wrr = wr * gs.reg_loss_factor;
      const float ca = wa / n / (float)(2 * J);
      const float cr = wrr * gs.spatial_factor / n / (float)(2 * J);
      const float cd = wrr / n / (float)J;
      const float* gj = gs.gt + joint_row * 3;
      const float g0 = gj[0], g1 = gj[1], g2 = gj[2];
      jv[1 * Jw + jj] = t;
      jv[2 * Jw + jj] = e0;
      jv[3 * Jw + jj] = e1;
      jv[4 * Jw + jj] = ku;
      jv[5 * Jw + jj] = kv;
      jv[6 * Jw + jj] = kd;
      jv[7 * Jw + jj] = ca * clip1(e0 - g0);
      jv[8 * Jw + jj] = ca * clip1(e1 - g1);
      jv[9 * Jw + jj] = cr * clip1(ku - g0);
      jv[10 * Jw + jj] = cr * clip1(kv - g1);
      jv[11 * Jw + jj] = cd * sign1(kd - g2);
    }
  }
  __syncthreads();
  if (active) {
#pragma clang fp contract(off)
    const float p0 = 2.f + 4.f * (float)(a >> 2), p1 = 2.f + 4.f * (float)(a & 3);
    const float mjj = jv[0 * Jw + jl], t = jv[1 * Jw + jl];
    const float ea0 = jv[2 * Jw + jl], ea1 = jv[3 * Jw + jl], er0 = jv[4 * Jw + jl], er1 = jv[5 * Jw + jl], ed = jv[6 * Jw + jl];
    const float ga0 = jv[7 * Jw + jl], ga1 = jv[8 * Jw + jl], gr0 = jv[9 * Jw + jl], gr1 = jv[10 * Jw + jl], gd = jv[11 * Jw + jl];
    // (offsets inside the crop's slice in 32 bits -- the entry refuses a slice of 2^31 elements --: the batch's addresses
    // would not fit the registers beside its operands otherwise)
    float* dck = gs.d_cls + (long)k * cells * AJ;
    float* ddk = gs.d_dep + (long)k * cells * AJ;
    float* drk = gs.d_reg + (long)k * cells * AJ * 2;
    for (int pb = g; pb < cells; pb += kBatch * G) {
      float vc[kBatch], vd[kBatch];
      float2 vr[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        const int q = (p < cells ? p : g) * AJ + c;   // (clamped, as above)
        vc[u] = clsk[q];
        vr[u] = *reinterpret_cast<const float2*>(regk + q * 2);
        vd[u] = depk[q];
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        if (p < cells) {
          const int hh = p / fw, ww = p - hh * fw;
          const float e = expf(vc[u] - mjj);
          const float w = e / t;
          const float a0 = (float)(hh * stride) + p0, a1 = (float)(ww * stride) + p1;
          float b = ga0 * (a0 - ea0);
          b += ga1 * (a1 - ea1);
          b += gr0 * ((a0 + vr[u].x) - er0);
          b += gr1 * ((a1 + vr[u].y) - er1);
          b += gd * (vd[u] - ed);
          const int q = p * AJ + c;
          dck[q] = w * b;
          *reinterpret_cast<float2*>(drk + q * 2) = make_float2(w * gr0, w * gr1);
          ddk[q] = w * gd;
        }
      }
    }
  }
}

// The criterion's reductions (a2j/anchor.py:130,140,150,153; a2j/a2j.py:233-238,318) in ONE workgroup and a fixed order, no
// atomics: thread i of a round of 256 samples adds its own sample's joints in joint order (a sample row depends on its own
// crop only), then thread 0 adds the round's samples in sample order.  valid == 0 rows are left out of the batch values
// (divisor = rows with valid != 0; none: 0 / 0 = NaN, like torch.mean of nothing), valid == 2 rows carry NaN terms.
// batch [5] = (classification, the criterion's regression mean, regression * reg_loss_factor, total, rmse over n * J * 3 values)
__global__ __launch_bounds__(256) void a2j_loss_reduce_kernel(const float* __restrict__ terms, const int* __restrict__ valid, int n,
                                                              int J, float spatial_factor, float reg_loss_factor,
                                                              float* __restrict__ sample, float* __restrict__ batch) {
#pragma clang fp contract(off)
  __shared__ float sh[3][256];
  __shared__ int use[256];
  float ba = 0.f, br = 0.f, bq = 0.f;   // (thread 0) running batch sums
  int rows = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + (int)threadIdx.x;
    if (i < n) {
      const f32x4* t = reinterpret_cast<const f32x4*>(terms + (long)i * J * kLossTerms);
      float la = 0.f, lr = 0.f, ld = 0.f, sq = 0.f;
      for (int j = 0; j < J; ++j) {
        const f32x4 lo = t[2 * j], hi = t[2 * j + 1];
        la += lo[0];
        la += lo[1];
        lr += lo[2];
        lr += lo[3];
        ld += hi[0];
        sq += hi[1];
        sq += hi[2];
        sq += hi[3];
      }
      const float anchor_loss = la / (float)(2 * J);
      const float regression_loss = lr / (float)(2 * J) * spatial_factor + ld / (float)J;
      sample[(long)i * 2 + 0] = anchor_loss;
      sample[(long)i * 2 + 1] = regression_loss;
      sh[0][threadIdx.x] = anchor_loss;
      sh[1][threadIdx.x] = regression_loss;
      sh[2][threadIdx.x] = sq;
      use[threadIdx.x] = !valid || valid[i] != 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(256, n - base);
      for (int r = 0; r < m; ++r)
        if (use[r]) {
          ba += sh[0][r];
          br += sh[1][r];
          bq += sh[2][r];
          ++rows;
        }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float cls_loss = ba / (float)rows, reg_mean = br / (float)rows;
    const float reg_loss = reg_mean * reg_loss_factor;
    batch[0] = cls_loss;
    batch[1] = reg_mean;
    batch[2] = reg_loss;
    batch[3] = cls_loss + reg_loss;
    batch[4] = sqrtf(bq / ((float)rows * (float)(J * 3)));
  }
}

// the stand-alone form (the reference form of the fused epilogue above), one thread per joint: out = camera xyz in mm when
// intrinsics are given, else image (u,v,d)
__global__ __launch_bounds__(256) void convert_joints_kernel(const float* __restrict__ kp, const int* __restrict__ valid, int n,
                                                             int J, const ConvertSpec cs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * J) return;
  const int img = i / J;
  if (valid && valid[img] == 0) {
    if (cs.image_uvd) cs.image_uvd[(long)i * 3 + 0] = cs.image_uvd[(long)i * 3 + 1] = cs.image_uvd[(long)i * 3 + 2] = 0.f;
    if (cs.xyz_mm && cs.has_paras) cs.xyz_mm[(long)i * 3 + 0] = cs.xyz_mm[(long)i * 3 + 1] = cs.xyz_mm[(long)i * 3 + 2] = 0.f;
    return;
  }
  convert_one(cs, img, i, kp[(long)i * 3 + 0], kp[(long)i * 3 + 1], kp[(long)i * 3 + 2]);
}

}  // namespace

// the conversion as the entries take it (paras: host (fx, fy, cx, cy) or null; opts: host or null = no clamps, no per-sample
// operands) -> the kernels' ConvertSpec
static int convert_spec(ConvertSpec& cs, const int64_t* crop_box, float crop_w, float crop_h, const float* paras,
                        const hn_convert_opts* opts, const int32_t* mirror, float* out_image_uvd, float* out_xyz_mm) {
  cs.box = (const long long*)crop_box;
  cs.crop_w = crop_w;
  cs.crop_h = crop_h;
  cs.box_f32 = opts ? opts->sample_box : nullptr;
  cs.sample_paras = opts ? opts->sample_paras : nullptr;
  cs.has_paras = (paras || cs.sample_paras) ? 1 : 0;
  cs.fx = paras ? paras[0] : 1.f;
  cs.fy = paras ? paras[1] : 1.f;
  cs.cx = paras ? paras[2] : 0.f;
  cs.cy = paras ? paras[3] : 0.f;
  cs.clamp_kp = opts ? opts->clamp_keypoints : 0;
  cs.clamp_h = opts ? opts->clamp_box_h : 0;
  cs.clamp_w = opts ? opts->clamp_box_w : 0;
  HN_CHECK_ARG((cs.clamp_h > 0) == (cs.clamp_w > 0), "clamp_box_h and clamp_box_w are given together");
  cs.image_uvd = out_image_uvd;
  cs.xyz_mm = out_xyz_mm;
  cs.mirror = mirror;
  return HN_OK;
}

// the head checks of the four aggregation entries; who: "" or "<the entry's name>: "
static int check_heads(const char* who, int k, int fh, int fw, int joints, int stride) {
  HN_CHECK_ARG(joints > 0 && joints * kAnchorsPerCell <= 1024, "%sjoints must be in [1, 64]", who);
  HN_CHECK_ARG(fh > 0 && fw > 0, "%sbad dims: fh * fw must not be 0", who);
  HN_CHECK_ARG(k >= 0 && stride > 0, "%sbad dims", who);
  return HN_OK;
}

extern "C" int hn_convert_joints_f32(const float* kp, const int64_t* crop_box, const int32_t* valid, int n, int joints,
                                     float crop_w, float crop_h, const float* paras, float* out, void* stream) {
  HN_CHECK_ARG(kp && crop_box && out, "hn_convert_joints_f32: null pointer");
  HN_CHECK_ARG(n >= 0 && joints > 0 && crop_w > 0.f && crop_h > 0.f, "bad dims");
  if (n == 0) return HN_OK;
  const int total = n * joints;
  ConvertSpec cs{};
  if (const int st = convert_spec(cs, crop_box, crop_w, crop_h, paras, nullptr, nullptr, paras ? nullptr : out, paras ? out : nullptr))
    return st;
  hipLaunchKernelGGL(convert_joints_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, kp, valid, n, joints, cs);
  HN_CHECK_LAUNCH("convert_joints_kernel");
  return HN_OK;
}

extern "C" int hn_convert_joints_samples_f32(const float* kp, const float* box_f32, const float* sample_paras, const int32_t* valid,
                                             int n, int joints, float crop_w, float crop_h, float* out_image_uvd, float* out_xyz_mm,
                                             void* stream) {
  HN_CHECK_ARG(kp && box_f32, "hn_convert_joints_samples_f32: null pointer");
  HN_CHECK_ARG(out_image_uvd || out_xyz_mm, "hn_convert_joints_samples_f32: no output requested");
  HN_CHECK_ARG(!out_xyz_mm || sample_paras, "hn_convert_joints_samples_f32: camera xyz needs the samples' intrinsics");
  HN_CHECK_ARG(n >= 0 && joints > 0 && crop_w > 0.f && crop_h > 0.f, "bad dims");
  if (n == 0) return HN_OK;
  const int total = n * joints;
  ConvertSpec cs{};
  const hn_convert_opts samples{0, 0, 0, 0, box_f32, sample_paras};
  if (const int st = convert_spec(cs, nullptr, crop_w, crop_h, nullptr, &samples, nullptr, out_image_uvd, out_xyz_mm)) return st;
  hipLaunchKernelGGL(convert_joints_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, kp, valid, n, joints, cs);
  HN_CHECK_LAUNCH("convert_joints_kernel");
  return HN_OK;
}

extern "C" int hn_maxpool3x3s2_nhwc_f32(const float* x, float* y, int n, int h, int w, int c, int oh, int ow,
                                        void* stream) {
  HN_CHECK_ARG(x && y, "hn_maxpool3x3s2_nhwc_f32: null pointer");
  HN_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, "bad dims (c must be a multiple of 4)");
  HN_CHECK_ARG(oh == (h + 2 - 3) / 2 + 1 && ow == (w + 2 - 3) / 2 + 1, "output size mismatch");
  const long total = (long)n * oh * ow * (c / 4);
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, y, n, h, w, c / 4, oh, ow);
  HN_CHECK_LAUNCH("maxpool3x3s2_kernel");
  return HN_OK;
}

extern "C" int hn_pack_depth_nhwc(const float* src, float* dst, int n, int hw, int cpad, void* stream) {
  HN_CHECK_ARG(src && dst, "hn_pack_depth_nhwc: null pointer");
  HN_CHECK_ARG(n > 0 && hw > 0 && cpad >= 4 && cpad % 4 == 0, "bad dims");
  const long npix = (long)n * hw;
  const long total = npix * (cpad / 4);
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(pack_depth_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, npix, cpad / 4);
  HN_CHECK_LAUNCH("pack_depth_kernel");
  return HN_OK;
}

// the launch geometry of the three aggregation kernels, from the joint count alone (tests/agg_ref.py geometry())
struct AggGeometry {
  int split, jw, aw, groups, threads;
  explicit AggGeometry(int joints) {
    // the cell-group count depends on the joint count only (it fixes the summation order): min(9, 1024 / (16 * joints per workgroup))
    split = joints >= 2 * kJointSplit ? kJointSplit : 1;
    jw = (joints + split - 1) / split;
    aw = kAnchorsPerCell * jw;
    groups = 1024 / aw;            // cell groups of a workgroup (16 * jw thread slots each)
    groups = groups > kMaxGroups ? kMaxGroups : groups;
    groups = groups < 1 ? 1 : groups;
    threads = ((groups * aw + 63) / 64) * 64;
  }
};

template <class... Loss>
static int launch_aggregate(const float* cls, const float* reg, const float* dep, const int32_t* valid, int k, int fh, int fw,
                            int joints, int stride, float* out, const ConvertSpec& cs, void* stream, const Loss... loss) {
  constexpr bool kLoss = sizeof...(Loss) != 0;
  constexpr int nq = kLoss ? 6 : 4;
  const AggGeometry geo(joints);
  const int split = geo.split, jw = geo.jw, aw = geo.aw, groups = geo.groups, threads = geo.threads;
  if constexpr (kLoss) {
    hipLaunchKernelGGL(a2j_loss_aggregate_kernel, dim3(k, split), dim3(threads), groups * nq * aw * sizeof(float),
                       (hipStream_t)stream, cls, reg, dep, valid, fh, fw, joints, jw, stride, groups, out, cs, loss...);
    HN_CHECK_LAUNCH("a2j_loss_aggregate_kernel");
  } else {
    hipLaunchKernelGGL(a2j_aggregate_kernel, dim3(k, split), dim3(threads), groups * nq * aw * sizeof(float),
                       (hipStream_t)stream, cls, reg, dep, valid, fh, fw, joints, jw, stride, groups, out, cs);
    HN_CHECK_LAUNCH("a2j_aggregate_kernel");
  }
  return HN_OK;
}

extern "C" int hn_a2j_aggregate_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid,
                                    int k, int fh, int fw, int joints, int stride, float* out, void* stream) {
  HN_CHECK_ARG(cls && reg && dep && out, "hn_a2j_aggregate_f32: null pointer");
  if (const int st = check_heads("", k, fh, fw, joints, stride)) return st;
  if (k == 0) return HN_OK;
  return launch_aggregate(cls, reg, dep, valid, k, fh, fw, joints, stride, out, ConvertSpec{}, stream);
}

static int aggregate_convert_run(const float* cls, const float* reg, const float* dep, const int32_t* valid, int k, int fh, int fw,
                                 int joints, int stride, const int64_t* crop_box, float crop_w, float crop_h, const float* paras,
                                 const hn_convert_opts* opts, const int32_t* mirror, float* out_uvd, float* out_image_uvd,
                                 float* out_xyz_mm, void* stream) {
  HN_CHECK_ARG(cls && reg && dep && out_uvd, "hn_a2j_aggregate_convert_f32: null pointer");
  HN_CHECK_ARG(crop_box || (opts && opts->sample_box), "hn_a2j_aggregate_convert_f32: no boxes (crop_box or opts->sample_box)");
  HN_CHECK_ARG(out_image_uvd || out_xyz_mm, "hn_a2j_aggregate_convert_f32: no converted output requested");
  HN_CHECK_ARG(!out_xyz_mm || paras || (opts && opts->sample_paras),
               "hn_a2j_aggregate_convert_f32: camera xyz needs the intrinsics (fx, fy, cx, cy)");
  HN_CHECK_ARG(crop_w > 0.f && crop_h > 0.f, "bad dims");
  if (const int st = check_heads("", k, fh, fw, joints, stride)) return st;
  if (k == 0) return HN_OK;
  ConvertSpec cs{};
  if (const int st = convert_spec(cs, crop_box, crop_w, crop_h, paras, opts, mirror, out_image_uvd, out_xyz_mm)) return st;
  return launch_aggregate(cls, reg, dep, valid, k, fh, fw, joints, stride, out_uvd, cs, stream);
}

extern "C" int hn_a2j_aggregate_loss_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid, const float* gt,
                                         int k, int fh, int fw, int joints, int stride, float spatial_factor,
                                         float reg_loss_factor, const int64_t* crop_box, float crop_w, float crop_h,
                                         const float* paras, const hn_convert_opts* opts, float* out_uvd, float* out_image_uvd,
                                         float* out_xyz_mm, float* out_terms, float* out_sample, float* out_batch, void* stream) {
  HN_CHECK_ARG(cls && reg && dep && gt && out_uvd && out_terms && out_sample && out_batch,
               "hn_a2j_aggregate_loss_f32: null pointer");
  if (const int st = check_heads("hn_a2j_aggregate_loss_f32: ", k, fh, fw, joints, stride)) return st;
  HN_CHECK_ARG((uintptr_t)out_terms % 16 == 0, "hn_a2j_aggregate_loss_f32: out_terms must be 16-byte aligned");
  ConvertSpec cs{};
  if (crop_box || (opts && opts->sample_box)) {   // the conversion, as hn_a2j_aggregate_convert_f32 takes it; absent: none
    HN_CHECK_ARG(out_image_uvd || out_xyz_mm, "hn_a2j_aggregate_loss_f32: boxes given but no converted output requested");
    HN_CHECK_ARG(!out_xyz_mm || paras || (opts && opts->sample_paras),
                 "hn_a2j_aggregate_loss_f32: camera xyz needs the intrinsics (fx, fy, cx, cy)");
    HN_CHECK_ARG(crop_w > 0.f && crop_h > 0.f, "hn_a2j_aggregate_loss_f32: bad crop size");
    if (const int st = convert_spec(cs, crop_box, crop_w, crop_h, paras, opts, nullptr, out_image_uvd, out_xyz_mm)) return st;
  } else {
    HN_CHECK_ARG(!out_image_uvd && !out_xyz_mm, "hn_a2j_aggregate_loss_f32: converted outputs need boxes (crop_box or opts->sample_box)");
  }
  if (k == 0) return HN_OK;
  const LossSpec ls{gt, out_terms};
  const int st = launch_aggregate(cls, reg, dep, valid, k, fh, fw, joints, stride, out_uvd, cs, stream, ls);
  if (st != HN_OK) return st;
  hipLaunchKernelGGL(a2j_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)out_terms, valid, k, joints,
                     spatial_factor, reg_loss_factor, out_sample, out_batch);
  HN_CHECK_LAUNCH("a2j_loss_reduce_kernel");
  return HN_OK;
}

extern "C" int hn_a2j_loss_grad_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid, const float* gt,
                                    int k, int fh, int fw, int joints, int stride, float spatial_factor, float reg_loss_factor,
                                    const float* upstream, float* d_cls, float* d_reg, float* d_dep, float* out_uvd,
                                    float* out_terms, void* stream) {
  HN_CHECK_ARG(cls && reg && dep && gt && d_cls && d_reg && d_dep, "hn_a2j_loss_grad_f32: null pointer");
  if (const int st = check_heads("hn_a2j_loss_grad_f32: ", k, fh, fw, joints, stride)) return st;
  HN_CHECK_ARG((long)fh * fw * kAnchorsPerCell * joints * 2 < (1L << 31),
               "hn_a2j_loss_grad_f32: one crop's reg slice (fh * fw * 32 * joints) must be below 2^31 elements");
  HN_CHECK_ARG((uintptr_t)reg % 8 == 0 && (uintptr_t)d_reg % 8 == 0, "hn_a2j_loss_grad_f32: reg and d_reg must be 8-byte aligned");
  HN_CHECK_ARG((uintptr_t)out_terms % 16 == 0, "hn_a2j_loss_grad_f32: out_terms must be 16-byte aligned");
  if (k == 0) return HN_OK;
  const AggGeometry geo(joints);
  const GradSpec gs{gt, upstream, spatial_factor, reg_loss_factor, d_cls, d_reg, d_dep, out_uvd, out_terms};
  hipLaunchKernelGGL(a2j_loss_grad_kernel, dim3(k, geo.split), dim3(geo.threads),
                     (geo.groups * 6 * geo.aw + kGradJoint * geo.jw) * sizeof(float), (hipStream_t)stream, cls, reg, dep, valid, fh,
                     fw, joints, geo.jw, stride, geo.groups, gs);
  HN_CHECK_LAUNCH("a2j_loss_grad_kernel");
  return HN_OK;
}

extern "C" int hn_a2j_aggregate_convert_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid, int k,
                                            int fh, int fw, int joints, int stride, const int64_t* crop_box, float crop_w,
                                            float crop_h, const float* paras, const hn_convert_opts* opts, float* out_uvd,
                                            float* out_image_uvd, float* out_xyz_mm, void* stream) {
  return aggregate_convert_run(cls, reg, dep, valid, k, fh, fw, joints, stride, crop_box, crop_w, crop_h, paras, opts, nullptr,
                               out_uvd, out_image_uvd, out_xyz_mm, stream);
}

extern "C" int hn_a2j_aggregate_convert_mirror_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid,
                                                   const int32_t* mirror, int k, int fh, int fw, int joints, int stride,
                                                   const int64_t* crop_box, float crop_w, float crop_h, const float* paras,
                                                   const hn_convert_opts* opts, float* out_uvd, float* out_image_uvd,
                                                   float* out_xyz_mm, void* stream) {
  HN_CHECK_ARG(mirror, "hn_a2j_aggregate_convert_mirror_f32: null pointer");
  return aggregate_convert_run(cls, reg, dep, valid, k, fh, fw, joints, stride, crop_box, crop_w, crop_h, paras, opts, mirror,
                               out_uvd, out_image_uvd, out_xyz_mm, stream);
}

// ---------------------------------------------------------------------------------------
// The lifter's input (include/handnet_hip.h): per frame and axis (x - mean) / std over the J joints, population std.
// One wave per frame; sums in fp64 in joint order (numpy's pairwise fp32 / fp64 summation differs from ANY fixed order by
// rounding only; the tests compare with a function-by-function fp64 restatement of the caller's chain).
// ---------------------------------------------------------------------------------------
namespace {
// one frame's row p [J][3] -> o [J][2], by one wave; flip: column 0 negated (the gated kernel's mirrored rows)
__device__ __forceinline__ void standardize_row(const float* __restrict__ p, int J, int lane, bool flip, float* __restrict__ o) {
  // every lane computes both axes' statistics itself (J <= 64 values each: 2 x 21 loads that hit the same cache line)
  double m0 = 0.0, m1 = 0.0;
  for (int j = 0; j < J; ++j) {
    m0 += (double)p[j * 3 + 0];
    m1 += (double)p[j * 3 + 1];
  }
  m0 /= J;
  m1 /= J;
  double v0 = 0.0, v1 = 0.0;
  for (int j = 0; j < J; ++j) {
    const double a = (double)p[j * 3 + 0] - m0, b = (double)p[j * 3 + 1] - m1;
    v0 += a * a;
    v1 += b * b;
  }
  const double s0 = sqrt(v0 / J), s1 = sqrt(v1 / J);
  for (int j = lane; j < J; j += 64) {
    const float x = (float)(((double)p[j * 3 + 0] - m0) / s0);
    o[j * 2 + 0] = flip ? -x : x;
    o[j * 2 + 1] = (float)(((double)p[j * 3 + 1] - m1) / s1);
  }
}

__global__ __launch_bounds__(64) void joints2d_standardize_kernel(const float* __restrict__ uvd, const int* __restrict__ valid,
                                                                  int J, float* __restrict__ out) {
  const int img = blockIdx.x, lane = threadIdx.x;
  float* o = out + (long)img * J * 2;
  if (valid && valid[img] != 1) {
    for (int i = lane; i < J * 2; i += 64) o[i] = 0.f;
    return;
  }
  standardize_row(uvd + (long)img * J * 3, J, lane, false, o);
}
}  // namespace

extern "C" int hn_joints2d_standardize_f32(const float* image_uvd, const int32_t* valid, int n, int joints, float* out,
                                           void* stream) {
  HN_CHECK_ARG(image_uvd && out, "hn_joints2d_standardize_f32: null pointer");
  HN_CHECK_ARG(n >= 0 && joints > 1, "bad dims");
  if (n == 0) return HN_OK;
  hipLaunchKernelGGL(joints2d_standardize_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, image_uvd, valid, joints, out);
  HN_CHECK_LAUNCH("joints2d_standardize_kernel");
  return HN_OK;
}

// ---------------------------------------------------------------------------------------
// The lifter's input with the live caller's skip rule (include/handnet_hip.h): ros_demo.py:288-300 drops a hand when
// process_bbox(get_bbox(joints2d)) is None (pose2mesh/lib/coord_utils.py:21-49).  One wave per slot: the bounding box from
// exact wave min / max reductions, the rule in fp32 one rounding per numpy operation (no contraction: this file is built with
// the compiler's default), then standardize_row for the accepted slots.
// ---------------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ void wave_minmax(float& lo, float& hi) {
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
}

// get_bbox along one axis (coord_utils.py:21-40): center = (min + max) / 2., half = 0.5 * (max - min), start = center - half,
// size = (center + half) - start; numpy 2 keeps every step in float32 (a Python float operand does not widen it)
__device__ __forceinline__ void bbox_axis(float lo, float hi, float& start, float& size) {
#pragma clang fp contract(off)
  const float center = (lo + hi) * 0.5f;      // (/ 2. and * 0.5 round identically: one rounding of the same exact value)
  const float half = 0.5f * (hi - lo);
  start = center - half;
  size = (center + half) - start;
}

// process_bbox's test (coord_utils.py:42-49): w * h > 0 and x + (w - 1) >= x and y + (h - 1) >= y, in float32
__device__ __forceinline__ bool bbox_kept(float x, float y, float w, float h) {
#pragma clang fp contract(off)
  const float x2 = x + (w - 1.f), y2 = y + (h - 1.f);
  return w * h > 0.f && x2 >= x && y2 >= y;
}

// mirror (or nullptr): a lifted row with mirror != 0 gets column 0 negated -- exactly the standardisation of the joints
// mirrored in x (the mean negates, the std stays); the gate itself is evaluated on the plain joints
__global__ __launch_bounds__(64) void lifter_input_gated_kernel(const float* __restrict__ uvd, const int* __restrict__ valid,
                                                                int J, float* __restrict__ out, int* __restrict__ lifted,
                                                                const int* __restrict__ mirror) {
  const int img = blockIdx.x, lane = threadIdx.x;
  float* o = out + (long)img * J * 2;
  const float* p = uvd + (long)img * J * 3;
  bool keep = !valid || valid[img] == 1;
  if (keep) {
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    bool finite = true;
    for (int j = lane; j < J; j += 64) {
      const float u = p[j * 3 + 0], v = p[j * 3 + 1];
      finite = finite && isfinite(u) && isfinite(v);
      x0 = fminf(x0, u);
      x1 = fmaxf(x1, u);
      y0 = fminf(y0, v);
      y1 = fmaxf(y1, v);
    }
    wave_minmax(x0, x1);
    wave_minmax(y0, y1);
    float bx, bw, by, bh;
    bbox_axis(x0, x1, bx, bw);
    bbox_axis(y0, y1, by, bh);
    // (a non-finite joint is refused outright: the reference's min() over NaN depends on the joint order)
    keep = __ballot(!finite) == 0ull && bbox_kept(bx, by, bw, bh);
  }
  if (lane == 0) lifted[img] = keep ? 1 : 0;
  if (!keep) {
    for (int i = lane; i < J * 2; i += 64) o[i] = 0.f;
    return;
  }
  standardize_row(p, J, lane, mirror && mirror[img], o);   // (joints2d_standardize_kernel's rows, bit for bit)
}
}  // namespace

extern "C" int hn_lifter_input_gated_f32(const float* image_uvd, const int32_t* valid, int n, int joints, float* out,
                                         int32_t* lifted, void* stream) {
  HN_CHECK_ARG(image_uvd && out && lifted, "hn_lifter_input_gated_f32: null pointer");
  HN_CHECK_ARG(n >= 0 && joints > 1, "bad dims");
  if (n == 0) return HN_OK;
  hipLaunchKernelGGL(lifter_input_gated_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, image_uvd, valid, joints, out,
                     lifted, (const int*)nullptr);
  HN_CHECK_LAUNCH("lifter_input_gated_kernel");
  return HN_OK;
}

extern "C" int hn_lifter_input_gated_mirror_f32(const float* image_uvd, const int32_t* valid, const int32_t* mirror, int n,
                                                int joints, float* out, int32_t* lifted, void* stream) {
  HN_CHECK_ARG(image_uvd && mirror && out && lifted, "hn_lifter_input_gated_mirror_f32: null pointer");
  HN_CHECK_ARG(n >= 0 && joints > 1, "bad dims");
  if (n == 0) return HN_OK;
  hipLaunchKernelGGL(lifter_input_gated_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, image_uvd, valid, joints, out,
                     lifted, (const int*)mirror);
  HN_CHECK_LAUNCH("lifter_input_gated_kernel");
  return HN_OK;
}

// ---------------------------------------------------------------------------------------
// Per-frame result records of the N > 1 all-gather (hn_amd/dist.py) and the always-on non-finite check
// ---------------------------------------------------------------------------------------
namespace {

constexpr int kRecHead = 40;  // 4 x int64 box, int32 has_hand, int32 row flag

// one thread per 4-byte word of a record
__global__ __launch_bounds__(256) void pack_records_kernel(const float* __restrict__ kp, const long long* __restrict__ box,
                                                           const int* __restrict__ has, int n, int rows, int j3,
                                                           int rec_words, unsigned* __restrict__ rec,
                                                           const float* __restrict__ e0, const float* __restrict__ e1) {
  const long total = (long)rows * rec_words;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / rec_words), w = (int)(i - (long)r * rec_words);
    unsigned v = 0u;
    if (r < n) {
      if (w < 8) {
        const long long b = box[(long)r * 4 + (w >> 1)];
        v = (unsigned)((unsigned long long)b >> ((w & 1) * 32));
      } else if (w == 8) {
        v = (unsigned)has[r];
      } else if (w == 9) {
        v = 1u;
      } else if (w - 10 < j3) {
        v = __float_as_uint(kp[(long)r * j3 + (w - 10)]);
      } else if (e0 && w - 10 < 2 * j3) {           // wide records: image (u,v,d) behind the crop (u,v,d) ...
        v = __float_as_uint(e0[(long)r * j3 + (w - 10 - j3)]);
      } else if (e1 && w - 10 < 3 * j3) {           // ... then camera xyz in mm
        v = __float_as_uint(e1[(long)r * j3 + (w - 10 - 2 * j3)]);
      }
    }
    rec[i] = v;
  }
}

__global__ __launch_bounds__(256) void unpack_records_kernel(const unsigned* __restrict__ rec, int rows, int j3, int rec_words,
                                                             float* __restrict__ kp, long long* __restrict__ box,
                                                             int* __restrict__ has, int* __restrict__ valid) {
  const long total = (long)rows * rec_words;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / rec_words), w = (int)(i - (long)r * rec_words);
    const unsigned v = rec[i];
    if (w < 8) {
      if ((w & 1) == 0) {
        const unsigned hi = rec[i + 1];
        box[(long)r * 4 + (w >> 1)] = (long long)(((unsigned long long)hi << 32) | v);
      }
    } else if (w == 8) {
      has[r] = (int)v;
    } else if (w == 9) {
      valid[r] = (int)v;
    } else if (w - 10 < j3) {
      kp[(long)r * j3 + (w - 10)] = __uint_as_float(v);
    }
  }
}

__global__ __launch_bounds__(256) void nonfinite_count_kernel(const float* __restrict__ x, long count, int* __restrict__ flag) {
  int bad = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x)
    bad += !(fabsf(x[i]) <= 3.402823466e38f) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(flag, bad);
}

}  // namespace

extern "C" int hn_pack_records_ex(const float* keypoints, const int64_t* crop_box, const int32_t* has_hand, int n, int rows,
                                  int joints, int rec_bytes, const float* extra0, const float* extra1, void* records,
                                  void* stream) {
  HN_CHECK_ARG(records && (n == 0 || (keypoints && crop_box && has_hand)), "hn_pack_records: null pointer");
  HN_CHECK_ARG(n >= 0 && rows >= n && joints > 0, "bad dims");
  HN_CHECK_ARG(extra0 || !extra1, "hn_pack_records_ex: extra1 without extra0");
  const int fields = 1 + (extra0 ? 1 : 0) + (extra1 ? 1 : 0);
  HN_CHECK_ARG(rec_bytes >= kRecHead + 12 * joints * fields && rec_bytes % 8 == 0,
               "rec_bytes must be a multiple of 8 >= 40 + 12*joints per keypoint field");
  if (rows == 0) return HN_OK;
  const long total = (long)rows * (rec_bytes / 4);
  const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(pack_records_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, keypoints, (const long long*)crop_box,
                     has_hand, n, rows, joints * 3, rec_bytes / 4, (unsigned*)records, extra0, extra1);
  HN_CHECK_LAUNCH("pack_records_kernel");
  return HN_OK;
}

extern "C" int hn_pack_records(const float* keypoints, const int64_t* crop_box, const int32_t* has_hand, int n, int rows,
                               int joints, int rec_bytes, void* records, void* stream) {
  return hn_pack_records_ex(keypoints, crop_box, has_hand, n, rows, joints, rec_bytes, nullptr, nullptr, records, stream);
}

extern "C" int hn_unpack_records(const void* records, int rows, int joints, int rec_bytes, float* keypoints,
                                 int64_t* crop_box, int32_t* has_hand, int32_t* valid, void* stream) {
  HN_CHECK_ARG(records && keypoints && crop_box && has_hand && valid, "hn_unpack_records: null pointer");
  HN_CHECK_ARG(rows >= 0 && joints > 0, "bad dims");
  HN_CHECK_ARG(rec_bytes >= kRecHead + 12 * joints && rec_bytes % 8 == 0, "rec_bytes must be a multiple of 8 >= 40 + 12*joints");
  if (rows == 0) return HN_OK;
  const long total = (long)rows * (rec_bytes / 4);
  const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(unpack_records_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const unsigned*)records, rows,
                     joints * 3, rec_bytes / 4, keypoints, (long long*)crop_box, has_hand, valid);
  HN_CHECK_LAUNCH("unpack_records_kernel");
  return HN_OK;
}

extern "C" int hn_nonfinite_count_f32(const float* x, int64_t count, int32_t* flag, void* stream) {
  HN_CHECK_ARG(x && flag && count >= 0, "hn_nonfinite_count_f32: bad arguments");
  if (count == 0) return HN_OK;
  const int grid = (int)((count + 255) / 256 < 256 ? (count + 255) / 256 : 256);
  hipLaunchKernelGGL(nonfinite_count_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (long)count, flag);
  HN_CHECK_LAUNCH("nonfinite_count_kernel");
  return HN_OK;
}

// ---------------------------------------------------------------------------------------
// fp32 NHWC(4) image -> the stem image of hn_conv_stem_f16x3 / hn_conv_stem_pool_f16x3: two fp16 planes (hi, lo) of
// [n][h + 2b][w + 2b][4] with a zero border of b pixels (the A2J crops; the FCOS image is written in this form by the
// preprocess kernel).  One thread per bordered pixel: 16 B read, 8 B + 8 B written.
// ---------------------------------------------------------------------------------------
namespace {
typedef _Float16 f16x4s __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stem_image_kernel(const float* __restrict__ x, _Float16* __restrict__ dst, int n, int h,
                                                         int w, int b, int* range_flag, int* __restrict__ valid) {
  const int hb = h + 2 * b, wb = w + 2 * b;
  const long total = (long)n * hb * wb;
  _Float16* lo_plane = dst + total * 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xx = (int)(i % wb);
    const long t = i / wb;
    const int yy = (int)(t % hb);
    const int img = (int)(t / hb);
    f16x4s hi = {(_Float16)0, (_Float16)0, (_Float16)0, (_Float16)0}, lo = hi;
    const int sy = yy - b, sx = xx - b;
    if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((long)img * h + sy) * w + sx) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (range_flag) hn::range_note_input(range_flag, v[e]);
        float ve = v[e];
        // a non-finite pixel: mark the image (every writer stores the same value; images with valid == 0 stay 0) and keep
        // the value OUT of the network -- the aggregation writes the NaN row of a marked image whatever the convolutions
        // compute for it, and with no NaN of the caller's inside, a NaN activation always means a defect (range contract)
        if (valid && !(fabsf(ve) <= 3.402823466e38f)) {
          if (valid[img] == 1) valid[img] = 2;
          ve = 0.f;
        }
        const _Float16 hh = (_Float16)ve;
        hi[e] = hh;
        lo[e] = (_Float16)(ve - (float)hh);
      }
    }
    *reinterpret_cast<f16x4s*>(dst + i * 4) = hi;
    *reinterpret_cast<f16x4s*>(lo_plane + i * 4) = lo;
  }
}
}  // namespace

extern "C" int hn_stem_image_nhwc4(const float* x, int n, int h, int w, int border, void* dst16, void* stream) {
  return hn_stem_image_nhwc4_valid(x, n, h, w, border, dst16, nullptr, stream);
}

extern "C" int hn_stem_image_nhwc4_valid(const float* x, int n, int h, int w, int border, void* dst16, int32_t* valid,
                                         void* stream) {
  HN_CHECK_ARG(x && dst16, "hn_stem_image_nhwc4: null pointer");
  HN_CHECK_ARG(n > 0 && h > 0 && w > 0 && border >= 0 && border <= 4, "bad dims");
  HN_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)dst16 % 8 == 0, "unaligned tensors");
  const long total = (long)n * (h + 2 * border) * (w + 2 * border);
  const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  hipLaunchKernelGGL(stem_image_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (_Float16*)dst16, n, h, w, border,
                     hn::range_flag_ptr(), valid);
  HN_CHECK_LAUNCH("stem_image_kernel");
  return HN_OK;
}
