// GroupNorm + ReLU backward over the FPN levels of one FCOS tower layer, and the statistics it needs.
// The forward keeps only the folded tables scale = gamma * rstd, shift = beta - mean * scale; the backward wants mean and rstd
// themselves, so hn_groupnorm_stats_levels_f32 recomputes them from the raw output y the way gn_partial + gn_finalize do
// (groupnorm.hip): fp32 partial sums per 64-pixel chunk in a fixed order, an fp64 combine.
//
// With z = fma(y, scale, shift) (the forward's expression, affine_split_body.h), gm = g where z > 0 else 0,
// xh = (y - mean) * rstd, t = gm * gamma[c] and per (level, image, group) s1 = sum t, s2 = sum t * xh, M = h w C / G:
//   dy = rstd * (t - s1 / M - xh * s2 / M),   d_gamma[c] = sum gm * xh,   d_beta[c] = sum gm   (over levels, images, pixels)
// Three launches over the fixed list of SLOTS (level, image, 64-pixel chunk):
//   partial : one workgroup per slot; per channel sum gm and sum gm * xh (a thread owns 4 channels of every rows_par-th pixel,
//             the threads of a channel are added through LDS in thread order) -> ws [slot][C][2]
//   finalize: one wave per output -- per (level, image, group) s1 / M and s2 / M, per channel d_gamma and d_beta: the lanes
//             stride over the partials (fixed assignment), fp64 butterfly
//   apply   : one workgroup per slot, elementwise, writes dy
// No atomics, every output written once, the same bytes on every run.  y, g and dy are fp32 NHWC, dense or channel slices;
// nothing here writes the split format.
#include "hn_common.h"
#include "../../include/handnet_hip_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kChunk = 64;     // pixels of a slot
constexpr int kNT = 256;
constexpr int kMaxC = 512;

struct GnLevel {
  const float *y, *g, *scale, *shift;
  float *mean, *rstd, *dy;
  int hw, chunks, first_slot;
};
struct GnParams {
  GnLevel lv[HN_FCOS_MAX_LEVELS];
  int levels, n, c, groups, ys, gs, dys, ts, slots;
  float eps;
  const float* gamma;
  float* part;      // [slot][C][2] (statistics: [slot][G][2])
  float* tab;       // [level][n][G][2]: s1 / M, s2 / M
  float *d_gamma, *d_beta;
};

__device__ __forceinline__ void load_levels(const GnParams& p, GnLevel* slv) {
#pragma unroll
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l)
    if ((int)threadIdx.x == l) slv[l] = p.lv[l];   // (a dynamic index into the by-value argument would go through scratch)
  __syncthreads();
}

__device__ __forceinline__ int level_of_slot(const GnLevel* slv, int levels, int slot) {
  int li = 0;
  for (int l = 1; l < levels; ++l)
    if (slot >= slv[l].first_slot) li = l;
  return li;
}

// ---- statistics ----
__global__ __launch_bounds__(kNT) void gn_stats_partial_levels_kernel(const GnParams p) {
  __shared__ GnLevel slv[HN_FCOS_MAX_LEVELS];
  __shared__ float lds[2 * kNT];
  load_levels(p, slv);
  const int slot = (int)blockIdx.x;
  const GnLevel L = slv[level_of_slot(slv, p.levels, slot)];
  const int ls = slot - L.first_slot;
  const int img = ls / L.chunks, chunk = ls - img * L.chunks;
  const int cols = p.c >> 2, rows_par = kNT / cols;
  const int tid = (int)threadIdx.x, col = tid % cols, rl = tid / cols;
  const int r0 = chunk * kChunk, r1 = min(r0 + kChunk, L.hw);
  float s = 0.f, ss = 0.f;
  if (rl < rows_par)
    for (int r = r0 + rl; r < r1; r += rows_par) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(L.y + ((size_t)img * L.hw + r) * (size_t)p.ys + col * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s += v[e];
        ss = __builtin_fmaf(v[e], v[e], ss);
      }
    }
  lds[tid] = s;
  lds[kNT + tid] = ss;
  __syncthreads();
  const int cpg4 = (p.c / p.groups) >> 2;
  for (int g = tid; g < p.groups; g += kNT) {
    float ts = 0.f, tss = 0.f;
    for (int rr = 0; rr < rows_par; ++rr)
      for (int q = 0; q < cpg4; ++q) {
        ts += lds[rr * cols + g * cpg4 + q];
        tss += lds[kNT + rr * cols + g * cpg4 + q];
      }
    float* o = p.part + ((size_t)slot * p.groups + g) * 2;
    o[0] = ts;
    o[1] = tss;
  }
}

// one wave per (level, image, group)
__global__ __launch_bounds__(kNT) void gn_stats_finalize_levels_kernel(const GnParams p) {
  __shared__ GnLevel slv[HN_FCOS_MAX_LEVELS];
  load_levels(p, slv);
  const int lane = threadIdx.x & 63;
  const int id = (int)blockIdx.x * (kNT >> 6) + ((int)threadIdx.x >> 6);
  const int per = p.n * p.groups;
  if (id >= p.levels * per) return;
  const int li = id / per, rem = id - li * per;
  const int img = rem / p.groups, g = rem - img * p.groups;
  const GnLevel L = slv[li];
  double s = 0.0, ss = 0.0;
  for (int k = lane; k < L.chunks; k += 64) {
    const float* pp = p.part + ((size_t)(L.first_slot + img * L.chunks + k) * p.groups + g) * 2;
    s += (double)pp[0];
    ss += (double)pp[1];
  }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    ss += __shfl_xor(ss, o);
  }
  if (lane == 0) {
    const double cnt = (double)L.hw * (p.c / p.groups);
    const double mean = s / cnt;
    double var = ss / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    L.mean[img * p.groups + g] = (float)mean;
    L.rstd[img * p.groups + g] = (float)(1.0 / sqrt(var + (double)p.eps));
  }
}

// ---- backward ----
__global__ __launch_bounds__(kNT) void gn_relu_bwd_partial_kernel(const GnParams p) {
  __shared__ GnLevel slv[HN_FCOS_MAX_LEVELS];
  __shared__ float lds[2 * 4 * kNT];
  load_levels(p, slv);
  const int slot = (int)blockIdx.x;
  const GnLevel L = slv[level_of_slot(slv, p.levels, slot)];
  const int ls = slot - L.first_slot;
  const int img = ls / L.chunks, chunk = ls - img * L.chunks;
  const int cols = p.c >> 2, rows_par = kNT / cols;
  const int tid = (int)threadIdx.x, col = tid % cols, rl = tid / cols;
  const int r0 = chunk * kChunk, r1 = min(r0 + kChunk, L.hw);
  float sg[4] = {0.f, 0.f, 0.f, 0.f}, sx[4] = {0.f, 0.f, 0.f, 0.f};
  if (rl < rows_par) {
    const int grp = (col * 4) / (p.c / p.groups);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(L.scale + (size_t)img * p.ts + col * 4);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(L.shift + (size_t)img * p.ts + col * 4);
    const float mean = L.mean[img * p.groups + grp], rstd = L.rstd[img * p.groups + grp];
    for (int r = r0 + rl; r < r1; r += rows_par) {
      const size_t pix = (size_t)img * L.hw + r;
      const f32x4 yv = *reinterpret_cast<const f32x4*>(L.y + pix * (size_t)p.ys + col * 4);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(L.g + pix * (size_t)p.gs + col * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gm = __builtin_fmaf(yv[e], sc[e], sh[e]) > 0.f ? gv[e] : 0.f;
        const float xh = (yv[e] - mean) * rstd;
        sg[e] += gm;
        sx[e] = __builtin_fmaf(gm, xh, sx[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lds[e * kNT + tid] = sg[e];
    lds[(4 + e) * kNT + tid] = sx[e];
  }
  __syncthreads();
  for (int ch = tid; ch < p.c; ch += kNT) {
    const int cq = ch >> 2, e = ch & 3;
    float a = 0.f, b = 0.f;
    for (int rr = 0; rr < rows_par; ++rr) {
      a += lds[e * kNT + rr * cols + cq];
      b += lds[(4 + e) * kNT + rr * cols + cq];
    }
    float* o = p.part + ((size_t)slot * p.c + ch) * 2;
    o[0] = a;
    o[1] = b;
  }
}

// one wave per output: first the (level, image, group) pairs s1 / M, s2 / M, then the channels' d_gamma, d_beta
__global__ __launch_bounds__(kNT) void gn_relu_bwd_finalize_kernel(const GnParams p) {
  __shared__ GnLevel slv[HN_FCOS_MAX_LEVELS];
  load_levels(p, slv);
  const int lane = threadIdx.x & 63;
  const int id = (int)blockIdx.x * (kNT >> 6) + ((int)threadIdx.x >> 6);
  const int per = p.n * p.groups, ngrp = p.levels * per;
  if (id >= ngrp + p.c) return;
  double s1 = 0.0, s2 = 0.0;
  if (id < ngrp) {
    const int li = id / per, rem = id - li * per;
    const int img = rem / p.groups, g = rem - img * p.groups;
    const GnLevel L = slv[li];
    const int cpg = p.c / p.groups;
    const int items = L.chunks * cpg;
    for (int k = lane; k < items; k += 64) {
      const int chunk = k / cpg, ch = g * cpg + (k - chunk * cpg);
      const float* pp = p.part + ((size_t)(L.first_slot + img * L.chunks + chunk) * p.c + ch) * 2;
      const double gm = (double)p.gamma[ch];
      s1 += gm * (double)pp[0];
      s2 += gm * (double)pp[1];
    }
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
      const double cnt = (double)L.hw * cpg;
      float* o = p.tab + (size_t)id * 2;
      o[0] = (float)(s1 / cnt);
      o[1] = (float)(s2 / cnt);
    }
  } else {
    const int ch = id - ngrp;
    for (int k = lane; k < p.slots; k += 64) {
      const float* pp = p.part + ((size_t)k * p.c + ch) * 2;
      s1 += (double)pp[0];
      s2 += (double)pp[1];
    }
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
      p.d_beta[ch] = (float)s1;
      p.d_gamma[ch] = (float)s2;
    }
  }
}

__global__ __launch_bounds__(kNT) void gn_relu_bwd_apply_kernel(const GnParams p) {
  __shared__ GnLevel slv[HN_FCOS_MAX_LEVELS];
  load_levels(p, slv);
  const int slot = (int)blockIdx.x;
  const int li = level_of_slot(slv, p.levels, slot);
  const GnLevel L = slv[li];
  const int ls = slot - L.first_slot;
  const int img = ls / L.chunks, chunk = ls - img * L.chunks;
  const int cols = p.c >> 2, rows_par = kNT / cols;
  const int tid = (int)threadIdx.x, col = tid % cols, rl = tid / cols;
  if (rl >= rows_par) return;
  const int r0 = chunk * kChunk, r1 = min(r0 + kChunk, L.hw);
  const int grp = (col * 4) / (p.c / p.groups);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(L.scale + (size_t)img * p.ts + col * 4);
  const f32x4 sh = *reinterpret_cast<const f32x4*>(L.shift + (size_t)img * p.ts + col * 4);
  const f32x4 gam = *reinterpret_cast<const f32x4*>(p.gamma + col * 4);
  const float mean = L.mean[img * p.groups + grp], rstd = L.rstd[img * p.groups + grp];
  const float* tb = p.tab + ((size_t)(li * p.n + img) * p.groups + grp) * 2;
  const float m1 = tb[0], m2 = tb[1];
  for (int r = r0 + rl; r < r1; r += rows_par) {
    const size_t pix = (size_t)img * L.hw + r;
    const f32x4 yv = *reinterpret_cast<const f32x4*>(L.y + pix * (size_t)p.ys + col * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(L.g + pix * (size_t)p.gs + col * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gm = __builtin_fmaf(yv[e], sc[e], sh[e]) > 0.f ? gv[e] : 0.f;
      const float xh = (yv[e] - mean) * rstd;
      const float t = gm * gam[e];
      o[e] = rstd * __builtin_fmaf(-xh, m2, t - m1);
    }
    *reinterpret_cast<f32x4*>(L.dy + pix * (size_t)p.dys + col * 4) = o;
  }
}

// the checks and the slot list that the workspace query and the launches share
int plan_of(const hn_gn_bwd_levels* lv, int n, int c, int groups, GnParams& p, int64_t& ws_bytes) {
  HN_CHECK_ARG(lv, "hn_groupnorm_relu_backward: null pointer");
  HN_CHECK_ARG(lv->count >= 1 && lv->count <= HN_FCOS_MAX_LEVELS, "level count must be 1..%d", HN_FCOS_MAX_LEVELS);
  HN_CHECK_ARG(n > 0 && c > 0 && c % 8 == 0 && c <= kMaxC, "need c %% 8 == 0 and c <= %d (got %d)", kMaxC, c);
  HN_CHECK_ARG(groups > 0 && c % groups == 0 && (c / groups) % 8 == 0, "channels per group must be a multiple of 8 (c %d, groups %d)",
               c, groups);
  int64_t slots = 0;
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l) {
    GnLevel& t = p.lv[l];
    t.y = t.g = t.scale = t.shift = nullptr;
    t.mean = t.rstd = t.dy = nullptr;
    t.hw = t.chunks = 1; t.first_slot = 0x7fffffff;
    if (l >= lv->count) continue;
    HN_CHECK_ARG(lv->h[l] > 0 && lv->w[l] > 0, "level %d: empty map", l);
    HN_CHECK_ARG((int64_t)lv->h[l] * lv->w[l] < ((int64_t)1 << 30), "level %d: too many pixels", l);
    t.hw = lv->h[l] * lv->w[l];
    t.chunks = hn::cdiv(t.hw, kChunk);
    t.first_slot = (int)slots;
    slots += (int64_t)n * t.chunks;
    HN_CHECK_ARG(slots < ((int64_t)1 << 30), "too many pixels");
  }
  p.levels = lv->count; p.n = n; p.c = c; p.groups = groups; p.slots = (int)slots;
  ws_bytes = (slots * c * 2 + (int64_t)lv->count * n * groups * 2) * 4;
  return HN_OK;
}

bool aligned16(const void* q) { return (uintptr_t)q % 16 == 0; }

}  // namespace

extern "C" int64_t hn_groupnorm_relu_backward_ws_bytes(const hn_gn_bwd_levels* lv, int n, int c, int groups) {
  GnParams p;
  int64_t bytes;
  return plan_of(lv, n, c, groups, p, bytes) == HN_OK ? bytes : -1;
}

extern "C" int hn_groupnorm_stats_levels_f32(const hn_gn_bwd_levels* lv, int n, int c, int groups, int y_pix_stride, float eps,
                                             void* ws, int64_t ws_bytes, void* stream) {
  GnParams p;
  int64_t need;
  const int st_ = plan_of(lv, n, c, groups, p, need);
  if (st_ != HN_OK) return st_;
  HN_CHECK_ARG(ws && ws_bytes >= need && aligned16(ws), "workspace too small (%lld < %lld bytes) or unaligned", (long long)ws_bytes,
               (long long)need);
  HN_CHECK_ARG(eps >= 0.f, "bad eps");
  p.ys = y_pix_stride ? y_pix_stride : c;
  HN_CHECK_ARG(p.ys >= c && p.ys % 4 == 0, "bad pixel stride %d (floats; a multiple of 4, >= c)", p.ys);
  p.gs = p.dys = p.ts = 0;
  for (int l = 0; l < lv->count; ++l) {
    HN_CHECK_ARG(lv->y[l] && lv->mean[l] && lv->rstd[l], "level %d: null pointer", l);
    HN_CHECK_ARG(aligned16(lv->y[l]), "level %d: y is not 16-byte aligned", l);
    p.lv[l].y = lv->y[l]; p.lv[l].mean = lv->mean[l]; p.lv[l].rstd = lv->rstd[l];
  }
  p.eps = eps; p.gamma = nullptr; p.part = (float*)ws; p.tab = nullptr; p.d_gamma = p.d_beta = nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_stats_partial_levels_kernel, dim3(p.slots), dim3(kNT), 0, st, p);
  HN_CHECK_LAUNCH("gn_stats_partial_levels_kernel");
  hipLaunchKernelGGL(gn_stats_finalize_levels_kernel, dim3(hn::cdiv((int64_t)p.levels * n * groups, kNT / 64)), dim3(kNT), 0, st, p);
  HN_CHECK_LAUNCH("gn_stats_finalize_levels_kernel");
  return HN_OK;
}

extern "C" int hn_groupnorm_relu_backward_f32(const hn_gn_bwd_levels* lv, int n, int c, int groups, int y_pix_stride,
                                              int g_pix_stride, int dy_pix_stride, int table_stride, const float* gamma,
                                              float* d_gamma, float* d_beta, void* ws, int64_t ws_bytes, void* stream) {
  GnParams p;
  int64_t need;
  const int st_ = plan_of(lv, n, c, groups, p, need);
  if (st_ != HN_OK) return st_;
  HN_CHECK_ARG(gamma && d_gamma && d_beta, "hn_groupnorm_relu_backward_f32: null pointer");
  HN_CHECK_ARG(ws && ws_bytes >= need && aligned16(ws), "workspace too small (%lld < %lld bytes) or unaligned", (long long)ws_bytes,
               (long long)need);
  p.ys = y_pix_stride ? y_pix_stride : c;
  p.gs = g_pix_stride ? g_pix_stride : c;
  p.dys = dy_pix_stride ? dy_pix_stride : c;
  p.ts = table_stride ? table_stride : c;
  HN_CHECK_ARG(p.ys >= c && p.ys % 4 == 0 && p.gs >= c && p.gs % 4 == 0 && p.dys >= c && p.dys % 4 == 0,
               "bad pixel stride (floats; multiples of 4, >= c): y %d, g %d, dy %d", p.ys, p.gs, p.dys);
  HN_CHECK_ARG(p.ts >= c && p.ts % 4 == 0, "bad table stride %d (floats; a multiple of 4, >= c)", p.ts);
  HN_CHECK_ARG(aligned16(gamma), "gamma is not 16-byte aligned");
  for (int l = 0; l < lv->count; ++l) {
    HN_CHECK_ARG(lv->y[l] && lv->g[l] && lv->scale[l] && lv->shift[l] && lv->mean[l] && lv->rstd[l] && lv->dy[l],
                 "level %d: null pointer", l);
    HN_CHECK_ARG(aligned16(lv->y[l]) && aligned16(lv->g[l]) && aligned16(lv->dy[l]) && aligned16(lv->scale[l]) && aligned16(lv->shift[l]),
                 "level %d: a tensor or table is not 16-byte aligned", l);
    GnLevel& t = p.lv[l];
    t.y = lv->y[l]; t.g = lv->g[l]; t.scale = lv->scale[l]; t.shift = lv->shift[l];
    t.mean = lv->mean[l]; t.rstd = lv->rstd[l]; t.dy = lv->dy[l];
  }
  p.eps = 0.f; p.gamma = gamma; p.d_gamma = d_gamma; p.d_beta = d_beta;
  p.part = (float*)ws;
  p.tab = p.part + (size_t)p.slots * c * 2;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_relu_bwd_partial_kernel, dim3(p.slots), dim3(kNT), 0, st, p);
  HN_CHECK_LAUNCH("gn_relu_bwd_partial_kernel");
  hipLaunchKernelGGL(gn_relu_bwd_finalize_kernel, dim3(hn::cdiv((int64_t)p.levels * n * groups + c, kNT / 64)), dim3(kNT), 0, st, p);
  HN_CHECK_LAUNCH("gn_relu_bwd_finalize_kernel");
  hipLaunchKernelGGL(gn_relu_bwd_apply_kernel, dim3(p.slots), dim3(kNT), 0, st, p);
  HN_CHECK_LAUNCH("gn_relu_bwd_apply_kernel");
  return HN_OK;
}
