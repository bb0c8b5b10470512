// Adjoint of the nearest-neighbour read of a coarser map: the top-down path of the FCOS FPN's backward.
// The forward (res_mode 2 of the convolution epilogues) adds coarse pixel (floor(o rh / oh), floor(p rw / ow)) to fine pixel
// (o, p); the adjoint hands every fine pixel's gradient to the coarse pixel it read:
//   out[i][s][t][ch] = sum of g[i][o][p][ch] over the o with floor(o rh / oh) = s and the p with floor(p rw / ow) = t.
// floor(o rh / oh) = s  <=>  ceil(s oh / rh) <= o < ceil((s + 1) oh / rh): a contiguous range per axis, never empty while
// rh <= oh (consecutive o map to coarse rows at most one apart, and o = 0 maps to 0, o = oh - 1 to rh - 1).
// A thread owns four channels of one coarse pixel and adds its source pixels as ONE fp32 chain in (row, column) order, started
// from the first term.  Every element is written once; no atomics, no memset.  Plain loads and stores.
#include "hn_common.h"
#include "../../include/handnet_hip_train_fpn.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kNT = 256;

struct UpParams {
  const float* g;
  float* out;
  int oh, ow, rh, rw, c4, gs, os;         // c4 = c / 4; strides in floats
  int64_t total;                          // n * rh * rw * c4 threads with work
};

__device__ __forceinline__ int ceil_div(int64_t a, int b) { return (int)((a + b - 1) / b); }

__global__ __launch_bounds__(kNT) void upsample_nearest_bwd_f32_kernel(const UpParams p) {
  const int64_t e = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (e >= p.total) return;
  const int q = (int)(e % p.c4);
  const int64_t pix = e / p.c4;
  const int t = (int)(pix % p.rw);
  const int64_t rest = pix / p.rw;
  const int s = (int)(rest % p.rh);
  const int64_t img = rest / p.rh;
  const int o0 = ceil_div((int64_t)s * p.oh, p.rh), o1 = min(p.oh, ceil_div((int64_t)(s + 1) * p.oh, p.rh));
  const int p0 = ceil_div((int64_t)t * p.ow, p.rw), p1 = min(p.ow, ceil_div((int64_t)(t + 1) * p.ow, p.rw));
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  bool first = true;
  for (int o = o0; o < o1; ++o) {
    const float* row = p.g + ((size_t)(img * p.oh + o) * p.ow) * (size_t)p.gs + 4 * q;
    for (int x = p0; x < p1; ++x) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + (size_t)x * p.gs);
      sum = first ? v : sum + v;
      first = false;
    }
  }
  *reinterpret_cast<f32x4*>(p.out + (size_t)pix * p.os + 4 * q) = sum;
}

}  // namespace

extern "C" int hn_upsample_nearest_backward_f32(const float* g, int n, int oh, int ow, int rh, int rw, int c, int g_pix_stride,
                                                int out_pix_stride, float* out, void* stream) {
  HN_CHECK_ARG(g && out, "hn_upsample_nearest_backward_f32: null pointer");
  HN_CHECK_ARG(n > 0 && oh > 0 && ow > 0 && rh > 0 && rw > 0, "hn_upsample_nearest_backward_f32: empty map");
  HN_CHECK_ARG(c > 0 && c % 4 == 0, "need c %% 4 == 0 (got %d)", c);
  // the plan: every coarse pixel has at least one source (the ranges above are never empty) exactly while rh <= oh, rw <= ow
  HN_CHECK_ARG(rh <= oh && rw <= ow, "the coarse map %d x %d is larger than the fine map %d x %d", rh, rw, oh, ow);
  UpParams p;
  p.g = g; p.out = out; p.oh = oh; p.ow = ow; p.rh = rh; p.rw = rw; p.c4 = c / 4;
  p.gs = g_pix_stride ? g_pix_stride : c;
  p.os = out_pix_stride ? out_pix_stride : c;
  HN_CHECK_ARG(p.gs >= c && p.gs % 4 == 0 && p.os >= c && p.os % 4 == 0, "bad pixel stride %d / %d (floats; multiples of 4, >= c)",
               p.gs, p.os);
  HN_CHECK_ARG((uintptr_t)g % 16 == 0 && (uintptr_t)out % 16 == 0, "unaligned gradient / output (16 bytes)");
  HN_CHECK_ARG((int64_t)n * oh * ow < ((int64_t)1 << 30), "too many pixels");
  p.total = (int64_t)n * rh * rw * p.c4;
  hipLaunchKernelGGL(upsample_nearest_bwd_f32_kernel, dim3(hn::cdiv(p.total, kNT)), dim3(kNT), 0, (hipStream_t)stream, p);
  HN_CHECK_LAUNCH("upsample_nearest_bwd_f32_kernel");
  return HN_OK;
}
