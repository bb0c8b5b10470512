// Weight and bias gradient of a 3x3 / stride 1 / pad 1 convolution on the f32-input MFMA (v_mfma_f32_32x32x2_f32): the hot
// path of the FCOS towers' backward.
//   dW[co][r][s][ci] = sum over levels, images, pixels q   dy[q][co] * a[q + (r - 1, s - 1)][ci]   (zero outside the map)
//   db[co]           = sum dy[.][co]
// a = float(hi) + float(lo) of the S32 activation the forward read (exact in fp32), dy fp32 NHWC; both may be channel slices.
//
// Per tap this is a GEMM with M = Cout, N = Cin and K = all pixels.  Both operands are k-major already: lane l of the A operand
// wants dy[pixel k = l >> 5][co = l & 31], lane l of B wants a[pixel k + tap][ci = l & 31] -- 32 consecutive channels of one
// pixel in NHWC and in S32 alike, so nothing is transposed.
//
// The sweep.  K is walked in SEGMENTS of at most 16 pixels of one map row, in the fixed order (level, image, row, column).  A
// workgroup (4 waves) owns a 32-channel co tile, a 128-channel ci group and a RANGE of consecutive segments.  Per segment it
// stages, as fp32 in LDS, the three rows of `a` around the segment with a one-pixel halo (hi + lo added once on the way in,
// zeros outside the map) and the segment's dy (zeros past the row's end).  Wave v keeps the nine taps of the 32 x 32 tile
// (co tile, ci group's block v) in 9 x 16 accumulator registers; a tap is a shifted LDS address of the same staged `a`.  One
// MFMA consumes two pixels (k = 0, 1), in pixel order: an accumulator is ONE fmaf chain over the pixels of the range.  A pixel
// past the end of a row multiplies a staged zero: the chain passes it unchanged.
// The pixel pitch of `a` in LDS is 160 floats: the two half-waves (pixels k and k + 1) read disjoint bank halves.
// Every workgroup writes its partial dW (and, from ci group 0, a plainly summed partial db) to the workspace; the second launch
// adds the partials in range order and writes every element once.  No memset, no atomics; two runs give the same bytes.
// Plain compiler-scheduled loads and stores: no counted waits.
#include "hn_common.h"
#include "../../include/handnet_hip_train.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int kSeg = 16;                  // pixels of a segment
constexpr int kHC = kSeg + 2;             // with the halo
constexpr int kCiGroup = 128;             // input channels of a workgroup (4 waves x 32)
constexpr int kPitch = 160;               // floats per staged pixel of `a`
constexpr int kNT = 256;
constexpr int kMaxRanges = 64;            // K ranges (partial sums: ranges x 9 x Cout x Cin floats)
constexpr int kWantGroups = 512;          // workgroups the plan aims at (two per CU)
constexpr int kMaxC = 512;

struct WgLevel {
  const _Float16* a;
  const float* dy;
  int h, w, sx, segs_img, first_seg;      // sx = segments per row, segs_img = h * sx
};
struct WgParams {
  WgLevel lv[HN_FCOS_MAX_LEVELS];
  int levels, n, cin, cout, as, dys, segs, spr, ranges;
  float* ws;                              // [range][co][tap][ci] partial dW, then [range][co] partial db
};

__global__ __launch_bounds__(kNT, 2) void wgrad3x3_f32_sweep_kernel(const WgParams p) {
  __shared__ __attribute__((aligned(16))) float alds[3 * kHC * kPitch];
  __shared__ __attribute__((aligned(16))) float glds[kSeg * 32];
  __shared__ WgLevel slv[HN_FCOS_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l)
    if ((int)threadIdx.x == l) slv[l] = p.lv[l];   // (a dynamic index into the by-value argument would go through scratch)
  __syncthreads();
  const int range = (int)blockIdx.x, co0 = (int)blockIdx.y * 32, ci0 = (int)blockIdx.z * kCiGroup;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cw = min(kCiGroup, p.cin - ci0);       // channels of this group: a multiple of 32
  const bool wave_on = wave * 32 < cw;
  const int s0 = range * p.spr, s1 = min(p.segs, s0 + p.spr);

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float dbv = 0.f;

  for (int seg = s0; seg < s1; ++seg) {
    int li = 0;
    for (int l = 1; l < p.levels; ++l)
      if (seg >= slv[l].first_seg) li = l;
    const WgLevel L = slv[li];
    const int ls = seg - L.first_seg;
    const int img = ls / L.segs_img;
    const int rem = ls - img * L.segs_img;
    const int y = rem / L.sx;
    const int x0 = (rem - y * L.sx) * kSeg;
    const int cols = min(kSeg, L.w - x0);
    __syncthreads();   // the previous segment's reads are done
    // a: 3 rows x 18 pixels x cw channels, a channel pair per thread
    for (int e = tid; e < 3 * kHC * (kCiGroup / 2); e += kNT) {
      const int hp = e >> 6, c = (e & 63) * 2;
      if (c >= cw) continue;
      const int hy = hp / kHC, hx = hp - hy * kHC;
      const int gy = y - 1 + hy, gx = x0 - 1 + hx;
      f32x2 v = {0.f, 0.f};
      if ((unsigned)gy < (unsigned)L.h && (unsigned)gx < (unsigned)L.w) {
        const int ch = ci0 + c;
        const _Float16* src = L.a + (((size_t)img * L.h + gy) * L.w + gx) * (size_t)p.as + (ch >> 5) * 64 + (ch & 31);
        const f16x2 hi = *reinterpret_cast<const f16x2*>(src);
        const f16x2 lo = *reinterpret_cast<const f16x2*>(src + 32);
        v[0] = (float)hi[0] + (float)lo[0];
        v[1] = (float)hi[1] + (float)lo[1];
      }
      *reinterpret_cast<f32x2*>(alds + hp * kPitch + c) = v;
    }
    // dy: 16 pixels x 32 columns, a column pair per thread
    {
      const int px = tid >> 4, c = (tid & 15) * 2;
      f32x2 v = {0.f, 0.f};
      if (px < cols)
        v = *reinterpret_cast<const f32x2*>(L.dy + (((size_t)img * L.h + y) * L.w + (x0 + px)) * (size_t)p.dys + co0 + c);
      *reinterpret_cast<f32x2*>(glds + px * 32 + c) = v;
    }
    __syncthreads();
    if (blockIdx.z == 0 && tid < 32)
      for (int px = 0; px < cols; ++px) dbv += glds[px * 32 + tid];
    if (wave_on) {
      const int pairs = (cols + 1) >> 1;
      const float* bl = alds + wave * 32 + (lane & 31);
      for (int j = 0; j < pairs; ++j) {
        const int px = 2 * j + (lane >> 5);
        const float av = glds[px * 32 + (lane & 31)];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            const float bv = bl[(r * kHC + px + s) * kPitch];
            acc[r * 3 + s] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[r * 3 + s], 0, 0, 0);
          }
      }
    }
  }
  if (wave_on) {
    // C/D layout of the 32x32 MFMA: column (ci) = lane & 31, row (co) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int ci = ci0 + wave * 32 + (lane & 31);
    float* dst = p.ws + (size_t)range * p.cout * 9 * p.cin;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        dst[((size_t)co * 9 + t) * p.cin + ci] = acc[t][r];
      }
  }
  if (blockIdx.z == 0 && tid < 32) p.ws[(size_t)p.ranges * p.cout * 9 * p.cin + (size_t)range * p.cout + co0 + tid] = dbv;
}

// one thread per dW element (then per db element): the ranges' partial sums in range order
__global__ __launch_bounds__(kNT) void wgrad3x3_f32_reduce_kernel(const float* __restrict__ ws, int ranges, int nw, int cout,
                                                                  float* __restrict__ dw, float* __restrict__ db) {
  const int e = (int)(blockIdx.x * kNT + threadIdx.x);
  if (e < nw) {
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < ranges; ++r) s += ws[(size_t)r * nw + e];
    dw[e] = s;
  } else if (e < nw + cout) {
    const float* src = ws + (size_t)ranges * nw + (e - nw);
    float s = 0.f;
    for (int r = 0; r < ranges; ++r) s += src[(size_t)r * cout];
    db[e - nw] = s;
  }
}

// the plan that the workspace query and the launch share
struct WgPlan {
  int segs, spr, ranges;
  int64_t ws_bytes;
};

int plan_of(const hn_wgrad_levels* lv, int n, int cin, int cout, WgPlan& pl) {
  HN_CHECK_ARG(lv, "hn_conv3x3_wgrad: null pointer");
  HN_CHECK_ARG(lv->count >= 1 && lv->count <= HN_FCOS_MAX_LEVELS, "level count must be 1..%d", HN_FCOS_MAX_LEVELS);
  HN_CHECK_ARG(n > 0 && cin > 0 && cin % 32 == 0 && cin <= kMaxC, "need cin %% 32 == 0 and cin <= %d (got %d)", kMaxC, cin);
  HN_CHECK_ARG(cout > 0 && cout % 32 == 0 && cout <= kMaxC, "need cout %% 32 == 0 and cout <= %d (got %d)", kMaxC, cout);
  int64_t segs = 0;
  for (int l = 0; l < lv->count; ++l) {
    HN_CHECK_ARG(lv->h[l] > 0 && lv->w[l] > 0, "level %d: empty map", l);
    segs += (int64_t)n * lv->h[l] * hn::cdiv(lv->w[l], kSeg);
    HN_CHECK_ARG(segs < ((int64_t)1 << 30), "too many pixels");
  }
  const int groups = (cout / 32) * hn::cdiv(cin, kCiGroup);
  const int cap = groups >= kWantGroups ? 1 : (kWantGroups / groups > kMaxRanges ? kMaxRanges : kWantGroups / groups);
  pl.segs = (int)segs;
  pl.spr = hn::cdiv(segs, cap);
  pl.ranges = hn::cdiv(segs, pl.spr);
  pl.ws_bytes = ((int64_t)pl.ranges * cout * 9 * cin + (int64_t)pl.ranges * cout) * 4;
  return HN_OK;
}

}  // namespace

extern "C" int64_t hn_conv3x3_wgrad_ws_bytes(const hn_wgrad_levels* lv, int n, int cin, int cout) {
  WgPlan pl;
  return plan_of(lv, n, cin, cout, pl) == HN_OK ? pl.ws_bytes : -1;
}

extern "C" int hn_conv3x3_wgrad_f32(const hn_wgrad_levels* lv, int n, int cin, int cout, int a_pix_stride, int dy_pix_stride,
                                    float* dw, float* db, void* ws, int64_t ws_bytes, void* stream) {
  WgPlan pl;
  const int st_ = plan_of(lv, n, cin, cout, pl);
  if (st_ != HN_OK) return st_;
  HN_CHECK_ARG(dw && db && ws, "hn_conv3x3_wgrad_f32: null pointer");
  HN_CHECK_ARG(ws_bytes >= pl.ws_bytes && (uintptr_t)ws % 4 == 0, "workspace too small (%lld < %lld bytes) or unaligned",
               (long long)ws_bytes, (long long)pl.ws_bytes);
  WgParams p;
  p.levels = lv->count; p.n = n; p.cin = cin; p.cout = cout;
  p.as = a_pix_stride ? a_pix_stride : 2 * cin;
  p.dys = dy_pix_stride ? dy_pix_stride : cout;
  HN_CHECK_ARG(p.as >= 2 * cin && p.as % 64 == 0, "bad activation pixel stride %d (halfs; a multiple of 64, >= 2 cin)", p.as);
  HN_CHECK_ARG(p.dys >= cout && p.dys % 4 == 0, "bad gradient pixel stride %d (floats; a multiple of 4, >= cout)", p.dys);
  p.segs = pl.segs; p.spr = pl.spr; p.ranges = pl.ranges;
  p.ws = (float*)ws;
  int segs = 0;
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l) {
    WgLevel& t = p.lv[l];
    if (l < lv->count) {
      HN_CHECK_ARG(lv->a16[l] && lv->dy[l], "level %d: null activation / gradient", l);
      HN_CHECK_ARG((uintptr_t)lv->a16[l] % 4 == 0 && (uintptr_t)lv->dy[l] % 16 == 0, "level %d: unaligned activation / gradient", l);
      t.a = (const _Float16*)lv->a16[l];
      t.dy = lv->dy[l];
      t.h = lv->h[l]; t.w = lv->w[l];
      t.sx = hn::cdiv(t.w, kSeg);
      t.segs_img = t.h * t.sx;
      t.first_seg = segs;
      segs += n * t.segs_img;
    } else {
      t.a = nullptr; t.dy = nullptr;
      t.h = t.w = t.sx = t.segs_img = 1; t.first_seg = 0x7fffffff;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wgrad3x3_f32_sweep_kernel, dim3(pl.ranges, cout / 32, hn::cdiv(cin, kCiGroup)), dim3(kNT), 0, st, p);
  HN_CHECK_LAUNCH("wgrad3x3_f32_sweep_kernel");
  const int nw = cout * 9 * cin;
  hipLaunchKernelGGL(wgrad3x3_f32_reduce_kernel, dim3(hn::cdiv(nw + cout, kNT)), dim3(kNT), 0, st, (const float*)ws, pl.ranges,
                     nw, cout, dw, db);
  HN_CHECK_LAUNCH("wgrad3x3_f32_reduce_kernel");
  return HN_OK;
}
