// Weight and bias gradient of a 1x1 / stride 1 convolution on the f32-input MFMA (v_mfma_f32_32x32x2_f32): the laterals of the
// FCOS FPN's backward.
//   dW[co][ci] = sum over the rows q   dy[q][co] * a[q][ci]          db[co] = sum dy[.][co]
// a = float(hi) + float(lo) of the S32 activation the forward read (exact in fp32), dy fp32 NHWC; both may be channel slices;
// a row is a pixel of any image of the map, a flat index: no rows of a map, no halo, no partly empty segments.
//
// One GEMM with M = Cout, N = Cin and K = the rows.  Both operands are k-major already, as in conv3x3_wgrad_f32.hip: lane l of
// the A operand wants dy[row k = l >> 5][co = l & 31], lane l of B wants a[row k][ci = l & 31] -- 32 consecutive channels of one
// pixel in NHWC and in S32 alike, so nothing is transposed.
//
// The sweep.  K is walked in CHUNKS of 32 rows.  A workgroup (4 waves) owns a 64-channel co tile, a 128-channel ci group and a
// RANGE of consecutive chunks.  Per chunk it stages, as fp32 in LDS, the chunk's `a` (hi + lo added once on the way in) and dy;
// rows past the end and channels past the tile's width are staged as zeros.  Wave v keeps two 32 x 32 tiles -- co half v & 1,
// ci blocks 2 (v >> 1) and 2 (v >> 1) + 1 of the group -- in 2 x 16 accumulator registers: with one tap there is room, and one dy
// read serves two MFMAs.  One MFMA consumes two rows (k = 0, 1), in row order: an accumulator is ONE fmaf chain over the rows
// of the range.  A row past the end multiplies a staged zero: the chain passes it unchanged.
// A half-wave reads 32 consecutive floats of one staged row: conflict-free at any pitch.
// Every workgroup writes its partial dW (and, from ci group 0, a plainly summed partial db) to the workspace; the second launch
// adds the partials in range order and writes every element once.  No memset, no atomics; two runs give the same bytes.
// Plain compiler-scheduled loads and stores: no counted waits.
#include "hn_common.h"
#include "../../include/handnet_hip_train_fpn.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kChunk = 32;                // rows of a chunk
constexpr int kCoTile = 64;               // output channels of a workgroup (2 wave halves x 32)
constexpr int kCiGroup = 128;             // input channels of a workgroup (2 wave halves x 2 tiles x 32)
constexpr int kNT = 256;
constexpr int kMaxRanges = 64;            // K ranges (partial sums: ranges x Cout x Cin floats)
constexpr int kWantGroups = 512;          // workgroups the plan aims at (two per CU)
constexpr int kMaxC = 512;

struct W1Params {
  const _Float16* a;
  const float* dy;
  int64_t rows;
  int cin, cout, as, dys, cpr, ranges;    // cpr = chunks per range
  float* ws;                              // [range][co][ci] partial dW, then [range][co] partial db
};

__global__ __launch_bounds__(kNT, 2) void wgrad1x1_f32_sweep_kernel(const W1Params p) {
  __shared__ __attribute__((aligned(16))) float alds[kChunk * kCiGroup];
  __shared__ __attribute__((aligned(16))) float glds[kChunk * kCoTile];
  const int range = (int)blockIdx.x, co0 = (int)blockIdx.y * kCoTile, ci0 = (int)blockIdx.z * kCiGroup;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cow = min(kCoTile, p.cout - co0);      // channels of this tile / group: multiples of 32
  const int ciw = min(kCiGroup, p.cin - ci0);
  const int coh = (wave & 1) * 32, cib = (wave >> 1) * 64;
  const bool on0 = coh < cow && cib < ciw, on1 = coh < cow && cib + 32 < ciw;
  const int64_t q0 = (int64_t)range * p.cpr * kChunk;
  const int64_t qe = q0 + (int64_t)p.cpr * kChunk, q1 = qe < p.rows ? qe : p.rows;

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  float dbv = 0.f;

  for (int64_t q = q0; q < q1; q += kChunk) {
    const int live = q1 - q < kChunk ? (int)(q1 - q) : kChunk;
    __syncthreads();   // the previous chunk's reads are done
    // a: 32 rows x 128 channels, four channels per thread
    for (int e = tid; e < kChunk * (kCiGroup / 4); e += kNT) {
      const int px = e >> 5, c = (e & 31) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (px < live && c < ciw) {
        const int ch = ci0 + c;
        const _Float16* src = p.a + (size_t)(q + px) * (size_t)p.as + (ch >> 5) * 64 + (ch & 31);
        const f16x4 hi = *reinterpret_cast<const f16x4*>(src);
        const f16x4 lo = *reinterpret_cast<const f16x4*>(src + 32);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (float)hi[k] + (float)lo[k];
      }
      *reinterpret_cast<f32x4*>(alds + px * kCiGroup + c) = v;
    }
    // dy: 32 rows x 64 columns, four columns per thread
    for (int e = tid; e < kChunk * (kCoTile / 4); e += kNT) {
      const int px = e >> 4, c = (e & 15) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (px < live && c < cow) v = *reinterpret_cast<const f32x4*>(p.dy + (size_t)(q + px) * (size_t)p.dys + co0 + c);
      *reinterpret_cast<f32x4*>(glds + px * kCoTile + c) = v;
    }
    __syncthreads();
    if (blockIdx.z == 0 && tid < cow)
      for (int px = 0; px < live; ++px) dbv += glds[px * kCoTile + tid];
    if (on0) {
      const int pairs = (live + 1) >> 1;
      const float* gl = glds + coh + (lane & 31);
      const float* bl = alds + cib + (lane & 31);
      for (int j = 0; j < pairs; ++j) {
        const int px = 2 * j + (lane >> 5);
        const float av = gl[px * kCoTile];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bl[px * kCiGroup], acc0, 0, 0, 0);
        if (on1) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bl[px * kCiGroup + 32], acc1, 0, 0, 0);
      }
    }
  }
  // C/D layout of the 32x32 MFMA: column (ci) = lane & 31, row (co) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  float* dst = p.ws + (size_t)range * p.cout * p.cin;
  const int ci = ci0 + cib + (lane & 31);
  if (on0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + coh + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      dst[(size_t)co * p.cin + ci] = acc0[r];
    }
  }
  if (on1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + coh + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      dst[(size_t)co * p.cin + ci + 32] = acc1[r];
    }
  }
  if (blockIdx.z == 0 && tid < cow) p.ws[(size_t)p.ranges * p.cout * p.cin + (size_t)range * p.cout + co0 + tid] = dbv;
}

// one thread per dW element (then per db element): the ranges' partial sums in range order
__global__ __launch_bounds__(kNT) void wgrad1x1_f32_reduce_kernel(const float* __restrict__ ws, int ranges, int nw, int cout,
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
struct W1Plan {
  int cpr, ranges;
  int64_t ws_bytes;
};

int plan_of(int64_t rows, int cin, int cout, W1Plan& pl) {
  HN_CHECK_ARG(rows > 0 && rows < ((int64_t)1 << 30), "hn_conv1x1_wgrad: rows must be 1 .. 2^30 - 1 (got %lld)", (long long)rows);
  HN_CHECK_ARG(cin > 0 && cin % 32 == 0 && cin <= kMaxC, "need cin %% 32 == 0 and cin <= %d (got %d)", kMaxC, cin);
  HN_CHECK_ARG(cout > 0 && cout % 32 == 0 && cout <= kMaxC, "need cout %% 32 == 0 and cout <= %d (got %d)", kMaxC, cout);
  const int chunks = hn::cdiv(rows, kChunk);
  const int groups = hn::cdiv(cout, kCoTile) * hn::cdiv(cin, kCiGroup);
  const int cap = groups >= kWantGroups ? 1 : (kWantGroups / groups > kMaxRanges ? kMaxRanges : kWantGroups / groups);
  pl.cpr = hn::cdiv(chunks, cap);
  pl.ranges = hn::cdiv(chunks, pl.cpr);
  pl.ws_bytes = ((int64_t)pl.ranges * cout * cin + (int64_t)pl.ranges * cout) * 4;
  return HN_OK;
}

}  // namespace

extern "C" int64_t hn_conv1x1_wgrad_ws_bytes(int64_t rows, int cin, int cout) {
  W1Plan pl;
  return plan_of(rows, cin, cout, pl) == HN_OK ? pl.ws_bytes : -1;
}

extern "C" int hn_conv1x1_wgrad_f32(const void* a16, const float* dy, int64_t rows, int cin, int cout, int a_pix_stride,
                                    int dy_pix_stride, float* dw, float* db, void* ws, int64_t ws_bytes, void* stream) {
  W1Plan pl;
  const int st_ = plan_of(rows, cin, cout, pl);
  if (st_ != HN_OK) return st_;
  HN_CHECK_ARG(a16 && dy && dw && db && ws, "hn_conv1x1_wgrad_f32: null pointer");
  HN_CHECK_ARG(ws_bytes >= pl.ws_bytes && (uintptr_t)ws % 4 == 0, "workspace too small (%lld < %lld bytes) or unaligned",
               (long long)ws_bytes, (long long)pl.ws_bytes);
  W1Params p;
  p.a = (const _Float16*)a16; p.dy = dy; p.rows = rows; p.cin = cin; p.cout = cout;
  p.as = a_pix_stride ? a_pix_stride : 2 * cin;
  p.dys = dy_pix_stride ? dy_pix_stride : cout;
  HN_CHECK_ARG(p.as >= 2 * cin && p.as % 64 == 0, "bad activation pixel stride %d (halfs; a multiple of 64, >= 2 cin)", p.as);
  HN_CHECK_ARG(p.dys >= cout && p.dys % 4 == 0, "bad gradient pixel stride %d (floats; a multiple of 4, >= cout)", p.dys);
  HN_CHECK_ARG((uintptr_t)a16 % 8 == 0 && (uintptr_t)dy % 16 == 0 && (uintptr_t)dw % 4 == 0 && (uintptr_t)db % 4 == 0,
               "unaligned activation (8 bytes) / gradient (16 bytes) / output");
  p.cpr = pl.cpr; p.ranges = pl.ranges;
  p.ws = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wgrad1x1_f32_sweep_kernel, dim3(pl.ranges, hn::cdiv(cout, kCoTile), hn::cdiv(cin, kCiGroup)), dim3(kNT), 0,
                     st, p);
  HN_CHECK_LAUNCH("wgrad1x1_f32_sweep_kernel");
  const int nw = cout * cin;
  hipLaunchKernelGGL(wgrad1x1_f32_reduce_kernel, dim3(hn::cdiv(nw + cout, kNT)), dim3(kNT), 0, st, (const float*)ws, pl.ranges,
                     nw, cout, dw, db);
  HN_CHECK_LAUNCH("wgrad1x1_f32_reduce_kernel");
  return HN_OK;
}
