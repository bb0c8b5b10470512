// Backward of the 3x3 / stride 1 / pad 1 head-output convolution of conv3x3_thin.hip (Cin % 32 == 0, at most 16 output
// columns on a map, weights shared over up to HN_FCOS_MAX_LEVELS maps): weight, bias and input gradients in fp32
// (DESIGN.md section 9t).  With gm = g where (col >= relu_cols or y > 0), else 0 -- torch's ReLU backward on the stored
// result -- and q = p - (r - 1, s - 1):
//   dW[co][r][s][ci] = sum over levels, images, pixels p   gm[q][co] * a[p][ci]          (a = float(hi) + float(lo), exact)
//   db[co]           = sum gm[.][co]
//   dA[p][ci]        = sum over members, co, r, s          gm[q][co] * w[co][r][s][ci]   (zero outside the map)
// One or two members (filter banks) read the same map; their columns are stacked (at most 16 together).
//
// The sweep: a lane owns ONE input channel; the masked gradients of a 2 x 32 pixel tile and its one-pixel halo sit in LDS
// (zeros outside the map and in the padding columns), every lane reads the same words (broadcast reads).  A workgroup
// (256 channels) owns a contiguous range of tiles of the fixed list (level, image, tile row, tile column):
//   phase A (dA): the lane's 9 x CT weights in registers, one accumulator per pixel, taps outer / columns inner, one store;
//   phase B (dW): 9 x CT accumulators in registers across ALL tiles of the range, per pixel one `a` value (two 2-byte
//                 loads, coalesced over the lanes: the hi and lo runs of S32 are contiguous) and 9 x CT FMAs.
// The two phases hold their registers one after the other (144 + 144 would not fit), so the tile's gradients are staged
// twice; `a` is read once and has no halo.  Partial dW / db of every workgroup go to the workspace; the second launch adds
// them in workgroup order.  Every output element is written exactly once, no memset, no atomics, fixed order.  Plain loads
// and stores, compiler-scheduled: no counted waits.
#include "hn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTR = 2, kTC = 32;                 // tile: rows x columns of pixels
constexpr int kHR = kTR + 2, kHC = kTC + 2;      // with the halo
constexpr int kNT = 256;                         // lanes = input channels of a workgroup
constexpr int kMaxCols = 16;                     // stacked output columns of the members of a map
constexpr int kMaxMembers = 2;
constexpr int kMaxUnits = 512;                   // workgroups per channel chunk (partial sums: kMaxUnits x 9 x cols x Cin floats)

struct BwdLevel {
  const _Float16* a;                 // S32 activation the forward read
  float* da;                         // gradient at it (already at the caller's channel offset), or null
  const float* y[kMaxMembers];       // the forward's outputs [n][h][w][cout_m]
  const float* g[kMaxMembers];       // upstream gradients, same layout
  int h, w, tx, tiles_img, first_tile;
};
struct BwdParams {
  BwdLevel lv[HN_FCOS_MAX_LEVELS];
  const float* wt[kMaxMembers];      // [cout_m][3][3][cin] fp32
  int cout[kMaxMembers], relu[kMaxMembers];
  int levels, n, cin, xs, das, ctot, tiles, tpu, units, want_dx;
  float* ws;                         // [chunk][unit][9 * ctot][256] partial dW, then [unit][ctot] partial db
};

template <int CT>
__device__ __forceinline__ void stage_tile(const BwdParams p, const BwdLevel L, int img, int y0, int x0, float* glds) {
  for (int e = threadIdx.x; e < kHR * kHC * CT; e += kNT) {
    const int hp = e / CT, c = e - hp * CT;
    const int hy = hp / kHC, hx = hp - hy * kHC;
    const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
    float v = 0.f;
    if (c < p.ctot && (unsigned)gy < (unsigned)L.h && (unsigned)gx < (unsigned)L.w) {
      const int m = c < p.cout[0] ? 0 : 1;
      const int cc = m ? c - p.cout[0] : c;
      // (selects, not a dynamic index: the by-value tables stay out of private memory)
      const size_t idx = (((size_t)img * L.h + gy) * L.w + gx) * (size_t)(m ? p.cout[1] : p.cout[0]) + cc;
      v = (m ? L.g[1] : L.g[0])[idx];
      if (cc < (m ? p.relu[1] : p.relu[0]) && !((m ? L.y[1] : L.y[0])[idx] > 0.f)) v = 0.f;
    }
    glds[e] = v;
  }
}

// level / image / origin of tile t of the fixed list; the level table is read from LDS (a dynamic index into the by-value
// kernel argument would send the whole argument through private memory)
__device__ __forceinline__ void tile_of(const BwdLevel* slv, int levels, int t, BwdLevel& L, int& img, int& y0, int& x0) {
  int li = 0;
  for (int l = 1; l < levels; ++l)
    if (t >= slv[l].first_tile) li = l;
  L = slv[li];
  const int lt = t - L.first_tile;
  img = lt / L.tiles_img;
  const int rem = lt - img * L.tiles_img;
  const int tyi = rem / L.tx;
  y0 = tyi * kTR;
  x0 = (rem - tyi * L.tx) * kTC;
}

// Two workgroups per CU (two waves per SIMD hide the LDS reads behind the other wave's FMAs): at CT = 16 the compiler then
// spills eight loop-invariant registers; plain compiler-scheduled loads, so a spill is only a cost, and it is the smaller one
// (profiles/NOTEBOOK.md, 2026-10-21).
template <int CT>
__global__ __launch_bounds__(kNT, 2) void thin_bwd_sweep_kernel(const BwdParams p) {
  __shared__ __attribute__((aligned(16))) float glds[kHR * kHC * CT];
  __shared__ BwdLevel slv[HN_FCOS_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l)
    if ((int)threadIdx.x == l) slv[l] = p.lv[l];
  __syncthreads();
  const int unit = (int)blockIdx.x, chunk = (int)blockIdx.y;
  const int ci = chunk * kNT + (int)threadIdx.x;
  // Cin below 256 (the tests' 32 and 64; the detector's maps have 256): the lanes past Cin are not switched off -- they run the
  // loops on channel 0, store nothing to dA and write workspace slots that the reduction never reads.  Correct, and wasteful
  // only off the production shape.
  const bool active = ci < p.cin;
  const int cic = active ? ci : 0;
  const int t0 = unit * p.tpu, t1 = min(p.tiles, t0 + p.tpu);
  const int a_off = (cic >> 5) * 64 + (cic & 31);

  if (p.want_dx) {
    // ---- phase A: dA of the range's pixels, complete per pixel ----
    float wr[9 * CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int m = c < p.cout[0] ? 0 : 1;
      const int cc = m ? c - p.cout[0] : c;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        wr[tap * CT + c] = (c < p.ctot && active) ? (m ? p.wt[1] : p.wt[0])[((size_t)cc * 9 + tap) * p.cin + cic] : 0.f;
    }
    for (int t = t0; t < t1; ++t) {
      BwdLevel L;
      int img, y0, x0;
      tile_of(slv, p.levels, t, L, img, y0, x0);
      __syncthreads();   // the previous tile's reads are done
      stage_tile<CT>(p, L, img, y0, x0, glds);
      __syncthreads();
      const int rows = min(kTR, L.h - y0), cols = min(kTC, L.w - x0);
      for (int ty = 0; ty < rows; ++ty)
        for (int tx = 0; tx < cols; ++tx) {
          float acc = 0.f;
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
              const f32x4* gp = reinterpret_cast<const f32x4*>(glds + ((ty + 2 - r) * kHC + (tx + 2 - s)) * CT);
#pragma unroll
              for (int c4 = 0; c4 < CT / 4; ++c4) {
                const f32x4 gv = gp[c4];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(gv[e], wr[(r * 3 + s) * CT + c4 * 4 + e], acc);
              }
            }
          if (active) L.da[(((size_t)img * L.h + (y0 + ty)) * L.w + (x0 + tx)) * (size_t)p.das + ci] = acc;
        }
    }
  }

  // ---- phase B: dW and db partial sums over the range ----
  float acc[9 * CT];
#pragma unroll
  for (int k = 0; k < 9 * CT; ++k) acc[k] = 0.f;
  float dbv = 0.f;
  for (int t = t0; t < t1; ++t) {
    BwdLevel L;
    int img, y0, x0;
    tile_of(slv, p.levels, t, L, img, y0, x0);
    __syncthreads();
    stage_tile<CT>(p, L, img, y0, x0, glds);
    __syncthreads();
    const int rows = min(kTR, L.h - y0), cols = min(kTC, L.w - x0);
    if (chunk == 0 && (int)threadIdx.x < p.ctot) {   // db: lane = column, the tile's pixels in order
      for (int ty = 0; ty < rows; ++ty)
        for (int tx = 0; tx < cols; ++tx) dbv += glds[((ty + 1) * kHC + (tx + 1)) * CT + (int)threadIdx.x];
    }
    for (int ty = 0; ty < rows; ++ty) {
      const _Float16* arow = L.a + (((size_t)img * L.h + (y0 + ty)) * L.w + x0) * (size_t)p.xs + a_off;
      float av = (float)arow[0] + (float)arow[32];
      for (int tx = 0; tx < cols; ++tx) {
        const float a = av;
        if (tx + 1 < cols) {   // the next pixel's value under this pixel's FMAs
          const _Float16* an = arow + (size_t)(tx + 1) * p.xs;
          av = (float)an[0] + (float)an[32];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            const f32x4* gp = reinterpret_cast<const f32x4*>(glds + ((ty + 2 - r) * kHC + (tx + 2 - s)) * CT);
#pragma unroll
            for (int c4 = 0; c4 < CT / 4; ++c4) {
              const f32x4 gv = gp[c4];
#pragma unroll
              for (int e = 0; e < 4; ++e)
                acc[(r * 3 + s) * CT + c4 * 4 + e] = __builtin_fmaf(gv[e], a, acc[(r * 3 + s) * CT + c4 * 4 + e]);
            }
          }
      }
    }
  }
  const int chunks = (int)gridDim.y;
  float* wsw = p.ws + ((size_t)chunk * p.units + unit) * (size_t)(9 * p.ctot) * kNT;
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
      if (c < p.ctot) wsw[(size_t)(c * 9 + tap) * kNT + threadIdx.x] = acc[tap * CT + c];
  if (chunk == 0 && (int)threadIdx.x < p.ctot)
    p.ws[(size_t)chunks * p.units * (size_t)(9 * p.ctot) * kNT + (size_t)unit * p.ctot + threadIdx.x] = dbv;
}

struct ReduceParams {
  const float* ws;
  float* dw[kMaxMembers];
  float* db[kMaxMembers];
  int cout[kMaxMembers];
  int cin, ctot, units, chunks;
};

// one thread per dW element (then per db element): the workgroups' partial sums in workgroup order
__global__ __launch_bounds__(kNT) void thin_bwd_reduce_kernel(const ReduceParams p) {
  const int e = (int)(blockIdx.x * kNT + threadIdx.x);
  const int nw = p.ctot * 9 * p.cin;
  if (e < nw) {
    const int row = e / p.cin, ci = e - row * p.cin;     // row = c * 9 + tap
    const int chunk = ci / kNT, lane = ci - chunk * kNT;
    const float* src = p.ws + ((size_t)chunk * p.units * (size_t)(9 * p.ctot) + row) * kNT + lane;
    float s = 0.f;
#pragma unroll 16   // (the loads of sixteen workgroups in flight; the additions stay in workgroup order)
    for (int u = 0; u < p.units; ++u) s += src[(size_t)u * (9 * p.ctot) * kNT];
    const int c = row / 9;
    const int m = c < p.cout[0] ? 0 : 1;
    const int rr = m ? row - p.cout[0] * 9 : row;
    (m ? p.dw[1] : p.dw[0])[(size_t)rr * p.cin + ci] = s;
  } else if (e < nw + p.ctot) {
    const int c = e - nw;
    const float* src = p.ws + (size_t)p.chunks * p.units * (size_t)(9 * p.ctot) * kNT + c;
    float s = 0.f;
    for (int u = 0; u < p.units; ++u) s += src[(size_t)u * p.ctot];
    const int m = c < p.cout[0] ? 0 : 1;
    (m ? p.db[1] : p.db[0])[m ? c - p.cout[0] : c] = s;
  }
}

// the launch plan that the workspace query and the launch share: tiles of the fixed list, tiles per workgroup, workgroups
struct BwdPlan {
  int ctot, chunks, tiles, tpu, units;
  int64_t ws_bytes;
};

int plan_of(const hn_thin_levels* lv, int n, int cin, int members, const int32_t* couts, BwdPlan& pl) {
  HN_CHECK_ARG(lv && couts, "hn_conv3x3_thin_backward: null pointer");
  HN_CHECK_ARG(lv->count >= 1 && lv->count <= HN_FCOS_MAX_LEVELS, "level count must be 1..%d", HN_FCOS_MAX_LEVELS);
  HN_CHECK_ARG(members >= 1 && members <= kMaxMembers, "1..%d members on a map", kMaxMembers);
  HN_CHECK_ARG(n > 0 && cin > 0 && cin % 32 == 0, "need cin %% 32 == 0");
  pl.ctot = 0;
  for (int m = 0; m < members; ++m) {
    HN_CHECK_ARG(couts[m] >= 1 && couts[m] <= 16, "member %d: need 1 <= cout <= 16", m);
    pl.ctot += couts[m];
  }
  HN_CHECK_ARG(pl.ctot <= kMaxCols, "the members of a map have %d output columns together, more than %d", pl.ctot, kMaxCols);
  int64_t tiles = 0;
  for (int l = 0; l < lv->count; ++l) {
    HN_CHECK_ARG(lv->h[l] > 0 && lv->w[l] > 0, "level %d: empty map", l);
    tiles += (int64_t)n * hn::cdiv(lv->h[l], kTR) * hn::cdiv(lv->w[l], kTC);
    HN_CHECK_ARG(tiles < ((int64_t)1 << 30), "too many tiles");
  }
  pl.tiles = (int)tiles;
  pl.tpu = hn::cdiv(tiles, kMaxUnits);
  pl.units = hn::cdiv(tiles, pl.tpu);
  pl.chunks = hn::cdiv(cin, kNT);
  pl.ws_bytes = ((int64_t)pl.chunks * pl.units * 9 * pl.ctot * kNT + (int64_t)pl.units * pl.ctot) * 4;
  return HN_OK;
}

template <int CT>
void launch_sweep(const BwdParams& p, int chunks, hipStream_t st) {
  hipLaunchKernelGGL(thin_bwd_sweep_kernel<CT>, dim3(p.units, chunks), dim3(kNT), 0, st, p);
}

}  // namespace

extern "C" int64_t hn_conv3x3_thin_backward_ws_bytes(const hn_thin_levels* lv, int n, int cin, int members, const int32_t* couts) {
  BwdPlan pl;
  return plan_of(lv, n, cin, members, couts, pl) == HN_OK ? pl.ws_bytes : -1;
}

extern "C" int hn_conv3x3_thin_backward_f32(const hn_thin_levels* lv, int n, int cin, int in_pix_stride, int members,
                                            const int32_t* couts, const int32_t* relu_cols, const float* const* w,
                                            const float* const* y, const float* const* g, float* const* dw, float* const* db,
                                            int dx_pix_stride, int dx_channel_offset, void* ws, int64_t ws_bytes, void* stream) {
  BwdPlan pl;
  const int st_ = plan_of(lv, n, cin, members, couts, pl);
  if (st_ != HN_OK) return st_;
  HN_CHECK_ARG(relu_cols && w && y && g && dw && db && ws, "hn_conv3x3_thin_backward_f32: null pointer");
  HN_CHECK_ARG(ws_bytes >= pl.ws_bytes && (uintptr_t)ws % 4 == 0, "workspace too small (%lld < %lld bytes) or unaligned",
               (long long)ws_bytes, (long long)pl.ws_bytes);
  BwdParams p;
  p.levels = lv->count; p.n = n; p.cin = cin; p.ctot = pl.ctot;
  p.xs = in_pix_stride ? in_pix_stride : 2 * cin;
  HN_CHECK_ARG(p.xs >= 2 * cin && p.xs % 64 == 0, "bad input pixel stride");
  p.tiles = pl.tiles; p.tpu = pl.tpu; p.units = pl.units;
  p.ws = (float*)ws;
  bool any_dx = false, all_dx = true;
  for (int l = 0; l < lv->count; ++l) {
    any_dx = any_dx || lv->y[l];
    all_dx = all_dx && lv->y[l];
  }
  HN_CHECK_ARG(any_dx == all_dx, "the input gradient needs every level (or none)");
  p.want_dx = any_dx ? 1 : 0;
  p.das = dx_pix_stride ? dx_pix_stride : cin;
  HN_CHECK_ARG(!any_dx || (dx_channel_offset >= 0 && p.das >= dx_channel_offset + cin), "bad input-gradient pixel stride / channel offset");
  for (int m = 0; m < kMaxMembers; ++m) {
    const int mm = m < members ? m : 0;
    HN_CHECK_ARG(w[mm] && dw[mm] && db[mm], "member %d: null pointer", mm);
    HN_CHECK_ARG(relu_cols[mm] >= 0 && relu_cols[mm] <= couts[mm], "member %d: bad relu_cols", mm);
    p.wt[m] = w[mm];
    p.cout[m] = m < members ? couts[m] : 0;   // (an absent member owns no column: every column below ctot is member 0's)
    p.relu[m] = relu_cols[mm];
  }
  int tiles = 0;
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l) {
    BwdLevel& t = p.lv[l];
    if (l < lv->count) {
      HN_CHECK_ARG(lv->x16[l], "level %d: null activation", l);
      HN_CHECK_ARG((uintptr_t)lv->x16[l] % 2 == 0, "level %d: unaligned activation", l);
      t.a = (const _Float16*)lv->x16[l];
      t.da = lv->y[l] ? lv->y[l] + dx_channel_offset : nullptr;
      for (int m = 0; m < kMaxMembers; ++m) {
        const int mm = m < members ? m : 0;
        t.y[m] = y[mm * lv->count + l];
        t.g[m] = g[mm * lv->count + l];
        HN_CHECK_ARG(t.y[m] && t.g[m], "level %d, member %d: null output / gradient", l, mm);
      }
      t.h = lv->h[l]; t.w = lv->w[l];
      t.tx = hn::cdiv(t.w, kTC);
      t.tiles_img = hn::cdiv(t.h, kTR) * t.tx;
      t.first_tile = tiles;
      tiles += n * t.tiles_img;
    } else {
      t.a = nullptr; t.da = nullptr;
      for (int m = 0; m < kMaxMembers; ++m) t.y[m] = t.g[m] = nullptr;
      t.h = t.w = t.tx = t.tiles_img = 1; t.first_tile = 0x7fffffff;
    }
  }
  ReduceParams r;
  r.ws = p.ws; r.cin = cin; r.ctot = pl.ctot; r.units = pl.units; r.chunks = pl.chunks;
  for (int m = 0; m < kMaxMembers; ++m) {
    const int mm = m < members ? m : 0;
    r.dw[m] = dw[mm]; r.db[m] = db[mm]; r.cout[m] = p.cout[m];
  }
  hipStream_t st = (hipStream_t)stream;
  if (pl.ctot <= 4) launch_sweep<4>(p, pl.chunks, st);
  else if (pl.ctot <= 8) launch_sweep<8>(p, pl.chunks, st);
  else if (pl.ctot <= 12) launch_sweep<12>(p, pl.chunks, st);
  else launch_sweep<16>(p, pl.chunks, st);
  HN_CHECK_LAUNCH("thin_bwd_sweep_kernel");
  const int elems = pl.ctot * 9 * cin + pl.ctot;
  hipLaunchKernelGGL(thin_bwd_reduce_kernel, dim3(hn::cdiv(elems, kNT)), dim3(kNT), 0, st, r);
  HN_CHECK_LAUNCH("thin_bwd_reduce_kernel");
  return HN_OK;
}
