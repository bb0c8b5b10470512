// The per-lane arithmetic of the GroupNorm apply pass (fp32 -> S32): y = relu(x * scale + shift), the NaN-aware range note,
// the hi | lo split and the two 16-byte stores of one pixel's 8-channel group.  ONE definition for the stand-alone kernels
// (split_ops.hip) and for the pass carried in the tail of a tower convolution (conv_igemm_f16x3_carry.hip): the two must agree
// bit for bit, whatever contraction flags their translation units are built with, so the affine is an explicit fma (what the
// stand-alone kernels always compiled to) and nothing else in here can be contracted.
#pragma once
#include "hn_common.h"

namespace hn {

typedef float as_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 as_f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split8(const as_f32x4& a, const as_f32x4& b, as_f16x8& hi, as_f16x8& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const _Float16 h0 = (_Float16)a[e], h1 = (_Float16)b[e];
    hi[e] = h0;
    hi[4 + e] = h1;
    lo[e] = (_Float16)(a[e] - (float)h0);
    lo[4 + e] = (_Float16)(b[e] - (float)h1);
  }
}

// a | b: channels ch .. ch+7 of one pixel; s0 | s1 and t0 | t1: their scale and shift -> the pixel's hi and lo halves.  Returns
// whether a value cannot be split (only looked at when `check`: NaN-aware, this pass is HBM-bound and its input may be any
// fp32 tensor).  `affine` is a compile-time constant at most call sites.
__device__ __forceinline__ bool affine_split_values(as_f32x4 a, as_f32x4 b, const as_f32x4& s0, const as_f32x4& s1,
                                                    const as_f32x4& t0, const as_f32x4& t1, bool affine, int relu, bool check,
                                                    as_f16x8& hi, as_f16x8& lo) {
  if (affine) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = __builtin_fmaf(a[e], s0[e], t0[e]);
      b[e] = __builtin_fmaf(b[e], s1[e], t1[e]);
    }
  }
  if (relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = hn::relu(a[e]);
      b[e] = hn::relu(b[e]);
    }
  }
  bool bad = false;
  if (check) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bad |= hn::range_bad(a[e]) | hn::range_bad(b[e]);
  }
  split8(a, b, hi, lo);
  return bad;
}

// dst: the pixel's hi run of the 32-channel block at channel ch (the lo run starts 32 halfs behind it)
__device__ __forceinline__ void split_store(const as_f16x8& hi, const as_f16x8& lo, _Float16* dst, bool nt_store) {
  if (nt_store) {
    __builtin_nontemporal_store(hi, reinterpret_cast<as_f16x8*>(dst));
    __builtin_nontemporal_store(lo, reinterpret_cast<as_f16x8*>(dst + 32));
  } else {
    *reinterpret_cast<as_f16x8*>(dst) = hi;
    *reinterpret_cast<as_f16x8*>(dst + 32) = lo;
  }
}

// one pixel's group, start to end: values, range note, the two 16-byte stores
__device__ __forceinline__ void affine_split_store(const as_f32x4& a, const as_f32x4& b, const as_f32x4& s0, const as_f32x4& s1,
                                                   const as_f32x4& t0, const as_f32x4& t1, bool affine, int relu,
                                                   int* range_flag, _Float16* dst, bool nt_store) {
  as_f16x8 hi, lo;
  if (affine_split_values(a, b, s0, s1, t0, t1, affine, relu, range_flag != nullptr, hi, lo)) *range_flag = 1;
  split_store(hi, lo, dst, nt_store);
}

}  // namespace hn
