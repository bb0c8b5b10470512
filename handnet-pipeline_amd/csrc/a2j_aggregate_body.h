// The body of the aggregation kernel, included twice by a2j_ops.hip (no include guard):
//   A2J_AGG_LOSS 0 -> a2j_aggregate_kernel, the plain form: the text it had before the switch, with nothing added
//   A2J_AGG_LOSS 1 -> a2j_loss_aggregate_kernel, the loss form (hn_a2j_aggregate_loss_f32), whose one
//                     further argument is a LossSpec: two more running sums (e * anchor) through the same cell batches and the
//                     same combination -- six LDS planes per group instead of four; the s, s0, s1, sd chains are the plain form's
// (a textual switch and not a template: each kernel has a name of its own in the build's resource record, and the plain kernel's
// gfx950 code is, instruction for instruction, what the compiler made of it before the switch)
#ifndef A2J_AGG_LOSS
#error "define A2J_AGG_LOSS to 0 or 1 before including a2j_aggregate_body.h"
#endif
#if A2J_AGG_LOSS
#define A2J_AGG_KERNEL a2j_loss_aggregate_kernel
#define A2J_AGG_PLANES 6
#else
#define A2J_AGG_KERNEL a2j_aggregate_kernel
#define A2J_AGG_PLANES 4
#endif

__global__ __launch_bounds__(1024) void A2J_AGG_KERNEL(const float* __restrict__ cls,
                                                       const float* __restrict__ reg,
                                                       const float* __restrict__ dep,
                                                       const int* __restrict__ valid, int fh, int fw,
                                                       int J, int Jw, int stride, int G, float* __restrict__ out,
                                                       const ConvertSpec cs
#if A2J_AGG_LOSS
                                                       , const LossSpec ls
#endif
) {
  constexpr int NQ = A2J_AGG_PLANES;   // summed quantities = LDS planes per group
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [G][NQ][A*Jw]
  const int k = blockIdx.x;
  const int j0 = blockIdx.y * Jw;
  const int jn = min(Jw, J - j0);      // joints of this workgroup (the last one may have fewer, or none)
  if (jn <= 0) return;
  const int AJ = kAnchorsPerCell * J;   // channels per cell in memory
  const int AW = kAnchorsPerCell * Jw;  // thread slots per cell group
  const int g = threadIdx.x / AW, cl = threadIdx.x - g * AW;
  const int a = cl / Jw, jl = cl - a * Jw;
  const bool active = g < G && jl < jn;
  const int c = a * J + j0 + jl;        // channel in memory
  if (valid && valid[k] != 1) {  // uniform per workgroup: 0 = no crop (zero row), 2 = non-finite crop (NaN row, as the
    // reference's network returns for it: every cell of the 11 x 11 maps sees every pixel of the crop)
    if ((int)threadIdx.x < jn * 3) {
      const float fill = valid[k] == 0 ? 0.f : __builtin_nanf("");
      const long at = ((long)k * J + j0) * 3 + threadIdx.x;
      out[at] = fill;
      if ((cs.box || cs.box_f32) && cs.image_uvd) cs.image_uvd[at] = fill;
      if ((cs.box || cs.box_f32) && cs.xyz_mm && cs.has_paras) cs.xyz_mm[at] = fill;
    }
#if A2J_AGG_LOSS   // the row's terms: zeros (the reduction leaves the row out) or NaN
    if ((int)threadIdx.x < jn * kLossTerms)
      ls.terms[((long)k * J + j0) * kLossTerms + threadIdx.x] = valid[k] == 0 ? 0.f : __builtin_nanf("");
#endif
    return;
  }
  const int cells = fh * fw;
  const float* clsk = cls + (long)k * cells * AJ;
  const float* depk = dep + (long)k * cells * AJ;
  const float* regk = reg + (long)k * cells * AJ * 2;

  // Both cell loops fetch kBatch (14: three rounds for the 41 cells a thread owns on an 11 x 11 map) cells' operands before they use any (same operations in the same order): written as
  // load -> use per cell, each of the 2 x 41 iterations waited for its own L2 round trip -- 27 us per launch.
  constexpr int kBatch = 14;
  float mx = -FLT_MAX;
  if (active)
    for (int pb = g; pb < cells; pb += kBatch * G) {
      float v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        v[u] = p < cells ? clsk[(long)p * AJ + c] : -FLT_MAX;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) mx = fmaxf(mx, v[u]);
    }
  if (g < G) lds[g * AW + cl] = mx;
  __syncthreads();
  if ((int)threadIdx.x < AW) {   // (group 0's threads: slot cl = threadIdx.x) maximum over the groups, then over the anchors below
    float m = lds[threadIdx.x];
    for (int gg = 1; gg < G; ++gg) m = fmaxf(m, lds[gg * AW + threadIdx.x]);
    lds[threadIdx.x] = m;
  }
  __syncthreads();
  float mj = -FLT_MAX;
  if (active)
    for (int aa = 0; aa < kAnchorsPerCell; ++aa) mj = fmaxf(mj, lds[aa * Jw + jl]);
  __syncthreads();

  if (active) {
    float s = 0.f, s0 = 0.f, s1 = 0.f, sd = 0.f;
#if A2J_AGG_LOSS
    float sa0 = 0.f, sa1 = 0.f;   // e * anchor
#endif
    const float p0 = 2.f + 4.f * (float)(a >> 2), p1 = 2.f + 4.f * (float)(a & 3);
    for (int pb = g; pb < cells; pb += kBatch * G) {
      float vc[kBatch], vd[kBatch];
      float2 vr[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        const long q = (long)(p < cells ? p : g) * AJ + c;   // (clamped: the tail batch's extra cells are not used)
        vc[u] = clsk[q];
        vr[u] = *reinterpret_cast<const float2*>(regk + q * 2);
        vd[u] = depk[q];
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int p = pb + u * G;
        if (p < cells) {
          const int hh = p / fw, ww = p - hh * fw;
          const float e = expf(vc[u] - mj);
          const float a0 = (float)(hh * stride) + p0, a1 = (float)(ww * stride) + p1;
          s += e;
          s0 += e * (a0 + vr[u].x);
          s1 += e * (a1 + vr[u].y);
          sd += e * vd[u];
#if A2J_AGG_LOSS
          sa0 += e * a0;
          sa1 += e * a1;
#endif
        }
      }
    }
    float* o = lds + (long)g * NQ * AW;
    o[cl] = s;
    o[AW + cl] = s0;
    o[2 * AW + cl] = s1;
    o[3 * AW + cl] = sd;
#if A2J_AGG_LOSS
    o[4 * AW + cl] = sa0;
    o[5 * AW + cl] = sa1;
#endif
  }
  __syncthreads();
  // fixed-order combination in two steps: thread (quantity q, anchor a, joint jl) of the first NQ * AW sums its slot over the
  // groups 0 .. G-1, then thread jj sums the 16 anchors of its joint (G + 16 dependent additions instead of 16 G)
  for (int s4 = threadIdx.x; s4 < NQ * AW; s4 += blockDim.x) {
    float acc = lds[s4];
    for (int gg = 1; gg < G; ++gg) acc += lds[(long)gg * NQ * AW + s4];
    lds[s4] = acc;   // (group 0's slot: only this thread reads or writes it here)
  }
  __syncthreads();
  if ((int)threadIdx.x < jn) {
    const int jj = threadIdx.x;
    float t = 0.f, t0 = 0.f, t1 = 0.f, td = 0.f;
#if A2J_AGG_LOSS
    float ta0 = 0.f, ta1 = 0.f;
#endif
    for (int aa = 0; aa < kAnchorsPerCell; ++aa) {
      t += lds[aa * Jw + jj];
      t0 += lds[AW + aa * Jw + jj];
      t1 += lds[2 * AW + aa * Jw + jj];
      td += lds[3 * AW + aa * Jw + jj];
#if A2J_AGG_LOSS
      ta0 += lds[4 * AW + aa * Jw + jj];
      ta1 += lds[5 * AW + aa * Jw + jj];
#endif
    }
    float* o = out + ((long)k * J + j0 + jj) * 3;
    float ku = t0 / t;
    const float kv = t1 / t, kd = td / t;
#if !A2J_AGG_LOSS   // (the loss form's entry takes no mirror flags: gt is in the coordinates of the crop as cut)
    if (cs.mirror && cs.mirror[k]) ku = cs.crop_w - ku;   // (one fp32 subtraction, before anything else sees the value)
#endif
    o[0] = ku;
    o[1] = kv;
    o[2] = kd;
    // convert_joints + uvd2xyz in the aggregation's epilogue (what every caller does next: ros_demo.py:289,
    // 329-330, a2j/a2j.py:341-348) -- from the registers that hold the joint, no second launch
    if (cs.box || cs.box_f32) convert_one(cs, k, (long)k * J + j0 + jj, ku, kv, kd);
#if A2J_AGG_LOSS
    loss_terms_one(ls, (long)k * J + j0 + jj, ta0 / t, ta1 / t, ku, kv, kd);
#endif
  }
}

#undef A2J_AGG_KERNEL
#undef A2J_AGG_PLANES
#undef A2J_AGG_LOSS
