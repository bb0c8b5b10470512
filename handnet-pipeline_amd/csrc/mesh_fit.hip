// Each hand's mesh fitted to its measured depth (tests/fit_ref.py restates the rule in numpy, operation
// for operation): ONE Gauss-Newton step of projective point-to-plane alignment per hand slot.  The candidate pixels (every
// `stride`-th row and column, not on the frame's border) whose silhouette byte and whose four neighbours' bytes name slot k,
// whose scene depth D is valid and lies within the band of the raster's nearest mesh Z (`best`), give a surface point p =
// P(r, c, best), a normal n from the mesh depth map and a residual rho = n . (P(r, c, D) - p); the 6 x 6 normal equations of
// the rigid motion about the slot's root joint are summed as INTEGERS (every term rint(x * 2^30) of one fp32 product), solved in
// fp64 by one lane, and the motion -- a Cayley rotation and a shift -- is applied to the slot's vertices and joints.
//
// Two launches, ordered by their kernel boundary.  The unit of work of the first is a STRIP of hand_cloud.hip's kind:
// `strip_rows(h)` consecutive rows, walked by ONE wave, 64 candidates at a time, once per slot (the grid's y).
//   mesh_fit_accumulate  a lane keeps its 29 int64 sums in registers across the strip (the silhouette byte is loaded first,
//                        everything else only on lanes whose byte names the slot); the wave reduces them once at the strip's
//                        end and lane j writes sum j into the table [frame][slot][strip][29].
//   mesh_fit_apply       one workgroup per slot: all threads sum the slot's table rows, thread 0 solves and hands R, t, c0 and
//                        the status over through LDS, all threads move the vertices and the joints (status != 0: dword copies).
// No workgroup waits for another inside a launch and there is no atomic: integer sums do not depend on their order, so the
// outputs are a pure function of the inputs and two runs give the same bytes.  The file is built with -ffp-contract=off
// (hn_amd/build.py) and without any fast-math flag: every fp32 and fp64 operation is rounded on its own.
#include <algorithm>
#include <cmath>

#include "depth_pass.h"

namespace {

using namespace hn;                 // depth_pass.h: the strips, kMaxSlots, wave_sum, the camera, back_x / back_y, valid_depth

constexpr int kTerms = 29;          // 21 of A (j <= k, row by row), 6 of b, the cost, the count
constexpr float kMinCos = 0.2f;     // FIT_MIN_COS: pixels seen at a steeper grazing angle carry no usable normal
constexpr float kReach = 1.0f;      // FIT_REACH: a hand's surface lies within a metre of its wrist -- this bounds the sums
constexpr double kArm = 0.1;        // FIT_ARM: the lever arm that puts the rotation damping on the translation's scale
constexpr float kQ30 = 1073741824.0f;

struct FitIn {
  const float* best;                // [n][h][w] the raster's out_depth
  const unsigned char* sil;         // [n][h][w]
  const float* depth;               // frame i at depth + i * frame_stride, [h][w]
  long long frame_stride;
  const float* cams;                // device [n][4], or null: the four values below
  float fx, fy, cx, cy;
  const float* xyz_mm;              // [n * k][joints][3]
  int k, h, w, q, joints;
  float band;
};

// (int64)rint(x * 2^30) of one fp32 product
__device__ __forceinline__ long long q30(float a, float b) { return (long long)rintf(__fmul_rn(__fmul_rn(a, b), kQ30)); }

// grid (strips / 4, k, frames), 256 threads: wave wv of block (b, kk, i) walks strip 4 b + wv of frame i for slot kk
__global__ __launch_bounds__(256) void mesh_fit_accumulate(FitIn in, long long* __restrict__ table) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, kk = blockIdx.y, i = blockIdx.z;
  const int strips = gridDim.x * 4, u = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int h = in.h, w = in.w, q = in.q;
  const int rows = strip_rows(h), wc = (w + q - 1) / q;
  const Cam cam = camera(in.cams, i, in.fx, in.fy, in.cx, in.cy);
  const size_t slot = (size_t)i * in.k + kk;
  const float* root = in.xyz_mm + slot * in.joints * 3;
  const float c0x = __fdiv_rn(root[0], 1000.f), c0y = __fdiv_rn(root[1], 1000.f), c0z = __fdiv_rn(root[2], 1000.f);
  const unsigned char* sil = in.sil + (size_t)i * h * w;
  const float* best = in.best + (size_t)i * h * w;
  const float* depth = in.depth + (size_t)i * in.frame_stride;
  const unsigned char mine = (unsigned char)(kk + 1);
  long long acc[kTerms];
#pragma unroll
  for (int a = 0; a < kTerms; ++a) acc[a] = 0;
  const int r1 = min(h - 1, (u + 1) * rows);                              // (the last row is no candidate: 1 <= r <= h - 2)
  for (int r = max(q, (u * rows + q - 1) / q * q); r < r1; r += q) {      // (q >= 1: the first multiple of q that is >= 1)
    for (int j0 = 0; j0 < wc; j0 += 64) {
      const int j = j0 + lane, c = j * q;
      if (j >= wc || c < 1 || c > w - 2) continue;
      const size_t at = (size_t)r * w + c;
      if ((sil[at] & 0x7F) != mine) continue;                             // (the hidden flag is ignored)
      if ((sil[at - 1] & 0x7F) != mine || (sil[at + 1] & 0x7F) != mine || (sil[at - w] & 0x7F) != mine || (sil[at + w] & 0x7F) != mine)
        continue;
      const float b = best[at], bl = best[at - 1], br = best[at + 1], bu = best[at - w], bd = best[at + w];
      if (!(b > 0.f && bl > 0.f && br > 0.f && bu > 0.f && bd > 0.f)) continue;
      const float d = depth[at];
      if (!valid_depth(d)) continue;
      if (!(fabsf(__fsub_rn(d, b)) <= in.band)) continue;                 // (NaN fails)
      // the normal from the mesh depth map: gx = P(r, c + 1) - P(r, c - 1), gy = P(r + 1, c) - P(r - 1, c), n = gx x gy
      const float gxx = __fsub_rn(back_x(cam, c + 1, br), back_x(cam, c - 1, bl));
      const float gxy = __fsub_rn(back_y(cam, r, br), back_y(cam, r, bl));
      const float gxz = __fsub_rn(br, bl);
      const float gyx = __fsub_rn(back_x(cam, c, bd), back_x(cam, c, bu));
      const float gyy = __fsub_rn(back_y(cam, r + 1, bd), back_y(cam, r - 1, bu));
      const float gyz = __fsub_rn(bd, bu);
      float nx = __fsub_rn(__fmul_rn(gxy, gyz), __fmul_rn(gxz, gyy));
      float ny = __fsub_rn(__fmul_rn(gxz, gyx), __fmul_rn(gxx, gyz));
      float nz = __fsub_rn(__fmul_rn(gxx, gyy), __fmul_rn(gxy, gyx));
      // (sqrtf, not __fsqrt_rn: without OCML's rounded operations the latter is the NATIVE square root, an approximation)
      const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
      if (!(len > 0.f && len <= 3.402823466e38f)) continue;
      nx = __fdiv_rn(nx, len);
      ny = __fdiv_rn(ny, len);
      nz = __fdiv_rn(nz, len);
      if (!(fabsf(nz) >= kMinCos)) continue;
      // the lever about the root joint
      const float px = back_x(cam, c, b), py = back_y(cam, r, b);
      const float dx = __fsub_rn(px, c0x), dy = __fsub_rn(py, c0y), dz = __fsub_rn(b, c0z);
      if (!(fabsf(dx) <= kReach && fabsf(dy) <= kReach && fabsf(dz) <= kReach)) continue;
      const float mx = __fsub_rn(__fmul_rn(dy, nz), __fmul_rn(dz, ny));
      const float my = __fsub_rn(__fmul_rn(dz, nx), __fmul_rn(dx, nz));
      const float mz = __fsub_rn(__fmul_rn(dx, ny), __fmul_rn(dy, nx));
      // the residual along the normal
      const float ex = __fsub_rn(back_x(cam, c, d), px), ey = __fsub_rn(back_y(cam, r, d), py), ez = __fsub_rn(d, b);
      const float rho = __fadd_rn(__fadd_rn(__fmul_rn(nx, ex), __fmul_rn(ny, ey)), __fmul_rn(nz, ez));
      if (!(fabsf(rho) <= 1.f)) continue;
      const float jac[6] = {nx, ny, nz, mx, my, mz};
      int a = 0;
#pragma unroll
      for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int s = p; s < 6; ++s) acc[a++] += q30(jac[p], jac[s]);
      }
#pragma unroll
      for (int p = 0; p < 6; ++p) acc[21 + p] += q30(jac[p], rho);
      acc[27] += q30(rho, rho);
      acc[28] += 1;
    }
  }
  long long out = 0;
#pragma unroll
  for (int a = 0; a < kTerms; ++a) {
    const long long sum = wave_sum(acc[a]);
    if (lane == a) out = sum;
  }
  if (lane < kTerms) table[((slot * strips) + u) * kTerms + lane] = out;
}

struct Solved {
  float rt[12];
  int status;
};

// the 29 sums of a slot -> status and motion (fit_ref.solve: scalar fp64 operations, one by one, in index order)
__device__ Solved solve(const long long* sums, int min_points, double damp, double shift2, double tan2) {
#pragma clang fp contract(off)
  Solved out = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f}, 0};
  const long long npts = sums[28];
  if (npts < (long long)min_points) {
    out.status = 1;
    return out;
  }
  double a[6][6], b[6], low[6][6], y[6], x[6];
  int at = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
#pragma unroll
    for (int k = j; k < 6; ++k) a[j][k] = (double)sums[at++] / 1073741824.0;
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) b[j] = (double)sums[21 + j] / 1073741824.0;
  const double lam = damp * (double)npts;
#pragma unroll
  for (int j = 0; j < 3; ++j) a[j][j] = a[j][j] + lam;
#pragma unroll
  for (int j = 3; j < 6; ++j) a[j][j] = a[j][j] + lam * (kArm * kArm);
  bool failed = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = a[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - low[j][k] * low[j][k];
    if (!(s > 0.0)) failed = true;
    low[j][j] = sqrt(s);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = a[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k) v = v - low[i][k] * low[j][k];
      low[i][j] = v / low[j][j];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - low[i][k] * y[k];
    y[i] = s / low[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s = s - low[k][i] * x[k];
    x[i] = s / low[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (!(fabs(x[i]) <= 1.7976931348623157e308)) failed = true;           // (NaN or inf)
  }
  if (failed) {
    out.status = 2;
    return out;
  }
  const double a0 = x[3] * 0.5, a1 = x[4] * 0.5, a2 = x[5] * 0.5;
  const double tt = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
  const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
  if (tt > shift2 || aa > tan2) {
    out.status = 3;
    return out;
  }
  // Cayley: R = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) -- an exact rotation from + - * / only
  const double u = 1.0 - aa, den = 1.0 + aa;
  out.rt[0] = (float)((u + (2.0 * a0) * a0) / den);
  out.rt[1] = (float)(((2.0 * a0) * a1 - 2.0 * a2) / den);
  out.rt[2] = (float)(((2.0 * a0) * a2 + 2.0 * a1) / den);
  out.rt[3] = (float)(((2.0 * a1) * a0 + 2.0 * a2) / den);
  out.rt[4] = (float)((u + (2.0 * a1) * a1) / den);
  out.rt[5] = (float)(((2.0 * a1) * a2 - 2.0 * a0) / den);
  out.rt[6] = (float)(((2.0 * a2) * a0 - 2.0 * a1) / den);
  out.rt[7] = (float)(((2.0 * a2) * a1 + 2.0 * a0) / den);
  out.rt[8] = (float)((u + (2.0 * a2) * a2) / den);
  out.rt[9] = (float)x[0];
  out.rt[10] = (float)x[1];
  out.rt[11] = (float)x[2];
  return out;
}

// x' = (((R_r0 d0 + R_r1 d1) + R_r2 d2) + c0_r) + t_r with d = x - c0
__device__ __forceinline__ void move(const float* rt, const float* c0, float x0, float x1, float x2, float* o) {
  const float d0 = __fsub_rn(x0, c0[0]), d1 = __fsub_rn(x1, c0[1]), d2 = __fsub_rn(x2, c0[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(rt[3 * r], d0), __fmul_rn(rt[3 * r + 1], d1)), __fmul_rn(rt[3 * r + 2], d2)),
                               c0[r]), rt[9 + r]);
}

// grid (slots), 256 threads
__global__ __launch_bounds__(256) void mesh_fit_apply(const long long* __restrict__ table, int strips, const float* __restrict__ mesh,
                                                      const float* __restrict__ xyz_mm, int v, int joints, int min_points, double damp,
                                                      double shift2, double tan2, float* __restrict__ out_mesh,
                                                      float* __restrict__ out_xyz, float* __restrict__ out_rt,
                                                      int* __restrict__ out_count, long long* __restrict__ out_cost) {
#pragma clang fp contract(off)
  __shared__ long long part[8][32];
  __shared__ long long total[kTerms];
  __shared__ float s_rt[12], s_c0[3];
  __shared__ int s_status;
  const int t = threadIdx.x;
  const size_t slot = blockIdx.x;
  {
    // thread (p, j): sum j of the strips p, p + 8, ...
    const int j = t & 31, p = t >> 5;
    long long sum = 0;
    if (j < kTerms)
      for (int s = p; s < strips; s += 8) sum += table[(slot * strips + s) * kTerms + j];
    part[p][j] = sum;
  }
  __syncthreads();
  if (t < kTerms) {
    long long sum = 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) sum += part[p][t];
    total[t] = sum;
  }
  __syncthreads();
  const float* root = xyz_mm + slot * joints * 3;
  if (t == 0) {
    long long sums[kTerms];
#pragma unroll
    for (int a = 0; a < kTerms; ++a) sums[a] = total[a];
    const Solved got = solve(sums, min_points, damp, shift2, tan2);
#pragma unroll
    for (int a = 0; a < 12; ++a) {
      s_rt[a] = got.rt[a];
      out_rt[slot * 12 + a] = got.rt[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) s_c0[a] = __fdiv_rn(root[a], 1000.f);
    s_status = got.status;
    out_count[2 * slot] = (int)sums[28];
    out_count[2 * slot + 1] = got.status;
    out_cost[slot] = sums[27];
  }
  __syncthreads();
  const float* src = mesh + slot * v * 3;
  float* dst = out_mesh + slot * v * 3;
  float* jdst = out_xyz + slot * joints * 3;
  if (s_status != 0) {                                                    // (byte copies: not through the arithmetic)
    const unsigned* a = reinterpret_cast<const unsigned*>(src);
    unsigned* o = reinterpret_cast<unsigned*>(dst);
    for (int e = t; e < v * 3; e += 256) o[e] = a[e];
    const unsigned* ja = reinterpret_cast<const unsigned*>(root);
    unsigned* jo = reinterpret_cast<unsigned*>(jdst);
    for (int e = t; e < joints * 3; e += 256) jo[e] = ja[e];
    return;
  }
  float rt[12], c0[3], o[3];
#pragma unroll
  for (int a = 0; a < 12; ++a) rt[a] = s_rt[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) c0[a] = s_c0[a];
  for (int e = t; e < v; e += 256) {                                      // the mesh: (x, -y, -z) in and out, both exact
    move(rt, c0, src[3 * e], -src[3 * e + 1], -src[3 * e + 2], o);
    dst[3 * e] = o[0];
    dst[3 * e + 1] = -o[1];
    dst[3 * e + 2] = -o[2];
  }
  for (int e = t; e < joints; e += 256) {                                 // the joints: / 1000f in, * 1000f out
    move(rt, c0, __fdiv_rn(root[3 * e], 1000.f), __fdiv_rn(root[3 * e + 1], 1000.f), __fdiv_rn(root[3 * e + 2], 1000.f), o);
    jdst[3 * e] = __fmul_rn(o[0], 1000.f);
    jdst[3 * e + 1] = __fmul_rn(o[1], 1000.f);
    jdst[3 * e + 2] = __fmul_rn(o[2], 1000.f);
  }
}

}  // namespace

extern "C" int64_t hn_mesh_fit_scratch_bytes(int n, int k, int h) {
  if (n <= 0 || k <= 0 || k > kMaxSlots || h <= 0 || h > 16384) return 0;
  return (int64_t)((size_t)n * k * strips_padded(h) * kTerms * sizeof(long long));
}

extern "C" int hn_mesh_fit_f32(const float* mesh_depth, const uint8_t* silhouette, const float* scene_depth,
                               int64_t depth_frame_stride, const float* paras, const float* cams, const float* mesh,
                               const float* xyz_mm, int n, int k, int h, int w, int v, int joints, int stride, float band,
                               int min_points, double damp, double max_shift2, double tan2_half_angle, void* scratch,
                               int64_t scratch_bytes, float* out_mesh, float* out_xyz, float* out_rt, int32_t* out_count,
                               int64_t* out_cost, void* stream) {
  const char* fn = "hn_mesh_fit_f32";
  HN_CHECK_ARG(mesh_depth && silhouette && scene_depth && mesh && xyz_mm && scratch && out_mesh && out_xyz && out_rt && out_count &&
                   out_cost,
               "%s: null pointer", fn);
  if (int st = check_one_camera(fn, paras, cams)) return st;
  if (int st = check_frames(fn, n, k, h, w)) return st;
  if (int st = check_depth_stride(fn, depth_frame_stride, h, w)) return st;
  if (int st = check_fit_sizes(fn, v, nullptr, joints)) return st;
  if (int st = check_fit_options(fn, stride, band, min_points, damp, max_shift2, tan2_half_angle)) return st;
  if (int st = check_buffer(fn, "scratch", scratch, scratch_bytes, hn_mesh_fit_scratch_bytes(n, k, h), 8)) return st;
  HN_CHECK_ARG((((uintptr_t)out_cost & 7) | ((uintptr_t)out_count & 3) | ((uintptr_t)out_mesh & 3) | ((uintptr_t)out_xyz & 3) |
                ((uintptr_t)out_rt & 3)) == 0,
               "%s: out_mesh / out_xyz / out_rt / out_count must be aligned to 4 bytes and out_cost to 8", fn);
  FitIn in = {mesh_depth, silhouette, scene_depth, (long long)depth_frame_stride, cams, 0.f, 0.f, 0.f, 0.f, xyz_mm, k, h, w,
              std::min(stride, 16384), joints, band};  // (h, w <= 16384: every larger stride leaves no candidate, as this one)
  if (paras) { in.fx = paras[0]; in.fy = paras[1]; in.cx = paras[2]; in.cy = paras[3]; }
  long long* table = static_cast<long long*>(scratch);
  const int strips = strips_padded(h);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_fit_accumulate, dim3(strips / 4, k, n), dim3(256), 0, st, in, table);
  HN_CHECK_LAUNCH("mesh_fit_accumulate");
  hipLaunchKernelGGL(mesh_fit_apply, dim3(n * k), dim3(256), 0, st, table, strips, mesh, xyz_mm, v, joints, min_points, damp, max_shift2,
                     tan2_half_angle, out_mesh, out_xyz, out_rt, reinterpret_cast<int*>(out_count),
                     reinterpret_cast<long long*>(out_cost));
  HN_CHECK_LAUNCH("mesh_fit_apply");
  return HN_OK;
}
