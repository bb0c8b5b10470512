// The depth fit iterated (tests/refit_ref.py restates the rule in numpy, operation for operation): I
// Gauss-Newton steps of mesh_fit.hip's point-to-plane alignment per hand slot, the moved mesh drawn again before every further
// step.  Iteration 1 is hn_mesh_fit_f32 on the caller's mesh depth and silhouette; iteration t >= 2 is the geometry pass of
// mesh_raster.hip (hn_mesh_geometry_f32: the nearest Z and the slot byte of the current meshes, nothing else) and hn_mesh_fit_f32
// on what it drew, about the current root joint.  Both serve every iteration unchanged; the intermediate meshes ping-pong between
// two buffers of `work` (mesh_fit_apply reads the root joint on every thread, so it never runs in place), the joints of every
// iteration stay in `work`, and the last iteration writes the caller's outputs.  There is no early stop: the launches are fixed,
// 2 + 4 (I - 1) + 1 of them, so a step that holds them stays capturable.
//
// The one kernel of this file closes the chain: one thread per slot composes the iterations' motions into ONE motion about the
// original root joint, in fp64, scalar operation by scalar operation, and packs (matches, status, cost) of every iteration into
// the trace.  No atomic, no order dependence: two runs give the same bytes.  Built with -ffp-contract=off (hn_amd/build.py).
#include <cmath>

#include "handnet_hip.h"
#include "depth_pass.h"

namespace {

constexpr int kMaxIters = 8;

__host__ inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// the parts of `work`, each on 16 bytes
struct Work {
  size_t mesh[2];                   // the intermediate meshes [s][v][3] (iters >= 2: one, iters >= 3: two)
  size_t xyz;                       // [iters - 1][s][joints][3]: the joints after iteration 1 .. iters - 1
  size_t rt;                        // [iters][s][12]
  size_t count;                     // [iters][s][2]
  size_t cost;                      // [iters][s] int64
  size_t depth;                     // [n][h][w] fp32 (iters >= 2)
  size_t who;                       // [n][h][w] uint8 (iters >= 2)
  size_t raster;                    // the raster's scratch records (iters >= 2)
  size_t total;
};

__host__ Work work_layout(int n, int k, int h, int w, int v, int f, int joints, int iters) {
  const size_t s = (size_t)n * k;
  Work o;
  size_t at = 0;
  auto part = [&at](size_t bytes) { const size_t start = at; at += up16(bytes); return start; };
  o.mesh[0] = part(iters >= 2 ? s * v * 3 * sizeof(float) : 0);
  o.mesh[1] = part(iters >= 3 ? s * v * 3 * sizeof(float) : 0);
  o.xyz = part((size_t)(iters - 1) * s * joints * 3 * sizeof(float));
  o.rt = part((size_t)iters * s * 12 * sizeof(float));
  o.count = part((size_t)iters * s * 2 * sizeof(int));
  o.cost = part((size_t)iters * s * sizeof(long long));
  o.depth = part(iters >= 2 ? (size_t)n * h * w * sizeof(float) : 0);
  o.who = part(iters >= 2 ? (size_t)n * h * w : 0);
  o.raster = part(iters >= 2 ? (size_t)hn_mesh_render_scratch_bytes((int)s, f) : 0);
  o.total = at;
  return o;
}

// grid (ceil(slots / 64)), 64 threads: thread = slot.  xyz0: the caller's joints (iteration 1 turned about their root); xyz_it:
// the joints after iterations 1 .. iters - 1 (iteration t + 1 turned about the root of row t - 1).
__global__ __launch_bounds__(64) void mesh_refit_compose(const float* __restrict__ xyz0, const float* __restrict__ xyz_it,
                                                         const float* __restrict__ rts, const int* __restrict__ counts,
                                                         const long long* __restrict__ costs, int slots, int joints, int iters,
                                                         float* __restrict__ out_rt, int* __restrict__ out_count,
                                                         long long* __restrict__ out_cost, long long* __restrict__ out_trace) {
#pragma clang fp contract(off)
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= slots) return;
  const size_t row = (size_t)joints * 3;
  double c0[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) c0[j] = (double)__fdiv_rn(xyz0[slot * row + j], 1000.f);
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, T[3] = {0.0, 0.0, 0.0};
  bool moved = false;
  for (int t = 0; t < iters; ++t) {
    const size_t at = (size_t)t * slots + slot;
    const int matches = counts[2 * at], status = counts[2 * at + 1];
    out_trace[((size_t)slot * iters + t) * 3] = matches;
    out_trace[((size_t)slot * iters + t) * 3 + 1] = status;
    out_trace[((size_t)slot * iters + t) * 3 + 2] = costs[at];
    if (status != 0) continue;
    const float* rt = rts + at * 12;
    double rr[9], tt[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) rr[j] = (double)rt[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) tt[j] = (double)rt[9 + j];
    if (!moved) {                   // (nothing has moved yet: this iteration's root IS c0, and its motion is the whole motion)
#pragma unroll
      for (int j = 0; j < 9; ++j) R[j] = rr[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) T[j] = tt[j];
      moved = true;
      continue;
    }
    const float* root = (t == 0 ? xyz0 : xyz_it + (size_t)(t - 1) * slots * row) + slot * row;
    double c[3], u[3], nt[3], nr[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      c[j] = (double)__fdiv_rn(root[j], 1000.f);
      u[j] = (c0[j] + T[j]) - c[j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
      nt[j] = ((((rr[3 * j] * u[0] + rr[3 * j + 1] * u[1]) + rr[3 * j + 2] * u[2]) + c[j]) + tt[j]) - c0[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) nr[3 * i + j] = (rr[3 * i] * R[j] + rr[3 * i + 1] * R[3 + j]) + rr[3 * i + 2] * R[6 + j];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = nr[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) T[j] = nt[j];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) out_rt[(size_t)slot * 12 + j] = (float)R[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) out_rt[(size_t)slot * 12 + 9 + j] = (float)T[j];
  out_count[2 * slot] = counts[2 * slot];                     // iteration 1: what a single fit hands out
  out_count[2 * slot + 1] = counts[2 * slot + 1];
  out_cost[slot] = costs[slot];
}

}  // namespace

extern "C" int64_t hn_mesh_fit_iters_scratch_bytes(int n, int k, int h, int w, int v, int f, int joints, int iters) {
  if (n <= 0 || n > 65535 || k <= 0 || k > hn::kMaxSlots || h <= 0 || h > 16384 || w <= 0 || w > 16384 || v <= 0 || v > (1 << 24) || f <= 0 ||
      joints <= 0 || joints > 4096 || iters < 1 || iters > kMaxIters)
    return 0;
  return (int64_t)work_layout(n, k, h, w, v, f, joints, iters).total;
}

extern "C" int hn_mesh_fit_iters_f32(const float* mesh_depth, const uint8_t* silhouette, const float* scene_depth,
                                     int64_t depth_frame_stride, const float* paras, const float* cams, const float* mesh,
                                     const float* xyz_mm, const int32_t* faces, const int32_t* faces_host, const int32_t* lifted,
                                     int n, int k, int h, int w, int v, int f, int joints, int iters, int stride, float band,
                                     int min_points, double damp, double max_shift2, double tan2_half_angle, void* scratch,
                                     int64_t scratch_bytes, void* work, int64_t work_bytes, float* out_mesh, float* out_xyz,
                                     float* out_rt, int32_t* out_count, int64_t* out_cost, int64_t* out_trace, void* stream) {
  const char* fn = "hn_mesh_fit_iters_f32";
  // every check of hn_mesh_fit_f32 and of hn_mesh_geometry_f32 (depth_pass.h), under this entry's name and before the first launch
  using namespace hn;
  HN_CHECK_ARG(mesh_depth && silhouette && scene_depth && mesh && xyz_mm && faces && scratch && work && out_mesh && out_xyz && out_rt &&
                   out_count && out_cost && out_trace,
               "%s: null pointer", fn);
  if (int st = check_one_camera(fn, paras, cams)) return st;
  HN_CHECK_ARG(iters >= 1 && iters <= kMaxIters, "%s: iters = %d (1..%d)", fn, iters, kMaxIters);
  if (int st = check_frames(fn, n, k, h, w)) return st;
  if (int st = check_depth_stride(fn, depth_frame_stride, h, w)) return st;
  if (int st = check_fit_sizes(fn, v, &f, joints)) return st;
  if (int st = check_fit_options(fn, stride, band, min_points, damp, max_shift2, tan2_half_angle)) return st;
  if (int st = check_buffer(fn, "scratch", scratch, scratch_bytes, hn_mesh_fit_scratch_bytes(n, k, h), 8)) return st;
  const Work lay = work_layout(n, k, h, w, v, f, joints, iters);
  if (int st = check_buffer(fn, "work", work, work_bytes, (int64_t)lay.total, 16)) return st;
  if (int st = check_cams_aligned(fn, cams)) return st;
  HN_CHECK_ARG((((uintptr_t)out_cost & 7) | ((uintptr_t)out_trace & 7) | ((uintptr_t)out_count & 3) | ((uintptr_t)out_mesh & 3) |
                ((uintptr_t)out_xyz & 3) | ((uintptr_t)out_rt & 3)) == 0,
               "%s: out_mesh / out_xyz / out_rt / out_count must be aligned to 4 bytes, out_cost and out_trace to 8", fn);
  if (int st = check_faces_host(fn, faces_host, f, v)) return st;
  const int s = n * k;
  unsigned char* base = static_cast<unsigned char*>(work);
  float* meshes[2] = {reinterpret_cast<float*>(base + lay.mesh[0]), reinterpret_cast<float*>(base + lay.mesh[1])};
  float* xyzs = reinterpret_cast<float*>(base + lay.xyz);
  float* rts = reinterpret_cast<float*>(base + lay.rt);
  int32_t* counts = reinterpret_cast<int32_t*>(base + lay.count);
  int64_t* costs = reinterpret_cast<int64_t*>(base + lay.cost);
  float* depth = reinterpret_cast<float*>(base + lay.depth);
  uint8_t* who = base + lay.who;
  const size_t xyz_step = (size_t)s * joints * 3;
  const float* cur_mesh = mesh;
  const float* cur_xyz = xyz_mm;
  for (int t = 1; t <= iters; ++t) {
    const bool last = t == iters;
    float* to_mesh = last ? out_mesh : meshes[(t - 1) & 1];
    float* to_xyz = last ? out_xyz : xyzs + (size_t)(t - 1) * xyz_step;
    const float* best = mesh_depth;
    const uint8_t* sil = silhouette;
    if (t >= 2) {                   // the current meshes drawn again (slots with lifted == 0 are not, as in the step's raster)
      const int st = hn_mesh_geometry_f32(cur_mesh, faces, nullptr, lifted, s, v, f, k, paras, cams, h, w, base + lay.raster,
                                          (int64_t)(lay.total - lay.raster), depth, who, stream);
      if (st != HN_OK) return st;
      best = depth;
      sil = who;
    }
    const int st = hn_mesh_fit_f32(best, sil, scene_depth, depth_frame_stride, paras, cams, cur_mesh, cur_xyz, n, k, h, w, v, joints,
                                   stride, band, min_points, damp, max_shift2, tan2_half_angle, scratch, scratch_bytes, to_mesh,
                                   to_xyz, rts + (size_t)(t - 1) * s * 12, counts + (size_t)(t - 1) * s * 2,
                                   costs + (size_t)(t - 1) * s, stream);
    if (st != HN_OK) return st;
    cur_mesh = to_mesh;
    cur_xyz = to_xyz;
  }
  hipLaunchKernelGGL(mesh_refit_compose, dim3((s + 63) / 64), dim3(64), 0, (hipStream_t)stream, xyz_mm, xyzs, rts,
                     reinterpret_cast<const int*>(counts), reinterpret_cast<const long long*>(costs), s, joints, iters, out_rt,
                     reinterpret_cast<int*>(out_count), reinterpret_cast<long long*>(out_cost),
                     reinterpret_cast<long long*>(out_trace));
  HN_CHECK_LAUNCH("mesh_refit_compose");
  return HN_OK;
}
