// The hand-pose evaluator's tables on the device (tests/hpe_ref.py restates the rule in numpy fp64, operation
// for operation): per sample and joint the absolute, the root-relative and the Procrustes-aligned distance between prediction and
// ground truth (dex_ycb_toolkit/hpe_eval.py:198-218; freihand/eval.py:72-95 align_w_scale), added into an integer state -- a
// histogram over the PCK thresholds, a fixed-point sum for the MPJPE, the sample counts -- that the host turns into MPJPE, PCK and
// AUC once per epoch.
//
// One launch.  One wave per sample, one lane per joint (J <= 64), kWaves waves per workgroup.  What belongs to a joint is done by
// its lane; the reductions over the joints (means, norms, the 3 x 3 cross-covariance) are sequential loops in joint order over the
// wave's LDS rows, run by every lane alike, and so are the fixed-sweep Jacobi SVD and the rotation: no cross-lane arithmetic, one
// rounding per operation (built with -ffp-contract=off, hn_amd/build.py).  The only atomics are integer adds -- the sums and the
// counts first into LDS, one global add per workgroup and cell -- so the state's bytes do not depend on the order of anything
// (the argument of mesh_raster.hip's coverage counts).  Every barrier is at the kernel's top level: all waves of a workgroup
// reach each of them, whether their sample is fed, skipped or beyond the batch.
#include <cmath>

#include "hn_common.h"

namespace {

constexpr int kWaves = 4;
constexpr int kSweeps = 10;                         // tests/hpe_ref.py SWEEPS: five converge every measured case
constexpr double kLimit = 1048576.0;                // 2^20 mm
constexpr double kQ20 = 1048576.0;
constexpr double kLive = 1.4901161193847656e-08;    // 2^-26

typedef unsigned long long u64;

__device__ __forceinline__ double dist3(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
#pragma clang fp contract(off)
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// one Jacobi rotation of the columns (P, Q) of G, the same on V
template <int P, int Q>
__device__ __forceinline__ void rotate(double (&g)[3][3], double (&v)[3][3]) {
#pragma clang fp contract(off)
  const double alpha = (g[0][P] * g[0][P] + g[1][P] * g[1][P]) + g[2][P] * g[2][P];
  const double beta = (g[0][Q] * g[0][Q] + g[1][Q] * g[1][Q]) + g[2][Q] * g[2][Q];
  const double gamma = (g[0][P] * g[0][Q] + g[1][P] * g[1][Q]) + g[2][P] * g[2][Q];
  if (gamma == 0.0) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double sgn = zeta >= 0.0 ? 1.0 : -1.0;
  const double t = sgn / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t);
  const double sn = c * t;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double gp = g[r][P], gq = g[r][Q];
    g[r][P] = c * gp - sn * gq;
    g[r][Q] = sn * gp + c * gq;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double vp = v[r][P], vq = v[r][Q];
    v[r][P] = c * vp - sn * vq;
    v[r][Q] = sn * vp + c * vq;
  }
}

// M -> R = U V^T (reflections allowed) and s = the sum of the singular values; a rank-deficient M is completed as the rule says
__device__ void rotation(double (&g)[3][3], double (&rot)[3][3], double& ssum) {
#pragma clang fp contract(off)
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    rotate<0, 1>(g, v);
    rotate<0, 2>(g, v);
    rotate<1, 2>(g, v);
  }
  double sig[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) sig[i] = sqrt((g[0][i] * g[0][i] + g[1][i] * g[1][i]) + g[2][i] * g[2][i]);
  ssum = (sig[0] + sig[1]) + sig[2];
  const double top = fmax(fmax(sig[0], sig[1]), sig[2]);
  const double floor_ = kLive * top;
  bool live[3];
  int count = 0;
  double u[3][3];                                   // u[i] = COLUMN i of U
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    live[i] = sig[i] > 0.0 && sig[i] > floor_;
    count += live[i] ? 1 : 0;
    const double den = live[i] ? sig[i] : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) u[i][r] = live[i] ? g[r][i] / den : 0.0;
  }
  if (count == 2) {
    double c[3];
    if (!live[0]) {
      cross3(u[1], u[2], c);
      u[0][0] = c[0], u[0][1] = c[1], u[0][2] = c[2];
    } else if (!live[1]) {
      cross3(u[2], u[0], c);
      u[1][0] = c[0], u[1][1] = c[1], u[1][2] = c[2];
    } else {
      cross3(u[0], u[1], c);
      u[2][0] = c[0], u[2][1] = c[1], u[2][2] = c[2];
    }
  } else if (count == 1) {
    double x[3], w[3], y[3], z[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = live[0] ? u[0][r] : (live[1] ? u[1][r] : u[2][r]);
    double best = fabs(x[0]), xk = x[0];
    int k = 0;
    if (fabs(x[1]) < best) best = fabs(x[1]), xk = x[1], k = 1;
    if (fabs(x[2]) < best) xk = x[2], k = 2;
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = (r == k ? 1.0 : 0.0) - xk * x[r];
    const double len = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = w[r] / len;
    cross3(x, y, z);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      if (live[0]) u[1][r] = y[r], u[2][r] = z[r];
      else if (live[1]) u[2][r] = y[r], u[0][r] = z[r];
      else u[0][r] = y[r], u[1][r] = z[r];
    }
  } else if (count == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int r = 0; r < 3; ++r) u[i][r] = i == r ? 1.0 : 0.0;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) rot[a][b] = (u[0][a] * v[b][0] + u[1][a] * v[b][1]) + u[2][a] * v[b][2];
  }
}

// #{i : thr[i] < d} for non-decreasing thr[0..t)
__device__ __forceinline__ int bin_of(const double* __restrict__ thr, int t, double d) {
  int lo = 0, hi = t;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] < d) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// grid (ceil(s / kWaves)), kWaves * 64 threads: wave = sample, lane = joint
__global__ __launch_bounds__(kWaves * 64) void hpe_accumulate_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                      const int* __restrict__ valid, int s, int j,
                                                                      const double* __restrict__ thr, int t, u64* __restrict__ hist,
                                                                      u64* __restrict__ sum, u64* __restrict__ n,
                                                                      double* __restrict__ dist_out,
                                                                      double* __restrict__ aligned_out) {
#pragma clang fp contract(off)
  __shared__ double rows[kWaves][6][64];            // per wave: the sample's gt (0..2) and prediction (3..5), one column per joint
  __shared__ u64 l_sum[3][64];
  __shared__ unsigned int l_n[2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < 3 * 64) l_sum[tid >> 6][tid & 63] = 0;
  if (tid < 2) l_n[tid] = 0;
  const long long sample = (long long)blockIdx.x * kWaves + wave;
  const bool in_batch = sample < (long long)s;
  const bool mine = in_batch && lane < j;
  const size_t base = in_batch ? (size_t)sample * j * 3 : 0;
  double (&row)[6][64] = rows[wave];

  double g[3] = {0.0, 0.0, 0.0}, p[3] = {0.0, 0.0, 0.0};
  bool bad = false;
  if (mine) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g[c] = (double)gt[base + (size_t)lane * 3 + c];
      p[c] = (double)pred[base + (size_t)lane * 3 + c];
      bad = bad || !(fabs(g[c]) < kLimit) || !(fabs(p[c]) < kLimit);           // (NaN and inf compare false)
    }
  }
  const bool refused = __ballot(bad) != 0 || (in_batch && valid != nullptr && valid[sample] == 0);
  const bool fed = in_batch && !refused;            // uniform over the wave
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    row[c][lane] = g[c];
    row[3 + c][lane] = p[c];
  }
  __syncthreads();

  // the means, in joint order; then the centred sets back into the rows
  double t1[3] = {0.0, 0.0, 0.0}, t2[3] = {0.0, 0.0, 0.0};
  double g0[3] = {0.0, 0.0, 0.0}, p0[3] = {0.0, 0.0, 0.0};
  if (fed) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g0[c] = row[c][0];
      p0[c] = row[3 + c][0];
    }
    for (int i = 0; i < j; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        t1[c] = t1[c] + row[c][i];
        t2[c] = t2[c] + row[3 + c][i];
      }
    }
    const double dj = (double)j;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      t1[c] = t1[c] / dj;
      t2[c] = t2[c] / dj;
    }
  }
  __syncthreads();
  double a1[3], b1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a1[c] = g[c] - t1[c];
    b1[c] = p[c] - t2[c];
    row[c][lane] = a1[c];
    row[3 + c][lane] = b1[c];
  }
  __syncthreads();

  // the Frobenius norms; then the scaled sets back into the rows
  double s1 = 1.0, s2 = 1.0;
  if (fed) {
    double n1 = 0.0, n2 = 0.0;
    for (int i = 0; i < j; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double a = row[c][i], b = row[3 + c][i];
        n1 = n1 + a * a;
        n2 = n2 + b * b;
      }
    }
    s1 = sqrt(n1) + 1e-8;
    s2 = sqrt(n2) + 1e-8;
  }
  __syncthreads();
  double b2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    b2[c] = b1[c] / s2;
    row[c][lane] = a1[c] / s1;
    row[3 + c][lane] = b2[c];
  }
  __syncthreads();

  if (fed) {
    double m[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int i = 0; i < j; ++i) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) m[a][b] = m[a][b] + row[a][i] * row[3 + b][i];
      }
    }
    double rot[3][3], ssum;
    rotation(m, rot, ssum);
    if (mine) {
      double al[3], d[3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
        al[a] = ((((b2[0] * rot[a][0] + b2[1] * rot[a][1]) + b2[2] * rot[a][2]) * ssum) * s1) + t1[a];
      d[0] = dist3(g[0] - p[0], g[1] - p[1], g[2] - p[2]);
      d[1] = dist3((g[0] - g0[0]) - (p[0] - p0[0]), (g[1] - g0[1]) - (p[1] - p0[1]), (g[2] - g0[2]) - (p[2] - p0[2]));
      d[2] = dist3(g[0] - al[0], g[1] - al[1], g[2] - al[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int bin = bin_of(thr, t, d[a]);                                   // 0 .. t
        atomicAdd(hist + ((size_t)a * j + lane) * (size_t)(t + 1) + bin, (u64)1);
        atomicAdd(&l_sum[a][lane], (u64)(long long)rint(d[a] * kQ20));
        if (dist_out) dist_out[((size_t)sample * 3 + a) * j + lane] = d[a];
      }
      if (aligned_out) {
#pragma unroll
        for (int a = 0; a < 3; ++a) aligned_out[base + (size_t)lane * 3 + a] = al[a];
      }
    }
    if (lane == 0) atomicAdd(&l_n[0], 1u);
  } else if (in_batch) {                            // skipped: counted, NaN rows in the optional outputs, nothing else
    if (mine) {
      const double nan = __longlong_as_double(0x7FF8000000000000LL);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (dist_out) dist_out[((size_t)sample * 3 + a) * j + lane] = nan;
        if (aligned_out) aligned_out[base + (size_t)lane * 3 + a] = nan;
      }
    }
    if (lane == 0) atomicAdd(&l_n[1], 1u);
  }
  __syncthreads();
  if (tid < 3 * 64) {
    const int a = tid >> 6, jj = tid & 63;
    const u64 part = l_sum[a][jj];
    if (jj < j && part != 0) atomicAdd(sum + (size_t)a * j + jj, part);
  }
  if (tid < 2 && l_n[tid] != 0) atomicAdd(n + tid, (u64)l_n[tid]);
}

}  // namespace

extern "C" int hn_hpe_accumulate_f32(const float* pred, const float* gt, const int32_t* valid, int s, int j, const double* thresholds,
                                     int t, int64_t* hist, int64_t* sum, int64_t* n, double* dist_out, double* aligned_out,
                                     void* stream) {
  const char* fn = "hn_hpe_accumulate_f32";
  HN_CHECK_ARG(s >= 0, "%s: s = %d (>= 0)", fn, s);
  HN_CHECK_ARG(j >= 1 && j <= 64, "%s: j = %d (1..64: one lane per joint)", fn, j);
  HN_CHECK_ARG(t >= 1 && t <= 1024, "%s: t = %d (1..1024)", fn, t);
  HN_CHECK_ARG(thresholds && hist && sum && n, "%s: null pointer (thresholds, hist, sum, n)", fn);
  HN_CHECK_ARG((((uintptr_t)thresholds | (uintptr_t)hist | (uintptr_t)sum | (uintptr_t)n | (uintptr_t)dist_out | (uintptr_t)aligned_out) & 7) == 0,
               "%s: thresholds, hist, sum, n, dist_out and aligned_out must be aligned to 8 bytes", fn);
  if (s == 0) return HN_OK;
  HN_CHECK_ARG(pred && gt, "%s: null pointer (pred, gt)", fn);
  HN_CHECK_ARG((((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)valid) & 3) == 0, "%s: pred, gt and valid must be aligned to 4 bytes", fn);
  hipLaunchKernelGGL(hpe_accumulate_kernel, dim3(hn::cdiv(s, kWaves)), dim3(kWaves * 64), 0, (hipStream_t)stream, pred, gt,
                     reinterpret_cast<const int*>(valid), s, j, thresholds, t, reinterpret_cast<u64*>(hist),
                     reinterpret_cast<u64*>(sum), reinterpret_cast<u64*>(n), dist_out, aligned_out);
  HN_CHECK_LAUNCH("hpe_accumulate_kernel");
  return HN_OK;
}
