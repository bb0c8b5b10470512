// The rig frame of a multi-camera live step (tests/rig_ref.py restates the rule in numpy float32, operation
// for operation): every slot's joints and final mesh moved into the caller's rig frame with its camera's extrinsics, the slots
// of different cameras that show one physical hand put into one rig hand, and the members of a rig hand fused into one estimate
// weighted by their detection scores.
//
// Three launches, ordered by their kernel boundaries: no workgroup waits for another inside a launch and there is no atomic,
// so the outputs are a pure function of the inputs and two runs give the same bytes.
//   rig_transform_kernel   one workgroup column per slot, striding over its 21 joints and V vertices (V is no multiple of 64)
//   rig_associate_kernel   ONE workgroup of 256 threads (n * k <= 256 slots), thread s = slot s: the slots' centres, then the
//                          greedy rule seed by seed, every slot weighing itself against the k slots of its own camera
//   rig_fuse_kernel        one workgroup column per rig hand: its members from rig_hand, then every coordinate summed in member order
// The file is built with -ffp-contract=off (hn_amd/build.py): one rounding per operation, as numpy rounds.
#include "hn_common.h"

namespace {

constexpr int kRigMaxSlots = 256;

// out[r] = ((R[r][0] * c.x + R[r][1] * c.y) + R[r][2] * c.z) + t[r] for the coordinate r of one point
__device__ __forceinline__ float rig_row(const float* __restrict__ e, int r, float x, float y, float z) {
#pragma clang fp contract(off)
  const float a = e[r * 4 + 0] * x;
  const float b = e[r * 4 + 1] * y;
  const float c = e[r * 4 + 2] * z;
  return ((a + b) + c) + e[r * 4 + 3];
}

// grid (chunks, slots): block (., s) strides over the (joints + v) * 3 output coordinates of slot s
__global__ __launch_bounds__(256) void rig_transform_kernel(const float* __restrict__ xyz_mm, const float* __restrict__ mesh,
                                                            const int* __restrict__ has_hand, const int* __restrict__ lifted,
                                                            const float* __restrict__ ext, int k, int joints, int v,
                                                            float* __restrict__ rig_xyz, float* __restrict__ rig_mesh) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const float* e = ext + (long)(s / k) * 12;
  const bool has = has_hand[s] == 1, lift = lifted[s] == 1;
  const int total = (joints + v) * 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int p = i / 3, r = i - p * 3;
    // (a row that is not valid is never read: NaN or inf in it cannot reach the output)
    if (p < joints) {
      float val = 0.f;
      if (has) {
        const float* c = xyz_mm + ((long)s * joints + p) * 3;
        val = rig_row(e, r, c[0] / 1000.f, c[1] / 1000.f, c[2] / 1000.f);
      }
      rig_xyz[((long)s * joints + p) * 3 + r] = val;
    } else {
      const int q = p - joints;
      float val = 0.f;
      if (lift) {
        const float* m = mesh + ((long)s * v + q) * 3;                   // out['mesh'] is (x, -y, -z) of the camera frame
        val = rig_row(e, r, m[0], -m[1], -m[2]);
      }
      rig_mesh[((long)s * v + q) * 3 + r] = val;
    }
  }
}

// ONE workgroup, thread t = slot t (its centre, flags and rig hand in registers; the seeds' in LDS).  The seeds are walked in
// order; for a taken seed every free lifted slot of a LATER camera within the radius posts its d2 as a key, and the slot whose
// key no other slot of its camera beats (smaller d2, or the same d2 at a lower k) joins.  A thread writes its own entries only;
// two barriers per taken seed order the rest.
__global__ __launch_bounds__(kRigMaxSlots) void rig_associate_kernel(const float* __restrict__ rig_xyz, const int* __restrict__ lifted,
                                                                     const int* __restrict__ side, int n, int k, int joints,
                                                                     float radius, int* __restrict__ rig_hand,
                                                                     int* __restrict__ rig_count, int* __restrict__ rig_views,
                                                                     int* __restrict__ rig_seed) {
#pragma clang fp contract(off)
  __shared__ float cx[kRigMaxSlots], cy[kRigMaxSlots], cz[kRigMaxSlots], key[kRigMaxSlots];
  __shared__ int group[kRigMaxSlots], lift[kRigMaxSlots], sd[kRigMaxSlots], seed[kRigMaxSlots];
  const int t = threadIdx.x, slots = n * k;
  const bool slot = t < slots;
  float mx = 0.f, my = 0.f, mz = 0.f;
  bool mlift = false;
  int mside = 0, mgroup = -1;
  if (slot) {
    // the slot's centre: its rig-frame joints summed one after the other, one divide (the association key only)
    const float* p = rig_xyz + (long)t * joints * 3;
    float ax = p[0], ay = p[1], az = p[2];
    for (int j = 1; j < joints; ++j) {
      ax = ax + p[j * 3 + 0];
      ay = ay + p[j * 3 + 1];
      az = az + p[j * 3 + 2];
    }
    const float div = (float)joints;
    mx = ax / div;
    my = ay / div;
    mz = az / div;
    mlift = lifted[t] == 1;
    mside = side ? side[t] : 0;
    cx[t] = mx;
    cy[t] = my;
    cz[t] = mz;
    group[t] = -1;
    seed[t] = -1;
    lift[t] = mlift;
    sd[t] = mside;
  }
  const float r2 = radius * radius;
  const int mycam = t / k, first = mycam * k;
  int count = 0;
  for (int s = 0; s < slots; ++s) {
    __syncthreads();                                                      // the writes of the seed before are visible
    if (!lift[s] || group[s] != -1) continue;                             // (the same answer in every thread)
    const int g = count++;
    float d2 = 0.f;
    bool ok = false;
    if (slot && mlift && mgroup == -1 && mycam > s / k && (!side || mside == sd[s])) {
      const float dx = mx - cx[s], dy = my - cy[s], dz = mz - cz[s];
      d2 = (dx * dx + dy * dy) + dz * dz;
      ok = d2 <= r2;                                                      // (a NaN centre fails)
    }
    if (slot) key[t] = ok ? d2 : -1.f;                                    // (a d2 is never negative)
    __syncthreads();                                                      // the keys are posted, and group[s] has been read
    if (t == s) {
      mgroup = g;
      group[s] = g;
      seed[g] = s;
    } else if (ok) {                                                      // at most one member per camera
      bool win = true;
      for (int kk = 0; kk < k; ++kk) {
        const float other = key[first + kk];
        if (other >= 0.f && (other < d2 || (other == d2 && first + kk < t))) win = false;      // a tie keeps the lower k
      }
      if (win) {
        mgroup = g;
        group[t] = g;
      }
    }
  }
  __syncthreads();
  if (slot) {
    int members = 0;
    for (int m = 0; m < slots; ++m) members += group[m] == t;
    rig_hand[t] = mgroup;
    rig_views[t] = members;                                               // (0 beyond the count: no slot holds such a group)
    rig_seed[t] = seed[t];
  }
  if (t == 0) *rig_count = count;
}

// grid (chunks, slots), 256 threads: block (., g) writes row g of fused_xyz and fused_mesh
__global__ __launch_bounds__(256) void rig_fuse_kernel(const float* __restrict__ rig_xyz, const float* __restrict__ rig_mesh,
                                                       const int* __restrict__ rig_hand, const float* __restrict__ score,
                                                       int slots, int joints, int v, float* __restrict__ fused_xyz,
                                                       float* __restrict__ fused_mesh) {
#pragma clang fp contract(off)
  __shared__ int member[kRigMaxSlots];
  __shared__ float weight[kRigMaxSlots];
  __shared__ int wave_members[4];
  const int g = blockIdx.y;
  // the members in slot order: thread t is slot t, its place is the number of members in front of it (ballots, wave by wave)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool mine = t < slots && rig_hand[t] == g;
  const unsigned long long votes = __ballot(mine);
  if (lane == 0) wave_members[wave] = __popcll(votes);
  __syncthreads();
  int before = 0, c = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += wave_members[w];
    c += wave_members[w];
  }
  if (mine) {
    const int at = before + __popcll(votes & ((1ull << lane) - 1ull));
    member[at] = t;
    weight[at] = score[t];
  }
  __syncthreads();
  const int nj = joints * 3, total = (joints + v) * 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const bool joint = i < nj;
    const float* src = joint ? rig_xyz : rig_mesh;
    const long row = joint ? nj : (long)v * 3;
    const int at = joint ? i : i - nj;
    float val = 0.f;                                                      // (rows at or beyond the count: zeros)
    if (c == 1) {
      val = src[member[0] * row + at];                                    // one view: the member, bit for bit
    } else if (c > 1) {
      float w = weight[0];
      float acc = w * src[member[0] * row + at], wsum = w;
      for (int m = 1; m < c; ++m) {
        w = weight[m];
        acc = acc + w * src[member[m] * row + at];
        wsum = wsum + w;
      }
      val = acc / wsum;
    }
    (joint ? fused_xyz : fused_mesh)[g * row + at] = val;
  }
}

}  // namespace

extern "C" int hn_rig_fuse_f32(const float* xyz_mm, const float* mesh, const int32_t* has_hand, const int32_t* lifted,
                               const float* score, const int32_t* side, const float* extrinsics, int n, int k, int joints, int v,
                               float radius, float* rig_xyz, float* rig_mesh, int32_t* rig_hand, int32_t* rig_count,
                               int32_t* rig_views, int32_t* rig_seed, float* fused_xyz, float* fused_mesh, void* stream) {
  HN_CHECK_ARG(n > 0 && k > 0 && joints > 0 && v > 0, "hn_rig_fuse_f32: bad dims (n %d, k %d, joints %d, v %d: all must be positive)",
               n, k, joints, v);
  HN_CHECK_ARG((int64_t)n * k <= kRigMaxSlots, "hn_rig_fuse_f32: %lld slots (n %d x k %d), at most %d", (long long)n * k, n, k,
               kRigMaxSlots);
  HN_CHECK_ARG((int64_t)joints + v <= (1 << 24), "hn_rig_fuse_f32: joints + v must be at most %d", 1 << 24);
  HN_CHECK_ARG(radius > 0.f && radius <= 3.402823466e38f, "hn_rig_fuse_f32: radius must be finite and > 0 (got %g)", (double)radius);
  HN_CHECK_ARG(xyz_mm && mesh && has_hand && lifted && score && extrinsics && rig_xyz && rig_mesh && rig_hand && rig_count &&
                   rig_views && rig_seed && fused_xyz && fused_mesh,
               "hn_rig_fuse_f32: null pointer");
  const int slots = n * k;
  const dim3 grid(hn::cdiv((int64_t)(joints + v) * 3, 1024), slots);     // (four coordinates per thread at the most)
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rig_transform_kernel, grid, dim3(256), 0, st, xyz_mm, mesh, has_hand, lifted, extrinsics, k, joints, v,
                     rig_xyz, rig_mesh);
  HN_CHECK_LAUNCH("rig_transform_kernel");
  hipLaunchKernelGGL(rig_associate_kernel, dim3(1), dim3(kRigMaxSlots), 0, st, rig_xyz, lifted, side, n, k, joints, radius,
                     rig_hand, rig_count, rig_views, rig_seed);
  HN_CHECK_LAUNCH("rig_associate_kernel");
  hipLaunchKernelGGL(rig_fuse_kernel, grid, dim3(256), 0, st, rig_xyz, rig_mesh, rig_hand, score, slots, joints, v, fused_xyz,
                     fused_mesh);
  HN_CHECK_LAUNCH("rig_fuse_kernel");
  return HN_OK;
}
