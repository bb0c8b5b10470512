// Each hand's depth pixels as a compact 3-D point cloud (tests/cloud_ref.py restates the rule in numpy
// float32, operation for operation): the candidate pixels (every `stride`-th row and column) whose silhouette byte names slot
// k, whose scene depth D is valid and whose residual e = D - best (best: the raster's nearest mesh Z) lies within the band are
// back-projected with the frame's camera, optionally moved into the rig frame with the frame's [R | t], and stored per slot
// in row-major order, the first `points` of them; per slot also the two counts and the summed residual in micrometres.
//
// Two launches over the same grid (blocks of four row strips, frames), ordered by their kernel boundary.  The unit of work is
// a STRIP: `strip_rows(h)` consecutive rows, walked by ONE wave in row-major order, 64 candidates at a time.
//   hand_cloud_count   every wave counts its strip's matches per slot (one ballot per slot present in a chunk, as the coverage
//                      counters of mesh_raster_tiles find the slots present) and sums their residuals (a wave reduction of
//                      integers); lane kk keeps slot kk's two numbers and writes them into the table [frame][strip][k].
//   hand_cloud_write   every workgroup sums the table's counts of the strips in front of its own (and over all strips: the
//                      totals), every wave adds the strips in front of it inside the workgroup; lane kk keeps slot kk's
//                      running offset.  The strip is walked again, a match is placed at offset + popcount(ballot & lanes
//                      below) and stored when that lies below `points`.  The totals, the residual sums (workgroup 0 of a
//                      frame) and the zero tail [written, points) (shared among the frame's workgroups) need the table alone.
// No workgroup waits for another inside a launch, no floating-point atomic (no atomic at all): the outputs are a pure function
// of the inputs and two runs give the same bytes.  The file is built with -ffp-contract=off (hn_amd/build.py).
#include "depth_pass.h"

namespace {

using namespace hn;                 // depth_pass.h: the strips, kMaxSlots, wave_sum, the camera, back_x / back_y, valid_depth

// the scratch: int64 sums [n][strips][k], then int32 counts [n][strips][k]
__host__ __device__ inline size_t table_entries(int n, int k, int h) { return (size_t)n * strips_padded(h) * k; }

struct CloudIn {
  const float* best;                // [n][h][w] the raster's out_depth
  const unsigned char* sil;         // [n][h][w]
  const float* depth;               // frame i at depth + i * frame_stride, [h][w]
  long long frame_stride;
  const float* cams;                // device [n][4], or null: the four values below
  float fx, fy, cx, cy;
  const float* ext;                 // device [n][12], or null: the camera frame
  int k, h, w, q;
  float band;
};

struct Match {
  bool hit;
  int slot;                         // within the frame
  float d, e;
};

// the candidate pixel (r, c) of frame i: does it match a slot, and which (the depth dword is loaded only under a silhouette byte)
__device__ __forceinline__ Match classify(const CloudIn& in, int i, int r, int c, bool active) {
#pragma clang fp contract(off)
  Match m = {false, 0, 0.f, 0.f};
  if (!active) return m;
  const size_t pix = ((size_t)i * in.h + r) * in.w + c;
  const int who = in.sil[pix] & 0x7F;                                     // (the hidden flag is ignored)
  if (who == 0 || who > in.k) return m;
  const float d = in.depth[(size_t)i * in.frame_stride + (size_t)r * in.w + c];
  if (!valid_depth(d)) return m;
  const float e = __fsub_rn(d, in.best[pix]);
  m.hit = fabsf(e) <= in.band;                                            // (NaN fails)
  m.slot = who - 1;
  m.d = d;
  m.e = e;
  return m;
}

// grid (strips / 4, frames), 256 threads: wave wv of block (b, i) walks strip 4 b + wv of frame i
__global__ __launch_bounds__(256) void hand_cloud_count(CloudIn in, long long* __restrict__ sums, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63, i = blockIdx.y;
  const int strips = gridDim.x * 4, u = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int rows = strip_rows(in.h), wc = (in.w + in.q - 1) / in.q;
  int mine = 0;                                                           // lane kk: slot kk's matches in this strip ...
  long long resid = 0;                                                    // ... and their summed residual, micrometres
  const int r1 = min(in.h, (u + 1) * rows);
  for (int r = (u * rows + in.q - 1) / in.q * in.q; r < r1; r += in.q) {
    for (int j0 = 0; j0 < wc; j0 += 64) {
      const int j = j0 + lane;
      const Match m = classify(in, i, r, j * in.q, j < wc);
      const int um = m.hit ? (int)rintf(__fmul_rn(m.e, 1e6f)) : 0;
      unsigned long long todo = __ballot(m.hit);
      while (todo) {                                                      // a ballot per slot present in the chunk
        const int kk = __shfl(m.slot, __builtin_ctzll(todo), 64);
        const bool of = m.hit && m.slot == kk;
        const unsigned long long votes = __ballot(of);
        todo &= ~votes;
        const long long sum = wave_sum(of ? (long long)um : 0ll);
        if (lane == kk) {
          mine += __popcll(votes);
          resid += sum;
        }
      }
    }
  }
  if (lane < in.k) {
    const size_t at = ((size_t)i * strips + u) * in.k + lane;
    counts[at] = mine;
    sums[at] = resid;
  }
}

// the same grid: the offsets from the table, the strip walked again, rows below `points` stored; totals, sums and zero tails
__global__ __launch_bounds__(256) void hand_cloud_write(CloudIn in, const long long* __restrict__ sums, const int* __restrict__ counts,
                                                        int points, float* __restrict__ cloud, int* __restrict__ out_count,
                                                        long long* __restrict__ out_resid) {
#pragma clang fp contract(off)
  __shared__ int part_before[16][kMaxSlots], part_total[16][kMaxSlots];
  __shared__ long long part_resid[16][kMaxSlots];
  __shared__ int before[kMaxSlots], total[kMaxSlots];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, i = blockIdx.y;
  const int strips = gridDim.x * 4, first = blockIdx.x * 4, u = first + wv;
  const size_t frame_at = (size_t)i * strips * in.k;
  {
    // thread (part, kk): slot kk's counts of the strips part, part + 16, ..., split at the workgroup's first strip
    const int kk = t & 15, part = t >> 4;
    int b = 0, all = 0;
    long long rs = 0;
    if (kk < in.k) {
      for (int s = part; s < strips; s += 16) {
        const int c = counts[frame_at + (size_t)s * in.k + kk];
        all += c;
        if (s < first) b += c;
        if (blockIdx.x == 0) rs += sums[frame_at + (size_t)s * in.k + kk];
      }
    }
    part_before[part][kk] = b;
    part_total[part][kk] = all;
    part_resid[part][kk] = rs;
  }
  __syncthreads();
  if (t < in.k) {
    int b = 0, all = 0;
    long long rs = 0;
    for (int p = 0; p < 16; ++p) {
      b += part_before[p][t];
      all += part_total[p][t];
      rs += part_resid[p][t];
    }
    before[t] = b;
    total[t] = all;
    if (blockIdx.x == 0) {                                                // (known from the table alone)
      const size_t s = (size_t)i * in.k + t;
      out_count[2 * s] = all;
      out_count[2 * s + 1] = min(all, points);
      out_resid[s] = rs;
    }
  }
  __syncthreads();
  // the zero tail [written, points) of the frame's slots, shared among the frame's workgroups
  for (int kk = 0; kk < in.k; ++kk) {
    float* rows = cloud + ((size_t)i * in.k + kk) * points * 3;
    const size_t end = (size_t)points * 3;
    for (size_t at = (size_t)min(total[kk], points) * 3 + (size_t)blockIdx.x * 256 + t; at < end; at += (size_t)gridDim.x * 256)
      rows[at] = 0.f;
  }
  // lane kk: slot kk's matches in front of this wave's strip
  int run = 0;
  if (lane < in.k) {
    run = before[lane];
    for (int s = first; s < u; ++s) run += counts[frame_at + (size_t)s * in.k + lane];
  }
  const Cam cam = camera(in.cams, i, in.fx, in.fy, in.cx, in.cy);
  const float* e = in.ext ? in.ext + 12 * (size_t)i : nullptr;
  const int rows = strip_rows(in.h), wc = (in.w + in.q - 1) / in.q;
  const int r1 = min(in.h, (u + 1) * rows);
  for (int r = (u * rows + in.q - 1) / in.q * in.q; r < r1; r += in.q) {
    for (int j0 = 0; j0 < wc; j0 += 64) {
      const int j = j0 + lane, c = j * in.q;
      const Match m = classify(in, i, r, c, j < wc);
      unsigned long long todo = __ballot(m.hit);
      while (todo) {
        const int kk = __shfl(m.slot, __builtin_ctzll(todo), 64);
        const bool of = m.hit && m.slot == kk;
        const unsigned long long votes = __ballot(of);
        todo &= ~votes;
        const int pos = __shfl(run, kk, 64) + __popcll(votes & ((1ull << lane) - 1ull));
        if (of && pos < points) {
          float x = back_x(cam, c, m.d), y = back_y(cam, r, m.d), z = m.d;
          if (e) {                                                        // 9i's transform, in its operation order
            const float px = x, py = y, pz = z;
            x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(e[0], px), __fmul_rn(e[1], py)), __fmul_rn(e[2], pz)), e[3]);
            y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(e[4], px), __fmul_rn(e[5], py)), __fmul_rn(e[6], pz)), e[7]);
            z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(e[8], px), __fmul_rn(e[9], py)), __fmul_rn(e[10], pz)), e[11]);
          }
          float* dst = cloud + (((size_t)i * in.k + kk) * points + pos) * 3;
          dst[0] = x;
          dst[1] = y;
          dst[2] = z;
        }
        if (lane == kk) run += __popcll(votes);
      }
    }
  }
}

}  // namespace

extern "C" int64_t hn_hand_cloud_scratch_bytes(int n, int k, int h) {
  if (n <= 0 || k <= 0 || k > kMaxSlots || h <= 0 || h > 16384) return 0;
  return (int64_t)(table_entries(n, k, h) * (sizeof(long long) + sizeof(int)));
}

extern "C" int hn_hand_cloud_f32(const float* mesh_depth, const uint8_t* silhouette, const float* scene_depth,
                                 int64_t depth_frame_stride, const float* paras, const float* cams, const float* extrinsics, int n,
                                 int k, int h, int w, int points, int stride, float band, void* scratch, int64_t scratch_bytes,
                                 float* out_cloud, int32_t* out_count, int64_t* out_resid, void* stream) {
  const char* fn = "hn_hand_cloud_f32";
  HN_CHECK_ARG(mesh_depth && silhouette && scene_depth && scratch && out_cloud && out_count && out_resid, "%s: null pointer", fn);
  if (int st = check_one_camera(fn, paras, cams)) return st;
  if (int st = check_frames(fn, n, k, h, w)) return st;
  if (int st = check_depth_stride(fn, depth_frame_stride, h, w)) return st;
  HN_CHECK_ARG(points >= 1, "%s: points = %d (at least 1)", fn, points);
  if (int st = check_sampling(fn, stride, band)) return st;
  if (int st = check_buffer(fn, "scratch", scratch, scratch_bytes, hn_hand_cloud_scratch_bytes(n, k, h), 8)) return st;
  HN_CHECK_ARG((((uintptr_t)out_resid & 7) | ((uintptr_t)out_count & 3) | ((uintptr_t)out_cloud & 3)) == 0,
               "%s: out_cloud / out_count must be aligned to 4 bytes and out_resid to 8", fn);
  CloudIn in = {mesh_depth, silhouette, scene_depth, (long long)depth_frame_stride, cams, 0.f, 0.f, 0.f, 0.f, extrinsics, k, h, w,
                std::min(stride, 16384), band};      // (h, w <= 16384: every larger stride leaves the pixel (0, 0) alone, as this one)
  if (paras) { in.fx = paras[0]; in.fy = paras[1]; in.cx = paras[2]; in.cy = paras[3]; }
  long long* sums = static_cast<long long*>(scratch);
  int* counts = reinterpret_cast<int*>(sums + table_entries(n, k, h));
  const dim3 grid(strips_padded(h) / 4, n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(hand_cloud_count, grid, dim3(256), 0, st, in, sums, counts);
  HN_CHECK_LAUNCH("hand_cloud_count");
  hipLaunchKernelGGL(hand_cloud_write, grid, dim3(256), 0, st, in, sums, counts, points, out_cloud, out_count,
                     reinterpret_cast<long long*>(out_resid));
  HN_CHECK_LAUNCH("hand_cloud_write");
  return HN_OK;
}
