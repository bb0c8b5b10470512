// The object each hand holds (tests/object_ref.py restates the rule in numpy float32, operation for
// operation): for every hand slot the detector's contact state, the detector's object that the hand's offset vector points at
// (the association of the reference's evaluation, lib/datasets/voc_eval.py:687-699, on the detections as they are), and that
// object's measured depth pixels reduced to a centroid and an extent in the camera frame.
//
// Three launches, ordered by their kernel boundaries:
//   hand_object_associate  one workgroup per frame.  Its threads stride ONCE over the frame's `count` detection rows; a row of
//                          the object label gives its centre, and every thread keeps, per slot in contact, the nearest object
//                          among ITS rows (rows come in rising rank, so `d < best` keeps the earlier one of a tie).  A
//                          workgroup reduction of (distance, rank) pairs -- smaller distance, then smaller rank; NaN distances
//                          never enter -- and of the first object's rank gives what the reference's sequential scan keeps:
//                          the first object when ITS distance is NaN (nothing compares below NaN), else the pair's rank.
//                          Thread kk writes slot kk's five outputs and its record for the next two launches: the pixel rows
//                          and columns that can hold candidates (a superset: the walk tests every pixel) and the status.
//   hand_object_walk       grid (strips / 4, slots per frame, frames): ONE wave per strip and slot walks the candidates of
//                          the strip's rows inside the record's bounds, 64 at a time, and writes the strip's partial: the
//                          match count, three integer sums, three minima and three maxima.  A strip outside the bounds
//                          writes the empty partial, so every partial is written on every run.
//   hand_object_finish     one wave per slot adds its strips' partials and writes object_count, object_xyz, object_extent.
// Integer sums, minima and maxima: any split of the pixels gives the same bytes.  No atomics, no workgroup waits for another.
// The file is built with -ffp-contract=off (hn_amd/build.py).
#include <climits>

#include "depth_pass.h"

namespace {

using namespace hn;                 // depth_pass.h: the strips, kMaxSlots, wave_sum, the camera, back_x / back_y, valid_depth

constexpr int kNone = INT_MAX;      // no rank yet
constexpr int kRecordWords = 8;     // a slot's record: r0, r1, c0, c1, status (-1 empty slot, 1 no object, 0 walk it), 3 unused
constexpr int kPartialWords = 8;    // a strip's partial, 8-byte words: sum x, y, z, count, (min x, min y), (min z, max x), (max y, max z), unused

// the scratch: the partials [n][k][strips] first (8-byte words), the records [n][k] behind them
__host__ __device__ inline size_t partial_entries(int n, int k, int h) { return (size_t)n * k * strips_padded(h); }

struct Best {
  float d;
  int r;                            // kNone: none
};

// does `o` come before `b` in the scan's order: a smaller distance, then the earlier rank (distances are never NaN here)
__device__ __forceinline__ bool before(const Best& o, const Best& b) {
  return o.r != kNone && (b.r == kNone || o.d < b.d || (o.d == b.d && o.r < b.r));
}

__device__ __forceinline__ float centre(float a, float b) { return __fmul_rn(__fadd_rn(a, b), 0.5f); }

// d = dx dx + dy dy from the object's centre to the point, each operation rounded once
__device__ __forceinline__ float distance2(float ox, float oy, float px, float py) {
  const float dx = __fsub_rn(ox, px), dy = __fsub_rn(oy, py);
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

struct AssocIn {
  const float* boxes;               // [n][cap][4]
  const float* scores;              // [n][cap]
  const int* labels;                // [n][cap]
  const int* count;                 // [n]
  const int* contacts;              // [n][cap]
  const float* dxdymags;            // [n][cap][3]
  const int* det_index;             // [n][k]
  int cap, k, object_label, h, w;
};

// grid (frames), 256 threads
__global__ __launch_bounds__(256) void hand_object_associate(AssocIn in, int* __restrict__ out_index, float* __restrict__ out_box,
                                                             float* __restrict__ out_score, float* __restrict__ out_point,
                                                             int* __restrict__ out_contact, int* __restrict__ records) {
#pragma clang fp contract(off)
  __shared__ float px[kMaxSlots], py[kMaxSlots];
  __shared__ int seeks[kMaxSlots];                                        // 1: the slot looks for an object
  __shared__ Best part[4][kMaxSlots];
  __shared__ int part_first[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, i = blockIdx.x;
  const int count = min(max(in.count[i], 0), in.cap);
  const size_t row0 = (size_t)i * in.cap;
  int contact = -1, j = -1;
  float hx = 0.f, hy = 0.f;
  if (t < kMaxSlots) {
    bool seek = false;
    if (t < in.k) {
      j = in.det_index[(size_t)i * in.k + t];
      if (j < 0 || j >= in.cap) j = -1;                                   // (a rank beyond the table names nothing: an empty slot)
      if (j >= 0) {
        contact = in.contacts[row0 + j];
        const float* hb = in.boxes + (row0 + j) * 4;
        const float* v = in.dxdymags + (row0 + j) * 3;
        const float m = __fmul_rn(v[0], 10000.f);                         // (m * 10000) * vx: left to right, as the reference writes it
        hx = __fadd_rn(centre(hb[0], hb[2]), __fmul_rn(m, v[1]));
        hy = __fadd_rn(centre(hb[1], hb[3]), __fmul_rn(m, v[2]));
        seek = contact > 0;
      }
    }
    px[t] = hx;
    py[t] = hy;
    seeks[t] = seek ? 1 : 0;
  }
  __syncthreads();
  Best best[kMaxSlots];
#pragma unroll
  for (int kk = 0; kk < kMaxSlots; ++kk) best[kk] = {0.f, kNone};
  int first = kNone;                                                      // this thread's first object row
  for (int r = t; r < count; r += 256) {                                  // (cap is the detector's point count: as many passes as it takes)
    if (in.labels[row0 + r] != in.object_label) continue;
    first = min(first, r);
    const float* ob = in.boxes + (row0 + r) * 4;
    const float ox = centre(ob[0], ob[2]), oy = centre(ob[1], ob[3]);
#pragma unroll
    for (int kk = 0; kk < kMaxSlots; ++kk) {
      if (kk < in.k && seeks[kk]) {
        const float d = distance2(ox, oy, px[kk], py[kk]);
        if (d == d && (best[kk].r == kNone || d < best[kk].d)) best[kk] = {d, r};      // (rising r: a tie keeps the earlier)
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
#pragma unroll
  for (int kk = 0; kk < kMaxSlots; ++kk) {
    if (kk < in.k) {                                                      // (uniform)
      Best b = best[kk];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        Best other;
        other.d = __shfl_xor(b.d, o, 64);
        other.r = __shfl_xor(b.r, o, 64);
        if (before(other, b)) b = other;
      }
      if (lane == 0) part[wv][kk] = b;
    }
  }
  if (lane == 0) part_first[wv] = first;
  __syncthreads();
  if (t >= in.k) return;
  // thread kk: slot kk
  const size_t s = (size_t)i * in.k + t;
  first = min(min(part_first[0], part_first[1]), min(part_first[2], part_first[3]));
  int chosen = -1, status = j < 0 ? -1 : 1;
  if (j >= 0 && contact > 0 && first != kNone) {
    Best b = part[0][t];
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (before(part[q][t], b)) b = part[q][t];
    const float* fb = in.boxes + (row0 + first) * 4;
    const float d0 = distance2(centre(fb[0], fb[2]), centre(fb[1], fb[3]), hx, hy);
    chosen = (d0 != d0 || b.r == kNone) ? first : b.r;                    // nothing compares below a NaN: the first object stays
    status = 0;
  }
  float bx[4] = {0.f, 0.f, 0.f, 0.f}, sc = 0.f;
  if (chosen >= 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bx[e] = in.boxes[(row0 + chosen) * 4 + e];
    sc = in.scores[row0 + chosen];
  }
  out_index[s] = chosen;
  out_contact[s] = contact;
#pragma unroll
  for (int e = 0; e < 4; ++e) out_box[s * 4 + e] = bx[e];
  out_score[s] = sc;
  out_point[s * 2 + 0] = hx;                                              // (zeros for an empty slot)
  out_point[s * 2 + 1] = hy;
  // the rows and columns whose centres can lie in the box: a superset (fmaxf(NaN, 0) is 0, so a NaN corner gives an empty or a
  // harmless range); the walk tests x1 <= c + 0.5 < x2 and y1 <= r + 0.5 < y2 on every pixel
  int* rec = records + s * kRecordWords;
  const float fw = (float)in.w, fh = (float)in.h;
  rec[0] = chosen < 0 ? 0 : (int)fminf(fmaxf(floorf(bx[1]) - 1.f, 0.f), fh);
  rec[1] = chosen < 0 ? 0 : (int)fminf(fmaxf(ceilf(bx[3]), 0.f), fh);
  rec[2] = chosen < 0 ? 0 : (int)fminf(fmaxf(floorf(bx[0]) - 1.f, 0.f), fw);
  rec[3] = chosen < 0 ? 0 : (int)fminf(fmaxf(ceilf(bx[2]), 0.f), fw);
  rec[4] = status;
  rec[5] = rec[6] = rec[7] = 0;
}

struct WalkIn {
  const float* depth;               // frame i at depth + i * frame_stride, [h][w]
  long long frame_stride;
  const unsigned char* sil;         // [n][h][w], or null: no exclusion
  const float* xyz_mm;              // [n * k][joints][3]
  const float* boxes;               // the chosen boxes [n * k][4]
  const float* cams;                // device [n][4], or null: the four values below
  float fx, fy, cx, cy;
  int k, h, w, q, joints;
  float band;
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ long long two_floats(float a, float b) {
  return (long long)(((unsigned long long)__float_as_uint(b) << 32) | (unsigned long long)__float_as_uint(a));
}
__device__ __forceinline__ float low_float(long long v) { return __uint_as_float((unsigned)((unsigned long long)v & 0xffffffffull)); }
__device__ __forceinline__ float high_float(long long v) { return __uint_as_float((unsigned)((unsigned long long)v >> 32)); }

// grid (strips / 4, slots per frame, frames), 256 threads: wave wv of block (b, kk, i) walks strip 4 b + wv for slot kk of frame i
__global__ __launch_bounds__(256) void hand_object_walk(WalkIn in, const int* __restrict__ records, long long* __restrict__ partials) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, i = blockIdx.z, kk = blockIdx.y;
  const int strips = gridDim.x * 4, u = blockIdx.x * 4 + (threadIdx.x >> 6);
  const size_t s = (size_t)i * in.k + kk;
  const int* rec = records + s * kRecordWords;
  const int rows = strip_rows(in.h);
  const bool walk = rec[4] == 0;
  const int r_lo = max(u * rows, rec[0]), r_hi = walk ? min(min(in.h, (u + 1) * rows), rec[1]) : 0;
  const int c_lo = rec[2], c_hi = rec[3];
  const float x1 = in.boxes[s * 4 + 0], y1 = in.boxes[s * 4 + 1], x2 = in.boxes[s * 4 + 2], y2 = in.boxes[s * 4 + 3];
  const float z_hand = __fmul_rn(in.xyz_mm[s * in.joints * 3 + 2], 0.001f);
  const Cam cam = camera(in.cams, i, in.fx, in.fy, in.cx, in.cy);
  int m = 0;
  long long sx = 0, sy = 0, sz = 0;
  const float inf = __builtin_huge_valf();
  float lo_x = inf, lo_y = inf, lo_z = inf, hi_x = -inf, hi_y = -inf, hi_z = -inf;
  const int j_lo = (c_lo + in.q - 1) / in.q;
  for (int r = (r_lo + in.q - 1) / in.q * in.q; r < r_hi; r += in.q) {
    const float yc = __fadd_rn((float)r, 0.5f);
    if (!(y1 <= yc && yc < y2)) continue;                                 // (uniform)
    for (int j0 = j_lo; j0 * in.q < c_hi; j0 += 64) {
      const int c = (j0 + lane) * in.q;                                   // (j0 + 63 <= 16384 + 63, q <= 16384: inside an int)
      if (c >= c_hi) continue;
      const float xc = __fadd_rn((float)c, 0.5f);
      if (!(x1 <= xc && xc < x2)) continue;
      const size_t pix = (size_t)r * in.w + c;
      const float d = in.depth[(size_t)i * in.frame_stride + pix];
      if (!valid_depth(d)) continue;
      if (in.sil && (in.sil[(size_t)i * in.h * in.w + pix] & 0x7F) != 0) continue;       // under a hand's mesh: not the object
      if (!(fabsf(__fsub_rn(d, z_hand)) <= in.band)) continue;            // (NaN fails)
      const float x = back_x(cam, c, d), y = back_y(cam, r, d);
      ++m;
      sx += (long long)rintf(__fmul_rn(x, 1e6f));
      sy += (long long)rintf(__fmul_rn(y, 1e6f));
      sz += (long long)rintf(__fmul_rn(d, 1e6f));
      lo_x = fminf(lo_x, x); lo_y = fminf(lo_y, y); lo_z = fminf(lo_z, d);
      hi_x = fmaxf(hi_x, x); hi_y = fmaxf(hi_y, y); hi_z = fmaxf(hi_z, d);
    }
  }
  sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
  const long long all = wave_sum((long long)m);
  lo_x = wave_min(lo_x); lo_y = wave_min(lo_y); lo_z = wave_min(lo_z);
  hi_x = wave_max(hi_x); hi_y = wave_max(hi_y); hi_z = wave_max(hi_z);
  if (lane == 0) {
    long long* p = partials + (s * strips + u) * kPartialWords;
    p[0] = sx; p[1] = sy; p[2] = sz; p[3] = all;
    p[4] = two_floats(lo_x, lo_y); p[5] = two_floats(lo_z, hi_x); p[6] = two_floats(hi_y, hi_z); p[7] = 0;
  }
}

// grid (slots / 4), 256 threads: wave wv of block b finishes slot 4 b + wv
__global__ __launch_bounds__(256) void hand_object_finish(const int* __restrict__ records, const long long* __restrict__ partials,
                                                          int slots, int strips, int min_points, int* __restrict__ out_count,
                                                          float* __restrict__ out_xyz, float* __restrict__ out_extent) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const size_t s = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= (size_t)slots) return;                                         // (a whole wave)
  long long sx = 0, sy = 0, sz = 0, m = 0;
  const float inf = __builtin_huge_valf();
  float lo_x = inf, lo_y = inf, lo_z = inf, hi_x = -inf, hi_y = -inf, hi_z = -inf;
  for (int u = lane; u < strips; u += 64) {                               // (index order per lane; integers, minima and maxima)
    const long long* p = partials + (s * strips + u) * kPartialWords;
    sx += p[0]; sy += p[1]; sz += p[2]; m += p[3];
    lo_x = fminf(lo_x, low_float(p[4])); lo_y = fminf(lo_y, high_float(p[4])); lo_z = fminf(lo_z, low_float(p[5]));
    hi_x = fmaxf(hi_x, high_float(p[5])); hi_y = fmaxf(hi_y, low_float(p[6])); hi_z = fmaxf(hi_z, high_float(p[6]));
  }
  sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); m = wave_sum(m);
  lo_x = wave_min(lo_x); lo_y = wave_min(lo_y); lo_z = wave_min(lo_z);
  hi_x = wave_max(hi_x); hi_y = wave_max(hi_y); hi_z = wave_max(hi_z);
  if (lane != 0) return;
  int status = records[s * kRecordWords + 4];
  if (status == 0 && m < (long long)min_points) status = 2;
  out_count[2 * s] = (int)m;
  out_count[2 * s + 1] = status;
  const double scale = (double)m * 1e6;
  out_xyz[3 * s + 0] = status == 0 ? (float)((double)sx / scale) : 0.f;
  out_xyz[3 * s + 1] = status == 0 ? (float)((double)sy / scale) : 0.f;
  out_xyz[3 * s + 2] = status == 0 ? (float)((double)sz / scale) : 0.f;
  const bool any = m > 0;
  float* e = out_extent + 6 * s;
  e[0] = any ? lo_x : 0.f; e[1] = any ? lo_y : 0.f; e[2] = any ? lo_z : 0.f;
  e[3] = any ? hi_x : 0.f; e[4] = any ? hi_y : 0.f; e[5] = any ? hi_z : 0.f;
}

// ------------------------------------------------------------------------------------------------------------- the label image
constexpr long long kBoxLimit = 1 << 20;        // corners and centres saturate here, as label_draw.hip's slot_box

// rint, saturated; NaN: 0
__device__ __forceinline__ long long pixel_of(float v) {
  if (v != v) return 0;
  return (long long)fminf(fmaxf(rintf(v), (float)-kBoxLimit), (float)kBoxLimit);
}

// tests/draw_ref.py line_points in closed form, from (x0, y0) to (x1, y1)
__device__ __forceinline__ bool on_line(long long x0, long long y0, long long x1, long long y1, long long px, long long py) {
  const long long ex = px - x0, ey = py - y0;
  const long long dx = x1 >= x0 ? x1 - x0 : x0 - x1, dy = y1 >= y0 ? y1 - y0 : y0 - y1;
  const long long sx = x1 >= x0 ? 1 : -1, sy = y1 >= y0 ? 1 : -1;
  const bool xmajor = dx >= dy;
  const long long major = xmajor ? dx : dy, minor = xmajor ? dy : dx;
  if (major == 0) return ex == 0 && ey == 0;
  const long long i = xmajor ? ex * sx : ey * sy, t = xmajor ? ey * sy : ex * sx;
  const long long num = 2 * minor * i + major - 1;                        // (all below 2^44)
  return i >= 0 && i <= major && 2 * major * t <= num && num < 2 * major * (t + 1);
}

// grid (pixels / 256, frames): a thread owns one pixel of box_label and rewrites it only where a primitive covers it
__global__ __launch_bounds__(256) void object_label_kernel(const float* __restrict__ boxes, const int* __restrict__ det_index,
                                                           const int* __restrict__ object_index, int cap, int k, int h, int w,
                                                           unsigned char* __restrict__ image) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;                           // (h, w <= 16384: at most 2^28)
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  bool hit = false;
  for (int kk = 0; kk < k; ++kk) {                                        // wave-uniform: scalar loads
    const size_t s = (size_t)n * k + kk;
    const int o = object_index[s], j = det_index[s];
    if (o < 0 || o >= cap || j < 0 || j >= cap) continue;
    const float* ob = boxes + ((size_t)n * cap + o) * 4;
    const float* hb = boxes + ((size_t)n * cap + j) * 4;
    const long long x1 = pixel_of(ob[0]), y1 = pixel_of(ob[1]), x2 = pixel_of(ob[2]), y2 = pixel_of(ob[3]);
    hit |= (((x == x1) | (x == x2)) & (y >= y1) & (y <= y2)) | (((y == y1) | (y == y2)) & (x >= x1) & (x <= x2));
    hit |= on_line(pixel_of(centre(hb[0], hb[2])), pixel_of(centre(hb[1], hb[3])), pixel_of(centre(ob[0], ob[2])),
                   pixel_of(centre(ob[1], ob[3])), x, y);
  }
  if (hit) {
    unsigned char* dst = image + ((size_t)n * h * w + p) * 3;
    dst[0] = 0; dst[1] = 0; dst[2] = 255;                                 // (0, 0, 255): one colour, so the draw order is no matter
  }
}

}  // namespace

extern "C" int64_t hn_hand_objects_scratch_bytes(int n, int k, int h) {
  if (n <= 0 || k <= 0 || k > kMaxSlots || h <= 0 || h > 16384) return 0;
  return (int64_t)(partial_entries(n, k, h) * kPartialWords * sizeof(long long) + (size_t)n * k * kRecordWords * sizeof(int));
}

extern "C" int hn_hand_objects_f32(const float* det_boxes, const float* det_scores, const int32_t* det_labels, const int32_t* det_count,
                                   const int32_t* contacts, const float* dxdymags, const int32_t* det_index, int cap, int object_label,
                                   const float* scene_depth, int64_t depth_frame_stride, const uint8_t* silhouette, const float* xyz_mm,
                                   int joints, const float* paras, const float* cams, int n, int k, int h, int w, int stride, float band,
                                   int min_points, void* scratch, int64_t scratch_bytes, int32_t* out_contact, int32_t* out_index,
                                   float* out_box, float* out_score, float* out_point, float* out_xyz, float* out_extent,
                                   int32_t* out_count, void* stream) {
  const char* fn = "hn_hand_objects_f32";
  HN_CHECK_ARG(det_boxes && det_scores && det_labels && det_count && contacts && dxdymags && det_index && scene_depth && xyz_mm && scratch &&
                   out_contact && out_index && out_box && out_score && out_point && out_xyz && out_extent && out_count,
               "%s: null pointer", fn);
  if (int st = check_one_camera(fn, paras, cams)) return st;
  if (int st = check_cams_aligned(fn, cams)) return st;
  if (int st = check_frames(fn, n, k, h, w)) return st;
  if (int st = check_depth_stride(fn, depth_frame_stride, h, w)) return st;
  HN_CHECK_ARG(cap >= 1 && cap <= (1 << 24), "%s: cap = %d detection rows per frame (1..2^24)", fn, cap);
  HN_CHECK_ARG(joints >= 1 && joints <= 4096, "%s: joints = %d (1..4096)", fn, joints);
  if (int st = check_sampling(fn, stride, band)) return st;
  HN_CHECK_ARG(min_points >= 1, "%s: min_points = %d (at least 1)", fn, min_points);
  if (int st = check_buffer(fn, "scratch", scratch, scratch_bytes, hn_hand_objects_scratch_bytes(n, k, h), 8)) return st;
  HN_CHECK_ARG((((uintptr_t)out_contact | (uintptr_t)out_index | (uintptr_t)out_box | (uintptr_t)out_score | (uintptr_t)out_point |
                 (uintptr_t)out_xyz | (uintptr_t)out_extent | (uintptr_t)out_count) & 3) == 0,
               "%s: the outputs must be aligned to 4 bytes", fn);
  long long* partials = static_cast<long long*>(scratch);
  int* records = reinterpret_cast<int*>(partials + partial_entries(n, k, h) * kPartialWords);
  hipStream_t st = (hipStream_t)stream;
  const AssocIn a = {det_boxes, det_scores, det_labels, det_count, contacts, dxdymags, det_index, cap, k, object_label, h, w};
  hipLaunchKernelGGL(hand_object_associate, dim3(n), dim3(256), 0, st, a, out_index, out_box, out_score, out_point, out_contact, records);
  HN_CHECK_LAUNCH("hand_object_associate");
  WalkIn in = {scene_depth, (long long)depth_frame_stride, silhouette, xyz_mm, out_box, cams, 0.f, 0.f, 0.f, 0.f, k, h, w,
               std::min(stride, 16384), joints, band};      // (h, w <= 16384: every larger stride leaves the pixel (0, 0) alone, as this one)
  if (paras) { in.fx = paras[0]; in.fy = paras[1]; in.cx = paras[2]; in.cy = paras[3]; }
  const int strips = strips_padded(h);
  hipLaunchKernelGGL(hand_object_walk, dim3(strips / 4, k, n), dim3(256), 0, st, in, records, partials);
  HN_CHECK_LAUNCH("hand_object_walk");
  const int slots = n * k;
  hipLaunchKernelGGL(hand_object_finish, dim3((slots + 3) / 4), dim3(256), 0, st, records, partials, slots, strips, min_points, out_count,
                     out_xyz, out_extent);
  HN_CHECK_LAUNCH("hand_object_finish");
  return HN_OK;
}

extern "C" int hn_draw_object_labels_u8(const float* det_boxes, const int32_t* det_index, const int32_t* object_index, int cap, int n,
                                        int k, int h, int w, uint8_t* box_label, void* stream) {
  const char* fn = "hn_draw_object_labels_u8";
  HN_CHECK_ARG(det_boxes && det_index && object_index && box_label, "%s: null pointer", fn);
  if (int st = check_frames(fn, n, k, h, w)) return st;
  HN_CHECK_ARG(cap >= 1 && cap <= (1 << 24), "%s: cap = %d detection rows per frame (1..2^24)", fn, cap);
  const long long hw = (long long)h * w;
  hipLaunchKernelGGL(object_label_kernel, dim3((unsigned)hn::cdiv(hw, 256), n), dim3(256), 0, (hipStream_t)stream, det_boxes, det_index,
                     object_index, cap, k, h, w, box_label);
  HN_CHECK_LAUNCH("object_label_kernel");
  return HN_OK;
}
