// What the passes over a frame's depth share (mesh_raster.hip, hand_cloud.hip, mesh_fit.hip, mesh_refit.hip): the strip
// geometry, the slots-per-frame limit, the camera fetch, the back-projection and the valid-depth test on the device; the entries'
// common argument checks on the host.  Header-only: every helper is compiled with the flags of the file that includes it
// (hn_amd/build.py EXTRA_FLAGS: all four with -ffp-contract=off), and the __f*_rn operations are rounded one by one anyway.
#pragma once
#include <cmath>

#include "hn_common.h"

namespace hn {

constexpr int kMaxSlots = 16;       // slots per frame: what the silhouette's byte (0x80 | slot + 1) and a lane per slot hold
constexpr int kMaxStrips = 1024;    // of a frame: a sum over a strip table stays at most 64 (cloud) / 128 (fit) loads per thread

// A STRIP is the unit of work of the cloud and the fit: consecutive rows walked by ONE wave, 64 candidates at a time.
// rows per strip, a function of the frame's height alone (the *_scratch_bytes entries know nothing else)
__host__ __device__ inline int strip_rows(int h) { return max(2, (h + kMaxStrips - 1) / kMaxStrips); }
// strips per frame, padded to whole workgroups of four
__host__ __device__ inline int strips_padded(int h) { return ((h + strip_rows(h) - 1) / strip_rows(h) + 3) / 4 * 4; }

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Cam {
  float fx, fy, cx, cy;
};

// frame i's camera: row i of the device table [frames][4], or -- cams null -- the four values
__device__ __forceinline__ Cam camera(const float* cams, int i, float fx, float fy, float cx, float cy) {
  Cam cam = {fx, fy, cx, cy};
  if (cams) {                                                             // (the row's address is uniform: four scalar loads)
    const float* row = cams + 4 * (size_t)i;
    cam.fx = row[0]; cam.fy = row[1]; cam.cx = row[2]; cam.cy = row[3];
  }
  return cam;
}

// P(r, c, z), x and y: (((float)c + 0.5) - cx) * z / fx -- subtract, multiply, divide, each rounded on its own
__device__ __forceinline__ float back_x(const Cam& cam, int c, float z) {
  return __fdiv_rn(__fmul_rn(__fsub_rn(__fadd_rn((float)c, 0.5f), cam.cx), z), cam.fx);
}
__device__ __forceinline__ float back_y(const Cam& cam, int r, float z) {
  return __fdiv_rn(__fmul_rn(__fsub_rn(__fadd_rn((float)r, 0.5f), cam.cy), z), cam.fy);
}

// a scene depth that measures something: a hole -- 0, NaN --, inf or a negative value does not
__device__ __forceinline__ bool valid_depth(float d) { return d > 0.f && d <= 3.402823466e38f; }

// The entries' argument checks.  HN_CHECK_ARG returns from the function it stands in, so each check is a function that hands
// the status back: `if (int st = check_...(fn, ...)) return st;`.  `fn` is the entry's name, which every message carries.
static inline int check_one_camera(const char* fn, const float* paras, const float* cams) {
  HN_CHECK_ARG((paras != nullptr) != (cams != nullptr), "%s: exactly one of paras (host) and cams (device) must be given", fn);
  return HN_OK;
}
static inline int check_cams_aligned(const char* fn, const float* cams) {
  HN_CHECK_ARG(!cams || ((uintptr_t)cams & 3) == 0, "%s: cams must be aligned to a float", fn);
  return HN_OK;
}
static inline int check_frame_size(const char* fn, int h, int w) {
  HN_CHECK_ARG(h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "%s: bad frame size %d x %d (1..16384)", fn, h, w);
  return HN_OK;
}
// the passes over [n][h][w] maps: frames, slots per frame, size
static inline int check_frames(const char* fn, int n, int k, int h, int w) {
  HN_CHECK_ARG(n >= 1 && n <= 65535, "%s: n = %d frames (1..65535)", fn, n);
  HN_CHECK_ARG(k >= 1 && k <= kMaxSlots, "%s: k = %d slots per frame (1..16)", fn, k);
  return check_frame_size(fn, h, w);
}
// the raster's entries, which count slots: s slots of v vertices and f faces, k to a frame
static inline int check_slots(const char* fn, int s, int v, int f, int k) {
  HN_CHECK_ARG(s > 0 && v > 0 && f > 0, "%s: bad dims (s %d, v %d, f %d: all must be positive)", fn, s, v, f);
  HN_CHECK_ARG(k > 0 && s % k == 0, "%s: %d slots are not a multiple of k = %d slots per frame", fn, s, k);
  return HN_OK;
}
// ... whose outputs name a slot in a byte (`byte`: which one, in the entry's words)
static inline int check_slot_byte(const char* fn, int k, const char* byte) {
  HN_CHECK_ARG(k <= kMaxSlots, "%s: k = %d slots per frame do not fit %s (1..16)", fn, k, byte);
  return HN_OK;
}
// ... and whose grid's z is the frame
static inline int check_raster_frames(const char* fn, int s, int k, int h, int w) {
  if (int st = check_frame_size(fn, h, w)) return st;
  HN_CHECK_ARG(s / k <= 65535, "%s: more than 65535 frames", fn);
  return HN_OK;
}
static inline int check_depth_stride(const char* fn, int64_t depth_frame_stride, int h, int w) {
  HN_CHECK_ARG(depth_frame_stride >= (int64_t)h * w, "%s: depth_frame_stride %lld is less than a frame of %d x %d", fn,
               (long long)depth_frame_stride, h, w);
  return HN_OK;
}
// which pixels are candidates, and which of them match
static inline int check_sampling(const char* fn, int stride, float band) {
  HN_CHECK_ARG(stride >= 1, "%s: stride = %d (at least 1)", fn, stride);
  HN_CHECK_ARG(band > 0.f && band <= 100.f, "%s: band must be finite and in (0, 100] metres (got %g)", fn, (double)band);
  return HN_OK;
}
// the fit's sizes (f: null for the entry that takes no faces) ...
static inline int check_fit_sizes(const char* fn, int v, const int* f, int joints) {
  HN_CHECK_ARG(v >= 1 && v <= (1 << 24), "%s: v = %d vertices (1..2^24)", fn, v);
  HN_CHECK_ARG(!f || *f >= 1, "%s: f = %d faces (at least 1)", fn, f ? *f : 0);
  HN_CHECK_ARG(joints >= 1 && joints <= 4096, "%s: joints = %d (1..4096)", fn, joints);
  return HN_OK;
}
// ... and its options
static inline int check_fit_options(const char* fn, int stride, float band, int min_points, double damp, double max_shift2,
                                    double tan2_half_angle) {
  if (int st = check_sampling(fn, stride, band)) return st;
  HN_CHECK_ARG(min_points >= 1, "%s: min_points = %d (at least 1)", fn, min_points);
  HN_CHECK_ARG(damp >= 0.0 && std::isfinite(damp), "%s: damp must be finite and >= 0 (got %g)", fn, damp);
  HN_CHECK_ARG(max_shift2 > 0.0 && std::isfinite(max_shift2), "%s: max_shift2 must be finite and > 0 (got %g)", fn, max_shift2);
  HN_CHECK_ARG(tan2_half_angle > 0.0 && std::isfinite(tan2_half_angle), "%s: tan2_half_angle must be finite and > 0 (got %g)", fn,
               tan2_half_angle);
  return HN_OK;
}
// a caller's buffer (`what`: "scratch", "work") of at least `need` bytes on `align` bytes
static inline int check_buffer(const char* fn, const char* what, const void* p, int64_t bytes, int64_t need, int align) {
  HN_CHECK_ARG(bytes >= need, "%s: %s of %lld bytes, %lld needed", fn, what, (long long)bytes, (long long)need);
  HN_CHECK_ARG(((uintptr_t)p & (uintptr_t)(align - 1)) == 0, "%s: %s must be %d-byte aligned", fn, what, align);
  return HN_OK;
}
// a face list the host still holds: every index names a vertex
static inline int check_faces_host(const char* fn, const int32_t* faces_host, int f, int v) {
  if (faces_host)
    for (int64_t i = 0; i < (int64_t)f * 3; ++i)
      HN_CHECK_ARG(faces_host[i] >= 0 && faces_host[i] < v, "%s: face %lld uses vertex %d of %d", fn, (long long)(i / 3),
                   faces_host[i], v);
  return HN_OK;
}

}  // namespace hn
