// The live loop's two other images (ros_demo.py:310-326), as two launches behind the step:
//
//   label_box_kernel   box_label: the camera frame as uint8 RGB with the crop rectangle of every drawn slot of the frame in
//                      (0,255,0) (cv2.rectangle, thickness 1).  A lane owns four consecutive pixels of one frame: it loads them
//                      (three float4 or three dwords when the rows allow it), tests them against the frame's K rectangles -- the
//                      loop over the boxes is wave-uniform, the boxes come through scalar loads -- and writes the twelve bytes as
//                      three dwords in one store.
//   label_pose_kernel  pose_label: the slot's colour crop resized to 176 x 176 (OpenCV's 8-bit bilinear in fixed point) with the
//                      predicted skeleton over it (VisualUtil('dexycb').plot, utils/vistool.py:23-47).  A workgroup owns 256
//                      consecutive four-pixel groups of one slot's image.  It builds the slot's 41 primitives (21 discs, 20
//                      segments, with their colours) in LDS once, in REVERSE draw order; a lane computes its four resize samples
//                      and searches the primitives: the first hit is the colour the reference's last draw would have left.
//
// Both are gathers: a pixel is written once, by the lane that owns it; nothing is drawn "on top" in memory.  No atomics, no
// allocation, no synchronisation: the images are a pure function of the arguments.  The rule is stated in DESIGN.md section 9c
// and restated in numpy by tests/draw_ref.py; integer arithmetic throughout, except the resize's sample positions (double ->
// float32, one rounding per operation: the file is built with -ffp-contract=off).
#include "hn_common.h"

namespace {

constexpr int kCrop = 176;                      // the pose image's side
constexpr int kJoints = 21;
constexpr int kPrims = 41;                      // 21 discs + 20 segments
constexpr int kGroupsPerRow = kCrop / 4;        // a lane's unit: four pixels = twelve bytes
constexpr int kGroups = kGroupsPerRow * kCrop;
constexpr int kPoseBytes = kCrop * kCrop * 3;
constexpr int kCoordLimit = 8191;               // joint pixels saturate here: the line arithmetic stays inside int32
constexpr long long kBoxLimit = 1 << 20;        // box corners saturate here (frames are at most 16384 wide: nothing visible changes)

struct DrawBox {
  int x1, y1, x2, y2;        // the rectangle's corners (after the caller's clamps, when asked for)
  int cx1, cy1, sw, sh;      // the crop frame[cy1 : cy1 + sh, cx1 : cx1 + sw]
  bool drawn;
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (uniform over the wave wherever `slot` is: the loads are scalar loads)
__device__ __forceinline__ DrawBox slot_box(const long long* __restrict__ box, const int* __restrict__ drawn, int slot, int h, int w,
                                            int clamp) {
  long long x1 = clampll(box[4 * slot + 0], -kBoxLimit, kBoxLimit), y1 = clampll(box[4 * slot + 1], -kBoxLimit, kBoxLimit);
  long long x2 = clampll(box[4 * slot + 2], -kBoxLimit, kBoxLimit), y2 = clampll(box[4 * slot + 3], -kBoxLimit, kBoxLimit);
  if (clamp) {               // ros_demo.py:280-281 as written there: the first two to [0, H], the last two to [0, W]
    x1 = clampll(x1, 0, h); y1 = clampll(y1, 0, h);
    x2 = clampll(x2, 0, w); y2 = clampll(y2, 0, w);
  }
  DrawBox b;
  b.x1 = (int)x1; b.y1 = (int)y1; b.x2 = (int)x2; b.y2 = (int)y2;
  b.cx1 = min(max(b.x1, 0), w);
  b.cy1 = min(max(b.y1, 0), h);
  b.sw = min(max(b.x2, 0), w) - b.cx1;
  b.sh = min(max(b.y2, 0), h) - b.cy1;
  b.drawn = (!drawn || drawn[slot] == 1) && b.sw > 0 && b.sh > 0;
  return b;
}

__device__ __forceinline__ unsigned quant(float x) {       // rint(255 x) to 0..255 (fmaxf(NaN, 0) is 0)
  return (unsigned)fminf(fmaxf(rintf(255.f * x), 0.f), 255.f);
}

// pixel (row, col) of frame n as r | g << 8 | b << 16; the caller keeps (row, col) inside the frame
template <int FMT>
__device__ __forceinline__ unsigned frame_rgb(const void* __restrict__ frame, int n, int h, int w, int row, int col) {
  const size_t hw = (size_t)h * w, pix = (size_t)row * w + col;
  if (FMT == HN_FRAME_F32_CHW) {
    const float* src = static_cast<const float*>(frame) + (size_t)n * 3 * hw + pix;
    return quant(src[0]) | quant(src[hw]) << 8 | quant(src[2 * hw]) << 16;
  }
  const unsigned char* src = static_cast<const unsigned char*>(frame) + ((size_t)n * hw + pix) * 3;
  return (unsigned)src[2] | (unsigned)src[1] << 8 | (unsigned)src[0] << 16;     // bgr8 -> RGB
}

struct __attribute__((aligned(4))) Dwords3 { unsigned a, b, c; };

// four RGB pixels -> twelve bytes at dst: three dwords in one store, or byte by byte
__device__ __forceinline__ void store_pixels(unsigned char* __restrict__ dst, const unsigned (&rgb)[4], int count, bool packed) {
  if (packed && count == 4) {
    Dwords3 d;
    d.a = (rgb[0] & 0xffffffu) | rgb[1] << 24;
    d.b = ((rgb[1] >> 8) & 0xffffu) | rgb[2] << 16;
    d.c = ((rgb[2] >> 16) & 0xffu) | rgb[3] << 8;
    *reinterpret_cast<Dwords3*>(dst) = d;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < count) {
      dst[3 * e + 0] = (unsigned char)(rgb[e] & 255u);
      dst[3 * e + 1] = (unsigned char)((rgb[e] >> 8) & 255u);
      dst[3 * e + 2] = (unsigned char)((rgb[e] >> 16) & 255u);
    }
  }
}

// FAST: w % 4 == 0 and the frame's address allows 16-byte (fp32) / 4-byte (bgr8) loads: a lane's four pixels share a row
template <int FMT, bool FAST>
__global__ __launch_bounds__(256) void label_box_kernel(const long long* __restrict__ box, const int* __restrict__ drawn, int k,
                                                        const void* __restrict__ frame, int h, int w, int clamp,
                                                        unsigned char* __restrict__ out, int packed) {
  const int n = blockIdx.y;
  const int hw = h * w;                                   // (h, w <= 16384: at most 2^28)
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;    // the lane's first pixel of frame n, row-major
  if (p0 >= hw) return;
  const int count = min(4, hw - p0);
  int row[4], col[4];
  row[0] = p0 / w;
  col[0] = p0 - row[0] * w;
#pragma unroll
  for (int e = 1; e < 4; ++e) {
    const bool wrap = col[e - 1] + 1 == w;
    col[e] = wrap ? 0 : col[e - 1] + 1;
    row[e] = row[e - 1] + (wrap ? 1 : 0);
  }
  unsigned rgb[4] = {0, 0, 0, 0};
  if (FAST) {
    if (FMT == HN_FRAME_F32_CHW) {
      const float* src = static_cast<const float*>(frame) + (size_t)n * 3 * hw + p0;
      const float4 r = *reinterpret_cast<const float4*>(src), g = *reinterpret_cast<const float4*>(src + hw),
                   b = *reinterpret_cast<const float4*>(src + 2 * (size_t)hw);
      rgb[0] = quant(r.x) | quant(g.x) << 8 | quant(b.x) << 16;
      rgb[1] = quant(r.y) | quant(g.y) << 8 | quant(b.y) << 16;
      rgb[2] = quant(r.z) | quant(g.z) << 8 | quant(b.z) << 16;
      rgb[3] = quant(r.w) | quant(g.w) << 8 | quant(b.w) << 16;
    } else {
      const Dwords3 d = *reinterpret_cast<const Dwords3*>(static_cast<const unsigned char*>(frame) + ((size_t)n * hw + p0) * 3);
      // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
      rgb[0] = ((d.a >> 16) & 255u) | (d.a & 0xff00u) | (d.a & 255u) << 16;
      rgb[1] = ((d.b >> 8) & 255u) | (d.b & 255u) << 8 | (d.a >> 24) << 16;
      rgb[2] = (d.c & 255u) | (d.b >> 24) << 8 | ((d.b >> 16) & 255u) << 16;
      rgb[3] = (d.c >> 24) | ((d.c >> 16) & 255u) << 8 | ((d.c >> 8) & 255u) << 16;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < count) rgb[e] = frame_rgb<FMT>(frame, n, h, w, row[e], col[e]);
  }
  for (int kk = 0; kk < k; ++kk) {                        // wave-uniform: the boxes do not depend on the lane
    const DrawBox b = slot_box(box, drawn, n * k + kk, h, w, clamp);
    if (!b.drawn) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = col[e], y = row[e];
      // (bitwise on purpose: four selects, no branches)
      const bool on = (((x == b.x1) | (x == b.x2)) & (y >= b.y1) & (y <= b.y2)) | (((y == b.y1) | (y == b.y2)) & (x >= b.x1) & (x <= b.x2));
      rgb[e] = on ? 0x00ff00u : rgb[e];                   // (0, 255, 0)
    }
  }
  store_pixels(out + ((size_t)n * hw + p0) * 3, rgb, count, packed != 0);
}

struct Prim {
  int line;                  // 0: disc around (x0, y0); 1: segment from (x0, y0)
  int x0, y0;
  int dx, dy, sx, sy;        // segment: |x1 - x0|, |y1 - y0| and the two step signs
  unsigned rgb;
};

// the joint's pixel (int(u), int(v)): truncation toward zero (vistool.py:40)
__device__ __forceinline__ int joint_pixel(float v, int clamp) {
  if (v != v) return 0;
  if (clamp) v = fminf(fmaxf(v, 0.f), (float)kCrop);
  return (int)fminf(fmaxf(v, (float)-kCoordLimit), (float)kCoordLimit);
}

__device__ __forceinline__ bool prim_hit(const Prim& p, int px, int py) {
  const int ex = px - p.x0, ey = py - p.y0;
  if (!p.line) return ex * ex + ey * ey <= 4;
  // 8-connected Bresenham from (x0, y0): step i along the major axis, minor = floor((2 minor i + major - 1) / (2 major))
  const bool xmajor = p.dx >= p.dy;
  const int major = xmajor ? p.dx : p.dy, minor = xmajor ? p.dy : p.dx;
  const int i = xmajor ? ex * p.sx : ey * p.sy;           // steps along the major axis
  const int t = xmajor ? ey * p.sy : ex * p.sx;           // steps along the minor axis
  if (major == 0) return ex == 0 && ey == 0;
  const int num = 2 * minor * i + major - 1;
  return i >= 0 && i <= major && 2 * major * t <= num && num < 2 * major * (t + 1);
}

// one axis of cv2.resize's INTER_LINEAR table for output index j of 176 from s source pixels: taps i0, i1, weights w0 + w1 = 2048
__device__ __forceinline__ void resize_tap(int j, int s, int& i0, int& i1, int& w0, int& w1) {
#pragma clang fp contract(off)
  const double scale = 1.0 / (176.0 / (double)s);
  float f = (float)(((double)j + 0.5) * scale - 0.5);
  int i = (int)floorf(f);
  f = f - (float)i;
  if (i < 0) { i = 0; f = 0.f; }
  i1 = i + 1;
  if (i >= s - 1) { i = s - 1; i1 = i; f = 0.f; }
  i0 = i;
  w1 = (int)rintf(f * 2048.f);
  w0 = (int)rintf((1.f - f) * 2048.f);
}

template <int FMT>
__global__ __launch_bounds__(256) void label_pose_kernel(const float* __restrict__ kp, const long long* __restrict__ box,
                                                         const int* __restrict__ drawn, int k, const void* __restrict__ frame, int h,
                                                         int w, int clamp, unsigned char* __restrict__ out, int packed) {
  __shared__ Prim prims[kPrims];
  const int slot = blockIdx.y, n = slot / k;
  const int g = blockIdx.x * 256 + threadIdx.x;           // the lane's four-pixel group of the slot's image
  const DrawBox b = slot_box(box, drawn, slot, h, w, clamp);        // (uniform over the workgroup)
  unsigned char* dst = out + (size_t)slot * kPoseBytes + (size_t)g * 12;
  unsigned rgb[4] = {0, 0, 0, 0};
  if (!b.drawn) {                                         // the reference's empty_label
    if (g < kGroups) store_pixels(dst, rgb, 4, packed != 0);
    return;
  }
  if (threadIdx.x < kPrims) {
    // reverse draw order: finger 4's segments (last first), its discs (last first), then finger 3 ... finger 0
    const int r = threadIdx.x;
    const int f = r < 9 ? 4 : 3 - (r - 9) / 8, q = r < 9 ? r : (r - 9) % 8;
    const int a = 4 * f + 1;
    int j0, j1 = -1;
    if (q < 4) {                                          // segment l: (0, a), (a, a + 1), (a + 1, a + 2), (a + 2, a + 3)
      const int l = 3 - q;
      j0 = l == 0 ? 0 : a + l - 1;
      j1 = a + l;
    } else {                                              // disc d of [a .. a + 3] (finger 4: and joint 0 last)
      const int d = (f == 4 ? 8 : 7) - q;
      j0 = d == 4 ? 0 : a + d;
    }
    const float* p0 = kp + ((size_t)slot * kJoints + j0) * 3;
    Prim p;
    p.line = j1 >= 0;
    p.x0 = joint_pixel(p0[0], clamp);
    p.y0 = joint_pixel(p0[1], clamp);
    p.dx = p.dy = p.sx = p.sy = 0;
    if (j1 >= 0) {
      const float* p1 = kp + ((size_t)slot * kJoints + j1) * 3;
      const int ex = joint_pixel(p1[0], clamp) - p.x0, ey = joint_pixel(p1[1], clamp) - p.y0;
      p.dx = abs(ex); p.dy = abs(ey);
      p.sx = ex < 0 ? -1 : 1; p.sy = ey < 0 ? -1 : 1;
    }
    // the reference's "BGR" tuples land on an RGB image: channel 0 gets the first value
    const unsigned c0 = f == 0 ? 102u : (f == 1 ? 179u : 255u), c12 = f == 3 ? 77u : (f == 4 ? 153u : 0u);
    p.rgb = c0 | c12 << 8 | c12 << 16;
    prims[r] = p;
  }
  __syncthreads();
  if (g >= kGroups) return;
  const int oy = g / kGroupsPerRow, ox0 = (g - oy * kGroupsPerRow) * 4;
  int iy0, iy1, b0, b1;
  resize_tap(oy, b.sh, iy0, iy1, b0, b1);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ox = ox0 + e;
    int ix0, ix1, a0, a1;
    resize_tap(ox, b.sw, ix0, ix1, a0, a1);
    // (taps are inside the crop, the crop is inside the frame)
    const unsigned s00 = frame_rgb<FMT>(frame, n, h, w, b.cy1 + iy0, b.cx1 + ix0), s01 = frame_rgb<FMT>(frame, n, h, w, b.cy1 + iy0, b.cx1 + ix1);
    const unsigned s10 = frame_rgb<FMT>(frame, n, h, w, b.cy1 + iy1, b.cx1 + ix0), s11 = frame_rgb<FMT>(frame, n, h, w, b.cy1 + iy1, b.cx1 + ix1);
    unsigned c = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int sh = 8 * ch;
      const int h0 = (int)((s00 >> sh) & 255u) * a0 + (int)((s01 >> sh) & 255u) * a1;
      const int h1 = (int)((s10 >> sh) & 255u) * a0 + (int)((s11 >> sh) & 255u) * a1;
      const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
      c |= (unsigned)v << sh;
    }
    for (int p = 0; p < kPrims; ++p) {
      if (prim_hit(prims[p], ox, oy)) {
        c = prims[p].rgb;
        break;
      }
    }
    rgb[e] = c;
  }
  store_pixels(dst, rgb, 4, packed != 0);
}

}  // namespace

extern "C" int hn_draw_labels_u8(const float* keypoints, const int64_t* crop_box, const int32_t* drawn, int s, int k, const void* frame,
                                 int frame_format, int h, int w, int clamp, uint8_t* out_box, uint8_t* out_pose, void* stream) {
  HN_CHECK_ARG(keypoints, "hn_draw_labels_u8: keypoints is NULL");
  HN_CHECK_ARG(crop_box, "hn_draw_labels_u8: crop_box is NULL");
  HN_CHECK_ARG(frame, "hn_draw_labels_u8: frame is NULL");
  HN_CHECK_ARG(out_box || out_pose, "hn_draw_labels_u8: out_box and out_pose are both NULL");
  HN_CHECK_ARG(k >= 1, "hn_draw_labels_u8: k = %d slots per frame (at least 1)", k);
  HN_CHECK_ARG(s > 0 && s % k == 0, "hn_draw_labels_u8: %d slots are not a positive multiple of k = %d slots per frame", s, k);
  HN_CHECK_ARG(h > 0 && w > 0 && h <= 16384 && w <= 16384, "hn_draw_labels_u8: bad frame size %d x %d (1..16384)", h, w);
  HN_CHECK_ARG(s / k <= 65535 && s <= 65535, "hn_draw_labels_u8: more than 65535 slots");
  HN_CHECK_ARG(frame_format == HN_FRAME_F32_CHW || frame_format == HN_FRAME_U8_BGR_HWC, "hn_draw_labels_u8: unknown frame format %d",
               frame_format);
  hipStream_t st = (hipStream_t)stream;
  const int n = s / k;
  const long long hw = (long long)h * w;
  const long long* box = reinterpret_cast<const long long*>(crop_box);
  const bool f32 = frame_format == HN_FRAME_F32_CHW;
  if (out_box) {
    // dword stores need every frame's first byte on a dword; else the same pixels leave byte by byte
    const int packed = ((uintptr_t)out_box & 3) == 0 && (n == 1 || (hw * 3) % 4 == 0);
    const bool fast = w % 4 == 0 && ((uintptr_t)frame & (f32 ? 15 : 3)) == 0;
    const dim3 grid(hn::cdiv(hn::cdiv(hw, 4), 256), n);
#define HN_LAUNCH_BOX(FMT, FAST) \
  hipLaunchKernelGGL((label_box_kernel<FMT, FAST>), grid, dim3(256), 0, st, box, drawn, k, frame, h, w, clamp, out_box, packed)
    if (f32 && fast) HN_LAUNCH_BOX(HN_FRAME_F32_CHW, true);
    else if (f32) HN_LAUNCH_BOX(HN_FRAME_F32_CHW, false);
    else if (fast) HN_LAUNCH_BOX(HN_FRAME_U8_BGR_HWC, true);
    else HN_LAUNCH_BOX(HN_FRAME_U8_BGR_HWC, false);
#undef HN_LAUNCH_BOX
    HN_CHECK_LAUNCH("label_box_kernel");
  }
  if (out_pose) {
    const int packed = ((uintptr_t)out_pose & 3) == 0;       // (a slot's image is 92928 bytes, a group 12)
    const dim3 grid(hn::cdiv(kGroups, 256), s);
    if (f32)
      hipLaunchKernelGGL(label_pose_kernel<HN_FRAME_F32_CHW>, grid, dim3(256), 0, st, keypoints, box, drawn, k, frame, h, w, clamp,
                         out_pose, packed);
    else
      hipLaunchKernelGGL(label_pose_kernel<HN_FRAME_U8_BGR_HWC>, grid, dim3(256), 0, st, keypoints, box, drawn, k, frame, h, w, clamp,
                         out_pose, packed);
    HN_CHECK_LAUNCH("label_pose_kernel");
  }
  return HN_OK;
}
