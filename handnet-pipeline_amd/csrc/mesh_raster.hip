// The live loop's last call, render(out, paras, h, w, full_image, face) of ros_demo.py:86-116,329-337, as two launches:
// the lifted meshes of all N*K hand slots rasterised over the camera frame, one depth buffer per frame.
//
//   mesh_raster_setup  one workgroup per slot, one thread per face (strided): projects the face's three vertices with the
//                      plain pinhole (fp32, one rounding per operation), snaps them to 1/256 pixel, and writes the face's
//                      record (snapped corners wound so that the doubled area is positive, the three Z, 1 / area, the flat
//                      8-bit colour) and its pixel bounding box; reduces the slot's pixel bounding box.
//   mesh_raster_tiles  one wave per 8x8 pixel tile, one pixel per lane.  The tile walks the K slots of its frame, skips a
//                      slot whose box misses it, tests 64 face boxes at a time (one per lane, one ballot) and evaluates
//                      only the faces whose box touches the tile: 64-bit integer edge functions with the top-left rule,
//                      fp32 barycentric depth, nearest Z kept in registers.  Each pixel is written once: the nearest
//                      face's colour, or the frame's own pixel.
//
// No atomics, no order dependence between workgroups: the image is a pure function of the inputs (slot-major, then face
// order decides an exact depth tie).  The rule itself is stated in DESIGN.md ("The overlay") and restated in numpy by
// tests/raster_ref.py.
//
// The occluded form (hn_mesh_render_occluded_u8; DESIGN.md "The overlay behind the scene", tests/occlude_ref.py) is the same
// two launches with a compile-time switch: the tile kernel also keeps the winner's slot, loads the camera's depth D on covered
// lanes only, hides the pixel where D is valid and best > D + margin, writes the silhouette byte, and adds two ballots'
// popcounts per slot that touched the tile to the slot's two counters, which the setup kernel's thread 0 zeroed.  The only
// atomics are those integer adds: sums of integers do not depend on their order, so the outputs stay a pure function of the
// inputs.  The instantiations without the switch take no further argument and hold no further instruction.
//
// The per-frame cameras (hn_mesh_render_cams_u8 / _cams_occluded_u8; DESIGN.md "A camera per frame", tests/cams_ref.py) are a
// second compile-time switch, of the setup kernel alone: slot s of a step with k slots per frame reads row s / k of a device
// table [frames][4] where the other instantiations read four scalar arguments.  The projection and the tile kernel are the same.
//
// The geometry pass (hn_mesh_geometry_f32; DESIGN.md section 9l, tests/refit_ref.py::geometry) is a third tile kernel behind the
// same setup launch: mesh_geometry_tiles makes the same walk (walk_tile: slots, box test, ballots, edge functions, Z) and keeps
// the nearest Z and its slot, and that is all it writes -- fp32 Z (0: nothing drawn) and the byte slot + 1 (0: nothing drawn) per pixel.  It
// reads no frame and no scene depth and stores no image: what the iterated fit needs to see its moved mesh again.
#include "depth_pass.h"

#include <type_traits>

namespace {

using namespace hn;                 // depth_pass.h: kMaxSlots, valid_depth, the entries' argument checks

constexpr int kSub = 256;           // sub-pixel grid: 1/256 pixel
constexpr int kHalf = 128;          // a pixel's sample point: (256 col + 128, 256 row + 128)
constexpr float kSnapLimit = 16777216.f;   // |snapped coordinate| < 2^24
constexpr float kNear = 0.05f, kFar = 100.f;

struct __attribute__((aligned(16))) FaceRec {
  int ax, ay, bx, by, cx, cy;       // snapped corners, wound so that (bx-ax)(cy-ay) - (cx-ax)(by-ay) > 0
  float za, zb, zc;                 // camera Z of the corners (metres, > 0 in front)
  float inv_area;                   // 1 / doubled area
  unsigned rgb;                     // r | g << 8 | b << 16
  int pad;
};
static_assert(sizeof(FaceRec) == 48, "face record");

struct Box { short x0, x1, y0, y1; };   // inclusive pixel range; x0 > x1: nothing to draw
static_assert(sizeof(Box) == 8, "face box");

struct SlotBox { int x0, x1, y0, y1; };

__host__ __device__ inline size_t rec_offset(int s) { return (size_t)s * sizeof(SlotBox); }
__host__ __device__ inline size_t box_offset(int s, int f) { return rec_offset(s) + (size_t)s * f * sizeof(FaceRec); }
__host__ __device__ inline size_t scratch_total(int s, int f) { return box_offset(s, f) + (size_t)s * f * sizeof(Box); }

// what the occluded form adds to both kernels' arguments
struct Occlusion {
  const float* depth;               // the camera's depth map, metres: frame i at depth + i * frame_stride, [h][w]
  long long frame_stride;           // in elements (h * w; 4 * h * w for channel 3 of an RGBD tensor)
  float margin;                     // metres
  unsigned char* silhouette;        // [n][h][w]: 0, slot + 1 (shown) or 0x80 | (slot + 1) (hidden)
  int* coverage;                    // [slots][2]: (pixels where the slot's mesh is the nearest, of those shown), or null
};

struct Snapped { int x, y; float z; bool ok; };

// (x, y, z) of out['mesh'] (OpenGL camera: y up, z towards the viewer) -> (X, Y, Z) = (x, -y, -z) -> u = (fx X) / Z + cx,
// v = (fy Y) / Z + cy -> rint(256 u), rint(256 v); every operation rounded on its own
__device__ __forceinline__ Snapped project(const float* __restrict__ p, float fx, float fy, float cx, float cy) {
#pragma clang fp contract(off)
  const float X = p[0], Y = -p[1], Z = -p[2];
  Snapped r;
  r.z = Z;
  r.ok = (fabsf(X) <= 3.402823466e38f) && (fabsf(Y) <= 3.402823466e38f) && (Z >= kNear) && (Z <= kFar);
  const float zs = r.ok ? Z : 1.f;
  const float u = __fadd_rn(__fdiv_rn(__fmul_rn(fx, X), zs), cx);
  const float v = __fadd_rn(__fdiv_rn(__fmul_rn(fy, Y), zs), cy);
  const float xs = rintf(__fmul_rn(u, (float)kSub)), ys = rintf(__fmul_rn(v, (float)kSub));
  r.ok = r.ok && (fabsf(xs) < kSnapLimit) && (fabsf(ys) < kSnapLimit);     // (false for NaN / inf as well)
  r.x = r.ok ? (int)xs : 0;
  r.y = r.ok ? (int)ys : 0;
  return r;
}

// shade = min(1, 0.3 + 2.4 l / pi), l = |n_z| / |n| of the face's camera-space normal; base colour (1, 1, 0.9)
__device__ __forceinline__ unsigned face_colour(const float* a, const float* b, const float* c) {
  const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  const float l = len > 0.f ? fabsf(nz) / len : 0.f;
  const float shade = fminf(1.f, 0.3f + 2.4f * l / 3.14159265358979323846f);
  const float base[3] = {1.f, 1.f, 0.9f};
  unsigned rgb = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float q = floorf(255.f * shade * base[ch] + 0.5f);
    rgb |= (unsigned)fminf(fmaxf(q, 0.f), 255.f) << (8 * ch);
  }
  return rgb;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// Where the setup kernel gets its intrinsics.  CAMS off: the four scalars fx, fy, cx, cy, by value, one camera for every slot.
// CAMS on -- the per-frame form (DESIGN.md "A camera per frame") --: the first two arguments are a table on the device, fp32
// [frames][4] with rows (fx, fy, cx, cy), and k, the slots per frame; slot s belongs to frame s / k and reads row s / k, and a
// captured graph reads the table anew at every replay.  (The scalars stay plain float arguments, not a struct: the
// instantiations without CAMS are then the kernels they were before the switch existed, instruction for instruction.)
template <bool CAMS> using CamA = std::conditional_t<CAMS, const float*, float>;   // the table, or fx
template <bool CAMS> using CamB = std::conditional_t<CAMS, int, float>;            // k, or fy

// Coverage: nothing, or -- the occluded form -- the slots' counters (int*), which thread 0 zeroes
template <bool CAMS, class... Coverage>
__global__ __launch_bounds__(256) void mesh_raster_setup(const float* __restrict__ mesh, const int* __restrict__ faces,
                                                         const int* __restrict__ lifted, int v, int f, CamA<CAMS> fx_or_cams,
                                                         CamB<CAMS> fy_or_k, float cx, float cy, int h, int w,
                                                         unsigned char* __restrict__ scratch, int slots, Coverage... coverage) {
  const int slot = blockIdx.x;
  if constexpr (sizeof...(Coverage) != 0) {
    int* counters = (coverage, ...);
    if (counters && threadIdx.x == 0) counters[2 * slot] = counters[2 * slot + 1] = 0;   // (the tiles launch adds to them)
  }
  SlotBox* slot_box = reinterpret_cast<SlotBox*>(scratch + (size_t)slot * sizeof(SlotBox));
  FaceRec* recs = reinterpret_cast<FaceRec*>(scratch + rec_offset(slots)) + (size_t)slot * f;
  Box* boxes = reinterpret_cast<Box*>(scratch + box_offset(slots, f)) + (size_t)slot * f;
  const bool drawn = !lifted || lifted[slot] != 0;        // (uniform over the workgroup)
  float fx, fy;
  if constexpr (CAMS) {             // (the row's address depends on blockIdx alone: uniform, four scalar loads; cx, cy unused)
    const float* __restrict__ row = fx_or_cams + 4 * (size_t)(slot / fy_or_k);
    fx = row[0]; fy = row[1]; cx = row[2]; cy = row[3];
  } else {
    fx = fx_or_cams; fy = fy_or_k;
  }
  int bx0 = w, bx1 = -1, by0 = h, by1 = -1;
  for (int i = threadIdx.x; i < f && drawn; i += blockDim.x) {
    const int i0 = faces[3 * i], i1 = faces[3 * i + 1], i2 = faces[3 * i + 2];
    Box box = {1, 0, 1, 0};
    FaceRec rec = {};
    if ((unsigned)i0 < (unsigned)v && (unsigned)i1 < (unsigned)v && (unsigned)i2 < (unsigned)v) {   // (a bad index draws nothing)
      const float* pa = mesh + ((size_t)slot * v + i0) * 3;
      const float* pb = mesh + ((size_t)slot * v + i1) * 3;
      const float* pc = mesh + ((size_t)slot * v + i2) * 3;
      const Snapped a = project(pa, fx, fy, cx, cy);
      Snapped b = project(pb, fx, fy, cx, cy), c = project(pc, fx, fy, cx, cy);
      const long long area = (long long)(b.x - a.x) * (c.y - a.y) - (long long)(c.x - a.x) * (b.y - a.y);
      if (a.ok && b.ok && c.ok && area != 0) {
        if (area < 0) { const Snapped t = b; b = c; c = t; }
        const int lo_x = min(a.x, min(b.x, c.x)), hi_x = max(a.x, max(b.x, c.x));
        const int lo_y = min(a.y, min(b.y, c.y)), hi_y = max(a.y, max(b.y, c.y));
        // pixels whose sample point 256 p + 128 lies in [lo, hi] (>> is an arithmetic shift: floor for negative values too)
        const int x0 = max((lo_x + kHalf - 1) >> 8, 0), x1 = min((hi_x - kHalf) >> 8, w - 1);
        const int y0 = max((lo_y + kHalf - 1) >> 8, 0), y1 = min((hi_y - kHalf) >> 8, h - 1);
        if (x0 <= x1 && y0 <= y1) {
          box = {(short)x0, (short)x1, (short)y0, (short)y1};
          rec.ax = a.x; rec.ay = a.y; rec.bx = b.x; rec.by = b.y; rec.cx = c.x; rec.cy = c.y;
          rec.za = a.z; rec.zb = b.z; rec.zc = c.z;
          rec.inv_area = 1.f / (float)(area < 0 ? -area : area);
          rec.rgb = face_colour(pa, pb, pc);
          bx0 = min(bx0, x0); bx1 = max(bx1, x1); by0 = min(by0, y0); by1 = max(by1, y1);
        }
      }
    }
    recs[i] = rec;
    boxes[i] = box;
  }
  __shared__ int part[4][4];
  bx0 = wave_min(bx0); bx1 = -wave_min(-bx1); by0 = wave_min(by0); by1 = -wave_min(-by1);
  if ((threadIdx.x & 63) == 0) {
    int* p = part[threadIdx.x >> 6];
    p[0] = bx0; p[1] = bx1; p[2] = by0; p[3] = by1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    SlotBox sb = {part[0][0], part[0][1], part[0][2], part[0][3]};
    for (int wv = 1; wv < 4; ++wv) {
      sb.x0 = min(sb.x0, part[wv][0]); sb.x1 = max(sb.x1, part[wv][1]);
      sb.y0 = min(sb.y0, part[wv][2]); sb.y1 = max(sb.y1, part[wv][3]);
    }
    *slot_box = sb;
  }
}

// edge a -> b of a face with positive doubled area (clockwise on the screen, y down): the inside is E > 0, and a sample
// exactly on the edge belongs to the face when the edge is a top edge (dy == 0, dx > 0) or a left edge (dy < 0)
__device__ __forceinline__ long long edge(int ax, int ay, int bx, int by, int px, int py, bool& in) {
  const int dx = bx - ax, dy = by - ay;
  const long long e = (long long)dx * (py - ay) - (long long)dy * (px - ax);
  const bool top_left = dy < 0 || (dy == 0 && dx > 0);
  in = in && (e > 0 || (e == 0 && top_left));
  return e;
}

// The walk of a tile kernel (one wave per 8 x 8 tile at (tx, ty) of frame n, one pixel per lane, sampled at (px, py)): the
// frame's k slots in order, a slot whose box misses the tile skipped, 64 face boxes tested at a time (one per lane, one
// ballot), and for every face whose box touches the tile the three edge functions and the barycentric Z.  on_slot(kk) is
// called once per slot that touches the tile (wave-uniform), on_hit(kk, z, rec) on the lanes whose sample the face covers, in
// slot-major, then ascending face order: a caller that keeps `z < best` gives an exact tie to the lower index.
template <class OnSlot, class OnHit>
__device__ __forceinline__ void walk_tile(const unsigned char* __restrict__ scratch, int slots, int f, int k, int n, int tx, int ty,
                                          int lane, int px, int py, bool inside_frame, OnSlot on_slot, OnHit on_hit) {
  const FaceRec* all_recs = reinterpret_cast<const FaceRec*>(scratch + rec_offset(slots));
  const Box* all_boxes = reinterpret_cast<const Box*>(scratch + box_offset(slots, f));
  for (int kk = 0; kk < k; ++kk) {
    const int slot = n * k + kk;
    const SlotBox sb = *reinterpret_cast<const SlotBox*>(scratch + (size_t)slot * sizeof(SlotBox));
    if (sb.x0 > tx + 7 || sb.x1 < tx || sb.y0 > ty + 7 || sb.y1 < ty) continue;      // (wave-uniform)
    on_slot(kk);
    const FaceRec* recs = all_recs + (size_t)slot * f;
    const Box* boxes = all_boxes + (size_t)slot * f;
    for (int base = 0; base < f; base += 64) {
      bool hit = false;
      if (base + lane < f) {
        const Box b = boxes[base + lane];
        hit = b.x0 <= tx + 7 && b.x1 >= tx && b.y0 <= ty + 7 && b.y1 >= ty;
      }
      unsigned long long todo = __ballot(hit);
      while (todo) {
        const int bit = __builtin_ctzll(todo);
        todo &= todo - 1;
        const FaceRec r = recs[__builtin_amdgcn_readfirstlane(base + bit)];
        bool in = inside_frame;
        const long long wa = edge(r.bx, r.by, r.cx, r.cy, px, py, in);      // weight of corner a
        const long long wb = edge(r.cx, r.cy, r.ax, r.ay, px, py, in);
        const long long wc = edge(r.ax, r.ay, r.bx, r.by, px, py, in);
        if (in) on_hit(kk, ((float)wa * r.za + (float)wb * r.zb + (float)wc * r.zc) * r.inv_area, r);
      }
    }
  }
}

// FMT: HN_FRAME_F32_CHW / HN_FRAME_U8_BGR_HWC; OCC: the occluded form, whose one further argument is an Occlusion
template <int FMT, bool OCC = false, class... Occ>
__global__ __launch_bounds__(256) void mesh_raster_tiles(const unsigned char* __restrict__ scratch, int slots, int f, int k,
                                                         const void* __restrict__ frame, int h, int w,
                                                         unsigned char* __restrict__ out, float* __restrict__ depth_out,
                                                         Occ... occ) {
  static_assert(sizeof...(Occ) == (OCC ? 1 : 0), "the occluded form takes one Occlusion");
  // a workgroup is 4 tiles side by side: 32 x 8 pixels
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tx = (blockIdx.x * 4 + wave) * 8, ty = blockIdx.y * 8, n = blockIdx.z;
  if (tx >= w) return;                                        // (wave-uniform)
  const int col = tx + (lane & 7), row = ty + (lane >> 3);
  const bool inside_frame = col < w && row < h;
  const int px = col * kSub + kHalf, py = row * kSub + kHalf;
  float best = 3.402823466e38f;
  unsigned rgb = 0;
  bool covered = false;
  int winner = 0;                                             // (OCC) slot within the frame of the nearest face
  unsigned touched = 0;                                       // (OCC) bit kk: slot kk's box meets the tile (wave-uniform)
  walk_tile(
      scratch, slots, f, k, n, tx, ty, lane, px, py, inside_frame, [&](int kk) { if (OCC) touched |= 1u << kk; },
      [&](int kk, float z, const FaceRec& r) {
        if (z < best) {
          best = z; rgb = r.rgb; covered = true;
          if (OCC) winner = kk;
        }
      });
  bool shown = covered;
  if constexpr (OCC) {
#pragma clang fp contract(off)
    const Occlusion o = (occ, ...);
    if (covered) {                                            // (covered lanes are inside the frame)
      const float d = o.depth[(size_t)n * o.frame_stride + (size_t)row * w + col];
      shown = !(valid_depth(d) && best > __fadd_rn(d, o.margin));   // (a depth that measures nothing hides nothing)
    }
    // all 64 lanes are here: two ballots per slot that touched the tile, lane 0 adds their popcounts
    while (touched) {
      const int kk = __builtin_ctz(touched);
      touched &= touched - 1;
      const unsigned long long mine = __ballot(covered && winner == kk);
      const unsigned long long seen = __ballot(covered && winner == kk && shown);
      if (o.coverage && lane == 0 && mine) {
        atomicAdd(o.coverage + 2 * (n * k + kk), __popcll(mine));
        if (seen) atomicAdd(o.coverage + 2 * (n * k + kk) + 1, __popcll(seen));
      }
    }
    if (inside_frame)
      o.silhouette[((size_t)n * h + row) * w + col] = covered ? (unsigned char)((shown ? 0 : 0x80) | (winner + 1)) : 0;
  }
  if (!inside_frame) return;
  const size_t pix = ((size_t)n * h + row) * w + col;
  if (!shown) {
    if (FMT == HN_FRAME_F32_CHW) {
      const float* src = static_cast<const float*>(frame) + (size_t)n * 3 * h * w + (size_t)row * w + col;
      rgb = 0;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float q = rintf(255.f * src[(size_t)ch * h * w]);
        rgb |= (unsigned)fminf(fmaxf(q, 0.f), 255.f) << (8 * ch);           // (fmaxf(NaN, 0) is 0)
      }
    } else {
      const unsigned char* src = static_cast<const unsigned char*>(frame) + pix * 3;
      rgb = (unsigned)src[2] | (unsigned)src[1] << 8 | (unsigned)src[0] << 16;   // bgr8 -> RGB
    }
  }
  unsigned char* dst = out + pix * 3;
  dst[0] = (unsigned char)(rgb & 255u);
  dst[1] = (unsigned char)((rgb >> 8) & 255u);
  dst[2] = (unsigned char)((rgb >> 16) & 255u);
  if (depth_out) depth_out[pix] = covered ? best : 0.f;
}

// The geometry pass: the walk of mesh_raster_tiles, the nearest Z and its slot, nothing else.  Every pixel of the frame is
// written on every call.
__global__ __launch_bounds__(256) void mesh_geometry_tiles(const unsigned char* __restrict__ scratch, int slots, int f, int k, int h,
                                                           int w, float* __restrict__ out_depth,
                                                           unsigned char* __restrict__ out_who) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tx = (blockIdx.x * 4 + wave) * 8, ty = blockIdx.y * 8, n = blockIdx.z;
  if (tx >= w) return;                                        // (wave-uniform)
  const int col = tx + (lane & 7), row = ty + (lane >> 3);
  const bool inside_frame = col < w && row < h;
  const int px = col * kSub + kHalf, py = row * kSub + kHalf;
  float best = 3.402823466e38f;
  int who = 0;                                                // 0, or the nearest face's slot within the frame + 1
  walk_tile(
      scratch, slots, f, k, n, tx, ty, lane, px, py, inside_frame, [](int) {},
      [&](int kk, float z, const FaceRec&) {
        const bool nearer = z < best;       // (two selects, as the kernel had them before the walk was shared: an `if` here
        best = nearer ? z : best;           // becomes an exec-masked branch inside the face loop)
        who = nearer ? kk + 1 : who;
      });
  if (!inside_frame) return;
  const size_t pix = ((size_t)n * h + row) * w + col;
  out_depth[pix] = who ? best : 0.f;
  out_who[pix] = (unsigned char)who;
}

}  // namespace

extern "C" int64_t hn_mesh_render_scratch_bytes(int s, int f) {
  if (s <= 0 || f <= 0) return 0;
  return (int64_t)scratch_total(s, f);
}

// the setup launch of every entry, one of four instantiations: a camera per frame (cams, device) or one (paras, host); no
// further argument, or -- the occluded form -- the slots' counters, which the kernel zeroes
template <class... Coverage>
static void launch_setup(const float* mesh, const int32_t* faces, const int32_t* lifted, int s, int v, int f, int k, const float* paras,
                         const float* cams, int h, int w, unsigned char* sc, hipStream_t st, Coverage... coverage) {
  if (cams)
    hipLaunchKernelGGL((mesh_raster_setup<true, Coverage...>), dim3(s), dim3(256), 0, st, mesh, faces, lifted, v, f, cams, k, 0.f, 0.f, h,
                       w, sc, s, coverage...);
  else
    hipLaunchKernelGGL((mesh_raster_setup<false, Coverage...>), dim3(s), dim3(256), 0, st, mesh, faces, lifted, v, f, paras[0], paras[1],
                       paras[2], paras[3], h, w, sc, s, coverage...);
}

// the argument checks every render entry shares (`fn`: the name the messages carry), then the two launches; exactly one of
// paras (host, one camera) and cams (device, a row per frame) is given
static int render(const char* fn, const float* mesh, const int32_t* faces, const int32_t* faces_host, const int32_t* lifted, int s,
                  int v, int f, int k, const float* paras, const float* cams, const void* frame, int frame_format, int h, int w,
                  void* scratch, int64_t scratch_bytes, uint8_t* out_image, float* out_depth, const Occlusion* occ,
                  int64_t depth_frame_stride, void* stream) {
  HN_CHECK_ARG(mesh && faces && (paras || cams) && frame && scratch, "%s: null pointer", fn);
  HN_CHECK_ARG(out_image, "%s: out_image is NULL", fn);
  if (int st = check_slots(fn, s, v, f, k)) return st;
  if (int st = check_raster_frames(fn, s, k, h, w)) return st;
  HN_CHECK_ARG(frame_format == HN_FRAME_F32_CHW || frame_format == HN_FRAME_U8_BGR_HWC, "%s: unknown frame format %d", fn,
               frame_format);
  if (int st = check_buffer(fn, "scratch", scratch, scratch_bytes, (int64_t)scratch_total(s, f), 16)) return st;
  if (int st = check_cams_aligned(fn, cams)) return st;
  if (occ) {
    HN_CHECK_ARG(occ->depth, "%s: scene_depth is NULL", fn);
    HN_CHECK_ARG(occ->silhouette, "%s: out_silhouette is NULL", fn);
    if (int st = check_slot_byte(fn, k, "the silhouette's byte")) return st;
    if (int st = check_depth_stride(fn, depth_frame_stride, h, w)) return st;
    HN_CHECK_ARG(occ->margin == occ->margin && fabsf(occ->margin) <= 3.402823466e38f, "%s: margin must be finite", fn);
  }
  if (int st = check_faces_host(fn, faces_host, f, v)) return st;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* sc = static_cast<unsigned char*>(scratch);
  const dim3 grid((w + 31) / 32, (h + 7) / 8, s / k);
  if (!occ)
    launch_setup(mesh, faces, lifted, s, v, f, k, paras, cams, h, w, sc, st);
  else
    launch_setup(mesh, faces, lifted, s, v, f, k, paras, cams, h, w, sc, st, occ->coverage);
  HN_CHECK_LAUNCH("mesh_raster_setup");
  if (!occ) {
    if (frame_format == HN_FRAME_F32_CHW)
      hipLaunchKernelGGL(mesh_raster_tiles<HN_FRAME_F32_CHW>, grid, dim3(256), 0, st, sc, s, f, k, frame, h, w, out_image, out_depth);
    else
      hipLaunchKernelGGL(mesh_raster_tiles<HN_FRAME_U8_BGR_HWC>, grid, dim3(256), 0, st, sc, s, f, k, frame, h, w, out_image,
                         out_depth);
  } else if (frame_format == HN_FRAME_F32_CHW) {
    hipLaunchKernelGGL((mesh_raster_tiles<HN_FRAME_F32_CHW, true, Occlusion>), grid, dim3(256), 0, st, sc, s, f, k, frame, h, w,
                       out_image, out_depth, *occ);
  } else {
    hipLaunchKernelGGL((mesh_raster_tiles<HN_FRAME_U8_BGR_HWC, true, Occlusion>), grid, dim3(256), 0, st, sc, s, f, k, frame, h, w,
                       out_image, out_depth, *occ);
  }
  HN_CHECK_LAUNCH("mesh_raster_tiles");
  return HN_OK;
}

extern "C" int hn_mesh_render_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host, const int32_t* lifted, int s,
                                 int v, int f, int k, const float* paras, const void* frame, int frame_format, int h, int w,
                                 void* scratch, int64_t scratch_bytes, uint8_t* out_image, float* out_depth, void* stream) {
  HN_CHECK_ARG(paras, "hn_mesh_render_u8: null pointer");
  return render("hn_mesh_render_u8", mesh, faces, faces_host, lifted, s, v, f, k, paras, nullptr, frame, frame_format, h, w,
                scratch, scratch_bytes, out_image, out_depth, nullptr, 0, stream);
}

extern "C" int hn_mesh_render_occluded_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host, const int32_t* lifted,
                                          int s, int v, int f, int k, const float* paras, const void* frame, int frame_format,
                                          int h, int w, const float* scene_depth, int64_t depth_frame_stride, float margin,
                                          void* scratch, int64_t scratch_bytes, uint8_t* out_image, float* out_depth,
                                          uint8_t* out_silhouette, int32_t* out_coverage, void* stream) {
  HN_CHECK_ARG(paras, "hn_mesh_render_occluded_u8: null pointer");
  const Occlusion occ = {scene_depth, (long long)depth_frame_stride, margin, out_silhouette, out_coverage};
  return render("hn_mesh_render_occluded_u8", mesh, faces, faces_host, lifted, s, v, f, k, paras, nullptr, frame, frame_format, h,
                w, scratch, scratch_bytes, out_image, out_depth, &occ, depth_frame_stride, stream);
}

// the two entries above with a camera per frame: cams = DEVICE fp32 [s / k][4] in place of the host's four values
extern "C" int hn_mesh_render_cams_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host, const int32_t* lifted,
                                      int s, int v, int f, int k, const float* cams, const void* frame, int frame_format, int h,
                                      int w, void* scratch, int64_t scratch_bytes, uint8_t* out_image, float* out_depth,
                                      void* stream) {
  HN_CHECK_ARG(cams, "hn_mesh_render_cams_u8: null pointer");
  return render("hn_mesh_render_cams_u8", mesh, faces, faces_host, lifted, s, v, f, k, nullptr, cams, frame, frame_format, h, w,
                scratch, scratch_bytes, out_image, out_depth, nullptr, 0, stream);
}

extern "C" int hn_mesh_render_cams_occluded_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host,
                                               const int32_t* lifted, int s, int v, int f, int k, const float* cams,
                                               const void* frame, int frame_format, int h, int w, const float* scene_depth,
                                               int64_t depth_frame_stride, float margin, void* scratch, int64_t scratch_bytes,
                                               uint8_t* out_image, float* out_depth, uint8_t* out_silhouette,
                                               int32_t* out_coverage, void* stream) {
  HN_CHECK_ARG(cams, "hn_mesh_render_cams_occluded_u8: null pointer");
  const Occlusion occ = {scene_depth, (long long)depth_frame_stride, margin, out_silhouette, out_coverage};
  return render("hn_mesh_render_cams_occluded_u8", mesh, faces, faces_host, lifted, s, v, f, k, nullptr, cams, frame, frame_format,
                h, w, scratch, scratch_bytes, out_image, out_depth, &occ, depth_frame_stride, stream);
}

// the geometry pass: render()'s argument checks without a frame, an image or a scene depth, the same setup launch, and
// mesh_geometry_tiles in place of the raster
extern "C" int hn_mesh_geometry_f32(const float* mesh, const int32_t* faces, const int32_t* faces_host, const int32_t* lifted, int s,
                                    int v, int f, int k, const float* paras, const float* cams, int h, int w, void* scratch,
                                    int64_t scratch_bytes, float* out_depth, uint8_t* out_who, void* stream) {
  const char* fn = "hn_mesh_geometry_f32";
  HN_CHECK_ARG(mesh && faces && scratch && out_depth && out_who, "%s: null pointer", fn);
  if (int st = check_one_camera(fn, paras, cams)) return st;
  if (int st = check_slots(fn, s, v, f, k)) return st;
  if (int st = check_slot_byte(fn, k, "the slot byte")) return st;
  if (int st = check_raster_frames(fn, s, k, h, w)) return st;
  if (int st = check_buffer(fn, "scratch", scratch, scratch_bytes, (int64_t)scratch_total(s, f), 16)) return st;
  if (int st = check_cams_aligned(fn, cams)) return st;
  HN_CHECK_ARG(((uintptr_t)out_depth & 3) == 0, "%s: out_depth must be aligned to a float", fn);
  if (int st = check_faces_host(fn, faces_host, f, v)) return st;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* sc = static_cast<unsigned char*>(scratch);
  launch_setup(mesh, faces, lifted, s, v, f, k, paras, cams, h, w, sc, st);
  HN_CHECK_LAUNCH("mesh_raster_setup");
  hipLaunchKernelGGL(mesh_geometry_tiles, dim3((w + 31) / 32, (h + 7) / 8, s / k), dim3(256), 0, st, sc, s, f, k, h, w, out_depth,
                     out_who);
  HN_CHECK_LAUNCH("mesh_geometry_tiles");
  return HN_OK;
}
