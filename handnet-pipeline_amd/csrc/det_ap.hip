// The detector evaluation's per-image part on the device (tests/ap_ref.py restates the rule in numpy fp64,
// operation for operation): what trainval_net_fcos.py:132-169 selects from a batch of detections, what the VOC text files do to
// every number on the way to voc_eval.py (pascal_voc.py:339-343: %.3f scores, float32 coordinate + 1 as %.1f, parsed back as
// fp64), the hand -> object association of voc_eval.py:662-704 and the matching of voc_eval.py:191-225,386-496 against the
// image's ground truth, for the object class and the five hand tables ('', handstate, handside, objectbbox, all).  The outcome
// of every record -- its score in thousandths, a TP and an FP bit per table -- is one int32 word stored at [image id, rank];
// the host sorts and integrates once per epoch (hn_amd/metrics.py compute).
//
// One launch per batch.  One wave per image, kWaves waves per workgroup, one lane per ground-truth box (at most 64 per class and
// image).  The walk over an image's detections is sequential in the wave, 64 selection flags at a time from a ballot; the six sets
// of "taken" flags are 64-bit words every lane holds alike.  What belongs to one detection alone -- the file round trip of its
// box and vector, an object record's centre -- is done 64 rows at once, one lane per row, and handed to the walk by a lane read.
// The association's argmin walks the image's detections 64 at a time, one lane per object record.  Argmax and argmin across the lanes are comparisons and moves only (value, then the lower
// index), so every fp64 value is rounded once, where the rule rounds it (built with -ffp-contract=off, hn_amd/build.py), and
// np.argmax / np.argmin's first-wins order is kept.  The file round trip is float(format(x, '.1f')) == rint(double(x) * 10) / 10
// for a float32 x (and 1000 for '.3f'): the product is exact, rint rounds half to even as the formatting does, the division is
// correctly rounded (tests/test_ap_cpu.py proves the identity over a sweep).
//
// No LDS and no barrier: a wave shares nothing with its neighbours.  Records go out as plain vector stores of lane 0, the
// per-image `fed` count and the one `overflow` counter as integer atomic adds: position-addressed and integer, so the order of
// the images, the batch size and a split over devices do not change a byte.
#include <climits>
#include <cmath>

#include "hn_common.h"

namespace {

constexpr int kWaves = 4;
constexpr int kOwn = 4;                                           // object centres a lane keeps in registers: rows below kOwn * 64
constexpr int kTpShift = 10, kFpShift = 15, kValid = 1 << 20;     // the record word: score 0..9, TP 10..14, FP 15..19

typedef unsigned long long u64;

struct DetApArgs {
  const float* boxes;           // [n][cap][4]
  const float* scores;          // [n][cap]
  const int* labels;            // [n][cap]
  const int* sides;             // [n][cap]
  const int* count;             // [n]
  const int* contacts;          // [n][cap]
  const float* dxdymags;        // [n][cap][3]
  const int* image_ids;         // [n]
  const int* hand_off;          // [images + 1]
  const int* hand_box;          // [hand_total][4]
  const int* hand_meta;         // [hand_total][4]: difficult, handstate, leftright, has objectbbox
  const double* hand_obj;       // [hand_total][4]
  const int* obj_off;           // [images + 1]
  const int* obj_box;           // [obj_total][4]
  const int* obj_diff;          // [obj_total]
  int* hand;                    // [images][max_dets]
  int* obj;                     // [images][max_dets]
  int* fed;                     // [images]
  int* overflow;                // [1]
  double ovthresh;
  float score_min;
  int n, cap, images, hand_total, obj_total, max_dets, hand_label, object_label;
};

__device__ __forceinline__ double file_1f(float x) { return rint((double)x * 10.0) / 10.0; }
__device__ __forceinline__ double file_3f(float x) { return rint((double)x * 1000.0) / 1000.0; }
// np.maximum / np.minimum: a NaN operand is the result
__device__ __forceinline__ double np_max(double a, double b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ double np_min(double a, double b) { return (a <= b || a != a) ? a : b; }

// The largest / smallest value of the wave (no NaN among them), by comparisons and moves: every lane leaves with a value that
// compares equal to it.  WHERE it sits is then a ballot of `==`, whose lowest bit is np.argmax's / np.argmin's first one.
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const double o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const double o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

// voc_eval.py:199-213, the +1 pixel convention
__device__ __forceinline__ double overlap(const double (&bb)[4], const double (&g)[4]) {
#pragma clang fp contract(off)
  const double ixmin = np_max(g[0], bb[0]), iymin = np_max(g[1], bb[1]);
  const double ixmax = np_min(g[2], bb[2]), iymax = np_min(g[3], bb[3]);
  const double iw = np_max((ixmax - ixmin) + 1.0, 0.0);
  const double ih = np_max((iymax - iymin) + 1.0, 0.0);
  const double inters = iw * ih;
  const double uni = (((bb[2] - bb[0]) + 1.0) * ((bb[3] - bb[1]) + 1.0) + ((g[2] - g[0]) + 1.0) * ((g[3] - g[1]) + 1.0)) - inters;
  return inters / uni;
}

// np.max / np.argmax of the overlaps with this wave's ground truth (lane < ngt holds box g) -> ovmax > thr, and jmax
__device__ __forceinline__ bool best_gt(const double (&bb)[4], const double (&g)[4], int ngt, int lane, double thr, int& jmax) {
  jmax = 0;
  if (ngt == 0) return false;                                      // ovmax = -inf
  const bool has = lane < ngt;
  double ov = has ? overlap(bb, g) : -INFINITY;
  if (__ballot(has && ov != ov) != 0) return false;                // np.max keeps a NaN, and a NaN is not above the threshold
  const double ovmax = wave_max(ov);
  const u64 at = __ballot(has && ov == ovmax);                     // (never empty: a lane without a box holds -inf)
  jmax = at != 0 ? __builtin_ctzll(at) : 0;
  return ovmax > thr;
}

// voc_eval.py:593-615 without its asserts: no +1; bb1 is the ground truth's box, bb2 the detection's
__device__ __forceinline__ double plain_iou(const double (&a)[4], const double (&b)[4]) {
#pragma clang fp contract(off)
  const double x_left = b[0] > a[0] ? b[0] : a[0], y_top = b[1] > a[1] ? b[1] : a[1];
  const double x_right = b[2] < a[2] ? b[2] : a[2], y_bottom = b[3] < a[3] ? b[3] : a[3];
  if (x_right < x_left || y_bottom < y_top) return 0.0;
  const double inter = (x_right - x_left) * (y_bottom - y_top);
  const double area_a = (a[2] - a[0]) * (a[3] - a[1]);
  const double area_b = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / ((area_a + area_b) - inter);
}

// gen_det_result's distance of the object centre (cx, cy) in row k2 to the point (px, py), into this lane's first smallest one
// (or its first NaN: np.argmin's winner)
__device__ __forceinline__ void consider(double cx, double cy, double px, double py, int k2, double& mine, int& mine_k, int& nan_k) {
#pragma clang fp contract(off)
  const double dx = cx - px, dy = cy - py;
  const double d = dx * dx + dy * dy;
  const bool is_nan = d != d;
  const bool take = !is_nan && (mine_k == INT_MAX || d < mine);     // (selects of values, so that all three stay in registers)
  nan_k = is_nan && nan_k == INT_MAX ? k2 : nan_k;
  mine = take ? d : mine;
  mine_k = take ? k2 : mine_k;
}

// grid (ceil(n / kWaves)), kWaves * 64 threads: wave = image of the batch, lane = ground-truth box
__global__ __launch_bounds__(kWaves * 64) void det_ap_accumulate_kernel(const DetApArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int n = (int)blockIdx.x * kWaves + wave;
  if (n >= a.n) return;
  const int image = a.image_ids[n];
  if (image < 0 || image >= a.images) {                            // nothing is written for it
    if (lane == 0) atomicAdd(a.overflow, 1);
    return;
  }
  const int raw = a.count[n];
  const int cnt = raw < 0 ? 0 : (raw > a.cap ? a.cap : raw);
  const size_t row = (size_t)n * a.cap;

  // step 1: how many hand and object records the image has
  int n_hand = 0, n_obj = 0;
  for (int base = 0; base < cnt; base += 64) {
    const int k = base + lane;
    const bool picked = k < cnt && a.scores[row + k] > a.score_min;
    const int label = k < cnt ? a.labels[row + k] : 0;
    n_hand += __popcll(__ballot(picked && label == a.hand_label));
    n_obj += __popcll(__ballot(picked && label == a.object_label));
  }
  if (lane == 0) atomicAdd(a.fed + image, 1);
  if (n_hand == 0) return;                                         // step 2, the drop rule: no hand records, no object records

  const size_t out_row = (size_t)image * a.max_dets;
  int unstored = 0;

  // the object class: plain voc_eval
  {
    const int g0 = a.obj_off[image];
    int ngt = a.obj_off[image + 1] - g0;
    if (g0 < 0 || ngt < 0 || ngt > 64 || (long long)g0 + ngt > (long long)a.obj_total) ngt = 0;      // (refused on the host)
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < ngt) {
#pragma unroll
      for (int c = 0; c < 4; ++c) g[c] = (double)a.obj_box[(size_t)(g0 + lane) * 4 + c];
    }
    u64 taken = 0;
    int rank = 0;
    for (int base = 0; base < cnt; base += 64) {
      const int kk = base + lane;
      const bool sel = kk < cnt && a.scores[row + kk] > a.score_min && a.labels[row + kk] == a.object_label;
      u64 todo = __ballot(sel);
      double filed[4] = {0.0, 0.0, 0.0, 0.0};                      // the file round trip of this lane's row: 64 rows at once
      if (sel) {
#pragma unroll
        for (int c = 0; c < 4; ++c) filed[c] = file_1f(a.boxes[(row + kk) * 4 + c] + 1.0f);
      }
      while (todo != 0) {
        const int from = __builtin_ctzll(todo), k = base + from;
        todo &= todo - 1;
        const float score = a.scores[row + k];
        double bb[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bb[c] = __shfl(filed[c], from, 64);
        int jmax;
        int tp = 0, fp = 0;
        if (best_gt(bb, g, ngt, lane, a.ovthresh, jmax)) {
          if (a.obj_diff[g0 + jmax] == 0) {
            if (((taken >> jmax) & 1) == 0) tp = 1, taken |= (u64)1 << jmax;
            else fp = 1;
          }
        } else {
          fp = 1;
        }
        if (rank < a.max_dets && score <= 1.0f) {
          if (lane == 0) a.obj[out_row + rank] = kValid | (int)rint((double)score * 1000.0) | (tp << kTpShift) | (fp << kFpShift);
        } else {
          ++unstored;
        }
        ++rank;
      }
    }
  }

  // the hand class: the association, then the five tables with their own flags
  {
    const int g0 = a.hand_off[image];
    int ngt = a.hand_off[image + 1] - g0;
    if (g0 < 0 || ngt < 0 || ngt > 64 || (long long)g0 + ngt > (long long)a.hand_total) ngt = 0;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < ngt) {
#pragma unroll
      for (int c = 0; c < 4; ++c) g[c] = (double)a.hand_box[(size_t)(g0 + lane) * 4 + c];
    }
    // the centres of the object records in rows lane, lane + 64, ... of the first kOwn * 64 rows, as gen_det_result lists them
    double own_cx[kOwn], own_cy[kOwn];
    unsigned own = 0;
#pragma unroll
    for (int c = 0; c < kOwn; ++c) {
      const int k2 = c * 64 + lane;
      own_cx[c] = own_cy[c] = 0.0;
      if (n_obj > 0 && k2 < cnt && a.scores[row + k2] > a.score_min && a.labels[row + k2] == a.object_label) {
        double o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = file_1f(a.boxes[(row + k2) * 4 + q] + 1.0f);
        own_cx[c] = (o[0] + o[2]) / 2.0, own_cy[c] = (o[1] + o[3]) / 2.0;
        own |= 1u << c;
      }
    }
    u64 taken[5] = {0, 0, 0, 0, 0};
    int rank = 0;
    for (int base = 0; base < cnt; base += 64) {
      const int kk = base + lane;
      const bool sel = kk < cnt && a.scores[row + kk] > a.score_min && a.labels[row + kk] == a.hand_label;
      u64 todo = __ballot(sel);
      double filed[4] = {0.0, 0.0, 0.0, 0.0}, filed_v[3] = {0.0, 0.0, 0.0};
      if (sel) {
#pragma unroll
        for (int c = 0; c < 4; ++c) filed[c] = file_1f(a.boxes[(row + kk) * 4 + c] + 1.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) filed_v[c] = file_3f(a.dxdymags[(row + kk) * 3 + c]);
      }
      while (todo != 0) {
        const int from = __builtin_ctzll(todo), k = base + from;
        todo &= todo - 1;
        const float score = a.scores[row + k];
        double bb[4], v[3];
#pragma unroll
        for (int c = 0; c < 4; ++c) bb[c] = __shfl(filed[c], from, 64);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __shfl(filed_v[c], from, 64);
        const int state = a.contacts[row + k], side = a.sides[row + k];

        // gen_det_result: the object record nearest to the point the hand's vector shows
        bool det_has = false;
        double det_obj[4] = {0.0, 0.0, 0.0, 0.0};
        if (state > 0 && n_obj > 0) {
          const double px = (bb[0] + bb[2]) / 2.0 + (v[0] * 10000.0) * v[1];
          const double py = (bb[1] + bb[3]) / 2.0 + (v[0] * 10000.0) * v[2];
          // every lane keeps the first smallest distance of ITS object records (rows lane, lane + 64, ...); one reduction
          // per hand then finds the smallest of the wave, and the lowest row among the lanes that hold it
          double mine = INFINITY;
          int mine_k = INT_MAX, nan_k = INT_MAX;
#pragma unroll
          for (int c = 0; c < kOwn; ++c) {
            if ((own >> c) & 1) consider(own_cx[c], own_cy[c], px, py, c * 64 + lane, mine, mine_k, nan_k);
          }
          for (int ob = kOwn * 64; ob < cnt; ob += 64) {           // beyond the centres kept in registers: on the fly
            const int k2 = ob + lane;
            if (k2 < cnt && a.scores[row + k2] > a.score_min && a.labels[row + k2] == a.object_label) {
              double o[4];
#pragma unroll
              for (int c = 0; c < 4; ++c) o[c] = file_1f(a.boxes[(row + k2) * 4 + c] + 1.0f);
              consider((o[0] + o[2]) / 2.0, (o[1] + o[3]) / 2.0, px, py, k2, mine, mine_k, nan_k);
            }
          }
          int best_k = INT_MAX;
          if (__ballot(nan_k != INT_MAX) != 0) {                   // np.argmin: the first NaN wins
            best_k = wave_min(nan_k);
          } else {
            const double best = wave_min(mine_k != INT_MAX ? mine : INFINITY);
            u64 at = __ballot(mine_k != INT_MAX && mine == best);
            while (at != 0) {
              const int k2 = __shfl(mine_k, __builtin_ctzll(at), 64);
              at &= at - 1;
              best_k = k2 < best_k ? k2 : best_k;
            }
          }
          if (best_k != INT_MAX) {
            det_has = true;
#pragma unroll
            for (int c = 0; c < 4; ++c) det_obj[c] = file_1f(a.boxes[(row + best_k) * 4 + c] + 1.0f);
          }
        }

        int jmax;
        int tp = 0, fp = 0;
        if (best_gt(bb, g, ngt, lane, a.ovthresh, jmax)) {
          const int* meta = a.hand_meta + (size_t)(g0 + jmax) * 4;
          if (meta[0] == 0) {
            const bool ok_state = meta[1] == state, ok_side = meta[2] == side;
            bool ok_obj;                                           // val_objectbbox
            if (meta[3] == 0 || !det_has) {
              ok_obj = meta[3] == 0 && !det_has;
            } else {
              double gt_obj[4];
#pragma unroll
              for (int c = 0; c < 4; ++c) gt_obj[c] = a.hand_obj[(size_t)(g0 + jmax) * 4 + c];
              ok_obj = plain_iou(gt_obj, det_obj) > 0.5;
            }
            const bool holds[5] = {true, ok_state, ok_side, ok_obj, ok_state && ok_side && ok_obj};
#pragma unroll
            for (int t = 0; t < 5; ++t) {
              if (((taken[t] >> jmax) & 1) == 0 && holds[t]) tp |= 1 << t, taken[t] |= (u64)1 << jmax;
              else fp |= 1 << t;
            }
          }
        } else {
          fp = 31;
        }
        if (rank < a.max_dets && score <= 1.0f) {
          if (lane == 0) a.hand[out_row + rank] = kValid | (int)rint((double)score * 1000.0) | (tp << kTpShift) | (fp << kFpShift);
        } else {
          ++unstored;
        }
        ++rank;
      }
    }
  }
  if (unstored != 0 && lane == 0) atomicAdd(a.overflow, unstored);
}

}  // namespace

extern "C" int hn_det_ap_accumulate_f32(const float* boxes, const float* scores, const int32_t* labels, const int32_t* sides,
                                        const int32_t* count, const int32_t* contacts, const float* dxdymags,
                                        const int32_t* image_ids, int n, int cap, const int32_t* hand_off, const int32_t* hand_box,
                                        const int32_t* hand_meta, const double* hand_obj, int hand_total, const int32_t* obj_off,
                                        const int32_t* obj_box, const int32_t* obj_diff, int obj_total, int images, int hand_label,
                                        int object_label, float score_min, double ovthresh, int32_t* hand, int32_t* obj,
                                        int32_t* fed, int32_t* overflow, int max_dets, void* stream) {
  const char* fn = "hn_det_ap_accumulate_f32";
  HN_CHECK_ARG(n >= 0 && cap >= 0, "%s: n = %d, cap = %d (>= 0)", fn, n, cap);
  HN_CHECK_ARG((int64_t)n * cap <= (int64_t)1 << 28, "%s: n * cap = %lld (at most 2^28 detections a batch)", fn, (long long)n * cap);
  HN_CHECK_ARG(images >= 1 && max_dets >= 1, "%s: images = %d, max_dets = %d (>= 1)", fn, images, max_dets);
  HN_CHECK_ARG((int64_t)images * max_dets <= (int64_t)1 << 27, "%s: images * max_dets = %lld (at most 2^27 records a table)", fn,
               (long long)images * max_dets);
  HN_CHECK_ARG(hand_total >= 0 && obj_total >= 0, "%s: hand_total = %d, obj_total = %d (>= 0)", fn, hand_total, obj_total);
  HN_CHECK_ARG(hand_label != object_label, "%s: hand_label == object_label == %d", fn, hand_label);
  HN_CHECK_ARG(score_min >= 0.f && score_min < 1.f, "%s: score_min = %g (0 <= score_min < 1)", fn, (double)score_min);
  HN_CHECK_ARG(ovthresh == ovthresh, "%s: ovthresh is NaN", fn);
  HN_CHECK_ARG(hand_off && obj_off && hand && obj && fed && overflow, "%s: null pointer (hand_off, obj_off, hand, obj, fed, overflow)", fn);
  HN_CHECK_ARG((hand_total == 0 || (hand_box && hand_meta && hand_obj)) && (obj_total == 0 || (obj_box && obj_diff)),
               "%s: null pointer in a non-empty ground-truth table", fn);
  HN_CHECK_ARG(((uintptr_t)hand_obj & 7) == 0, "%s: hand_obj must be aligned to 8 bytes", fn);
  HN_CHECK_ARG((((uintptr_t)hand_off | (uintptr_t)hand_box | (uintptr_t)hand_meta | (uintptr_t)obj_off | (uintptr_t)obj_box |
                 (uintptr_t)obj_diff | (uintptr_t)hand | (uintptr_t)obj | (uintptr_t)fed | (uintptr_t)overflow) & 3) == 0,
               "%s: the tables and the state must be aligned to 4 bytes", fn);
  if (n == 0) return HN_OK;
  HN_CHECK_ARG(count && image_ids, "%s: null pointer (count, image_ids)", fn);
  HN_CHECK_ARG(cap == 0 || (boxes && scores && labels && sides && contacts && dxdymags),
               "%s: null pointer (boxes, scores, labels, sides, contacts, dxdymags)", fn);
  HN_CHECK_ARG((((uintptr_t)boxes | (uintptr_t)scores | (uintptr_t)labels | (uintptr_t)sides | (uintptr_t)count | (uintptr_t)contacts |
                 (uintptr_t)dxdymags | (uintptr_t)image_ids) & 3) == 0, "%s: the batch's tensors must be aligned to 4 bytes", fn);
  DetApArgs a;
  a.boxes = boxes, a.scores = scores, a.labels = labels, a.sides = sides, a.count = count, a.contacts = contacts;
  a.dxdymags = dxdymags, a.image_ids = image_ids;
  a.hand_off = hand_off, a.hand_box = hand_box, a.hand_meta = hand_meta, a.hand_obj = hand_obj;
  a.obj_off = obj_off, a.obj_box = obj_box, a.obj_diff = obj_diff;
  a.hand = hand, a.obj = obj, a.fed = fed, a.overflow = overflow;
  a.ovthresh = ovthresh, a.score_min = score_min;
  a.n = n, a.cap = cap, a.images = images, a.hand_total = hand_total, a.obj_total = obj_total, a.max_dets = max_dets;
  a.hand_label = hand_label, a.object_label = object_label;
  hipLaunchKernelGGL(det_ap_accumulate_kernel, dim3(hn::cdiv(n, kWaves)), dim3(kWaves * 64), 0, (hipStream_t)stream, a);
  HN_CHECK_LAUNCH("det_ap_accumulate_kernel");
  return HN_OK;
}
