// The HandNet crop stage, between the detector and the pose network: hand detections -> slots (padded integer boxes) ->
// nearest-neighbour crops.  Integer and order-sensitive fp32 work -- built with -ffp-contract=off so every multiply and add
// rounds separately, exactly like the reference's chain of torch ops (tests/crop_ref.py restates the rules).
//
//   hn_crop_resize               : handnet_pipeline/handnet_pipeline.py:74-105, the first hand detection of each frame
//   hn_crop_resize_hands         : the same rule for the first K hand detections of each frame (K crops per frame)
//   hn_crop_resize_hands_sided   : ... with the slots' handedness; a left hand's crop is cut mirrored
//   hn_crop_resize_hands_tracked : ... with the slots carried over from one call to the next
//
// Each rule stands here once: the padded box (pad_hand_box), the slot's outputs (write_slot), the gather
// (hand_crop_gather_kernel), the argument checks and the choice of kernels (crop_stage_run).  The top-1 entry is the K = 1
// case of the same launches, not a copy of them.
#include "hn_common.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxHands = 16;

// the detection list of n frames, the frame geometry and where the slots go: the by-value argument of both slot kernels
// (its members are handed on one by one, never its address: a by-value kernel argument whose address escapes is copied to scratch)
struct SlotArgs {
  const float* __restrict__ det_boxes;     // [n][cap][4]
  const float* __restrict__ det_scores;    // [n][cap]; null: no score wanted (the top-1 entry)
  const int* __restrict__ det_labels;      // [n][cap]
  const int* __restrict__ det_sides;       // [n][cap]; SIDED kernels only
  const int* __restrict__ det_count;       // [n]
  int cap, hand_label, max_hands, h, w, left_side;
  long long* __restrict__ crop_box;        // [n][max_hands][4]
  int* __restrict__ has_hand;              // [n][max_hands], as every output below
  float* __restrict__ score;               // null: not written
  int* __restrict__ det_index;             // null: not written
  int* __restrict__ side;                  // SIDED kernels only, as mirror
  int* __restrict__ mirror;
};

// The padded box of one detection: handnet_pipeline.py:88-97 on 0-d tensors -- the box truncated toward zero, 0.4 of its
// integer width and height added on each side in fp32 (no contraction in this file: a fused multiply-add here is a wrong
// box), truncated again on store and clamped to the frame.  Returns 0 when the inclusive slice [b1 : b3 + 1, b0 : b2 + 1],
// clamped to the image, is empty (o[] then zero).
__device__ __forceinline__ int pad_hand_box(const float* b, int h, int w, long long o[4]) {
  long long b0 = (long long)b[0], b1 = (long long)b[1], b2 = (long long)b[2], b3 = (long long)b[3];
  const long long bw = b2 - b0, bh = b3 - b1;
  const float pw = 0.4f * (float)bw, phh = 0.4f * (float)bh;
  const float t0 = (float)b0 - pw, t1 = (float)b1 - phh;
  const float t2 = (float)b2 + pw, t3 = (float)b3 + phh;
  b0 = t0 > 0.f ? (long long)t0 : 0;
  b1 = t1 > 0.f ? (long long)t1 : 0;
  b2 = t2 < (float)w ? (long long)t2 : (long long)w;
  b3 = t3 < (float)h ? (long long)t3 : (long long)h;
  const long long ch = (b3 + 1 < h ? b3 + 1 : h) - b1, cwid = (b2 + 1 < w ? b2 + 1 : w) - b0;
  const int ok = (ch > 0 && cwid > 0 && b1 >= 0 && b0 >= 0) ? 1 : 0;
  o[0] = ok ? b0 : 0; o[1] = ok ? b1 : 0; o[2] = ok ? b2 : 0; o[3] = ok ? b3 : 0;
  return ok;
}

// Everything a slot hands out.  ok = 0 is the empty slot: score 0, det_index -1, side -1, mirror 0 (b[] is zero then).
// The box goes out as four 64-bit words: the top-1 entry's crop_box is the C caller's own int64 array, 8-byte aligned only.
// score / det_index may be null (the same on every lane); side / mirror are touched by the SIDED kernels only.
template <bool SIDED>
__device__ __forceinline__ void write_slot(long slot, const long long b[4], int ok, float sc, int idx, int sd, int left_side,
                                           long long* __restrict__ crop_box, int* __restrict__ has_hand,
                                           float* __restrict__ score, int* __restrict__ det_index,
                                           int* __restrict__ side, int* __restrict__ mirror) {
  long long* cb = crop_box + slot * 4;
  cb[0] = b[0]; cb[1] = b[1]; cb[2] = b[2]; cb[3] = b[3];
  has_hand[slot] = ok;
  if (score) score[slot] = ok ? sc : 0.f;
  if (det_index) det_index[slot] = ok ? idx : -1;
  if (SIDED) {
    side[slot] = ok ? sd : -1;
    mirror[slot] = (ok && sd == left_side) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------
// hands: slot k of frame i = the k-th hand-label detection of the frame's score-ordered list
// ---------------------------------------------------------------------------------------
// One wave64 per frame.  The survivor list is walked 64 entries at a time: a ballot of the hand-label lanes, and a
// lane's rank among the frame's hand detections is the popcount of the matching lanes below it plus those of earlier
// chunks.  The walk ends as soon as max_hands are found (real frames: the first chunk); slots left over are zeroed.
// max_hands = 1 is the reference's top-1 crop: slot 0 is the first detection with the hand label.
// SIDED: the slot's handedness in the same launch -- side = det_sides of the slot's detection (-1: empty slot), mirror = 1
// for a filled slot whose side is left_side (such a slot goes through the right-handed pose network and lifter mirrored)
template <bool SIDED>
__global__ __launch_bounds__(64) void hand_slots_kernel(const SlotArgs a) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int cnt = min(a.det_count[img], a.cap);
  const long row = (long)img * a.cap;
  int found = 0;
  for (int base = 0; base < cnt && found < a.max_hands; base += 64) {
    const int i = base + lane;
    const bool hand = i < cnt && a.det_labels[row + i] == a.hand_label;
    const unsigned long long mask = __ballot(hand);
    const int rank = found + __popcll(mask & ((1ull << lane) - 1ull));
    if (hand && rank < a.max_hands) {
      long long b[4];
      const int ok = pad_hand_box(a.det_boxes + (row + i) * 4, a.h, a.w, b);
      write_slot<SIDED>((long)img * a.max_hands + rank, b, ok, a.det_scores ? a.det_scores[row + i] : 0.f, i,
                        SIDED ? a.det_sides[row + i] : -1, a.left_side, a.crop_box, a.has_hand, a.score, a.det_index, a.side,
                        a.mirror);
    }
    found += __popcll(mask);
  }
  if (lane >= found && lane < a.max_hands) {
    const long long z[4] = {0, 0, 0, 0};
    write_slot<SIDED>((long)img * a.max_hands + lane, z, 0, 0.f, -1, -1, a.left_side, a.crop_box, a.has_hand, a.score,
                      a.det_index, a.side, a.mirror);
  }
}

// ---------------------------------------------------------------------------------------
// tracked hands: the slots carry over from one step to the next
// ---------------------------------------------------------------------------------------
constexpr int kTrackWords = 12;     // int32 words of a state row: box (4 x int64) | id | age | missed | 0

// position of the n-th (0-based) set bit of m, -1 when m has no more than n (n <= 15)
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int n) {
  for (int j = 0; j < kMaxHands - 1; ++j)
    if (j < n) m &= m - 1ull;
  return m ? __ffsll((long long)m) - 1 : -1;
}

// (I, U, key) of one slot x candidate pair; key = slot * 16 + cand, the lower key wins an exact tie.  I == 0: not eligible.
struct TrackPair {
  unsigned i, u, key;
};

// a beats b: larger I / U (cross-multiplied, 32 x 32 -> 64 bits: I, U < 2^31 for frames up to 32767 a side), then lower key
__device__ __forceinline__ bool pair_beats(const TrackPair& a, const TrackPair& b) {
  const unsigned long long l = (unsigned long long)a.i * b.u, r = (unsigned long long)b.i * a.u;
  return l > r || (l == r && a.key < b.key);
}

// hand_slots_kernel with the association of DESIGN.md 9e, one wave64 per frame: the first 16 hand detections of the frame's
// list are the candidates (candidate c in the registers of lane c), lane s < K holds track slot s of the frame's state row (read
// whole before anything is written; updated in place), the K x 16 pairs lie four to a lane (lane = 16 * (slot % 4) + cand, its
// j-th pair is slot lane / 16 + 4 j) and every greedy round is one wave-wide arg-max.  Integer arithmetic on the padded boxes
// only: h, w <= 32767 keeps a coordinate in 15 bits, an area in 30 and I * U in 61.
template <bool SIDED>
__global__ __launch_bounds__(64) void hand_slots_tracked_kernel(const SlotArgs a, int* __restrict__ state, int thr_milli, int hold,
                                                                int* __restrict__ track_id, int* __restrict__ track_age) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  const int img = blockIdx.x, lane = threadIdx.x;
  const int max_hands = a.max_hands;
  const int cnt = min(a.det_count[img], a.cap);
  const long row = (long)img * a.cap;

  // the frame's state row, before anything is written
  int* st_row = state + (long)img * (1 + max_hands) * kTrackWords;
  const int header = st_row[0];
  int sx1 = 0, sy1 = 0, sx2 = 0, sy2 = 0, sid = 0, sage = 0, smiss = 0;
  if (lane < max_hands) {
    const int* p = st_row + (1 + lane) * kTrackWords;
    const i64x2 lo = *reinterpret_cast<const i64x2*>(p), hi = *reinterpret_cast<const i64x2*>(p + 4);
    const i32x4 t = *reinterpret_cast<const i32x4*>(p + 8);
    sx1 = (int)lo[0]; sy1 = (int)lo[1]; sx2 = (int)hi[0]; sy2 = (int)hi[1];
    sid = t[0]; sage = t[1]; smiss = t[2];
  }

  // 1. candidates: the first 16 hand detections, candidate c on lane c
  int ncand = 0;
  int cx1 = 0, cy1 = 0, cx2 = 0, cy2 = 0, cok = 0, cidx = -1, csd = -1;
  float csc = 0.f;
  for (int base = 0; base < cnt && ncand < kMaxHands; base += 64) {
    const int i = base + lane;
    const bool hand = i < cnt && a.det_labels[row + i] == a.hand_label;
    const unsigned long long mask = __ballot(hand);
    long long b[4] = {0, 0, 0, 0};
    int ok = 0, sd = -1;
    float sc = 0.f;
    if (hand) {
      ok = pad_hand_box(a.det_boxes + (row + i) * 4, a.h, a.w, b);
      sc = a.det_scores[row + i];
      if (SIDED) sd = a.det_sides[row + i];
    }
    const int want = lane - ncand;
    const bool take = lane < kMaxHands && want >= 0 && want < __popcll(mask);
    const int src = take ? nth_set_bit(mask, want) : lane;
    const int gx1 = __shfl((int)b[0], src), gy1 = __shfl((int)b[1], src), gx2 = __shfl((int)b[2], src),
              gy2 = __shfl((int)b[3], src), gok = __shfl(ok, src), gsd = __shfl(sd, src);
    const float gsc = __shfl(sc, src);
    if (take) {
      cx1 = gx1; cy1 = gy1; cx2 = gx2; cy2 = gy2; cok = gok; csd = gsd; csc = gsc; cidx = base + src;
    }
    ncand = min(kMaxHands, ncand + __popcll(mask));
  }
  const bool cvalid = lane < ncand && cok;

  // 2. pairs: this lane's candidate against its (up to) four slots
  const int pc = lane & 15, ps = lane >> 4;
  const int qx1 = __shfl(cx1, pc), qy1 = __shfl(cy1, pc), qx2 = __shfl(cx2, pc), qy2 = __shfl(cy2, pc);
  const int qvalid = __shfl((int)cvalid, pc);
  const unsigned carea = (unsigned)((qx2 - qx1) * (qy2 - qy1));
  TrackPair pr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int s = ps + 4 * j;
    const int tx1 = __shfl(sx1, s), ty1 = __shfl(sy1, s), tx2 = __shfl(sx2, s), ty2 = __shfl(sy2, s), tid = __shfl(sid, s);
    const int iw = max(0, min(tx2, qx2) - max(tx1, qx1)), ih = max(0, min(ty2, qy2) - max(ty1, qy1));
    const unsigned inter = (unsigned)(iw * ih);
    const unsigned uni = (unsigned)((tx2 - tx1) * (ty2 - ty1)) + carea - inter;
    const bool eligible = tid != 0 && qvalid && inter > 0 &&
                          1000ull * inter >= (unsigned long long)thr_milli * uni;
    pr[j].i = eligible ? inter : 0u;
    pr[j].u = eligible ? uni : 1u;
    pr[j].key = (unsigned)(s * 16 + pc);
  }

  // 3. greedy match: the best pair left, wave-wide, until none is eligible
  unsigned slot_done = 0, cand_done = 0;      // bit sets, the same on every lane
  int mycand = -1;                            // lane s < K: the candidate its slot took
  const int rounds = min(max_hands, kMaxHands);
  for (int r = 0; r < rounds; ++r) {
    TrackPair best = {0u, 1u, 0xffffu};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      TrackPair p = pr[j];
      if ((slot_done >> (ps + 4 * j)) & 1u || (cand_done >> pc) & 1u) { p.i = 0u; p.u = 1u; }
      if (pair_beats(p, best)) best = p;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      TrackPair o;
      o.i = __shfl_xor(best.i, m); o.u = __shfl_xor(best.u, m); o.key = __shfl_xor(best.key, m);
      if (pair_beats(o, best)) best = o;
    }
    if (best.i == 0u) break;                  // (the same on every lane: the arg-max is a total order)
    const int ms = (int)(best.key >> 4), mc = (int)(best.key & 15u);
    slot_done |= 1u << ms;
    cand_done |= 1u << mc;
    if (lane == ms) mycand = mc;
  }

  // 4. unmatched live slots: held, or freed once missed for more than `hold` steps
  const bool live = lane < max_hands && sid != 0;
  if (live && mycand < 0) {
    smiss += 1;
    if (smiss > hold) { sx1 = sy1 = sx2 = sy2 = 0; sid = sage = smiss = 0; }
  } else if (live) {
    sage += 1;
    smiss = 0;
  }

  // 5. unmatched candidates, in score order, into the free slots, lowest first
  const unsigned free_mask = (unsigned)__ballot(lane < max_hands && sid == 0);
  const unsigned new_mask = (unsigned)__ballot(cvalid && !((cand_done >> lane) & 1u));
  const int admitted = min(__popc(free_mask), __popc(new_mask));
  if (lane < max_hands && sid == 0) {
    const int q = __popc(free_mask & ((1u << lane) - 1u));
    if (q < admitted) {
      mycand = nth_set_bit(new_mask, q);
      sid = header + q + 1;
      sage = 0; smiss = 0;
    }
  }

  // 6. the slots' outputs and the new state (every lane takes part in the gather of its candidate's registers)
  const int from = mycand >= 0 ? mycand : lane;
  const int nx1 = __shfl(cx1, from), ny1 = __shfl(cy1, from), nx2 = __shfl(cx2, from), ny2 = __shfl(cy2, from),
            nidx = __shfl(cidx, from), nsd = __shfl(csd, from);
  const float nsc = __shfl(csc, from);
  if (lane < max_hands) {
    const long slot = (long)img * max_hands + lane;
    const bool filled = mycand >= 0;
    if (filled) { sx1 = nx1; sy1 = ny1; sx2 = nx2; sy2 = ny2; }
    const long long ob[4] = {filled ? sx1 : 0, filled ? sy1 : 0, filled ? sx2 : 0, filled ? sy2 : 0};
    write_slot<SIDED>(slot, ob, filled ? 1 : 0, nsc, nidx, nsd, a.left_side, a.crop_box, a.has_hand, a.score, a.det_index,
                      a.side, a.mirror);
    track_id[slot] = sid;
    track_age[slot] = sage;
    int* p = st_row + (1 + lane) * kTrackWords;
    *reinterpret_cast<i64x2*>(p) = i64x2{sx1, sy1};
    *reinterpret_cast<i64x2*>(p + 4) = i64x2{sx2, sy2};
    *reinterpret_cast<i32x4*>(p + 8) = i32x4{sid, sage, smiss, 0};
  }
  if (lane == 0) {
    const i32x4 z = {0, 0, 0, 0};
    *reinterpret_cast<i32x4*>(st_row) = i32x4{header + admitted, 0, 0, 0};
    *reinterpret_cast<i32x4*>(st_row + 4) = z;
    *reinterpret_cast<i32x4*>(st_row + 8) = z;
  }
}

// ---------------------------------------------------------------------------------------
// gather: nearest resize of every slot's slice to out x out (crop `slot` reads frame slot / max_hands)
// ---------------------------------------------------------------------------------------
// One thread per output pixel, all channels: an f32x4 store of the image's channels (RGBD: permuted), zero vectors for the
// padding channels, a zero pixel for an empty slot.
// SIDED: a slot with mirror != 0 is cut mirrored -- its pixel (oy, ox) is the plain crop's pixel (oy, out - 1 - ox): the
// source-column rule below, evaluated at out - 1 - ox
template <bool SIDED>
__global__ __launch_bounds__(256) void hand_crop_gather_kernel(const float* __restrict__ depth,
                                                               const long long* __restrict__ crop_box,
                                                               const int* __restrict__ has_hand, int n, int max_hands,
                                                               int h, int w, int in_ch, int reorder, int out, int c4,
                                                               float* __restrict__ crops, const int* __restrict__ mirror) {
  const long total = (long)n * max_hands * out * out;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int ox = (int)(i % out);
    const long t = i / out;
    const int oy = (int)(t % out);
    const long slot = t / out;
    if (SIDED && mirror[slot]) ox = out - 1 - ox;
    const long img = slot / max_hands;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (has_hand[slot]) {
      const long long* b = crop_box + slot * 4;
      const int x1 = (int)b[0], y1 = (int)b[1];
      const int cw = (int)((b[2] + 1 < w ? b[2] + 1 : w) - b[0]);
      const int ch = (int)((b[3] + 1 < h ? b[3] + 1 : h) - b[1]);
      // F.interpolate(mode='nearest'): src = min(floor(dst * (float)in / out), in - 1)
      int sy, sx;
      if (ch == out) sy = oy; else if (out == 2 * ch) sy = oy >> 1;
      else sy = min((int)floorf((float)oy * ((float)ch / (float)out)), ch - 1);
      if (cw == out) sx = ox; else if (out == 2 * cw) sx = ox >> 1;
      else sx = min((int)floorf((float)ox * ((float)cw / (float)out)), cw - 1);
      const long pix = (long)(y1 + sy) * w + (x1 + sx);
      for (int c = 0; c < in_ch; ++c) {
        // RGBD: depth_crop[[2,1,0,3]] (handnet_pipeline.py:102): output channel c reads input channel perm[c]
        const int src_c = (reorder && c < 3) ? 2 - c : c;
        o[c] = depth[(img * in_ch + src_c) * h * w + pix];
      }
    }
    *reinterpret_cast<f32x4*>(crops + i * c4 * 4) = o;
    for (int q = 1; q < c4; ++q) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(crops + i * c4 * 4 + q * 4) = z;
    }
  }
}

int grid_for(long total, int block) {
  const long g = (total + block - 1) / block;
  return (int)(g < 8192 ? (g > 0 ? g : 1) : 8192);
}

// One call of the stage.  The optional parts are all-or-nothing, and the entry that fills them has seen to that.
struct CropCall {
  // the detection list, as hn_fcos_nms writes it
  const float* det_boxes;
  const float* det_scores;
  const int32_t* det_labels;
  const int32_t* det_count;
  int cap, hand_label;
  // the frames and the crops' geometry
  const float* depth;
  int n, in_ch, reorder_bgr, h, w, out, cpad, max_hands;
  // the slots and their crops
  int64_t* crop_box;
  int32_t* has_hand;
  float* score;
  int32_t* det_index;
  float* crops;
  // top-1 (hn_crop_resize): no det_scores / score / det_index, and crop_box may be the C caller's own int64 array
  bool top1;
  // sided: det_sides != null
  const int32_t* det_sides;
  int left_side;
  int32_t* side;
  int32_t* mirror;
  // tracked
  bool tracked;
  int32_t* state;
  int thr_milli, hold;
  int32_t* track_id;
  int32_t* track_age;
};

}  // namespace

// Checks, then the slot kernel and the gather, once each.  (The alignment checks stand before the value checks, so that a
// host without a device can tell that an address was accepted from the refusal that follows it.)
static int crop_stage_run(const char* who, const CropCall& c, hipStream_t st) {
  HN_CHECK_ARG(c.det_boxes && c.det_labels && c.det_count && c.depth && c.crop_box && c.has_hand && c.crops &&
                   (c.top1 || (c.det_scores && c.score && c.det_index)) && (!c.tracked || (c.state && c.track_id && c.track_age)),
               "%s: null pointer", who);
  HN_CHECK_ARG(c.max_hands >= 1 && c.max_hands <= kMaxHands, "max_hands must be 1..%d (got %d)", kMaxHands, c.max_hands);
  HN_CHECK_ARG(c.n > 0 && c.h > 0 && c.w > 0 && c.out > 0 && c.cap > 0 && c.cpad >= 4 && c.cpad % 4 == 0, "bad dims");
  HN_CHECK_ARG((c.top1 || (uintptr_t)c.crop_box % 16 == 0) && (uintptr_t)c.crops % 16 == 0,
               "crop_box / crops must be 16-byte aligned");
  HN_CHECK_ARG(c.in_ch >= 1 && c.in_ch <= 4, "depth image must have 1..4 channels (got %d)", c.in_ch);
  if (c.tracked) {
    HN_CHECK_ARG(c.h <= 32767 && c.w <= 32767, "tracked hands: frames of at most 32767 x 32767 pixels (got %d x %d)", c.h, c.w);
    HN_CHECK_ARG(c.thr_milli >= 1 && c.thr_milli <= 1000, "thr_milli must be 1..1000 (got %d)", c.thr_milli);
    HN_CHECK_ARG(c.hold >= 0 && c.hold <= 1000000, "hold must be 0..1000000 (got %d)", c.hold);
    HN_CHECK_ARG((uintptr_t)c.state % 16 == 0, "state must be 16-byte aligned");
  }
  const bool sided = c.det_sides != nullptr;
  SlotArgs a;
  a.det_boxes = c.det_boxes; a.det_scores = c.det_scores; a.det_labels = c.det_labels; a.det_sides = c.det_sides;
  a.det_count = c.det_count; a.cap = c.cap; a.hand_label = c.hand_label; a.max_hands = c.max_hands; a.h = c.h; a.w = c.w;
  a.left_side = c.left_side; a.crop_box = (long long*)c.crop_box; a.has_hand = c.has_hand; a.score = c.score;
  a.det_index = c.det_index; a.side = c.side; a.mirror = c.mirror;
  if (c.tracked) {
    hipLaunchKernelGGL((sided ? hand_slots_tracked_kernel<true> : hand_slots_tracked_kernel<false>), dim3(c.n), dim3(64), 0, st, a,
                       c.state, c.thr_milli, c.hold, c.track_id, c.track_age);
    HN_CHECK_LAUNCH("hand_slots_tracked_kernel");
  } else {
    hipLaunchKernelGGL((sided ? hand_slots_kernel<true> : hand_slots_kernel<false>), dim3(c.n), dim3(64), 0, st, a);
    HN_CHECK_LAUNCH("hand_slots_kernel");
  }
  const long total = (long)c.n * c.max_hands * c.out * c.out;
  hipLaunchKernelGGL((sided ? hand_crop_gather_kernel<true> : hand_crop_gather_kernel<false>), dim3(grid_for(total, 256)), dim3(256),
                     0, st, c.depth, (const long long*)c.crop_box, c.has_hand, c.n, c.max_hands, c.h, c.w, c.in_ch, c.reorder_bgr,
                     c.out, c.cpad / 4, c.crops, (const int*)c.mirror);
  HN_CHECK_LAUNCH("hand_crop_gather_kernel");
  return HN_OK;
}

// what the four entries share: the detection list, the frames, the geometry and the slots' common outputs
static CropCall crop_call(const float* det_boxes, const float* det_scores, const int32_t* det_labels, const int32_t* det_count,
                          int cap, int hand_label, int max_hands, const float* depth, int n, int in_ch, int reorder_bgr, int h,
                          int w, int out, int cpad, int64_t* crop_box, int32_t* has_hand, float* score, int32_t* det_index,
                          float* crops) {
  CropCall c = {};
  c.det_boxes = det_boxes; c.det_scores = det_scores; c.det_labels = det_labels; c.det_count = det_count;
  c.cap = cap; c.hand_label = hand_label; c.max_hands = max_hands;
  c.depth = depth; c.n = n; c.in_ch = in_ch; c.reorder_bgr = reorder_bgr; c.h = h; c.w = w; c.out = out; c.cpad = cpad;
  c.crop_box = crop_box; c.has_hand = has_hand; c.score = score; c.det_index = det_index; c.crops = crops;
  return c;
}

extern "C" int hn_crop_resize(const float* det_boxes, const int32_t* det_labels, const int32_t* det_count, int cap,
                              int hand_label, const float* depth, int n, int in_ch, int reorder_bgr, int h, int w,
                              int out, int cpad,
                              int64_t* crop_box, int32_t* has_hand, float* crops, void* stream) {
  CropCall c = crop_call(det_boxes, nullptr, det_labels, det_count, cap, hand_label, 1, depth, n, in_ch, reorder_bgr, h, w, out,
                         cpad, crop_box, has_hand, nullptr, nullptr, crops);
  c.top1 = true;
  return crop_stage_run("hn_crop_resize", c, (hipStream_t)stream);
}

extern "C" int hn_crop_resize_hands(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                                    const int32_t* det_count, int cap, int hand_label, int max_hands, const float* depth,
                                    int n, int in_ch, int reorder_bgr, int h, int w, int out, int cpad, int64_t* crop_box,
                                    int32_t* has_hand, float* score, int32_t* det_index, float* crops, void* stream) {
  const CropCall c = crop_call(det_boxes, det_scores, det_labels, det_count, cap, hand_label, max_hands, depth, n, in_ch,
                               reorder_bgr, h, w, out, cpad, crop_box, has_hand, score, det_index, crops);
  return crop_stage_run("hn_crop_resize_hands", c, (hipStream_t)stream);
}

extern "C" int hn_crop_resize_hands_sided(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                                          const int32_t* det_sides, const int32_t* det_count, int cap, int hand_label,
                                          int left_side, int max_hands, const float* depth, int n, int in_ch, int reorder_bgr,
                                          int h, int w, int out, int cpad, int64_t* crop_box, int32_t* has_hand, float* score,
                                          int32_t* det_index, int32_t* side, int32_t* mirror, float* crops, void* stream) {
  HN_CHECK_ARG(det_sides && side && mirror, "hn_crop_resize_hands_sided: null pointer");
  CropCall c = crop_call(det_boxes, det_scores, det_labels, det_count, cap, hand_label, max_hands, depth, n, in_ch, reorder_bgr,
                         h, w, out, cpad, crop_box, has_hand, score, det_index, crops);
  c.det_sides = det_sides; c.left_side = left_side; c.side = side; c.mirror = mirror;
  return crop_stage_run("hn_crop_resize_hands_sided", c, (hipStream_t)stream);
}

extern "C" int64_t hn_track_state_bytes(int n, int max_hands) {
  if (n <= 0 || max_hands < 1 || max_hands > kMaxHands) return 0;
  return (int64_t)n * (1 + max_hands) * kTrackWords * 4;
}

extern "C" int hn_crop_resize_hands_tracked(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                                            const int32_t* det_sides, const int32_t* det_count, int cap, int hand_label,
                                            int left_side, int max_hands, const float* depth, int n, int in_ch, int reorder_bgr,
                                            int h, int w, int out, int cpad, int64_t* crop_box, int32_t* has_hand, float* score,
                                            int32_t* det_index, int32_t* side, int32_t* mirror, float* crops, int32_t* state,
                                            int thr_milli, int hold, int32_t* track_id, int32_t* track_age, void* stream) {
  HN_CHECK_ARG((det_sides && side && mirror) || (!det_sides && !side && !mirror),
               "hn_crop_resize_hands_tracked: det_sides, side and mirror go together (all given, or all NULL)");
  CropCall c = crop_call(det_boxes, det_scores, det_labels, det_count, cap, hand_label, max_hands, depth, n, in_ch, reorder_bgr,
                         h, w, out, cpad, crop_box, has_hand, score, det_index, crops);
  c.det_sides = det_sides; c.left_side = left_side; c.side = side; c.mirror = mirror;
  c.tracked = true; c.state = state; c.thr_milli = thr_milli; c.hold = hold; c.track_id = track_id; c.track_age = track_age;
  return crop_stage_run("hn_crop_resize_hands_tracked", c, (hipStream_t)stream);
}
