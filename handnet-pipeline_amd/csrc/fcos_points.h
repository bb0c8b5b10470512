// The detector's anchor points, shared by the candidate kernels (fcos_post.hip) and the criterion (fcos_loss.hip): the level
// table, a point's level and anchor (anchor_utils.py:82-132), and the ext head's (mag, dx, dy) normalisation (fcos.py:301-303).
// One source, one arithmetic: both files are built with -ffp-contract=off.
#pragma once
#include "hn_common.h"

namespace hn_fcos {

struct LevelTable {
  int num_levels;
  int h[HN_FCOS_MAX_LEVELS], w[HN_FCOS_MAX_LEVELS], stride[HN_FCOS_MAX_LEVELS];
  int start[HN_FCOS_MAX_LEVELS + 1];  // first point index of each level
  const float* cls_lr[HN_FCOS_MAX_LEVELS];
  const float* reg_ctr[HN_FCOS_MAX_LEVELS];
};

// hn_fcos_levels -> LevelTable (unused levels zeroed, their start = the number of points); HN_OK or the argument error
inline int level_table_fill(const hn_fcos_levels* lv, LevelTable& lt) {
  HN_CHECK_ARG(lv->num_levels > 0 && lv->num_levels <= HN_FCOS_MAX_LEVELS, "bad level count");
  lt.num_levels = lv->num_levels;
  lt.start[0] = 0;
  for (int l = 0; l < lv->num_levels; ++l) {
    HN_CHECK_ARG(lv->h[l] > 0 && lv->w[l] > 0 && lv->stride[l] > 0 && lv->cls_lr[l] && lv->reg_ctr[l], "bad level %d", l);
    lt.h[l] = lv->h[l];
    lt.w[l] = lv->w[l];
    lt.stride[l] = lv->stride[l];
    lt.cls_lr[l] = lv->cls_lr[l];
    lt.reg_ctr[l] = lv->reg_ctr[l];
    lt.start[l + 1] = lt.start[l] + lv->h[l] * lv->w[l];
  }
  for (int l = lv->num_levels; l < HN_FCOS_MAX_LEVELS; ++l) {
    lt.h[l] = lt.w[l] = lt.stride[l] = 0;
    lt.cls_lr[l] = lt.reg_ctr[l] = nullptr;
    lt.start[l + 1] = lt.start[lv->num_levels];
  }
  return HN_OK;
}

// the level of point i of the anchor order
__device__ __forceinline__ int point_level(const LevelTable& lt, int i) {
  int lv = 0;
  while (lv + 1 < lt.num_levels && i >= lt.start[lv + 1]) ++lv;
  return lv;
}

// The anchor of point q of level lv: base anchor [-s/2, -s/2, s/2, s/2].round() shifted to (gx, gy) * stride, as centre and
// size through its fp32 corners (det_utils.py:266-294 reads them that way)
struct PointAnchor {
  float cx, cy, bw, bh;
};
__device__ __forceinline__ PointAnchor point_anchor(const LevelTable& lt, int lv, int q) {
  const int gy = q / lt.w[lv], gx = q - gy * lt.w[lv];
  const float st = (float)lt.stride[lv];
  const float half = rintf(st * 0.5f);
  const float ax0 = (float)(gx * lt.stride[lv]) - half, ay0 = (float)(gy * lt.stride[lv]) - half;
  const float ax1 = (float)(gx * lt.stride[lv]) + half, ay1 = (float)(gy * lt.stride[lv]) + half;
  PointAnchor a;
  a.cx = 0.5f * (ax0 + ax1);
  a.cy = 0.5f * (ay0 + ay1);
  a.bw = ax1 - ax0;
  a.bh = ay1 - ay0;
  return a;
}

// e = the ext head's relu'd (mag, dx, dy) -> (mag, 0.1 * dx / max(||(dx, dy)||, 1e-12), 0.1 * dy / ...)
__device__ __forceinline__ void ext_dxdymag(const float* e, float out[3]) {
  const float dx = e[1], dy = e[2];
  const float denom = fmaxf(sqrtf(dx * dx + dy * dy), 1e-12f);
  out[0] = e[0];
  out[1] = 0.1f * (dx / denom);
  out[2] = 0.1f * (dy / denom);
}

}  // namespace hn_fcos
