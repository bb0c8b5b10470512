/*
 * handnet_hip_train.h -- the training-side entry points of libhandnet_hip.so that came after the inference header was
 * pinned: the backward of one FCOS tower layer (3x3 convolution -> GroupNorm -> ReLU).
 *
 * Same library, same conventions as handnet_hip.h (device pointers borrowed from the caller, nothing allocates or
 * synchronises, all work goes to `stream`, 0 = success and hn_last_error() otherwise).  HN_ABI_VERSION stays 36: functions
 * added, no struct of handnet_hip.h touched.  Every refusal happens before any launch and leaves the outputs untouched:
 * channel counts off the rules below, a null or empty level, a level count outside 1..HN_FCOS_MAX_LEVELS, a pixel or table
 * stride that breaks the kernels' 16-byte accesses, a workspace below the matching _ws_bytes().  No entry point uses atomics
 * or a memset; every output element is written exactly once and two runs give the same bytes.
 */
#ifndef HANDNET_HIP_TRAIN_H
#define HANDNET_HIP_TRAIN_H

#include "handnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- GroupNorm + ReLU backward over the levels of one tower layer (csrc/gn_relu_bwd.hip) ----
 * Per level l: y[l] = the raw convolution output, g[l] = the gradient at relu(y * scale + shift), dy[l] = the gradient at y,
 * all fp32 [n][h_l][w_l][c] (channel slices of wider tensors: the *_pix_stride arguments, in floats, 0 = dense c);
 * scale[l] / shift[l] = the forward's [n][c] tables (row stride table_stride floats, 0 = c); mean[l] / rstd[l] = dense
 * [n][groups] tables.  hn_groupnorm_stats_levels_f32 WRITES mean / rstd and reads y only; the backward reads them. */
typedef struct hn_gn_bwd_levels {
  int32_t count;
  int32_t h[HN_FCOS_MAX_LEVELS], w[HN_FCOS_MAX_LEVELS];
  const float* y[HN_FCOS_MAX_LEVELS];
  const float* g[HN_FCOS_MAX_LEVELS];
  const float* scale[HN_FCOS_MAX_LEVELS];
  const float* shift[HN_FCOS_MAX_LEVELS];
  float* mean[HN_FCOS_MAX_LEVELS];
  float* rstd[HN_FCOS_MAX_LEVELS];
  float* dy[HN_FCOS_MAX_LEVELS];
} hn_gn_bwd_levels;

/* Workspace of both GroupNorm entry points (host-only; -1 for a problem the calls refuse).  Only count, h[] and w[] are read.
 * c % 8 == 0, c <= 512, c % groups == 0, (c / groups) % 8 == 0. */
int64_t hn_groupnorm_relu_backward_ws_bytes(const hn_gn_bwd_levels* lv, int n, int c, int groups);

/* mean = sum(y) / M, rstd = 1 / sqrt(sum(y^2) / M - mean^2 + eps) per (level, image, group), M = h w c / groups (biased
 * variance, clamped at 0): fp32 partial sums per 64-pixel chunk in a fixed order, combined in fp64.  Two launches. */
int hn_groupnorm_stats_levels_f32(const hn_gn_bwd_levels* lv, int n, int c, int groups, int y_pix_stride, float eps, void* ws,
                                  int64_t ws_bytes, void* stream);

/* With z = fma(y, scale, shift) (the forward's own expression), gm = g where z > 0 else 0, xh = (y - mean) * rstd,
 * t = gm * gamma[ch] and, per (level, image, group), s1 = sum t, s2 = sum t * xh:
 *   dy          = rstd * (t - s1 / M - xh * s2 / M)
 *   d_gamma[ch] = sum over levels, images and pixels of gm * xh
 *   d_beta[ch]  = sum of gm
 * Three launches: per-(chunk, channel) partial sums, a fixed-order fp64 combine, the elementwise pass that writes dy. */
int hn_groupnorm_relu_backward_f32(const hn_gn_bwd_levels* lv, int n, int c, int groups, int y_pix_stride, int g_pix_stride,
                                   int dy_pix_stride, int table_stride, const float* gamma, float* d_gamma, float* d_beta,
                                   void* ws, int64_t ws_bytes, void* stream);

/* ---- weight and bias gradient of a 3x3 / stride 1 / pad 1 convolution on the f32-input MFMA (csrc/conv3x3_wgrad_f32.hip) ----
 * Per level l: a16[l] = the S32 activation the forward read ([n][h_l][w_l][cin/32][2][32] fp16, value float(hi) + float(lo);
 * a_pix_stride in halfs, 0 = dense 2 cin), dy[l] = the gradient at the convolution's output, fp32 [n][h_l][w_l][cout]
 * (dy_pix_stride in floats, 0 = dense cout).  cin and cout are multiples of 32, at most 512.
 *   dw[co][r][s][ci] = sum over levels, images and pixels q of dy[q][co] * a[q + (r - 1, s - 1)][ci]   (zero outside the map)
 *   db[co]           = sum of dy[..][co]
 * The pixels, in the order (level, image, row, column), are cut into consecutive ranges; a dw element is ONE fmaf chain over
 * the pixels of a range (the MFMA's k order), then the ranges' partial sums are added in range order by a second launch. */
typedef struct hn_wgrad_levels {
  int32_t count;
  int32_t h[HN_FCOS_MAX_LEVELS], w[HN_FCOS_MAX_LEVELS];
  const void* a16[HN_FCOS_MAX_LEVELS];
  const float* dy[HN_FCOS_MAX_LEVELS];
} hn_wgrad_levels;

int64_t hn_conv3x3_wgrad_ws_bytes(const hn_wgrad_levels* lv /* count, h[], w[] */, int n, int cin, int cout);
int hn_conv3x3_wgrad_f32(const hn_wgrad_levels* lv, int n, int cin, int cout, int a_pix_stride, int dy_pix_stride, float* dw,
                         float* db, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
