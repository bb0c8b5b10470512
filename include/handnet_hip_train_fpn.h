/*
 * handnet_hip_train_fpn.h -- the training-side entry points of libhandnet_hip.so for the backward of the FCOS FPN (DESIGN.md
 * section 9v): the weight and bias gradient of the 1x1 lateral convolutions and the adjoint of the top-down nearest-neighbour
 * read.  The 3x3 output convolutions' gradients reuse handnet_hip_train.h; this header adds functions only and no struct.
 *
 * Same library, same conventions as handnet_hip.h (device pointers borrowed from the caller, nothing allocates or
 * synchronises, all work goes to `stream`, 0 = success and hn_last_error() otherwise).  HN_ABI_VERSION stays 36.  Every refusal
 * happens before any launch and leaves the outputs untouched: channel counts off the rules below, a null pointer, zero rows or
 * an empty map, a pixel stride that breaks the kernels' 8-byte (S32 halves), S32-block or 16-byte (fp32) accesses, a workspace
 * below hn_conv1x1_wgrad_ws_bytes(), a coarse map larger than the fine one.  No entry point uses atomics or a memset; every
 * output element is written exactly once and two runs give the same bytes.
 */
#ifndef HANDNET_HIP_TRAIN_FPN_H
#define HANDNET_HIP_TRAIN_FPN_H

#include "handnet_hip_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- weight and bias gradient of a 1x1 / stride 1 convolution on the f32-input MFMA (csrc/conv1x1_wgrad_f32.hip) ----
 * a16 = the S32 activation the forward read ([rows][cin/32][2][32] fp16, value float(hi) + float(lo); a_pix_stride in halfs,
 * 0 = dense 2 cin), dy = the gradient at the convolution's output, fp32 [rows][cout] (dy_pix_stride in floats, 0 = dense cout);
 * rows = all pixels of all images of ONE map, a flat index.  cin and cout are multiples of 32, at most 512.
 *   dw[co][ci] = sum over the rows q of dy[q][co] * a[q][ci]          db[co] = sum of dy[..][co]
 * The rows are cut into consecutive ranges of whole 32-row chunks (the last one may be short); a dw element is ONE fmaf chain
 * over the rows of a range in row order (the MFMA's k order; a row past the end multiplies a staged zero), db a chain of plain
 * additions over the same partition; a second launch adds the ranges' partial sums in range order. */
int64_t hn_conv1x1_wgrad_ws_bytes(int64_t rows, int cin, int cout);   /* host-only; -1 for a problem the call refuses */
int hn_conv1x1_wgrad_f32(const void* a16, const float* dy, int64_t rows, int cin, int cout, int a_pix_stride, int dy_pix_stride,
                         float* dw, float* db, void* ws, int64_t ws_bytes, void* stream);

/* ---- adjoint of the nearest-neighbour read of a coarser map (csrc/upsample_bwd.hip) ----
 * The forward reads coarse pixel (floor(o rh / oh), floor(p rw / ow)) for fine pixel (o, p).  g = fp32 [n][oh][ow][c], the
 * gradient at the fine map; out = fp32 [n][rh][rw][c]; pixel strides in floats, 0 = dense c; c % 4 == 0; rh <= oh, rw <= ow.
 *   out[i][s][t][ch] = sum of g[i][o][p][ch] over the o with floor(o rh / oh) = s and the p with floor(p rw / ow) = t
 * as one fp32 chain of additions in (row, column) order, started from the first term.  One launch. */
int hn_upsample_nearest_backward_f32(const float* g, int n, int oh, int ow, int rh, int rw, int c, int g_pix_stride,
                                     int out_pix_stride, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
