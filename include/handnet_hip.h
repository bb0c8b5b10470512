/*
 * handnet_hip.h -- C ABI of libhandnet_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the FCOS -> crop -> A2J inference hot path of
 * IRVLUTD/handnet-pipeline.  The reference has NO FFI / plugin layer of its own
 * (its only seam is the Python nn.Module callable handnet_pipeline.HandNet,
 * handnet_pipeline/handnet_pipeline.py:38-116), so each entry point below names the
 * reference Python call site whose arithmetic it replaces.  Host code
 * (handnet-pipeline_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; hn_last_error()
 *    returns a thread-local description of the last failure.
 *  - all pointers are DEVICE pointers borrowed from the caller unless noted; no
 *    function allocates, frees or synchronises; all work is enqueued on `stream`
 *    (a hipStream_t passed as void*; NULL = default stream), so calls can be
 *    captured into a hipGraph.
 *  - activations are NHWC fp32; conv weights are [Cout][R][S][Cin] fp32
 *    (Cin % 4 == 0; pad with zeros), already folded with their BatchNorm.
 *  - "fp32" here is exact: f32-input MFMA accumulates as a k-ordered fmaf chain.
 */
#ifndef HANDNET_HIP_H
#define HANDNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HN_OK 0
#define HN_ERR_ARG 1
#define HN_ERR_HIP 2

/* ABI version; bumped whenever a struct below changes (functions added without touching a struct or an existing signature
 * keep it: hn_lifter_input_gated_f32 and hn_mesh_render_u8 came under 36, and so did the mirror / handedness entries
 * hn_ingest_u8bgr_u16mm_flip, hn_flip_w_f32, hn_crop_resize_hands_sided, hn_a2j_aggregate_convert_mirror_f32,
 * hn_lifter_input_gated_mirror_f32 and hn_mesh_finish_mirror_f32, the tracked slots' hn_crop_resize_hands_tracked and
 * hn_track_state_bytes, the smoothed step's hn_mesh_finish_smooth_f32 and hn_smooth_state_bytes, the per-frame cameras'
 * hn_mesh_render_cams_u8 and hn_mesh_render_cams_occluded_u8, the rig frame's hn_rig_fuse_f32, the hand cloud's
 * hn_hand_cloud_f32 and hn_hand_cloud_scratch_bytes, the mesh fit's hn_mesh_fit_f32 and hn_mesh_fit_scratch_bytes, and the
 * iterated fit's hn_mesh_geometry_f32, hn_mesh_fit_iters_f32 and hn_mesh_fit_iters_scratch_bytes, and the carried apply pass's
 * hn_conv2d_nhwc_f16x3_grouped_carry, hn_conv2d_f16x3_grouped_carry_applies and hn_affine_split_f32_levels_streams, the evaluator's hn_hpe_accumulate_f32, the
 * detector evaluation's hn_det_ap_accumulate_f32, the A2J criterion's hn_a2j_aggregate_loss_f32, and the FCOS criterion's
 * hn_fcos_loss_f32 and hn_fcos_loss_ws_bytes, and the held objects' hn_hand_objects_f32, hn_hand_objects_scratch_bytes and
 * hn_draw_object_labels_u8, and the A2J criterion's backward hn_a2j_loss_grad_f32, and the FCOS criterion's backward
 * hn_fcos_loss_grad_f32). */
#define HN_ABI_VERSION 36
int hn_abi_version(void);
const char* hn_last_error(void);

/* Device facts used by bench.py (no allocation; queries the current device). */
int hn_device_info(int* cu_count, int* clock_khz, char* arch_name, int arch_name_len);
/* PCI bus id ("0000:c1:00.0") of the current device: what a rank of an N > 1 run reports so that N ranks on fewer than N
 * devices cannot pass as N GPUs (bench.py config.devices). */
int hn_device_pci_bus_id(char* out /* host */, int out_len /* >= 16 */);

/* ---- timing helper: HIP events on the caller's stream (bench.py roofline leg) ---- */
int hn_event_create(void** ev);
int hn_event_destroy(void* ev);
int hn_event_record(void* ev, void* stream);
int hn_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */

/* Shader clock UNDER LOAD: one wave compares s_memtime with s_memrealtime for `micros` microseconds and writes
 * the MHz figure to *mhz (device float).  Launch it on a side stream while the kernels of interest run
 * (bench.py roofline leg: roofline.clock_mhz); the sampling loop is bounded by real time. */
int hn_clock_sample(int micros, float* mhz, void* stream);

/* ---- f16x3 range contract ---------------------------------------------------------------------------------
 * A value that is stored in the split format must be finite and |v| <= 65504 (hi = fp16(v) would be +-inf).
 * While hn_range_check_enable(1) is in force (the engines' default; HN_CHECK_RANGE=0 turns it off for A/B timing) every
 * launch of a split PRODUCER (f16x3 conv epilogue / split-K tail, hn_affine_split_f32, hn_fcos_preprocess_split / _list,
 * hn_stem_image_nhwc4, and the lifter's hn_graph_conv_cheby3_f16x3 -- its in-kernel basis and its S32 output --,
 * hn_cheby3_basis_split and hn_pad_split_rows_f32) sets a sticky per-device flag word when it meets such a value:
 *   HN_RANGE_ACTIVATION        an intermediate activation (results would be inf / NaN or -- ReLU maps NaN to 0 -- silently
 *                              wrong: this model needs the exact f32 mode)
 *   HN_RANGE_INPUT             a finite INPUT value beyond the range (preprocessed RGB; a depth crop: depth is metres)
 *   HN_RANGE_INPUT_NONFINITE   a NaN / inf input value (invalid pixels of a 32FC1 depth image, which the reference passes
 *                              through, ros_demo.py:227-231; see hn_stem_image_nhwc4_valid)
 * The words live in a block of 4 device int32 (activation, input, input-non-finite, 0): the library's own, or -- after
 * hn_range_check_bind(block), which like the switch is read on the host at LAUNCH time -- the caller's (NULL unbinds).
 * The switch and the bound block are state of the calling HOST THREAD.  An engine brackets the launches of one step with
 * hn_range_scope_begin(block, on) / hn_range_scope_end(): inside the scope this thread's producers note into `block` (on = 0:
 * nowhere), afterwards the thread's previous switch and block are back -- so engines driven from different threads of one
 * process never see, redirect or switch off each other's flags, and scopes nest (at most 8 deep).
 * hn_range_check_collect enqueues ONE tiny kernel on `stream` that copies the words of `block` (NULL: the library's) to
 * dst[0..3] and clears them -- no synchronisation; the host reads dst with the copy of the results it makes anyway (the
 * drop-in HandNet.forward does).  hn_range_check_fetch is the synchronous form: *flag (host)
 * = OR of the HN_RANGE_* bits, optionally clearing them.  Weight banks are checked on the host when they are split
 * (hn_amd.weights.split_f16x3 raises; hn_finalize fails). */
#define HN_RANGE_ACTIVATION 1
#define HN_RANGE_INPUT 2
#define HN_RANGE_INPUT_NONFINITE 4
int hn_range_check_enable(int on);
int hn_range_check_enabled(void);
int hn_range_check_fetch(int* flag /* host */, int reset, void* stream);
int hn_range_check_bind(int32_t* block /* device, 4 words, zeroed by the caller; or NULL */);
int hn_range_scope_begin(int32_t* block /* device, 4 words; NULL with on = 1: the library's block */, int on);
int hn_range_scope_end(void);
int hn_range_check_collect(int32_t* block /* or NULL */, int32_t* dst /* device, 4 words */, void* stream);

/* Kernel-form switches.  Older forms of some kernels stay in the library as bit-identity references for the tests and for
 * same-box A/B timing ("conv_no_rs", "conv_no_rs32", "split_generic", "conv_no_halo", "preprocess_generic",
 * "conv_no_multi", "no_fuse_last_gn", "no_thin_outputs", "thin_form_tap", "thin_form_flat", "halo_stamps", "splitk_fill512",
 * "conv_no_stream", "conv_no_mixed", "conv_no_deepk", "conv_no_fused_reduce"; results unchanged
 * unless a test says otherwise).  The library NEVER reads them from the environment: a development host sets them by name
 * (bench.py and tools/ translate their HN_* variables through hn_amd/forms.py); a product process leaves them alone. */
int hn_set_form(const char* name, int value);
/* Debug / test: the number of split-K ticket counters of the CURRENT device that are not zero.  SYNCHRONISES the device.  The
 * in-kernel split-K reduction (hn_conv2d_nhwc_f16x3_ws, _multi) draws tickets from library-owned counters that are zero at rest:
 * after any sequence of completed launches the answer is 0; anything else means a launch died between drawing a ticket and
 * putting it back (the next split launch on that workspace would then never elect a reducing workgroup). */
int hn_debug_tickets_nonzero(int64_t* count /* host */);
/* Development: scale factor (default 1.0) of a constant of the split-K cost model -- "splitk_fix", "splitk_tk", "splitk_red0",
 * "splitk_plane" (csrc/conv_igemm_f16x3.hip: plan_splits) -- for in-frame scans of the model; never set by the product. */
int hn_set_tuning(const char* name, double value);

/* ------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on f32 / f16 MFMA), fused epilogue.
 * Replaces: torch.nn.Conv2d + (Frozen)BatchNorm2d + ReLU + residual add at
 *   a2j/resnet.py:78-96 (Bottleneck), a2j/a2j.py:70-89,116-135,162-181 (heads),
 *   tv resnet34 BasicBlock / FPN called at fcos_utils/fcos.py:737,
 *   fcos_utils/fcos.py:276-289,377-380 (FCOS towers / outputs; GroupNorm of the
 *   PREVIOUS layer is applied on load via in_scale/in_shift).
 * ------------------------------------------------------------------------------------ */
typedef struct hn_conv_desc {
  int32_t n, h, w, cin;      /* input  [n][h][w][cin], cin % 4 == 0                      */
  int32_t cout;              /* output channels (any >= 1)                               */
  int32_t r, s;              /* filter taps                                              */
  int32_t stride, pad, dil;
  int32_t oh, ow;            /* output spatial size (caller computes; checked)           */
  int32_t relu_cols;         /* ReLU on output channels [0, relu_cols); 0 = none         */
  int32_t res_mode;          /* 0 none | 1 residual[n][oh][ow][cout] |
                                2 residual[n][res_h][res_w][cout] read at (oh*res_h/oh.., nearest) */
  int32_t res_h, res_w;      /* residual spatial size for res_mode 2                     */
  int32_t in_affine;         /* 1: x <- relu(x*in_scale[img][c] + in_shift[img][c]) on load
                                 (f32 kernel only)                                        */
  int32_t tile;              /* 0 = auto; else one of HN_TILE_*                          */
  int32_t out_split;         /* 1: write y in the S32 split format (cout % 32 == 0)      */
  int32_t res_split;         /* 1: residual is an S32 tensor (f16x3 kernel only)         */
  int32_t res_pix_stride;    /* elements between residual pixels; 0 = dense              */
  int32_t in_pix_stride;     /* elements between consecutive input pixels; 0 = dense.  Lets a
                                 conv read a channel slice of a wider tensor (pass the slice's
                                 first element).  fp32: floats (multiple of 4); S32: halfs
                                 (2 x parent channels)                                     */
  int32_t out_pix_stride;    /* elements between consecutive output pixels; 0 = dense    */
  int32_t in_affine_stride;  /* floats between rows of in_scale / in_shift; 0 = cin     */
  int32_t splitk;            /* f16x3 + workspace: 0 = split-K only for long k loops (an extra launch
                              * per conv costs eager callers more than it saves), 1 = also for short
                              * ones (launch cost hidden, e.g. under hipGraph replay), -1 = never; >= 2 = exactly that many
                              * splits, whatever the grid (sweeps: tools/splitk_sweep.py) */
  int32_t terms;             /* f16x3 kernels: 0 / 3 = the three-term split product (fp32-grade, the default);
                              * 1 = hi*hi only ("f16x1": plain fp16 operands, ONE MFMA per MAC, same data movement) --
                              * the throughput mode SURVEY D6 plans beside the parity mode; misses the 1e-3 keypoint
                              * contract by two orders and is reported beside the headline, never as it */
} hn_conv_desc;

#define HN_TILE_AUTO 0
#define HN_TILE_128x128 1
#define HN_TILE_128x64 2
#define HN_TILE_64x64 3
#define HN_TILE_128x32 4
/* 5 (256x128), 9 (256x128 with 8 waves), 10 (256x64 with 8 waves), 11 (128x256 with 8 waves): sweep-only forms of rounds 1-4,
 * retired in round 5 (measured and not taken: profiles/r04_tile_128x256.txt, profiles/NOTEBOOK.md); the ids stay reserved */
#define HN_TILE_64x128 6
#define HN_TILE_32x64 7   /* f16x3 only: 2-wave workgroups for small-M layers */
#define HN_TILE_256x64 8  /* f16x3 only: Cout <= 64 layers with 64x64 wave tiles (4 waves stacked along M) */
/* f16x3 only, round 5: the "deep k" form of the 64x64 tile for grids of at most one workgroup per CU (ResNet-34 layer3 at batch
 * 1): a ring stage holds TWO k tiles and the loop has one barrier per stage instead of one per tile; bit-identical to
 * HN_TILE_64x64; the auto heuristic picks it for such grids with at least 8 k tiles ("conv_no_deepk" turns that off).  Members of
 * a heterogeneous launch whose tile is 64x64 share its kernel. */
#define HN_TILE_64x64_K2 12

int hn_conv2d_nhwc_f32(const hn_conv_desc* d, const float* x, const float* w,
                       const float* bias /* [cout] or NULL */,
                       const float* residual /* or NULL */,
                       const float* in_scale, const float* in_shift /* [n][cin] or NULL */,
                       float* y, void* stream);

/* Tile id (HN_TILE_*) the auto heuristic picks for this shape (host-only; for tests/plans). */
int hn_conv2d_pick_tile(const hn_conv_desc* d);

/* Same convolution on the f16 MFMA with SPLIT operands: every fp32 value v = hi + lo,
 * hi = fp16(v), lo = fp16(v - hi); a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi accumulated in
 * fp32 (fp32-grade result, 16/3 x the f32-MFMA rate).  The input is an S32 split tensor
 * (below), written once by its producer; w16 is the filter bank split on the host the same
 * way: fp16 [cout][(cin/32)*r*s][2][32] (k tiles: 32-channel block outer, tap (r,s) inner;
 * hi run | lo run per tile).  Requires cin % 32 == 0.
 * GroupNorm-on-load (in_affine) is not available here: run hn_affine_split_f32 in between. */
int hn_conv2d_nhwc_f16x3(const hn_conv_desc* d, const void* x16 /* S32 */, const void* w16,
                         const float* bias, const void* residual /* fp32 or S32 */,
                         void* y /* fp32 or S32 (d->out_split) */, void* stream);
int hn_conv2d_f16x3_pick_tile(const hn_conv_desc* d);
/* 1 when a single-pass launch of this descriptor runs the row-shared-A kernels (3x3 / stride 1 / pad 1 / dilation 1 on the
 * 128x128, 128x64 or 128x32 tile, image rows long enough for the gap slots; HN_CONV_NO_RS=1 turns them off): the A
 * operand of a filter row is staged once and the three taps read it at slot offsets.  Same results bit for bit; the
 * profilers' kernel names differ (template argument RS), which is what bench.py asks this for.  For a grouped launch pass
 * the smallest member width in d->w and the picked tile in d->tile. */
int hn_conv2d_f16x3_uses_rs(const hn_conv_desc* d);
/* 1 when hn_conv2d_nhwc_f16x3(_ws) routes this descriptor to the halo-patch kernel (3x3 / stride 1 / pad 1, 64 output channels,
 * S32 in and out, ReLU, optional S32 residual of the output's shape, at least 512 tiles of 16 x 16 pixels; HN_CONV_NO_HALO=1
 * turns it off): a workgroup stages the 18 x 18 input patch of a 32-channel block once and reads all nine taps from it.
 * Same k order as the implicit-GEMM kernel: bit-identical results (ResNet-34 layer1, fcos_utils/fcos.py:737). */
int hn_conv2d_f16x3_uses_halo(const hn_conv_desc* d, int has_residual);
/* 1 when hn_conv2d_nhwc_f16x3(_ws) routes this descriptor to the streaming kernel for short-k 1x1 layers (1x1 / stride 1 / pad 0,
 * cin 64 or 128, cout % 256 == 0, dense S32 input, ReLU on all columns or none, at least 65536 output pixels; "conv_no_stream"
 * turns it off): a wave keeps the filter fragments of its 32 output channels in registers for the whole launch and the
 * activations are streamed through LDS once.  Same k order and epilogue arithmetic as the implicit-GEMM kernel: bit-identical
 * results (the FPN P3 lateral via fcos_utils/fcos.py:737, the bottleneck expansions of a2j/resnet.py:78-96 at batch >= ~32). */
int hn_conv2d_f16x3_uses_stream(const hn_conv_desc* d);

/* ---- S32 split activation format: fp16 [N][H][W][C/32][2][32] (hi[32] | lo[32] per block) ----
 * hn_affine_split_f32: fp32 NHWC -> S32; with scale/shift [n][c] it first applies
 *   y = x*scale[img][c] + shift[img][c] (the GroupNorm(32,256) of fcos_utils/fcos.py:232-239,
 *   352-359 expressed as a per-(image, channel) affine) and, if relu, max(y, 0).
 * hn_unsplit_f32: S32 -> fp32 (exact: hi + lo).   hn_maxpool3x3s2_s32: pooling on S32. */
int hn_affine_split_f32(const float* x, const float* scale, const float* shift, int relu,
                        int n, int hw, int c, int in_pix_stride, int affine_stride,
                        void* y16, int out_pix_stride, void* stream);
int hn_unsplit_f32(const void* x16, int n, int hw, int c, int in_pix_stride,
                   float* y, int out_pix_stride, void* stream);
int hn_maxpool3x3s2_s32(const void* x16, void* y16, int n, int h, int w, int c,
                        int oh, int ow, void* stream);

/* 3x3 / stride-2 / pad-1 max pooling, NHWC fp32 (c % 4 == 0).
 * Replaces nn.MaxPool2d at a2j/resnet.py:107,158 and tv resnet34 stem. */
int hn_maxpool3x3s2_nhwc_f32(const float* x, float* y, int n, int h, int w, int c,
                             int oh, int ow, void* stream);

/* ------------------------------------------------------------------------------------
 * GroupNorm statistics -> per-(image, channel) affine, consumed by the next conv's
 * in_scale / in_shift.  Replaces nn.GroupNorm(32, 256) + ReLU at
 * fcos_utils/fcos.py:232-239,352-359 (eps 1e-5, biased variance over group x H x W).
 *   scale[img][c] = gamma[c] * rstd[img][g],  shift[img][c] = beta[c] - mean*scale
 * `partial` is caller scratch of hn_groupnorm_scratch_floats(...) floats.
 * ------------------------------------------------------------------------------------ */
int64_t hn_groupnorm_scratch_floats(int n, int hw, int c, int groups);
int hn_groupnorm_affine_f32(const float* x /* [n][hw][c] */, const float* gamma,
                            const float* beta, int n, int hw, int c, int groups, float eps,
                            float* partial, float* scale, float* shift, void* stream);

/* hn_conv2d_nhwc_f16x3 with a caller-provided workspace (fp32 scratch, 16-byte aligned, any size; only used
 * between this call's own launches, so one buffer per stream serves all convolutions).  With it, layers
 * whose output grid would leave most CUs idle (n*oh*ow small: the 11x11 A2J maps, everything at batch 1)
 * run split-K: up to 16 workgroups share an output tile, partial tiles are summed in a fixed order -- for the 32- / 64-row
 * tiles by the workgroup that finishes a tile last (a ticket per tile in library-owned device memory, keyed by the workspace
 * ADDRESS: as before, launches that may be in flight together must not share a workspace), otherwise by a second launch;
 * the results are bit-identical either way ("conv_no_fused_reduce" forces the second launch). */
int hn_conv2d_nhwc_f16x3_ws(const hn_conv_desc* desc, const void* x16, const void* w16,
                            const float* bias, const void* residual, void* y,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* Up to HN_CONV_MAX_GROUP convolutions that share ONE descriptor (identical channels, filter, batch, strides and epilogue
 * flags -- only the spatial size may differ per member; no residual, no split-K) as a single launch: member g reads x16[g] / w16[g] / bias[g] (bias may be NULL) and writes
 * y[g]; gn_partial[g] is either given for every member (semantics of hn_conv2d_nhwc_f16x3_gn) or NULL for all.
 * Used for the cls / reg tower layers of an FPN level (fcos.py:276,377) and the three A2J head layers
 * (a2j/a2j.py:70-181), which are independent and identical in shape. */
#define HN_CONV_MAX_GROUP 6
typedef struct hn_conv_group {
  int32_t count;
  const void* x16[HN_CONV_MAX_GROUP];
  const void* w16[HN_CONV_MAX_GROUP];
  const float* bias[HN_CONV_MAX_GROUP];
  void* y[HN_CONV_MAX_GROUP];
  float* gn_partial[HN_CONV_MAX_GROUP];
  int32_t h[HN_CONV_MAX_GROUP], w[HN_CONV_MAX_GROUP];  /* per-member input size; 0 = the descriptor's (members may be the
                      * FPN levels of one layer: same channels / filter / batch, different maps) */
  int32_t gn_units;  /* 8-channel units per 32-row group in the GroupNorm slab; 0 = cout/8.  With y[g] / gn_partial[g]
                      * pointing at channel offset g*cout of ONE [rows][count*cout] tensor / slab (desc.out_pix_stride =
                      * count*cout, gn_units = count*cout/8) the members' outputs stay stacked, so one
                      * hn_groupnorm_finalize_rows32 and one hn_affine_split_f32 serve all of them. */
} hn_conv_group;
int hn_conv2d_nhwc_f16x3_grouped(const hn_conv_desc* desc, const hn_conv_group* group, void* stream);

/* Up to HN_CONV_MULTI_MAX INDEPENDENT convolutions of DIFFERENT shapes as one launch (plus one reduction launch for all their
 * split-K members): each member has its own descriptor (channels, filter, stride, dilation, residual, ReLU, output format,
 * splitk mode) and tensors, exactly as for hn_conv2d_nhwc_f16x3_ws, and computes exactly what that call would -- same
 * kernel body, same k order, the split-K plan it would get alone -- so results are bit-identical to separate calls.
 * The members run together when each of them alone would take the implicit-GEMM kernel of one common tile form
 * (hn_conv2d_f16x3_pick_tile); otherwise, or with HN_CONV_NO_MULTI=1, the call issues them one after the other.
 * Used where the layer graph has independent small grids: the 1x1 downsample beside conv1 of a residual block
 * (a2j/resnet.py:78-96, tv BasicBlock), the classification head beside layer4 of the A2J trunk (a2j/a2j.py:194-210,
 * 226-250).  No member may read another member's output. */
#define HN_CONV_MULTI_MAX 4
typedef struct hn_conv_multi {
  int32_t count;
  hn_conv_desc desc[HN_CONV_MULTI_MAX];
  const void* x16[HN_CONV_MULTI_MAX];
  const void* w16[HN_CONV_MULTI_MAX];
  const float* bias[HN_CONV_MULTI_MAX];      /* or NULL */
  const void* residual[HN_CONV_MULTI_MAX];   /* or NULL */
  void* y[HN_CONV_MULTI_MAX];
} hn_conv_multi;
int hn_conv2d_nhwc_f16x3_multi(const hn_conv_multi* mm, void* workspace, int64_t workspace_bytes, void* stream);
/* 1 when the call above would run these members as ONE launch (host-only). */
int hn_conv2d_f16x3_multi_fuses(const hn_conv_multi* mm, int64_t workspace_bytes);

/* Fused variant for the f16x3 path: hn_conv2d_nhwc_f16x3_gn is hn_conv2d_nhwc_f16x3 (fp32 output, no
 * residual / ReLU, cout % 8 == 0, oh*ow >= 32) whose epilogue also writes GroupNorm partial sums
 * gn_partial [ceil(n*oh*ow / 32)][cout/8][4] (hn_groupnorm_rows32_scratch_floats floats);
 * hn_groupnorm_finalize_rows32 reduces them to the same scale / shift tables as hn_groupnorm_affine_f32
 * without re-reading the conv output. */
int hn_conv2d_nhwc_f16x3_gn(const hn_conv_desc* desc, const void* x16, const void* w16,
                            const float* bias, void* y, float* gn_partial, void* stream);
int64_t hn_groupnorm_rows32_scratch_floats(int64_t rows, int c);
int hn_groupnorm_finalize_rows32(const float* partial, const float* gamma, const float* beta,
                                 int n, int hw, int c, int groups, float eps,
                                 float* scale, float* shift, void* stream);

/* The GroupNorm finalize / apply passes of ONE tower layer for all FPN levels at once (the tower weights and the
 * GroupNorm affine are shared across levels, fcos_utils/fcos.py:276-289,377-380; the levels differ in map size only).
 * Same arithmetic and bits as hn_groupnorm_finalize_rows32 / hn_affine_split_f32 per level; one launch instead of
 * `count` (at batch 1 every launch of this size is pure latency).  hn_affine_split_f32_levels falls back to the
 * per-level launches when a level is too large for any cache (>= 128 MiB), where the streaming-store form wins. */
#define HN_FCOS_MAX_LEVELS 5
typedef struct hn_gn_levels {
  int32_t count;
  int32_t hw[HN_FCOS_MAX_LEVELS];            /* pixels per image of each level (>= 32)        */
  const float* partial[HN_FCOS_MAX_LEVELS];  /* conv-epilogue partial sums of each level       */
  float* scale[HN_FCOS_MAX_LEVELS];          /* out: [n][c] per level                          */
  float* shift[HN_FCOS_MAX_LEVELS];
} hn_gn_levels;
int hn_groupnorm_finalize_rows32_levels(const hn_gn_levels* lv, const float* gamma, const float* beta,
                                        int n, int c, int groups, float eps, void* stream);
typedef struct hn_split_levels {
  int32_t count;
  int32_t hw[HN_FCOS_MAX_LEVELS];
  const float* x[HN_FCOS_MAX_LEVELS];        /* fp32 [n][hw][c] (pixel stride in_pix_stride)   */
  const float* scale[HN_FCOS_MAX_LEVELS];    /* [n][c] tables (row stride affine_stride)       */
  const float* shift[HN_FCOS_MAX_LEVELS];
  void* y16[HN_FCOS_MAX_LEVELS];             /* out: S32 [n][hw][c/32][2][32]                  */
} hn_split_levels;
int hn_affine_split_f32_levels(const hn_split_levels* lv, int relu, int n, int c, int in_pix_stride,
                               int affine_stride, int out_pix_stride, void* stream);
/* 1 when a level of this size makes the call above an HBM stream (per-level launches with streaming stores); host-only. */
int hn_affine_split_f32_levels_streams(const int32_t* hw, int count, int n, int c);

/* hn_conv2d_nhwc_f16x3_grouped that CARRIES hn_affine_split_f32_levels(lv, relu, n, c, ...) in ONE launch: every convolution
 * workgroup, its output tile stored, streams a slice of the apply pass and leaves -- the pass (an HBM stream) runs under the
 * matrix work of the other workgroups instead of after it.  The levels' tensors must be complete before the call and must not
 * be read or written by the convolution (the cls tower's launch carries the reg tower's pass and the other way round); their
 * n / c / levels are their own (c = 32 .. 2048, a power of two; 16-byte aligned pointers).  Same bits as the two calls one after
 * the other.  Only the plain row-shared 128 x 128 form of the grouped launch carries: for any other shape the call fails with
 * HN_ERR_ARG before it launches anything (hn_conv2d_f16x3_grouped_carry_applies() == 0, host-only) and the caller runs the
 * separate pass. */
int hn_conv2d_nhwc_f16x3_grouped_carry(const hn_conv_desc* desc, const hn_conv_group* group, const hn_split_levels* lv,
                                       int relu, int n, int c, int in_pix_stride, int affine_stride, int out_pix_stride,
                                       void* stream);
int hn_conv2d_f16x3_grouped_carry_applies(const hn_conv_desc* desc, const hn_conv_group* group);

/* The FCOS head OUTPUT convolutions (cls_logits + hand_lr, bbox_reg + bbox_ctrness, the ext heads: fcos_utils/fcos.py:
 * 247-264,299-320,362-363): 3x3 / stride 1 / pad 1, cin % 32 == 0, 1 <= cout <= 16, the same filter on every FPN level,
 * all levels in ONE launch.  x16[l] = S32 input of level l (a channel slice of a wider tensor: in_pix_stride in halfs,
 * 0 = dense), y[l] = fp32 [n][h_l][w_l][cout] dense, ReLU on channels [0, relu_cols).  Two kernels (csrc/conv3x3_thin.hip):
 *   - cout <= 5, cin % 128 == 0, level width <= ~170, >= 65536 pixels in all (hn_conv3x3_thin_uses_flat() == 1): the P form -- one GEMM
 *     P[(tap, oc)][pixel] over the flat pixel list, every input pixel read from HBM once, then nine shifted adds per output
 *     from an LDS ring.  Same products as the implicit GEMM, summed per tap first: equal to fp32 rounding, not bit for bit;
 *   - otherwise the tap kernel: 16 x 16 pixel tiles, the implicit GEMM's k / term order, bit-identical to
 *     hn_conv2d_nhwc_f16x3_grouped on the same operands. */
typedef struct hn_thin_levels {
  int32_t count;
  const void* x16[HN_FCOS_MAX_LEVELS];
  float* y[HN_FCOS_MAX_LEVELS];
  int32_t h[HN_FCOS_MAX_LEVELS], w[HN_FCOS_MAX_LEVELS];
} hn_thin_levels;
int hn_conv3x3_thin_f16x3_levels(const hn_thin_levels* lv, int n, int cin, int cout, const void* w16, const float* bias,
                                 int relu_cols, int in_pix_stride, void* stream);
int hn_conv3x3_thin_uses_flat(const hn_thin_levels* lv, int n, int cin, int cout);   /* only count, h[] and w[] are read */

/* Up to three such convolutions -- different filter banks on their own inputs: the FCOS head outputs cls_logits + hand_lr, the
 * ext heads, bbox_reg + ctrness (fcos.py:255-264,299-320) -- in ONE launch where they run the tap kernel (a single frame: 89
 * workgroups each on 256 CUs, latency-bound at 17-18 us per launch; together one round of the chip).  Every workgroup runs
 * exactly what its member's own launch would have run: bit-identical to `count` calls of hn_conv3x3_thin_f16x3_levels, which is
 * also what happens where a member takes the P form (large pixel counts: HBM-bound streams) or for count == 1. */
typedef struct hn_thin_member {
  hn_thin_levels lv;
  int32_t cout, relu_cols;
  const void* w16;
  const float* bias;
} hn_thin_member;
int hn_conv3x3_thin_f16x3_levels_group(const hn_thin_member* members, int count /* 1..3 */, int n, int cin, int in_pix_stride,
                                       void* stream);

/* The P form with the LAST GroupNorm apply pass of the towers fused in (fcos.py:232-239 conv -> GroupNorm -> ReLU, then the
 * output conv): x[l] = RAW fp32 conv output [n][h_l][w_l][in_pix_stride] at the head's first channel, scale[l] / shift[l] =
 * the tables of hn_groupnorm_finalize_rows32 [n][affine_stride] at the same channel; the kernel computes relu(x * scale +
 * shift), splits it into fp16 hi + lo in registers (hn_affine_split_f32's arithmetic) and convolves: bit-identical to
 * hn_affine_split_f32_levels + hn_conv3x3_thin_f16x3_levels, without the 8 bytes per element the separate pass moves.
 * lv->x16 is ignored; lv->y / h / w as above.  Only where hn_conv3x3_thin_affine_applies() == 1. */
typedef struct hn_thin_affine {
  const float* x[HN_FCOS_MAX_LEVELS];
  const float* scale[HN_FCOS_MAX_LEVELS];
  const float* shift[HN_FCOS_MAX_LEVELS];
  int32_t in_pix_stride;   /* floats per pixel of x */
  int32_t affine_stride;   /* floats per image row of scale / shift */
} hn_thin_affine;
int hn_conv3x3_thin_affine_applies(const hn_thin_levels* lv, int n, int cin, int cout);
int hn_conv3x3_thin_affine_f16x3_levels(const hn_thin_levels* lv, const hn_thin_affine* aff, int n, int cin, int cout,
                                        const void* w16, const float* bias, int relu_cols, void* stream);

/* The BACKWARD of those output convolutions (csrc/conv3x3_thin_bwd.hip), fp32, for the one or two
 * filter banks ("members") that read one map: lv->x16[l] = the S32 activation the forward read (a = float(hi) + float(lo);
 * channel slices: in_pix_stride in halfs, 0 = dense), lv->h / w its sizes, lv->y[l] = where the gradient at that activation
 * goes (fp32, dx_pix_stride floats per pixel, 0 = dense cin; written at channel dx_channel_offset .. + cin) or NULL on EVERY
 * level for none.  Per member m: couts[m] <= 16 (at most 16 together), relu_cols[m], w[m] = fp32 [cout][3][3][cin] (the
 * unsplit bank), and per level y[m * count + l] = the forward's own output and g[m * count + l] = the upstream gradient, both
 * fp32 [n][h_l][w_l][cout_m] dense.  With gm = g where (column >= relu_cols or y > 0), else 0 (torch's ReLU backward on the
 * stored result):
 *   dw[m][co][r][s][ci] = sum over levels, images and pixels of gm[y][x][co] * a[y + r - 1][x + s - 1][ci]   (zero padding)
 *   db[m][co]           = sum of gm[..][co]
 *   dA_l[y][x][ci]      = sum over members, co, r, s of gm[y - r + 1][x - s + 1][co] * w[m][co][r][s][ci]
 * Two launches: a sweep (partial sums per workgroup into `ws`) and a fixed-order reduction.  Every output element is written
 * exactly once, zeros included; no memset, no atomics; the same bytes on every run.  Every refusal (cin % 32, cout > 16, more
 * than two members or 16 columns on a map, a null level, a workspace below hn_conv3x3_thin_backward_ws_bytes(), which is
 * host-only and returns -1 for a problem the call refuses) happens before any launch.  Added under ABI 36: new functions only. */
int64_t hn_conv3x3_thin_backward_ws_bytes(const hn_thin_levels* lv /* count, h[], w[] */, int n, int cin, int members,
                                          const int32_t* couts);
int hn_conv3x3_thin_backward_f32(const hn_thin_levels* lv, int n, int cin, int in_pix_stride, int members, const int32_t* couts,
                                 const int32_t* relu_cols, const float* const* w, const float* const* y, const float* const* g,
                                 float* const* dw, float* const* db, int dx_pix_stride, int dx_channel_offset, void* ws,
                                 int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Caller-side ingest, fused: what ros_demo.py:227-231,266-269 does on the host before it calls the network --
 *   bgr8 HWC uint8 -> cv2.COLOR_BGR2RGB -> transpose(2,0,1) -> float32 / 255.0        -> rgb    [n][3][h][w]
 *   16UC1 depth in millimetres -> float32 / 1000.0 (32FC1 metres: passed through)      -> depth_m [n][1][h][w]
 *   RGB-D model: torch.cat([rgb, depth], dim=1)                                        -> rgbd   [n][4][h][w]
 * bgr [n][h][w][3] uint8 and depth [n][h][w] (depth_kind 1: uint16 mm, 2: float32 m, 0: none / NULL) only have to be
 * READABLE by the device: device memory, or pinned host memory read over PCIe by the kernel itself (1.5 MB per 640x480
 * frame instead of the 4.9 MB of the fp32 feed).  rgb / depth_m / rgbd are device tensors; any of them may be NULL if
 * not wanted (rgbd needs a depth input).  IEEE float32 divisions: bit-identical to the reference's numpy arithmetic.
 * ------------------------------------------------------------------------------------ */
int hn_ingest_u8bgr_u16mm(const uint8_t* bgr, const void* depth, int depth_kind, float* rgb, float* depth_m,
                          float* rgbd, int n, int h, int w, void* stream);
/* The same with the caller's `left` mode (ros_demo.py:259-262: cv2.flip(., 1) of the colour frame and of the depth map before
 * anything else): flip_w != 0 -- output column x is source column w - 1 - x in every output, in the same one launch (a lane
 * reads the mirrored twelve bytes and swaps its four pixels in registers; w % 4 != 0 takes the per-pixel path).  flip_w == 0
 * is hn_ingest_u8bgr_u16mm.  Added under ABI 36: a new function only. */
int hn_ingest_u8bgr_u16mm_flip(const uint8_t* bgr, const void* depth, int depth_kind, float* rgb, float* depth_m,
                               float* rgbd, int n, int h, int w, int flip_w, void* stream);
/* The mirror for fp32 feeds, ONE launch over two tensors of rows of w floats: a_out[r][x] = a[r][w - 1 - x] for rows_a rows,
 * and the same for b -> b_out (rows_b rows; b = b_out = NULL and rows_b = 0: one tensor).  Not in place.  16-byte loads and
 * stores, reversed in registers, when w % 4 == 0 and the pointers are 16-byte aligned.  Added under ABI 36. */
int hn_flip_w_f32(const float* a, float* a_out, int64_t rows_a, const float* b, float* b_out, int64_t rows_b, int w,
                  void* stream);

/* ------------------------------------------------------------------------------------
 * FCOS pre-processing: normalize + bilinear resize (align_corners=False, scale =
 * in/out as with recompute_scale_factor=True) + zero pad, NCHW fp32 in -> NHWC(4) out.
 * Replaces torchvision GeneralizedRCNNTransform called at fcos_utils/fcos.py:709.
 * src [n][3][h][w], dst [n][ph][pw][4] (channel 3 = 0, rows >= oh / cols >= ow = 0).
 * ------------------------------------------------------------------------------------ */
int hn_fcos_preprocess_f32(const float* src, float* dst, int n, int h, int w,
                           int oh, int ow, int ph, int pw,
                           const float mean[3], const float stdv[3], void* stream);

/* Split-precision stem path.  hn_fcos_preprocess_split is hn_fcos_preprocess_f32 with the output stored as
 * the stem image of hn_conv_stem_f16x3: two fp16 planes (hi then lo, hi + lo = the fp32 value to 2^-22) of
 * [n][ph + 2*border][pw + 2*border][4], zero outside the resized image (border, padding, channel 3).
 * hn_conv_stem_f16x3 runs the R x R / stride convolution (pad = border = R/2, R <= 8; torchvision resnet
 * conv1 at fcos_utils/fcos.py:737) on the f16x3 kernel: w16 is fp16 [cout][R][2][32] with k = kx*4 + c inside
 * a filter row (hn_amd.weights.pack_stem_split); y is [n][oh][ow][cout] fp32 or S32 (out_split). */
int hn_fcos_preprocess_split(const float* src, void* dst16, int n, int h, int w, int oh, int ow,
                             int ph, int pw, int border, const float mean[3], const float stdv[3],
                             void* stream);
/* Batches of differently sized images (torchvision batch_images, fcos_utils/fcos.py:702-709): srcs = DEVICE
 * array of n device pointers to [3][h_i][w_i] images, geom = DEVICE int32 [n][4] = {h_i, w_i, oh_i, ow_i};
 * each image is resized on its own into the top-left corner of the common zero canvas.
 * split = 0: dst = fp32 [n][ph][pw][4]; split = 1: dst = the stem image (border as above). */
int hn_fcos_preprocess_list(const float* const* srcs, const int32_t* geom, void* dst, int split, int n,
                            int ph, int pw, int border, const float mean[3], const float stdv[3],
                            void* stream);
int hn_conv_stem_f16x3(const void* x16, int n, int ph, int pw, int pad, int r, int stride, int cout,
                       const void* w16, const float* bias, int relu, void* y, int out_split,
                       void* stream);
/* The stem with the ResNet's 3x3 / stride-2 / pad-1 max pooling fused into its epilogue (conv1 -> bn1 -> relu -> maxpool of
 * torchvision resnet34, fcos_utils/fcos.py:737): cout = 64, ReLU on, y = the POOLED S32 map [n][(oh+1)/2][(ow+1)/2][64].
 * Bit-identical to hn_conv_stem_f16x3 followed by hn_maxpool3x3s2_s32; the half-resolution conv map (1.8 GB at batch
 * 32) never reaches HBM.  Written for the 7x7 / stride-2 / pad-3 ResNet stem (r = 7, stride = 2, pad = 3), the only stem of this
 * path: other filter geometries are refused (run hn_conv_stem_f16x3 + hn_maxpool3x3s2_s32). */
int hn_conv_stem_pool_f16x3(const void* x16, int n, int ph, int pw, int pad, int r, int stride, int cout,
                            const void* w16, const float* bias, void* y, void* stream);
/* hn_conv_stem_pool_f16x3 with the term count of hn_conv_desc.terms (1 = the f16x1 throughput mode). */
int hn_conv_stem_pool_f16x3_terms(const void* x16, int n, int ph, int pw, int pad, int r, int stride, int cout,
                                  const void* w16, const float* bias, void* y, int terms, void* stream);

/* ------------------------------------------------------------------------------------
 * FCOS post-processing.  Replaces fcos_utils/fcos.py:572-659 (postprocess_detections),
 * det_utils.py:266-294 (BoxLinearCoder.decode_single), anchor_utils.py:82-132,
 * torchvision.ops.batched_nms (call site fcos.py:635) and resize_boxes fcos.py:770-783.
 *
 * Head tensors are the raw conv outputs per level, NHWC:
 *   cls_lr[l]  [n][h_l][w_l][num_classes + 2]   (cls_logits then hand_lr)
 *   reg_ctr[l] [n][h_l][w_l][5]                 (relu(bbox_reg)[4] then ctrness)
 * Step 1 hn_fcos_candidates: score = sqrt(sigmoid(cls)*sigmoid(ctr)); max/argmax over
 *   classes (ties -> lowest class); keep score > thresh; decode box; compact in anchor
 *   order.  Output per image (capacity `cap` = total points): cand_* arrays + count.
 * Step 2 hn_fcos_nms: sort candidates by (score desc, index asc), greedy NMS exactly as
 *   torchvision 0.11.3 batched_nms (coordinate trick when 4*K <= 4000, per-class
 *   otherwise; CPU-kernel rule: suppress iff (double)iou > iou_thresh), write kept
 *   detections in score order, boxes rescaled by (ratio_h, ratio_w).
 * ------------------------------------------------------------------------------------ */
typedef struct hn_fcos_levels {
  int32_t num_levels;
  int32_t h[HN_FCOS_MAX_LEVELS], w[HN_FCOS_MAX_LEVELS], stride[HN_FCOS_MAX_LEVELS];
  const float* cls_lr[HN_FCOS_MAX_LEVELS];
  const float* reg_ctr[HN_FCOS_MAX_LEVELS];
} hn_fcos_levels;

int hn_fcos_candidates(const hn_fcos_levels* lv, int n, int num_classes, float score_thresh,
                       float* cand_boxes /* [n][cap][4] */, float* cand_scores /* [n][cap] */,
                       int32_t* cand_labels, int32_t* cand_sides, int32_t* cand_level /* [n][cap] */,
                       int32_t* cand_point /* [n][cap] anchor-point index, may be NULL */,
                       int32_t* cand_count /* [n] */, int cap, void* stream);
/* The same result from ceil(points / 1024) workgroups per image instead of one (two short launches; the single workgroup
 * costs 60 us per call at batch 1 whatever the number of candidates): workspace = hn_fcos_candidates_ws_bytes(n, total
 * points) bytes of device memory, contents irrelevant before and after. */
int64_t hn_fcos_candidates_ws_bytes(int n, int total_points);
int hn_fcos_candidates_ws(const hn_fcos_levels* lv, int n, int num_classes, float score_thresh, float* cand_boxes,
                          float* cand_scores, int32_t* cand_labels, int32_t* cand_sides, int32_t* cand_level,
                          int32_t* cand_point, int32_t* cand_count, int cap, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* ext=True detector outputs (fcos_utils/fcos.py:255-264 layers, :299-320 head maths, :605-607 argmax,
 * :631-647 gather) for the detections hn_fcos_nms kept.  ext[l] is the raw NHWC conv output
 * [n][h_l][w_l][8] = relu(hand_dydx_layer)[3] then hand_contact_state_layer[5] (host array of
 * lv->num_levels device pointers; lv supplies h/w only).  Row d of image i (d < det_count[i]):
 *   det_dxdymags[i][d] = (mag, 0.1*dx/max(|(dx,dy)|,1e-12), 0.1*dy/...), det_contacts[i][d] = argmax. */
int hn_fcos_ext_gather(const hn_fcos_levels* lv, const float* const* ext, const int32_t* det_keep,
                       const int32_t* cand_point, const int32_t* det_count, int n, int cap,
                       int32_t* det_contacts /* [n][cap] */, float* det_dxdymags /* [n][cap][3] */,
                       void* stream);

/* The FCOS criterion's forward (fcos_utils/fcos.py:523-570 the matching, :44-178 the six terms), on
 * the head tensors of hn_fcos_candidates plus, with the ext heads, ext[l] as hn_fcos_ext_gather takes it (NULL: no ext terms).
 * Ground truth per image, padded to G rows (device memory): gt_boxes ALREADY SCALED to the canvas, gt_info = (contactstate,
 * handside, mag, dx, dy), gt_count clamped to [0, G] by the kernel (a count of 0: all background, zero dxdy targets).
 * Outputs (device): terms [n][6] = the per-image sums before any factor or division, in the order classification (focal),
 * bbox_regression (GIoU), bbox_ctrness (BCE), hand_lr (focal), hand_contact_state (focal), hand_dxdy (squared differences; the
 * last two zero without ext); fg [n] = foreground points; losses [6] = the reference's dict values over max(1, sum fg);
 * matched [n][points] = each point's ground-truth row or -1 (NULL skips the store).  Two launches, no atomics, a fixed
 * order: the same bytes on every run, and image i of a batch gives the bytes of that image alone.  Null pointers, G outside
 * 1..HN_FCOS_MAX_GT and num_classes outside 1..8 are refused before any launch.
 * workspace = hn_fcos_loss_ws_bytes(n, total points) bytes, 8-byte aligned, contents irrelevant before and after. */
#define HN_FCOS_MAX_GT 64
int64_t hn_fcos_loss_ws_bytes(int n, int total_points);
int hn_fcos_loss_f32(const hn_fcos_levels* lv, const float* const* ext /* or NULL */, int n, int num_classes,
                     const float* gt_boxes /* [n][G][4], scaled */, const int32_t* gt_labels /* [n][G] */,
                     const float* gt_info /* [n][G][5] */, const int32_t* gt_count /* [n] */, int G, float radius,
                     float* terms, int32_t* fg, float* losses, int32_t* matched /* or NULL */, void* ws, int64_t ws_bytes,
                     void* stream);

/* The FCOS criterion's backward at the heads: hn_fcos_loss_f32's arguments, workspace and outputs (terms,
 * fg, losses and matched get the bytes hn_fcos_loss_f32 gives), then one more launch on the same stream that writes the gradient
 * of sum_k upstream[k] * losses[k] at cls_lr, reg_ctr and ext into d_cls_lr[l], d_reg_ctr[l] and d_ext[l] (device tensors in the
 * layouts of the heads; d_ext NULL exactly when ext is, otherwise 16-byte aligned).  upstream: six fp32 weights in DEVICE memory
 * (read by the kernel, no host read), NULL = ones; without ext upstream[4] and [5] are ignored.  The matching and the divisor
 * max(1, sum fg) are constants.  Every gradient element is written exactly once, zeros included (no memset, no atomics): the
 * same bytes on every run.  Every refusal (hn_fcos_loss_f32's, a null gradient level, d_ext without ext) happens before any
 * launch. */
int hn_fcos_loss_grad_f32(const hn_fcos_levels* lv, const float* const* ext /* or NULL */, int n, int num_classes,
                          const float* gt_boxes, const int32_t* gt_labels, const float* gt_info, const int32_t* gt_count, int G,
                          float radius, float* terms, int32_t* fg, float* losses, int32_t* matched /* or NULL */, void* ws,
                          int64_t ws_bytes, const float* upstream /* [6] or NULL */, float* const* d_cls_lr,
                          float* const* d_reg_ctr, float* const* d_ext /* or NULL */, void* stream);

int64_t hn_fcos_nms_scratch_bytes(int n, int cap);
int hn_fcos_nms(const float* cand_boxes, const float* cand_scores, const int32_t* cand_labels,
                const int32_t* cand_sides, const int32_t* cand_level, const int32_t* cand_count,
                int n, int cap, double iou_thresh, float ratio_h, float ratio_w,
                void* scratch,
                float* det_boxes /* [n][cap][4] */, float* det_scores, int32_t* det_labels,
                int32_t* det_sides, int32_t* det_level, int32_t* det_keep /* cand index */,
                int32_t* det_count /* [n] */, void* stream);

/* hn_fcos_nms with one (ratio_h, ratio_w) pair per image: ratios = DEVICE fp32 [n][2] (resize_boxes of a
 * batch whose images differ in size, fcos_utils/fcos.py:661-669). */
int hn_fcos_nms_ratios(const float* cand_boxes, const float* cand_scores, const int32_t* cand_labels,
                       const int32_t* cand_sides, const int32_t* cand_level, const int32_t* cand_count,
                       int n, int cap, double iou_thresh, const float* ratios, void* scratch,
                       float* det_boxes, float* det_scores, int32_t* det_labels, int32_t* det_sides,
                       int32_t* det_level, int32_t* det_keep, int32_t* det_count, void* stream);

/* Stand-alone NMS with torchvision.ops.nms semantics (tests / callers with own boxes). */
int hn_nms(const float* boxes, const float* scores, int k, double iou_thresh,
           void* scratch /* hn_fcos_nms_scratch_bytes(1,k) */, int32_t* keep, int32_t* num_keep,
           void* stream);

/* ------------------------------------------------------------------------------------
 * Crop: top-1 hand box -> int box -> pad 40 % -> clamp -> nearest resize to out x out.
 * Replaces handnet_pipeline/handnet_pipeline.py:74-105.
 * For each image: first detection (score order) with label == hand_label.  Writes
 *   crop_box [n][4] int64 (x1,y1,x2,y2 after padding; zeros if none), has_hand [n] int32 (0 / 1; the A2J stage of
 *   the pipeline raises it to 2 for a frame whose depth crop holds non-finite pixels: NaN keypoints, like the reference),
 *   crops [n][out][out][cpad] fp32 NHWC with depth in channel 0, other channels 0.
 * depth is [n][in_ch][h][w] fp32, in_ch = 1 (depth) or 4 (RGB-D; reorder_bgr = 1 applies the
 * reference's channel permutation [2,1,0,3], handnet_pipeline.py:102); crops channel c = image channel.
 * This is hn_crop_resize_hands with max_hands = 1, by construction: the same two launches, without score and det_index.
 * crops must be 16-byte aligned (else HN_ERR_ARG): it is written as 16-byte vectors, like the crops of the entries below.
 * (Until this was checked, a misaligned crops pointer was a misaligned vector store.)  crop_box needs no more than an
 * int64_t array's own 8 bytes.
 * ------------------------------------------------------------------------------------ */
int hn_crop_resize(const float* det_boxes, const int32_t* det_labels, const int32_t* det_count,
                   int cap, int hand_label, const float* depth, int n, int in_ch, int reorder_bgr,
                   int h, int w, int out, int cpad, int64_t* crop_box, int32_t* has_hand, float* crops,
                   void* stream);

/* The crop stage for up to max_hands (1..16, else HN_ERR_ARG) hands per frame.  Slot k of frame i is the k-th detection
 * with label == hand_label in frame i's score-ordered list; its box is padded, clamped and cut exactly as hn_crop_resize
 * does for the first one (max_hands = 1 gives hn_crop_resize's crop_box / has_hand / crops bit for bit).  A slot whose
 * padded box gives an empty slice, and every slot beyond the frame's hand detections, is empty: zero box, has_hand 0,
 * score 0, det_index -1, zero crop (an empty slot still uses up its rank).  Outputs, frame-major (slot = i * max_hands + k):
 *   crop_box [n][max_hands][4] int64, has_hand [n][max_hands] int32, score [n][max_hands] fp32 (det_scores of the slot's
 *   detection), det_index [n][max_hands] int32 (its row in the detection list), crops [n * max_hands][out][out][cpad] fp32.
 * det_scores [n][cap] as written by hn_fcos_nms; other arguments as in hn_crop_resize. */
int hn_crop_resize_hands(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                         const int32_t* det_count, int cap, int hand_label, int max_hands, const float* depth, int n,
                         int in_ch, int reorder_bgr, int h, int w, int out, int cpad, int64_t* crop_box, int32_t* has_hand,
                         float* score, int32_t* det_index, float* crops, void* stream);
/* hn_crop_resize_hands with the slots' handedness, in the same two launches (added under ABI 36: a new function only).
 * det_sides [n][cap] int32 as hn_fcos_nms writes it (the detector's hand_lr head); left_side = the value that means "left".
 *   side   [n][max_hands] int32: det_sides of the slot's detection, -1 for an empty slot
 *   mirror [n][max_hands] int32: 1 for a filled slot with side == left_side, else 0
 * The crop of a slot with mirror == 1 is cut mirrored along its width: its pixel (oy, ox) is the plain crop's pixel
 * (oy, out - 1 - ox) on every channel (a left hand on its way through a right-handed pose network); every other slot, and
 * every other output, is hn_crop_resize_hands' bit for bit. */
int hn_crop_resize_hands_sided(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                               const int32_t* det_sides, const int32_t* det_count, int cap, int hand_label, int left_side,
                               int max_hands, const float* depth, int n, int in_ch, int reorder_bgr, int h, int w, int out,
                               int cpad, int64_t* crop_box, int32_t* has_hand, float* score, int32_t* det_index, int32_t* side,
                               int32_t* mirror, float* crops, void* stream);
/* hn_crop_resize_hands_sided with the slots TRACKED from one call to the next (added under ABI 36: new functions only).
 * state: int32 [n][1 + max_hands][12] on the device, 16-byte aligned, hn_track_state_bytes(n, max_hands) bytes, updated in
 * place; all zeros = the empty tracker (reset: a memset).  Row 0 of a frame: word 0 = the last track id issued, the rest 0.
 * Row 1 + s = slot s: words 0..7 the padded box as four int64, word 8 id (0: free), word 9 age (steps since the track was
 * created on which it was seen), word 10 missed (consecutive steps without a match), word 11 zero.
 * Per frame: the candidates are the first 16 hand-label detections of the score-ordered list whose padded slice is not
 * empty; a live slot and a candidate are a pair when their padded boxes overlap (I > 0) with 1000 * I >= thr_milli * U
 * (thr_milli 1..1000); pairs are matched greedily by IoU (cross-multiplied in int64; ties: lower slot, then lower candidate); a
 * live slot without a match is held (empty outputs, no other hand may take it) for up to `hold` (0..1000000) steps and freed
 * after that; the candidates left over take the free slots, lowest first, in score order, each with a new id.
 * A matched or new slot is written as hn_crop_resize_hands[_sided] writes the slot of its detection; a held or free slot is an
 * empty slot.  track_id / track_age [n][max_hands] int32: the slot's id (0: free) and age, held slots included.
 * det_sides, side and mirror may be NULL together: the unsided step.  h, w <= 32767 (else HN_ERR_ARG). */
int hn_crop_resize_hands_tracked(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                                 const int32_t* det_sides, const int32_t* det_count, int cap, int hand_label, int left_side,
                                 int max_hands, const float* depth, int n, int in_ch, int reorder_bgr, int h, int w, int out,
                                 int cpad, int64_t* crop_box, int32_t* has_hand, float* score, int32_t* det_index, int32_t* side,
                                 int32_t* mirror, float* crops, int32_t* state, int thr_milli, int hold, int32_t* track_id,
                                 int32_t* track_age, void* stream);
/* bytes of the state of n frames with max_hands slots each (0 for arguments out of range) */
int64_t hn_track_state_bytes(int n, int max_hands);

/* fp32 NHWC(4) image [n][h][w][4] -> the stem image of hn_conv_stem_f16x3 / hn_conv_stem_pool_f16x3 (two fp16 planes hi, lo of
 * [n][h + 2*border][w + 2*border][4], zero border): the A2J crops on their way to the split-precision stem
 * (a2j/resnet.py:155-158 conv1 -> bn1 -> relu -> maxpool). */
int hn_stem_image_nhwc4(const float* x, int n, int h, int w, int border, void* dst16, void* stream);
/* The same with the per-image flags of the aggregation (valid [n] int32 on the device, or NULL): an image with
 * valid[i] == 1 that holds a non-finite pixel gets valid[i] = 2.  The reference's network returns NaN for EVERY joint of
 * such a crop (each cell of its 11 x 11 maps sees every pixel of the crop; ReLU and max pooling propagate NaN in torch),
 * and hn_a2j_aggregate_f32 writes exactly that for valid[i] == 2 -- the split-precision convolutions in between need not
 * (and do not) propagate NaN. */
int hn_stem_image_nhwc4_valid(const float* x, int n, int h, int w, int border, void* dst16, int32_t* valid, void* stream);

/* Pack [n][1][h][w] depth crops into NHWC(cpad) for the A2J stem (A2J-only entry). */
int hn_pack_depth_nhwc(const float* src, float* dst, int n, int hw, int cpad, void* stream);

/* ------------------------------------------------------------------------------------
 * A2J anchor aggregation.  Replaces a2j/anchor.py:57-82 (post_process.forward).
 * Inputs are the raw head conv outputs, NHWC over the 11x11 anchor grid:
 *   cls [k][fh][fw][A*J], reg [k][fh][fw][A*J*2], dep [k][fh][fw][A*J], A = 16 anchors.
 * out [k][J][3] = (sum w*(anchor_0 + reg_0), sum w*(anchor_1 + reg_1), sum w*depth),
 * w = softmax over all fh*fw*A anchors per joint.  Anchor coords follow
 * a2j/anchor.py:7-42: coordinate 0 = h*stride + P[a/4], coordinate 1 = w*stride + P[a%4].
 * With valid != NULL: rows with valid[k] == 0 are written as zeros (no crop), rows with valid[k] == 2 as NaN (a crop
 * with non-finite pixels, see hn_stem_image_nhwc4_valid), rows with valid[k] == 1 are computed.
 * ------------------------------------------------------------------------------------ */
int hn_a2j_aggregate_f32(const float* cls, const float* reg, const float* dep,
                         const int32_t* valid, int k, int fh, int fw, int joints, int stride,
                         float* out, void* stream);

/* crop-(u,v,d) keypoints -> image (u,v,d) or, with paras = host array (fx, fy, cx, cy), camera
 * xyz in millimetres.  Replaces convert_joints (a2j/a2j.py:17-34) + uvd2xyz
 * (datasets3d/a2jdataset.py:31-38), the step every caller runs right after the path
 * (ros_demo.py:289,329-330).  kp [n][joints][3], crop_box [n][4] int64 (x1,y1,x2,y2),
 * valid [n] or NULL (rows with valid == 0 are written as zeros). */
int hn_convert_joints_f32(const float* kp, const int64_t* crop_box, const int32_t* valid,
                          int n, int joints, float crop_w, float crop_h,
                          const float* paras /* host, 4 floats, or NULL */, float* out, void* stream);

/* The evaluation caller's form of the same conversion (A2JModelLightning.test_step, a2j/a2j.py:333-348 -- on the prediction
 * and on the ground truth): box_f32 [n][4] fp32 = the dataset's crop box with fractional corners, sample_paras [n][4] fp32 =
 * each sample's (fx, fy, cx, cy), both on the DEVICE (datasets3d/a2jdataset.py:262-265,279,293).  Writes the image (u,v,d)
 * (out_image_uvd, or NULL) and / or the camera xyz in millimetres (out_xyz_mm, or NULL; needs sample_paras), [n][joints][3]
 * each.  All fp32 in the reference's order: bit-identical to numpy on float32 operands.  valid as above. */
int hn_convert_joints_samples_f32(const float* kp, const float* box_f32, const float* sample_paras /* or NULL */,
                                  const int32_t* valid /* or NULL */, int n, int joints, float crop_w, float crop_h,
                                  float* out_image_uvd, float* out_xyz_mm, void* stream);

/* The aggregation with convert_joints + uvd2xyz in its EPILOGUE: what hn_a2j_aggregate_f32 writes to out_uvd,
 * plus -- from the registers that hold each joint, no second launch -- its image (u,v,d) (out_image_uvd, or NULL) and its
 * camera xyz in millimetres (out_xyz_mm, or NULL; needs paras = host array (fx, fy, cx, cy)), each [k][J][3]: bit-identical
 * to hn_convert_joints_f32 on out_uvd (one device function serves both).  crop_box [k][4] int64 = the padded crop boxes the
 * crops were cut with (hn_crop_resize).  Rows with valid[k] == 0 are zeros in all outputs, rows with valid[k] == 2 NaN.
 * opts (host, or NULL = none): the live caller's two clamps BEFORE the conversion, which it applies to the values it converts
 * (ros_demo.py:279-283) -- they touch the converted outputs only, out_uvd stays what the network returned:
 *   clamp_keypoints  1: the crop-(u,v,d) is clamped to [0, crop_w] (torch.clamp(keypoint_pred, 0, 176), all three columns)
 *   clamp_box_h / _w > 0: box x1,y1 are clamped to [0, clamp_box_h] and x2,y2 to [0, clamp_box_w] (as written there:
 *                    detection[:2] against the image HEIGHT, detection[2:] against the WIDTH) */
typedef struct hn_convert_opts {
  int32_t clamp_keypoints;
  int32_t clamp_box_h, clamp_box_w;
  int32_t reserved;           /* 0 */
  /* The evaluation caller's operands (A2JModelLightning.test_step, a2j/a2j.py:333-348: the DATASET's box and intrinsics per
   * sample, datasets3d/a2jdataset.py:262-265,279,293), device pointers or NULL:
   *   sample_box    [k][4] fp32 (x1,y1,x2,y2), fractional corners: used INSTEAD of crop_box (which may then be NULL); every
   *                 operation of the conversion stays in fp32 like numpy's on a float32 box (bit-identical to the reference)
   *   sample_paras  [k][4] fp32 (fx, fy, cx, cy) per sample: used INSTEAD of `paras` */
  const float* sample_box;
  const float* sample_paras;
} hn_convert_opts;
int hn_a2j_aggregate_convert_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid, int k, int fh,
                                 int fw, int joints, int stride, const int64_t* crop_box, float crop_w, float crop_h,
                                 const float* paras /* host, 4 floats, or NULL */, const hn_convert_opts* opts /* host or NULL */,
                                 float* out_uvd, float* out_image_uvd, float* out_xyz_mm, void* stream);
/* The same for crops of which some were cut mirrored (hn_crop_resize_hands_sided): mirror [k] int32 on the device; for a row
 * with mirror != 0 the thread that holds a joint replaces u by crop_w - u (one fp32 subtraction) before it writes out_uvd, so
 * out_uvd, the clamps and both conversions are in plain-crop coordinates.  Rows with mirror == 0: hn_a2j_aggregate_convert_f32
 * bit for bit.  Added under ABI 36: hn_convert_opts is unchanged. */
int hn_a2j_aggregate_convert_mirror_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid,
                                        const int32_t* mirror, int k, int fh, int fw, int joints, int stride,
                                        const int64_t* crop_box, float crop_w, float crop_h, const float* paras,
                                        const hn_convert_opts* opts, float* out_uvd, float* out_image_uvd, float* out_xyz_mm,
                                        void* stream);

/* The aggregation with the A2J criterion (a2j/anchor.py:99-153 A2J_loss.forward, a2j/a2j.py:231-238) in the SAME sweep over the
 * heads: out_uvd (and the conversion's outputs) are hn_a2j_aggregate_convert_f32's bit for bit, and the thread that holds a joint
 * also writes the joint's terms against gt [k][J][3] (crop (coord0, coord1, depth), the coordinates of an out_uvd row):
 *   out_terms [k][J][8] (16-byte aligned) = (La_h, La_w, Lr_h, Lr_w, d, (gt - out_uvd)^2 x 3)
 *     La = smooth-L1 (knee 1) of |gt - sum w anchor|, Lr the same of |gt - out_uvd| (first two columns), d = |gt_depth - out_depth|
 *     (a plain L1: the reference computes a smooth-L1 with knee 3 for the depth and never uses it).
 * A second, small launch reduces them in a fixed order (no atomics):
 *   out_sample [k][2] = (mean of La over 2J values, mean of Lr over 2J values * spatial_factor + mean of d over J values);
 *     row i depends on crop i only (bit-identical to the k = 1 call on that crop)
 *   out_batch [5] = (classification = mean over the samples of column 0, the criterion's regression = mean of column 1,
 *     regression * reg_loss_factor, total = classification + regression * reg_loss_factor,
 *     rmse = sqrt(mean (gt - out_uvd)^2 over all samples * J * 3 values), a2j/a2j.py:318)
 * valid (or NULL) as in hn_a2j_aggregate_f32; rows with valid == 0 are left out of every out_batch value (the divisor is the
 * number of rows with valid != 0; none gives 0 / 0 = NaN), rows with valid == 2 have NaN terms and make out_batch NaN.
 * The conversion's arguments (crop_box .. opts, out_image_uvd, out_xyz_mm) are those of hn_a2j_aggregate_convert_f32 and may all
 * be absent (NULL / 0): then nothing is converted.  k == 0 launches nothing. */
int hn_a2j_aggregate_loss_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid /* or NULL */,
                              const float* gt, int k, int fh, int fw, int joints, int stride, float spatial_factor,
                              float reg_loss_factor, const int64_t* crop_box /* or NULL */, float crop_w, float crop_h,
                              const float* paras /* host, 4 floats, or NULL */, const hn_convert_opts* opts /* host or NULL */,
                              float* out_uvd, float* out_image_uvd /* or NULL */, float* out_xyz_mm /* or NULL */,
                              float* out_terms, float* out_sample, float* out_batch, void* stream);

/* The A2J criterion's backward at the three heads, in ONE launch with the aggregation's grid and summation order (DESIGN.md
 * section 9r): the gradient of  wa * classification + wr * (reg_loss_factor * the criterion's regression mean)  -- out_batch [0]
 * and [2] of hn_a2j_aggregate_loss_f32 -- with respect to cls, reg and dep, written to d_cls, d_dep [k][fh][fw][16 J] and
 * d_reg [k][fh][fw][16 J][2] (8-byte aligned), the layouts of the heads.  upstream: DEVICE (wa, wr), or NULL for (1, 1), the
 * gradient of out_batch [3].  Per joint, with w the softmax weights, Ea = sum w anchor, Er = sum w (anchor + reg), Ed = sum w dep,
 * g = gt and n = the number of rows with valid != 0 (counted on the device):
 *   ga_c = wa / n / (2J) clip(Ea_c - g_c, -1, 1), gr_c = wr reg_loss_factor spatial_factor / n / (2J) clip(Er_c - g_c, -1, 1),
 *   gd = wr reg_loss_factor / n / J sign(Ed - g_d);
 *   d_reg = w gr_c, d_dep = w gd, d_cls = w (sum_c ga_c (anchor_c - Ea_c) + sum_c gr_c (anchor_c + reg_c - Er_c) + gd (dep - Ed)).
 * Every element is written once, in a fixed order (bitwise reproducible); rows with valid == 0 get zeros, rows with valid == 2
 * NaN; a NaN coordinate of gt makes that joint's d_cls and that coordinate's d_reg NaN, as the reference's autograd does.
 * out_uvd [k][J][3] and out_terms [k][J][8] (16-byte aligned), each or NULL: hn_a2j_aggregate_loss_f32's outputs of those names,
 * bit for bit.  k == 0 launches nothing.  Added under ABI 36: a new function only. */
int hn_a2j_loss_grad_f32(const float* cls, const float* reg, const float* dep, const int32_t* valid /* or NULL */,
                         const float* gt, int k, int fh, int fw, int joints, int stride, float spatial_factor,
                         float reg_loss_factor, const float* upstream /* device, 2 floats, or NULL */, float* d_cls, float* d_reg,
                         float* d_dep, float* out_uvd /* or NULL */, float* out_terms /* or NULL */, void* stream);

/* The lifter's input from a step's image-(u,v) joints (the live caller's glue between the path and Pose2Mesh,
 * ros_demo.py:148-157: get_bbox -> process_bbox -> j2d_processing (rot 0, no flip) -> / input_shape -> (x - mean) / std):
 * with no rotation that chain is a per-axis POSITIVE affine map followed by a per-axis standardisation over the J joints,
 * which cancels the map -- so the result is (x - mean_J(x)) / std_J(x) per frame and axis (population std, numpy's default).
 * image_uvd [n][J][3] (columns 0, 1 are read) -> out [n][J][2] fp32; rows with valid[i] != 1 are zeros. */
int hn_joints2d_standardize_f32(const float* image_uvd, const int32_t* valid /* or NULL */, int n, int joints, float* out,
                                void* stream);
/* The same with the live caller's skip rule (ros_demo.py:288-300): a row is lifted -- lifted[i] = 1 and out[i] is exactly what
 * hn_joints2d_standardize_f32 writes for it -- iff valid[i] == 1 (or valid is NULL), its (u,v) are finite and
 * process_bbox(get_bbox(uv)) is not None (pose2mesh/lib/coord_utils.py:21-49, evaluated in fp32 one rounding per numpy
 * operation); otherwise lifted[i] = 0 and out[i] is zeros.  One launch, one wave per row (the multi-hand live step:
 * hn_amd.live.LiveHandsEngine).  Added under ABI 36: a new function only, no struct or existing signature changed. */
int hn_lifter_input_gated_f32(const float* image_uvd /* [n][joints][3] */, const int32_t* valid /* or NULL */, int n,
                              int joints, float* out /* [n][joints][2] */, int32_t* lifted /* [n] */, void* stream);
/* The same for hands that went through the pose network mirrored: the gate is evaluated on image_uvd as it stands (plain
 * image joints); a LIFTED row with mirror[i] != 0 (device int32 [n]) has column 0 of its standardised row negated -- exactly
 * the standardisation of the joints mirrored in x (the mean negates, the std does not change).  Added under ABI 36. */
int hn_lifter_input_gated_mirror_f32(const float* image_uvd, const int32_t* valid /* or NULL */, const int32_t* mirror, int n,
                                     int joints, float* out, int32_t* lifted, void* stream);

/* Per-frame result records for the N > 1 all-gather (ONE collective of fixed-size records per step).
 * Record layout (rec_bytes >= 40 + 12*joints, multiple of 8): bytes 0..31 crop box 4 x int64, 32..35 has_hand,
 * 36..39 row-is-a-real-frame, 40.. keypoints joints*3 x fp32.  hn_pack_records writes rows [0, n) from the three
 * result tensors and zero rows [n, rows) (shard padding); hn_unpack_records is the inverse over `rows` records
 * (valid[r] = the row flag).  One launch each, so a step adds pack + collective + unpack to the engine's launches. */
int hn_pack_records(const float* keypoints, const int64_t* crop_box, const int32_t* has_hand, int n, int rows,
                    int joints, int rec_bytes, void* records, void* stream);
/* Wide records: up to two more [n][joints][3] fp32 fields behind the keypoints (the step's image (u,v,d) and camera xyz in mm,
 * hn_a2j_aggregate_convert_f32): bytes 40 + 12*joints .. and 40 + 24*joints ..; rec_bytes >= 40 + 12*joints per field.
 * hn_unpack_records reads the first field of records of any width. */
int hn_pack_records_ex(const float* keypoints, const int64_t* crop_box, const int32_t* has_hand, int n, int rows, int joints,
                       int rec_bytes, const float* extra0 /* or NULL */, const float* extra1 /* or NULL */, void* records,
                       void* stream);
int hn_unpack_records(const void* records, int rows, int joints, int rec_bytes, float* keypoints,
                      int64_t* crop_box, int32_t* has_hand, int32_t* valid, void* stream);

/* Always-on safety net of the f16x3 path (range contract): counts non-finite values of x[0..count) into
 * *flag (device int32; the caller zeroes it and reads it with the copy of the results it makes anyway). */
int hn_nonfinite_count_f32(const float* x, int64_t count, int32_t* flag, void* stream);

/* ------------------------------------------------------------------------------------
 * Pose2Mesh lifter: Chebyshev graph convolution helpers.  Replaces
 * pose2mesh/lib/models/backbones/cheby_graph_conv.py:5-42 (torch.sparse.mm recursion + concat / permute)
 * and the block residual of meshnet.py:105-113; the Linear + BatchNorm1d + ReLU of a graph conv run on
 * hn_conv2d_nhwc_f16x3_ws as a 1x1 convolution over [batch][vertex] rows (BatchNorm folded into the weights).
 * L is a CSR matrix (int32 indptr [v+1], indices, fp32 values; indices ascending per row); activations are
 * fp32 [batch][v][f], f % 4 == 0.
 *   hn_spmm_csr_f32        y = L x
 *   hn_cheby3_basis_split  x2 = 2 L x1 - x0; out16 = S32 rows [x0 | x1 | x2 | 0-pad] of cpad channels
 *                          (order k-major: channel k*f + i; the reference's (i, k) order is absorbed by
 *                          permuting the Linear's columns at load time, hn_amd/pose2mesh_engine.py); range contract:
 *                          notes HN_RANGE_ACTIVATION for an x0, x1 or x2 value that fails |v| <= 65504
 *   hn_feat_interp_add_f32 out[r*up + u][:] = y[r][:] + interp_linear(xin[r][:], fi -> fo), u < up
 *                          (F.interpolate(mode='linear') along the feature axis + nn.Upsample(2) on vertices)
 * ------------------------------------------------------------------------------------ */
int hn_spmm_csr_f32(const int32_t* indptr, const int32_t* indices, const float* values, int v,
                    const float* x, float* y, int batch, int f, void* stream);
/* One whole graph convolution of the 'mano' mesh net (K = 3; meshnet.py:95-100 = cheby_graph_conv.py:5-42 + F.relu) as ONE
 * launch, optionally with the block's residual and vertex up-sampling (meshnet.py:105-113) in its epilogue -- the lifter is
 * launch-bound at the live caller's batch:
 *   y[r*up + u][:] = act(W [x0 | L x0 | L2 x0 | 0][r] + bias) (+ interp_linear(xin[r][:], fi -> fout)),  u < up
 * L2 = 2 L L - I, precomputed by the host (the same second-order Chebyshev polynomial, one rounding per coefficient instead of
 * a second dependent sparse product); x fp32 [batch][v][fin] (fin % 4 == 0, <= 256); w16 = the split filter bank
 * [fout][K/32][2][32] over K = pad32(3*fin) k-major channels (as hn_cheby3_basis_split's operand) -- or, with w_frag = 1, the
 * same values in MFMA fragment order [ceil(fout/16)][K/32][2 (hi, lo)][64 lanes][8]: element i of lane l = column 16*nt +
 * (l & 15), channel 32*kt + 8*(l >> 4) + i, zero behind fout (a wave's load is then one contiguous KB); xin fp32 [batch][v][fi]
 * or NULL; y fp32 [batch][v*up][fout], or S32 rows when out_split (fout % 32 == 0).  fout <= 256.
 * Range contract: the three basis parts become fp16 pairs inside the kernel, so a value of x, L x or L2 x that fails
 * |v| <= 65504 is noted (HN_RANGE_ACTIVATION) whatever the output type; with out_split the stored values are noted as well. */
typedef struct hn_graph_csr {
  const int32_t* indptr;   /* [v + 1] */
  const int32_t* indices;  /* ascending per row */
  const float* values;
  int32_t v;
} hn_graph_csr;
int hn_graph_conv_cheby3_f16x3(const hn_graph_csr* L, const hn_graph_csr* L2, const float* x, int batch, int fin,
                               const void* w16, int w_frag, const float* bias, int fout, int relu, const float* xin, int fi,
                               int up, void* y, int out_split, void* stream);
/* Glue of the lifter as single launches: fp32 rows [rows][f] -> S32 rows of cpad channels, zero padded (the operand of
 * PoseNet's first Linear from the [batch][2J] joints); pose_combine (pose2mesh_net.py:20) = [pose2d | pose3d / 1000 | 0] per
 * joint as fp32 [batch*J][fpad] (the padded input of the first graph convolution; pose3d rows may be padded: PoseNet's last
 * Linear is run with 64 output columns so that it takes the vectorised / split-K form of the convolution kernel).
 * hn_pad_split_rows_f32 notes HN_RANGE_ACTIVATION for a value of x that fails |v| <= 65504 (the zero padding cannot). */
int hn_pad_split_rows_f32(const float* x, int64_t rows, int f, int cpad, void* out16, void* stream);
/* The last lines of the live caller's mesh path (ros_demo.py:162,332-337): out[i][k][:] = ((mesh[i][perm[k]][:] * 1000 +
 * xyz_mm[i][0][:]) / 1000) * (1, -1, -1) -- the real mesh's vertices in original order (perm = graph_perm_reverse[:v], int64
 * on the device, entries < v0), moved by the first joint's camera position, y and z negated; numpy's float32 arithmetic, one
 * rounding per operation (bit-identical).  mesh [n][v0][3], xyz_mm [n][joints][3], out [n][v][3]; rows with valid != 1 are zeros. */
int hn_mesh_finish_f32(const float* mesh, const int64_t* perm, const float* xyz_mm, const int32_t* valid /* or NULL */, int n,
                       int v0, int v, int joints, float* out, void* stream);
/* The same for meshes the lifter made of mirrored hands: for rows with mirror[i] != 0 (device int32 [n]) the x of the raw
 * vertex is negated before the arithmetic, ((-x) * 1000 + root_x) / 1000.  perm and xyz_mm may both be NULL (then v == v0):
 * no permutation and no camera offset -- out = the raw vertices, x negated where mirrored, zero rows where valid != 1.
 * Added under ABI 36. */
int hn_mesh_finish_mirror_f32(const float* mesh, const int64_t* perm /* or NULL */, const float* xyz_mm /* or NULL */,
                              const int32_t* valid /* or NULL */, const int32_t* mirror, int n, int v0, int v, int joints,
                              float* out, void* stream);
/* hn_mesh_finish_mirror_f32 (perm and xyz_mm given) and, in the same launch, a One Euro filter (Casiez et al. 2012) over time
 * on every coordinate of two signals of every row (= tracked hand slot): the final mesh as written to `out` (metres; gate:
 * lifted[i] == 1) -> smooth_mesh [n][v][3], and xyz_mm (camera millimetres; gate: has_hand[i] == 1) -> smooth_xyz
 * [n][joints][3].  `out` is hn_mesh_finish_mirror_f32's, bit for bit (valid = lifted; mirror may be NULL).
 * state: hn_smooth_state_bytes(n, joints, v) bytes on the device, 16-byte aligned, updated in place: one 16-byte record
 * {float xh, float dxh, int32 id, int32 0} per element, [n][joints + v][3] -- a row's joints first, then its vertices.  All
 * zeros = the empty filter (reset: a memset).  Every thread reads and writes its own record only.
 * Per element, x = the unfiltered value, t = track_id[i] (device int32 [n]):
 *   1. gate off: the output is 0 and the record is zeroed (a hand that returns restarts);
 *   2. x not finite: the output is x and the record is zeroed;
 *   3. record id == 0, or id != t, or t == 0, or a stored xh / dxh that is not finite: the output is x, the record {x, 0, t};
 *   4. else, with (xp, dxp) = the record's (xh, dxh), in fp32 with one rounding per operation and in this order:
 *        rd = (TWO_PI * d_cutoff) * dt;  ad = rd / (rd + 1);  dx = (x - xp) / dt;  edx = dxp + ad * (dx - dxp);
 *        fc = min_cutoff + beta * |edx|;  r = (TWO_PI * fc) * dt;  a = r / (r + 1);  xh = xp + a * (x - xp)
 *      (TWO_PI = 6.2831855f): the output is xh, the record {xh, edx, t}.
 * dt: ONE fp32 word on the device (seconds between steps, finite and > 0: the caller's to check), read by every thread and
 * never written -- a captured step takes another dt without a new capture.  min_cutoff, d_cutoff: finite and > 0; beta_xyz
 * (the joints' beta, speeds in mm/s) and beta_mesh (the vertices', speeds in m/s: 1000 * beta_xyz for the same behaviour):
 * finite and >= 0; else HN_ERR_ARG.  Added under ABI 36. */
int hn_mesh_finish_smooth_f32(const float* mesh, const int64_t* perm, const float* xyz_mm, const int32_t* lifted,
                              const int32_t* has_hand, const int32_t* mirror /* or NULL */, const int32_t* track_id,
                              const float* dt, void* state, int n, int v0, int v, int joints, float min_cutoff, float beta_xyz,
                              float beta_mesh, float d_cutoff, float* out, float* smooth_xyz, float* smooth_mesh, void* stream);
/* bytes of the filter state of `slots` rows with `joints` joints and v vertices each (0 for arguments that are not positive) */
int64_t hn_smooth_state_bytes(int slots, int joints, int v);
/* The live caller's last call, render(out, paras, h, w, full_image, face) (ros_demo.py:86-116,329-337), without a graphics
 * pipeline: the meshes of s = n * k hand slots (slot i * k + j = hand j of frame i) rasterised over their frames, one depth
 * buffer per frame.  mesh [s][v][3] fp32 as hn_mesh_finish_f32 writes it (metres, y and z negated), faces [f][3] int32 vertex
 * indices (device), lifted [s] int32 or NULL (a slot with lifted == 0 is not drawn), paras = HOST fx, fy, cx, cy of the one
 * camera.  Vertices are projected with the plain pinhole u = (fx X) / Z + cx, v = (fy Y) / Z + cy, (X, Y, Z) = (x, -y, -z), in
 * fp32 with one rounding per operation, and snapped to 1/256 pixel; pixel (col, row) is sampled at (col + 0.5, row + 0.5);
 * coverage is decided by 64-bit integer edge functions with the top-left rule, both windings; the nearest Z wins (the lower
 * slot, then the lower face on an exact tie); a face with a vertex that is non-finite, nearer than 0.05 m, farther than 100 m
 * or snapped beyond 2^24, a face of zero area and a face with an index outside [0, v) are not drawn (no clipping).  Covered
 * pixels get the face's flat colour, floor(255 min(1, 0.3 + 2.4 |n_z| / (|n| pi)) (1, 1, 0.9) + 0.5); every other pixel is
 * the frame's: frame = fp32 [n][3][h][w] in 0..1 (HN_FRAME_F32_CHW: rint(255 x)) or uint8 [n][h][w][3] 'bgr8'
 * (HN_FRAME_U8_BGR_HWC).  out_image [n][h][w][3] uint8 RGB; out_depth [n][h][w] fp32 or NULL: Z of the drawn face, 0 where
 * nothing was drawn.  Two launches on the caller's stream, no allocation, no atomics: the image is a pure function of the
 * arguments.  scratch: hn_mesh_render_scratch_bytes(s, f) bytes on the device, 16-byte aligned.  faces_host (or NULL): a host
 * copy of `faces`; when given, an index outside [0, v) is an argument error (nothing is launched).  h, w <= 16384.
 * Added under ABI 36: new functions only. */
#define HN_FRAME_F32_CHW 0
#define HN_FRAME_U8_BGR_HWC 1
int64_t hn_mesh_render_scratch_bytes(int s, int f);
int hn_mesh_render_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host /* or NULL */,
                      const int32_t* lifted /* or NULL */, int s, int v, int f, int k, const float* paras, const void* frame,
                      int frame_format, int h, int w, void* scratch, int64_t scratch_bytes, uint8_t* out_image,
                      float* out_depth /* or NULL */, void* stream);
/* hn_mesh_render_u8 with the mesh hidden behind nearer scene depth: the same arguments, rule and two
 * launches, plus scene_depth = the camera's depth map in metres, fp32, frame i at scene_depth + i * depth_frame_stride as
 * [h][w] (depth_frame_stride in elements, >= h * w: channel 3 of an [n][4][h][w] RGBD tensor is passed as its address with
 * 4 * h * w), and margin in metres (finite).  For a pixel covered by a mesh, with best = the nearest mesh Z and D = the depth
 * map's value: D is valid when it is finite and > 0 (holes -- 0 or NaN -- hide nothing), and the pixel is hidden when D is
 * valid and best > D + margin (one fp32 addition, a strict comparison).  out_image: the face's colour where covered and not
 * hidden, the frame's pixel elsewhere.  out_depth (or NULL): the nearest mesh Z on every covered pixel, hidden or not, else 0.
 * out_silhouette [n][h][w] uint8: 0 = no mesh, slot + 1 = covered and shown, 0x80 | (slot + 1) = covered and hidden, slot =
 * the winning face's slot within its frame (k <= 16).  out_coverage [s][2] int32 or NULL: per slot, (pixels where its mesh is
 * the nearest mesh, of those the shown ones); (0, 0) for a slot with lifted == 0.  The counters are zeroed by the first launch
 * and filled by integer atomic adds of the second: exact, and the same in every run.  No allocation, no launch beyond the two.
 * Added under ABI 36: a new function only. */
int hn_mesh_render_occluded_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host /* or NULL */,
                               const int32_t* lifted /* or NULL */, int s, int v, int f, int k, const float* paras,
                               const void* frame, int frame_format, int h, int w, const float* scene_depth,
                               int64_t depth_frame_stride, float margin, void* scratch, int64_t scratch_bytes,
                               uint8_t* out_image, float* out_depth /* or NULL */, uint8_t* out_silhouette,
                               int32_t* out_coverage /* or NULL */, void* stream);
/* hn_mesh_render_u8 / hn_mesh_render_occluded_u8 with a camera per frame: the same arguments, rule and
 * two launches, with cams = DEVICE fp32 [s / k][4], rows (fx, fy, cx, cy), in place of the host's paras.  Slot i * k + j (hand j
 * of frame i) is projected with row i.  The table is read by the first launch, on the stream: a captured graph holds its
 * address, not its values, so new values copied into it (on the same stream, or before the replay is enqueued) take effect at
 * the next replay.  A table of equal rows gives the bytes of the one-camera entries.  The occluded form is an entry of its own
 * beside the plain one, as hn_mesh_render_occluded_u8 is beside hn_mesh_render_u8.  Added under ABI 36: new functions only. */
int hn_mesh_render_cams_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host /* or NULL */,
                           const int32_t* lifted /* or NULL */, int s, int v, int f, int k, const float* cams, const void* frame,
                           int frame_format, int h, int w, void* scratch, int64_t scratch_bytes, uint8_t* out_image,
                           float* out_depth /* or NULL */, void* stream);
int hn_mesh_render_cams_occluded_u8(const float* mesh, const int32_t* faces, const int32_t* faces_host /* or NULL */,
                                    const int32_t* lifted /* or NULL */, int s, int v, int f, int k, const float* cams,
                                    const void* frame, int frame_format, int h, int w, const float* scene_depth,
                                    int64_t depth_frame_stride, float margin, void* scratch, int64_t scratch_bytes,
                                    uint8_t* out_image, float* out_depth /* or NULL */, uint8_t* out_silhouette,
                                    int32_t* out_coverage /* or NULL */, void* stream);
/* The live caller's two other images (ros_demo.py:310-326) for s = n * k hand slots: out_box [n][h][w][3] uint8 RGB = the frame
 * with the crop rectangle of every drawn slot of the frame in (0,255,0), thickness 1, inclusive corners (cv2.rectangle);
 * out_pose [s][176][176][3] uint8 RGB = frame[y1:y2, x1:x2] (clipped to the frame, exclusive ends) resized to 176 x 176 with
 * OpenCV's 8-bit fixed-point bilinear rule, the 21 joints (discs of radius 2) and 20 bones (8-connected lines) of
 * VisualUtil('dexycb').plot drawn over it at (int(u), int(v)); all zeros for a slot that is not drawn.  keypoints [s][21][3] fp32
 * crop-space (u, v, d), crop_box [s][4] int64 (x1, y1, x2, y2), drawn [s] int32 or NULL: a slot is drawn when drawn == 1 (NULL:
 * every slot) and its clipped crop is not empty.  clamp != 0: the caller's clamps first (x1, y1 to [0, h]; x2, y2 to [0, w], as
 * written at ros_demo.py:280-281; every keypoint coordinate to [0, 176]).  frame as for hn_mesh_render_u8.  Either output may
 * be NULL (not both).  At most two launches on the caller's stream; no allocation, no synchronisation, no atomics: every pixel
 * is written once and the images are a pure function of the arguments (DESIGN.md section 9c states the rule).  h, w <= 16384,
 * s <= 65535.  Added under ABI 36: a new function only. */
int hn_draw_labels_u8(const float* keypoints, const int64_t* crop_box, const int32_t* drawn /* or NULL */, int s, int k,
                      const void* frame, int frame_format, int h, int w, int clamp, uint8_t* out_box /* or NULL */,
                      uint8_t* out_pose /* or NULL */, void* stream);
/* The rig frame of a multi-camera K-hand step (tests/rig_ref.py is the rule in numpy float32, and the
 * outputs equal it bit for bit: fp32, one rounding per operation, fixed summation order, no atomics).  n cameras x k slots,
 * slot s = i * k + j uses row i of `extrinsics` (device, [n][12] = the rows of [R | t], camera -> rig, t in metres).
 *   rig_xyz  [n*k][joints][3]  transform of xyz_mm / 1000 where has_hand == 1, zero rows elsewhere
 *   rig_mesh [n*k][v][3]       transform of (x, -y, -z) of the final mesh (out['mesh']) where lifted == 1, zero rows elsewhere
 *   rig_hand [n*k]             the slot's rig hand, -1 for none: lifted slots of DIFFERENT cameras whose centres (mean rig_xyz)
 *                              lie within `radius` metres of the seed slot's centre -- greedy, frame-major, at most one slot
 *                              per camera, and of the same `side` when side is given (NULL: no side gate)
 *   rig_count [1], rig_views [n*k] (members per rig hand, 0 beyond the count), rig_seed [n*k] (seed slot, -1 beyond the count)
 *   fused_xyz [n*k][joints][3], fused_mesh [n*k][v][3]   per rig hand: its one member copied, or its members' mean weighted by
 *                              `score`, summed in slot order; zero rows beyond the count
 * Every output is fully written.  Three launches on `stream`; n * k <= 256 and every other size are checked before the first. */
int hn_rig_fuse_f32(const float* xyz_mm, const float* mesh, const int32_t* has_hand, const int32_t* lifted, const float* score,
                    const int32_t* side /* or NULL */, const float* extrinsics, int n, int k, int joints, int v, float radius,
                    float* rig_xyz, float* rig_mesh, int32_t* rig_hand, int32_t* rig_count, int32_t* rig_views,
                    int32_t* rig_seed, float* fused_xyz, float* fused_mesh, void* stream);
/* Each hand's depth pixels as a compact 3-D point cloud (tests/cloud_ref.py is the rule in numpy float32,
 * and the outputs equal it bit for bit: fp32, one rounding per operation, integer sums, no atomics).  Inputs are what the occluded
 * overlay leaves on the device: mesh_depth = its out_depth [n][h][w], silhouette = its out_silhouette [n][h][w], scene_depth and
 * depth_frame_stride as hn_mesh_render_occluded_u8 takes them; exactly one of paras (HOST, 4 floats: one camera) and cams (DEVICE,
 * [n][4]: a camera per frame); extrinsics DEVICE [n][12] = the rows of [R | t] (the points in the rig frame) or NULL (the camera
 * frame: x right, y down, z forward, metres).  A pixel (r, c) with r % stride == 0 and c % stride == 0 matches slot j of frame i
 * when (silhouette & 0x7F) == j + 1, D = scene_depth is finite and > 0, and |D - mesh_depth| <= band; its point is
 * ((c + 0.5 - cx) * D / fx, (r + 0.5 - cy) * D / fy, D) -- the pixel centre at +0.5, the raster's sample point.
 *   out_cloud [n*k][points][3]  slot s = i * k + j: its first min(total, points) matches in row-major order, zero rows behind them
 *   out_count [n*k][2]          (total matches, rows written)
 *   out_resid [n*k]             the sum of (int32)rint((D - mesh_depth) * 1e6) over ALL matches: micrometres, int64
 * Every output is fully written.  Two launches on `stream`; every argument is checked before the first (k 1..16, h and w
 * 1..16384, points and stride >= 1, 0 < band <= 100, scratch of hn_hand_cloud_scratch_bytes(n, k, h) bytes, 8-byte aligned). */
int64_t hn_hand_cloud_scratch_bytes(int n, int k, int h);
int hn_hand_cloud_f32(const float* mesh_depth, const uint8_t* silhouette, const float* scene_depth, int64_t depth_frame_stride,
                      const float* paras /* host, or NULL */, const float* cams /* device [n][4], or NULL */,
                      const float* extrinsics /* device [n][12] or NULL: camera frame */, int n, int k, int h, int w, int points,
                      int stride, float band, void* scratch, int64_t scratch_bytes, float* out_cloud, int32_t* out_count,
                      int64_t* out_resid, void* stream);
/* Each hand's mesh fitted to its measured depth: ONE Gauss-Newton step of projective point-to-plane alignment per hand slot
 * (tests/fit_ref.py is the rule in numpy, and the outputs equal it bit for bit: one rounding per fp32 and
 * fp64 operation, integer sums, no atomics).  mesh_depth, silhouette, scene_depth, depth_frame_stride, paras / cams: as
 * hn_hand_cloud_f32 takes them (exactly one of paras -- HOST, 4 floats -- and cams -- DEVICE [n][4]).  mesh DEVICE [n*k][v][3]: the
 * meshes the raster drew (metres, (x, -y, -z) of the camera point); xyz_mm DEVICE [n*k][joints][3]: camera millimetres (x right, y
 * down, z forward); joint 0 is the root the motion turns about.  A pixel (r, c), 1 <= r <= h - 2, 1 <= c <= w - 2, r % stride == 0
 * and c % stride == 0, matches slot j of frame i when (silhouette & 0x7F) == j + 1 there and at its four neighbours, mesh_depth > 0
 * at all five, D = scene_depth is finite and > 0, |D - mesh_depth| <= band, and its normal (from mesh_depth), lever and residual
 * pass the rule's bounds.  The 6 x 6 normal equations are damped by damp * matches (rotation rows: times 0.1^2 m^2), solved in
 * fp64; a step with fewer than min_points matches (status 1), a failed pivot or a non-finite solution (2) or a motion beyond
 * max_shift2 = max_shift^2 (metres^2) or tan2_half_angle = tan^2(max_angle / 2) (3) leaves the slot as it is.
 *   out_mesh [n*k][v][3], out_xyz [n*k][joints][3]   the moved mesh and joints (status != 0: byte copies of the inputs)
 *   out_rt [n*k][12]      R row-major, then t: x' = R (x - c0) + c0 + t in the camera frame, c0 = the root joint in metres
 *   out_count [n*k][2]    (matches, status)
 *   out_cost [n*k]        the sum of rint(rho^2 * 2^30) over the matches, int64: RMS = sqrt(cost / 2^30 / matches) metres
 * Every output is fully written.  Two launches on `stream`; every argument is checked before the first (k 1..16, h and w
 * 1..16384, v 1..2^24, joints 1..4096, stride and min_points >= 1, 0 < band <= 100, damp >= 0 and finite, both caps finite and > 0,
 * scratch of hn_mesh_fit_scratch_bytes(n, k, h) bytes, 8-byte aligned). */
int64_t hn_mesh_fit_scratch_bytes(int n, int k, int h);
int hn_mesh_fit_f32(const float* mesh_depth, const uint8_t* silhouette, const float* scene_depth, int64_t depth_frame_stride,
                    const float* paras /* host, or NULL */, const float* cams /* device [n][4], or NULL */, const float* mesh,
                    const float* xyz_mm, int n, int k, int h, int w, int v, int joints, int stride, float band, int min_points,
                    double damp, double max_shift2, double tan2_half_angle, void* scratch, int64_t scratch_bytes, float* out_mesh,
                    float* out_xyz, float* out_rt, int32_t* out_count, int64_t* out_cost, void* stream);
/* The geometry pass of the overlay's raster (tests/refit_ref.py::geometry is the rule in numpy float32, and
 * the outputs equal it bit for bit): the nearest mesh Z and its slot per pixel, and nothing else -- no frame, no image, no scene
 * depth, no hidden flag, no coverage.  mesh, faces, faces_host, lifted, s, v, f, k, h, w, scratch: as hn_mesh_render_u8 takes them
 * (scratch of hn_mesh_render_scratch_bytes(s, f) bytes, 16-byte aligned; k 1..16); exactly one of paras (HOST, 4 floats) and cams
 * (DEVICE [s / k][4]).  Projection, snapping, rejection, winding, boxes, coverage and depth are the raster's own: out_depth equals
 * the occluded raster's out_depth and out_who its silhouette & 0x7F, bit for bit.
 *   out_depth [s / k][h][w]  fp32: the nearest Z, 0 where nothing was drawn
 *   out_who   [s / k][h][w]  uint8: 0, or the nearest slot within the frame + 1
 * Both are fully written.  Two launches on `stream`; every argument is checked before the first. */
int hn_mesh_geometry_f32(const float* mesh, const int32_t* faces, const int32_t* faces_host /* or NULL */,
                         const int32_t* lifted /* or NULL */, int s, int v, int f, int k, const float* paras /* host, or NULL */,
                         const float* cams /* device [s / k][4], or NULL */, int h, int w, void* scratch, int64_t scratch_bytes,
                         float* out_depth, uint8_t* out_who, void* stream);
/* The depth fit iterated (tests/refit_ref.py::mesh_fit_iters is the rule, and the outputs equal it bit for
 * bit): `iters` (1..8) Gauss-Newton steps of hn_mesh_fit_f32.  Iteration 1 runs on the caller's mesh_depth / silhouette; before
 * every further iteration the current meshes are drawn again by hn_mesh_geometry_f32 (faces, faces_host, lifted, f: as it takes
 * them; a slot with lifted == 0 is not drawn) and the step turns about the current root joint.  Every iteration applies the
 * parameters and caps on its own; a slot whose iteration ends with a status other than 0 keeps its bytes for that iteration and is
 * tried again in the next.  There is no early stop: 2 + 4 (iters - 1) + 1 launches on `stream`, whatever the data.
 *   out_mesh, out_xyz     the state after the last iteration
 *   out_count, out_cost   those of iteration 1: what hn_mesh_fit_f32 hands out
 *   out_trace [n*k][iters][3]  int64 (matches, status, cost) of every iteration; the cost of iteration t is the residual after
 *                         t - 1 motions
 *   out_rt [n*k][12]      the composed motion about the ORIGINAL root joint c0 (fp64, rounded to fp32 at the end): the first
 *                         iteration with status 0 gives R = R_t, T = t_t; every further one, with u = (c0 + T) - c_t,
 *                         T <- (((R_t u)_j + c_t_j) + t_t_j) - c0_j and R <- R_t R; none: the identity
 * scratch: hn_mesh_fit_scratch_bytes(n, k, h) bytes, 8-byte aligned; work: hn_mesh_fit_iters_scratch_bytes(...) bytes, 16-byte
 * aligned (the intermediate meshes and joints, every iteration's motion, the geometry pass's outputs and scratch).  Every argument
 * is checked under this entry's name before the first launch. */
int64_t hn_mesh_fit_iters_scratch_bytes(int n, int k, int h, int w, int v, int f, int joints, int iters);
int hn_mesh_fit_iters_f32(const float* mesh_depth, const uint8_t* silhouette, const float* scene_depth, int64_t depth_frame_stride,
                          const float* paras /* host, or NULL */, const float* cams /* device [n][4], or NULL */, const float* mesh,
                          const float* xyz_mm, const int32_t* faces, const int32_t* faces_host /* or NULL */,
                          const int32_t* lifted /* or NULL */, int n, int k, int h, int w, int v, int f, int joints, int iters,
                          int stride, float band, int min_points, double damp, double max_shift2, double tan2_half_angle,
                          void* scratch, int64_t scratch_bytes, void* work, int64_t work_bytes, float* out_mesh, float* out_xyz,
                          float* out_rt, int32_t* out_count, int64_t* out_cost, int64_t* out_trace, void* stream);
/* The object each hand holds (tests/object_ref.py is the rule in numpy float32, and the outputs equal it bit
 * for bit: one rounding per operation, integer sums, no atomics).  det_* DEVICE: the detector's rows of n frames, `cap` rows each
 * (boxes [n][cap][4] x1 y1 x2 y2, scores, labels, count [n] -- clamped to 0..cap); contacts [n][cap] and dxdymags [n][cap][3]
 * (magnitude, x, y): what hn_fcos_ext_gather leaves; det_index [n][k]: each hand slot's detection row (< 0, or >= cap: an empty
 * slot).  scene_depth / depth_frame_stride, paras / cams: as hn_hand_cloud_f32 takes them (exactly one of paras -- HOST, 4 floats --
 * and cams -- DEVICE [n][4]); silhouette DEVICE [n][h][w] or NULL; xyz_mm DEVICE [n*k][joints][3], joint 0 the root.
 * Association (voc_eval.py:687-699 on the detections as they are): a slot whose contact state is > 0 takes, among the frame's rows
 * of `object_label`, the one whose centre is nearest to hand centre + (magnitude * 10000) * (x, y); the sequential scan's ties (the
 * earlier rank) and NaN behaviour (a NaN distance only stays when it is the first object's).  Then the candidates (r % stride == 0,
 * c % stride == 0) whose centre (c + 0.5, r + 0.5) lies in the object's box [x1, x2) x [y1, y2), whose depth D is finite and > 0,
 * whose silhouette byte names no slot ((byte & 0x7F) == 0; NULL: not tested) and |D - xyz_mm[s][0][2] * 0.001| <= band are
 * back-projected as hn_hand_cloud_f32 does and reduced.
 *   out_contact [n*k]     the slot's contact state (-1: empty slot)
 *   out_index   [n*k]     the object's detection row, or -1
 *   out_box     [n*k][4]  its box, out_score [n*k] its score (zeros: no object)
 *   out_point   [n*k][2]  the point the hand's vector names (zeros: empty slot)
 *   out_xyz     [n*k][3]  (float)((double)sum of rint(coordinate * 1e6) / (matches * 1e6)), metres; zeros unless the status is 0
 *   out_extent  [n*k][6]  minimum x y z, maximum x y z over the matches; zeros without a match
 *   out_count   [n*k][2]  (matches, status: 0 ok, 1 no object, 2 fewer than min_points matches, -1 empty slot)
 * Every output is fully written.  Three launches on `stream`; every argument is checked before the first (k 1..16, h and w
 * 1..16384, cap 1..2^24, stride and min_points >= 1, 0 < band <= 100, scratch of hn_hand_objects_scratch_bytes(n, k, h) bytes,
 * 8-byte aligned). */
int64_t hn_hand_objects_scratch_bytes(int n, int k, int h);
int hn_hand_objects_f32(const float* det_boxes, const float* det_scores, const int32_t* det_labels, const int32_t* det_count,
                        const int32_t* contacts, const float* dxdymags, const int32_t* det_index, int cap, int object_label,
                        const float* scene_depth, int64_t depth_frame_stride, const uint8_t* silhouette /* or NULL */,
                        const float* xyz_mm, int joints, const float* paras /* host, or NULL */,
                        const float* cams /* device [n][4], or NULL */, int n, int k, int h, int w, int stride, float band,
                        int min_points, void* scratch, int64_t scratch_bytes, int32_t* out_contact, int32_t* out_index,
                        float* out_box, float* out_score, float* out_point, float* out_xyz, float* out_extent, int32_t* out_count,
                        void* stream);
/* The held objects on the box label image, IN PLACE on box_label DEVICE uint8 [n][h][w][3] (tests/object_ref.py draw_object_labels
 * is the rule): for every slot with object_index >= 0, the object's rectangle (thickness 1, inclusive corners) and the line
 * (8-connected Bresenham, tests/draw_ref.py line_points) from the hand box's centre to the object box's centre, both in (0, 0, 255);
 * corners and centres ((a + b) * 0.5 in fp32) are rounded to the nearest integer, ties to even, and saturated at +-2^20 (NaN: 0).
 * Every other pixel is left as it is.  One launch. */
int hn_draw_object_labels_u8(const float* det_boxes, const int32_t* det_index, const int32_t* object_index, int cap, int n, int k,
                             int h, int w, uint8_t* box_label, void* stream);
/* The hand-pose evaluator's tables for the evaluation loop (tests/hpe_ref.py is the rule in numpy fp64, and
 * every output equals it bit for bit): what HPEEvaluator.evaluate feeds its three EvalUtil accumulators -- the absolute, the
 * root-relative and the Procrustes-aligned (align_w_scale, reflections allowed) distance of every joint -- added into an integer
 * state.  pred, gt DEVICE fp32 [s][j][3] in millimetres; valid DEVICE int32 [s] or NULL; thresholds DEVICE fp64 [t], non-decreasing.
 * A sample is fed when valid != 0 (or NULL) and all its values are finite and below 2^20 in magnitude; any other sample is counted
 * as skipped and adds nothing else.
 *   hist [3][j][t+1]  int64 += 1 at bin #{i : thresholds[i] < d} per alignment (ab, rr, pa), joint and fed sample
 *   sum  [3][j]       int64 += rint(d * 2^20), ties to even
 *   n    [2]          int64 += (fed, skipped)
 *   dist_out [s][3][j], aligned_out [s][j][3]   fp64, or NULL (not written): the distances and align_w_scale(gt, pred); every
 *                     row is written, NaN for a skipped sample
 * The state is ADDED to (the caller zeroes it once); integer adds only, so any order of samples and any split into calls gives
 * the same bytes.  One launch on `stream`, no allocation, no synchronisation.  Refused before the launch: s < 0, j outside 1..64
 * (one lane per joint), t outside 1..1024, a null required pointer, a misaligned one; s == 0 is a successful no-op.  Added under
 * ABI 36: a new function only. */
int hn_hpe_accumulate_f32(const float* pred, const float* gt, const int32_t* valid /* or NULL */, int s, int j,
                          const double* thresholds, int t, int64_t* hist, int64_t* sum, int64_t* n, double* dist_out /* or NULL */,
                          double* aligned_out /* or NULL */, void* stream);
/* The detector evaluation's per-image part (tests/ap_ref.py is the rule in numpy fp64, and every output
 * equals it byte for byte): the records trainval_net_fcos.py:132-169 selects from a batch of detections (score > score_min and
 * label == hand_label / object_label, in the detector's order; an image without hand records keeps no object records), passed
 * through the VOC text files' rounding (pascal_voc.py:339-343), associated (voc_eval.py:662-704) and matched against the image's
 * ground truth (voc_eval.py:191-225,386-496) for the object class and the five hand tables.
 *   the batch, DEVICE: boxes fp32 [n][cap][4], scores fp32 [n][cap], labels / sides / contacts int32 [n][cap], dxdymags fp32
 *   [n][cap][3], count int32 [n] (rows at or beyond it are not read), image_ids int32 [n]
 *   the ground truth, DEVICE, indexed by image id: hand_off int32 [images+1] into hand_box int32 [hand_total][4], hand_meta int32
 *   [hand_total][4] (difficult, handstate, leftright, objectbbox present) and hand_obj fp64 [hand_total][4]; obj_off int32
 *   [images+1] into obj_box int32 [obj_total][4] and obj_diff int32 [obj_total].  At most 64 boxes per image and class: an image
 *   with more (or with offsets outside the table) is matched as if it had none -- hn_amd.ops.det_ap_table refuses such a table.
 *   the state: hand, obj int32 [images][max_dets], one word per record at [image id][rank]: bits 0..9 the score in thousandths,
 *   bits 10..14 TP and 15..19 FP of the tables '', handstate, handside, objectbbox, all (obj: bits 10 and 15), bit 20 valid;
 *   fed int32 [images] += 1 per image of the batch; overflow int32 [1] += the records that do not fit (rank >= max_dets, or a
 *   score above 1) + the image ids outside 0..images-1 (nothing else is written for those).
 * Records are plain stores, the counts integer atomic adds.  One launch on `stream`, no allocation, no synchronisation.  Refused
 * before the launch: negative sizes, images * max_dets above 2^27, n * cap above 2^28, equal labels, score_min outside [0, 1),
 * a null required pointer, a misaligned one; n == 0 is a successful no-op.  Added under ABI 36: a new function only. */
int hn_det_ap_accumulate_f32(const float* boxes, const float* scores, const int32_t* labels, const int32_t* sides,
                             const int32_t* count, const int32_t* contacts, const float* dxdymags, const int32_t* image_ids, int n,
                             int cap, const int32_t* hand_off, const int32_t* hand_box, const int32_t* hand_meta,
                             const double* hand_obj, int hand_total, const int32_t* obj_off, const int32_t* obj_box,
                             const int32_t* obj_diff, int obj_total, int images, int hand_label, int object_label, float score_min,
                             double ovthresh, int32_t* hand, int32_t* obj, int32_t* fed, int32_t* overflow, int max_dets,
                             void* stream);
/* A Linear layer on 1..4 rows as a matrix-vector product on the vector ALU (PoseNet at the live caller's batch, posenet.py:24-41,
 * 78-88: 67 MB of filter bank per 17 M MACs): y[m][:] = act(W (pre(x[m])) + bias (+ residual[m])), pre = relu(x * scale + shift)
 * when scale / shift ([k_real] fp32: the pre-activation BatchNorm) are given.  x fp32 [batch][x_stride] (k_real columns used), w16 =
 * the split bank [n][k/32][2][32] (k % 32 == 0, columns >= k_real zero), y / residual fp32.  w = hi + lo exactly and fp32
 * activations: at least as precise as the three-term MFMA form. */
int hn_linear_rows_f16x3(const float* x, int batch, int x_stride, int k_real, const float* scale, const float* shift,
                         const void* w16, int k, int n, const float* bias, const float* residual, int res_stride, int relu,
                         float* y, int y_stride, void* stream);
int hn_lifter_combine_f32(const float* pose2d /* [batch][joints][2] */, const float* pose3d /* [batch][pose3d_stride], 3*joints used */,
                          int batch, int joints, int pose3d_stride, int fpad, float* out, void* stream);
int hn_cheby3_basis_split(const int32_t* indptr, const int32_t* indices, const float* values, int v,
                          const float* x0, const float* x1, void* out16, int batch, int f, int cpad,
                          void* stream);
int hn_feat_interp_add_f32(const float* xin, const float* y, float* out, int64_t rows, int fi, int fo,
                           int up, void* stream);

/* ------------------------------------------------------------------------------------
 * Model-level entry points: the layer graphs of the detector, the pose network and the HandNet glue in C++
 * (csrc/model.hip), for hosts that are not Python.  They issue exactly the launches the Python engines issue
 * (hn_amd/fcos_engine.py, a2j_engine.py, pipeline.py), so both hosts give bit-identical results.
 *   hn_create          configuration -> handle
 *   hn_load_weight     one entry of a REFERENCE-layout state_dict ("backbone.body.conv1.weight",
 *                      "head.classification_head.conv.0.weight", "Backbone.model.layer1.0.bn1.running_var", ...;
 *                      a leading "a2j." is stripped, a2j/a2j.py:277), fp32 HOST data in torch layout; unknown names
 *                      are kept and ignored (strict=False, handnet_pipeline.py:20,33)
 *   hn_finalize        folds (Frozen)BatchNorm in fp64, repacks to [Cout][R][S][Cin], splits into fp16 hi/lo banks
 *                      (fails if a folded weight leaves the fp16 range), uploads.  Allocates and synchronises.
 *   hn_fcos_forward    fcos_utils/fcos.py:675-767 (eval; hn_fcos_forward_ext adds the ext=True outputs): rgb [n][3][h][w] fp32 0..1 on the device ->
 *                      score-ordered detections, fixed capacity cap = hn_fcos_capacity(m, h, w) rows per image:
 *                      det_boxes [n][cap][4] (original-image pixels), det_scores / det_labels / det_sides /
 *                      det_level [n][cap], det_count [n]
 *   hn_a2j_forward     a2j/a2j.py:243-250: crops [k][1][h][w] fp32 metres -> keypoints [k][J][3] (u, v, d) on the
 *                      device (the reference's .cpu() is the caller's copy); rows with valid[i] == 0 are zeros
 *   hn_handnet_forward(_xyz) handnet_pipeline/handnet_pipeline.py:58-116: rgb [n][3][h][w] + depth [n][1][h][w] (RGB-D
 *                      model: [n][4][h][w]) -> keypoints [n][J][3], crop_box [n][4] int64 (padded, clamped
 *                      x1,y1,x2,y2), has_hand [n]; frames without a hand give zero rows (deviations)
 * All tensors are device pointers borrowed from the caller; work is enqueued on `stream`.  Activations live in one
 * arena per model, sized by a dry pass over the graph: a forward allocates (and synchronises the device) only when
 * it needs more memory than any earlier call of this model; steady-state calls do neither.  One model must not be
 * used from two host threads at once (the reference callable is not re-entered either, ros_demo.py:240-257).
 * ------------------------------------------------------------------------------------ */
#define HN_MODEL_FCOS 1
#define HN_MODEL_A2J 2
#define HN_PRECISION_SPLIT 0
#define HN_PRECISION_F32 1
typedef struct hn_model_config {
  int32_t parts;        /* HN_MODEL_FCOS | HN_MODEL_A2J */
  int32_t num_classes;  /* FCOS classes (ros_demo.py:374 uses 3); hand class = num_classes - 1 */
  int32_t num_joints;   /* 21 */
  int32_t rgbd;         /* 1: 4-channel A2J stem + RGB-D crops with the [2,1,0,3] permutation */
  int32_t min_size, max_size; /* GeneralizedRCNNTransform sizes; 0 = 800 / 1333 (fcos.py:460-461) */
  int32_t ext;          /* 1: also load the ext=True heads (hand_dydx_layer, hand_contact_state_layer; the FCOS class
                           default, fcos.py:255-264) for hn_fcos_forward_ext */
  int32_t f16_terms;    /* 0 or 3: f16x3, the parity-grade default.  1: the f16x1 THROUGHPUT mode -- every convolution of
                           the layer graphs issues the hi*hi term only (hn_conv_desc.terms = 1): 1.4x faster, keypoints
                           ~0.08 px from the reference, outside the 1e-3 contract */
  int32_t precision;    /* HN_PRECISION_SPLIT (0): the split-fp16 kernels above.  HN_PRECISION_F32 (1): the reference's own
                           arithmetic -- every convolution on the exact f32-MFMA kernel (hn_conv2d_nhwc_f32), fp32 activations,
                           GroupNorm applied while the next convolution stages its input; ~4x slower, no fp16-range contract
                           (the mode to run a checkpoint in that trips hn_finalize's / the engines' range check).  Same
                           launches as FCOSEngine / A2JEngine(precision="f32"): bit-identical results */
  float image_mean[3], image_std[3]; /* the transform's normalisation (FCOS ctor arguments, fcos.py:501-505); image_std all
                           zero = the reference's default (ImageNet's 0.485 / 0.456 / 0.406, 0.229 / 0.224 / 0.225) */
} hn_model_config;
typedef struct hn_model hn_model;

int hn_create(const hn_model_config* cfg, hn_model** out);
int hn_load_weight(hn_model* m, const char* name, const float* host_data, const int64_t* shape, int ndim);
int hn_finalize(hn_model* m);
int64_t hn_fcos_capacity(const hn_model* m, int h, int w);
int hn_fcos_forward(hn_model* m, const float* rgb, int n, int h, int w, float* det_boxes, float* det_scores,
                    int32_t* det_labels, int32_t* det_sides, int32_t* det_level, int32_t* det_count, int cap,
                    void* stream);
/* A list of differently sized images (torchvision batch_images, fcos.py:702-709, as FCOS.forward takes it): images = HOST
 * array of n DEVICE pointers to fp32 [3][hs[i]][ws[i]], hs / ws HOST arrays.  Each image is resized on its own into the
 * common canvas and its boxes are rescaled by its own ratios; cap = hn_fcos_capacity_list(m, hs, ws, n). */
int64_t hn_fcos_capacity_list(const hn_model* m, const int32_t* hs, const int32_t* ws, int n);
int hn_fcos_forward_list(hn_model* m, const float* const* images, const int32_t* hs, const int32_t* ws, int n,
                         float* det_boxes, float* det_scores, int32_t* det_labels, int32_t* det_sides, int32_t* det_level,
                         int32_t* det_count, int cap, void* stream);
/* ext=True detections (fcos.py:637-647): additionally det_contacts [n][cap] (argmax of the contact state) and
 * det_dxdymags [n][cap][3] (magnitude, 0.1 * unit dx, 0.1 * unit dy) per kept detection. */
int hn_fcos_forward_ext(hn_model* m, const float* rgb, int n, int h, int w, float* det_boxes, float* det_scores,
                        int32_t* det_labels, int32_t* det_sides, int32_t* det_level, int32_t* det_count,
                        int32_t* det_contacts, float* det_dxdymags, int cap, void* stream);
int hn_a2j_forward(hn_model* m, const float* crops, int k, int h, int w, const int32_t* valid /* or NULL */,
                   float* keypoints, void* stream);
int hn_handnet_forward(hn_model* m, const float* rgb, const float* depth, int n, int h, int w, float* keypoints,
                       int64_t* crop_box, int32_t* has_hand, void* stream);
/* hn_handnet_forward for up to max_hands (1..16) hands per frame: the detector, hn_crop_resize_hands, then A2J on the
 * n * max_hands crops.  keypoints [n][max_hands][J][3], crop_box [n][max_hands][4] int64, has_hand [n][max_hands] int32,
 * score [n][max_hands] fp32, all device; empty slots give zero rows.  max_hands = 1 is hn_handnet_forward. */
int hn_handnet_forward_hands(hn_model* m, const float* rgb, const float* depth, int n, int h, int w, int max_hands,
                             float* keypoints, int64_t* crop_box, int32_t* has_hand, float* score, void* stream);
/* hn_handnet_forward + what the reference's caller computes from its results right away (ros_demo.py:289,329-330;
 * a2j/a2j.py:17-43): image (u,v,d) and / or camera xyz in mm per joint, written by the aggregation's epilogue
 * (hn_a2j_aggregate_convert_f32) -- same launches as hn_handnet_forward.  image_uvd / xyz_mm [n][J][3] device, either may be
 * NULL (not both); paras (host: fx, fy, cx, cy) is needed for xyz_mm; opts as in hn_a2j_aggregate_convert_f32. */
int hn_handnet_forward_xyz(hn_model* m, const float* rgb, const float* depth, int n, int h, int w, const float* paras,
                           const hn_convert_opts* opts, float* keypoints, float* image_uvd, float* xyz_mm, int64_t* crop_box,
                           int32_t* has_hand, void* stream);
int hn_destroy(hn_model* m);

#ifdef __cplusplus
}
#endif
#endif /* HANDNET_HIP_H */
