// f16x3 implicit-GEMM convolution: the grouped row-shared 128 x 128 launch that CARRIES a GroupNorm apply pass
// (hn_conv2d_nhwc_f16x3_grouped_carry).  Device code of the convolution: conv_igemm_f16x3_kernel.h, unchanged; the apply
// arithmetic: affine_split_body.h, shared with the stand-alone pass (split_ops.hip).
//
// The FCOS tower convolutions are bound by the matrix pipe and by power and use a sixth of the HBM bandwidth; the GroupNorm
// apply pass between two tower layers (fp32 -> S32, 8 bytes per element) is a pure HBM stream.  The cls and the reg tower are
// independent chains, so the launch of one tower's layer can carry the apply pass of the OTHER tower's finished output: every
// workgroup, once its output tile is stored -- accumulators dead, registers free --, streams a few chunks of that tensor
// through the apply arithmetic and leaves.  No extra workgroups (an apply workgroup beside the convolution's inherits its LDS
// and register footprint and so takes a convolution slot of its CU: profiles/NOTEBOOK.md, two-role entry), no change to the k
// loop or the operand path, no second stream, and nothing a workgroup of this launch writes is read by another one: the
// carried tensor and its scale / shift tables were completed by EARLIER launches of the stream, the S32 blocks written here are
// read by LATER ones.
#include "affine_split_body.h"
#include "conv_igemm_f16x3_plan.h"

namespace {

constexpr int kCarryUnr = 8;   // pixels in flight per lane: a chunk is kCarryUnr passes of the 256 lanes (64 pixels x 256 channels)

// The carried pass, a by-value kernel argument (carry_tail reads it from the kernel-argument segment).  Chunks are numbered level by level, image by image: chunk i of level l covers pixels
// [k * chunk_px, (k + 1) * chunk_px) of image img with (img, k) = divmod(i - first_chunk[l], chunks_per_img[l]).
struct CarryJob {
  int count;                                   // levels; 0 = nothing to carry
  int relu, c8_log2, xs, as, ys;               // as hn_affine_split_f32_levels (strides in elements)
  int chunks;                                  // == first_chunk[count]
  int* range_flag;
  int hw[HN_FCOS_MAX_LEVELS];
  int nt[HN_FCOS_MAX_LEVELS];                  // streaming stores where the stand-alone pass uses them
  int first_chunk[HN_FCOS_MAX_LEVELS + 1];
  int cpi[HN_FCOS_MAX_LEVELS];                 // chunks per image
  unsigned mg_cpi[HN_FCOS_MAX_LEVELS], sh_cpi[HN_FCOS_MAX_LEVELS];   // magic pair of the division by cpi (magic_u31)
  const float* x[HN_FCOS_MAX_LEVELS];
  const float* scale[HN_FCOS_MAX_LEVELS];
  const float* shift[HN_FCOS_MAX_LEVELS];
  _Float16* y[HN_FCOS_MAX_LEVELS];
};

// Chunk i belongs to workgroup i mod total (wg = linear workgroup id, total = workgroups of the grid, those beyond a small
// member's tile count included): every chunk is done exactly once whatever the ratio of chunks to workgroups.  All loads of
// a chunk are issued before the first use; a lane keeps one 8-channel group, so its scale / shift are loaded once per chunk.
// No LDS, no barrier, no atomics (the range note is the stand-alone pass's plain store of 1).
__device__ __forceinline__ void carry_tail(const int wg, const int total) {
  typedef hn::as_f32x4 v4;
  // The job is read straight from the kernel-argument SEGMENT (constant address space), the level's fields with the uniform
  // index `lvl`: scalar loads with an SGPR offset, as the convolution body reads its member's fields.  (Handing the by-value
  // argument to this function, or indexing it dynamically, copies all of it to private memory: 296 bytes of scratch per lane.)
  typedef __attribute__((address_space(4))) const CarryJob KJob;
  typedef __attribute__((address_space(4))) const char KBytes;
  static_assert(sizeof(ConvParams16) % alignof(CarryJob) == 0, "the job follows the parameter block without padding");
  KJob& c = *(KJob*)((KBytes*)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(ConvParams16));
  if (c.count <= 0) return;
  const int c8_log2 = c.c8_log2;
  const int ch = ((int)threadIdx.x & ((1 << c8_log2) - 1)) * 8;
  const int prow = (int)threadIdx.x >> c8_log2, ppb = 256 >> c8_log2;
  for (int i = wg; i < c.chunks; i += total) {   // (wave-uniform)
    int lvl = 0;
#pragma unroll
    for (int l = 1; l < HN_FCOS_MAX_LEVELS; ++l)
      if (l < c.count && i >= c.first_chunk[l]) lvl = l;
    const int hw = c.hw[lvl], nt = c.nt[lvl], fc = c.first_chunk[lvl], cpi = c.cpi[lvl];
    const unsigned mg = c.mg_cpi[lvl], sh = c.sh_cpi[lvl];
    const float *x = c.x[lvl], *scale = c.scale[lvl], *shift = c.shift[lvl];
    _Float16* y = c.y[lvl];
    const int j = i - fc;
    const int img = fastdiv(j, mg, sh);
    const int pix0 = (j - img * cpi) * (kCarryUnr * ppb) + prow;
    const float* xi = x + ((long)img * hw) * c.xs + ch;
    _Float16* yi = y + ((long)img * hw) * c.ys + (ch >> 5) * 64 + (ch & 31);
    const long o = (long)img * c.as + ch;
    const v4 s0 = *reinterpret_cast<const v4*>(scale + o), s1 = *reinterpret_cast<const v4*>(scale + o + 4);
    const v4 t0 = *reinterpret_cast<const v4*>(shift + o), t1 = *reinterpret_cast<const v4*>(shift + o + 4);
    // ONE basic block from the first load to the last conversion: a branch between a store and the next pixel's arithmetic
    // makes the compiler wait for everything in flight, stores included (eight store round trips per chunk).  So the loads
    // are unconditional -- a short last chunk of an image reads its last pixel again --, the range note is taken once per
    // chunk, and only the stores are predicated.
    v4 a[kCarryUnr], b[kCarryUnr];
#pragma unroll
    for (int u = 0; u < kCarryUnr; ++u) {
      const int pix = pix0 + u * ppb;
      const float* q = xi + (long)(pix < hw ? pix : hw - 1) * c.xs;
      // plain loads: the stand-alone pass streams its stores only (streaming loads cost it 8 %)
      a[u] = *reinterpret_cast<const v4*>(q);
      b[u] = *reinterpret_cast<const v4*>(q + 4);
    }
    hn::as_f16x8 hi[kCarryUnr], lo[kCarryUnr];
    int* const flag = c.range_flag;
    const int relu = c.relu;
    bool bad = false;
#pragma unroll
    for (int u = 0; u < kCarryUnr; ++u)
      bad |= hn::affine_split_values(a[u], b[u], s0, s1, t0, t1, true, relu, flag != nullptr, hi[u], lo[u]) &
             (pix0 + u * ppb < hw);
    if (bad) *flag = 1;
    if (nt) {
#pragma unroll
      for (int u = 0; u < kCarryUnr; ++u)
        if (pix0 + u * ppb < hw) hn::split_store(hi[u], lo[u], yi + (long)(pix0 + u * ppb) * c.ys, true);
    } else {
#pragma unroll
      for (int u = 0; u < kCarryUnr; ++u)
        if (pix0 + u * ppb < hw) hn::split_store(hi[u], lo[u], yi + (long)(pix0 + u * ppb) * c.ys, false);
    }
  }
}

// The plain row-shared 128 x 128 kernel (conv_igemm_f16x3_kernel<128, 128, 2, 2, 2, true, true, TERMS>) + the tail.  `p` stays
// the FIRST kernel argument: the body reads the members' fields from the kernel-argument segment at offset 0.
template <int TERMS>
__global__ __launch_bounds__(256, 2) void conv_igemm_f16x3_carry_kernel(const ConvParams16 p, const CarryJob c) {
  conv_igemm_f16x3_body<128, 128, 2, 2, 2, true, true, TERMS>(p, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
  (void)c;   // (read from the kernel-argument segment, behind p)
  carry_tail((int)(blockIdx.z * gridDim.x + blockIdx.x), (int)(gridDim.x * gridDim.z));
}

template <int TERMS>
int launch_carry(const ConvParams16& p, int grid_x, int groups, int lds_bytes, const CarryJob& job, hipStream_t st) {
  static bool attr_set[64] = {};  // per device: the attribute belongs to the function's image on the current device
  int dev = 0;
  HN_CHECK_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    HN_CHECK_HIP(hipFuncSetAttribute((const void*)conv_igemm_f16x3_carry_kernel<TERMS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     lds_bytes));
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  hipLaunchKernelGGL((conv_igemm_f16x3_carry_kernel<TERMS>), dim3(grid_x, 1, groups), dim3(256), lds_bytes, st, p, job);
  HN_CHECK_LAUNCH("conv_igemm_f16x3_carry_kernel");
  return HN_OK;
}

// argument checks of hn_affine_split_f32_levels + the chunk table
int fill_job(const hn_split_levels* lv, int relu, int n, int c, int in_pix_stride, int affine_stride, int out_pix_stride,
             CarryJob& job) {
  HN_CHECK_ARG(lv, "hn_conv2d_nhwc_f16x3_grouped_carry: null levels");
  HN_CHECK_ARG(lv->count >= 1 && lv->count <= HN_FCOS_MAX_LEVELS, "level count must be 1..%d", HN_FCOS_MAX_LEVELS);
  HN_CHECK_ARG(n > 0 && c > 0 && c % 32 == 0, "bad dims (c must be a multiple of 32)");
  const int xs = in_pix_stride ? in_pix_stride : c;
  const int as = affine_stride ? affine_stride : c;
  const int ys = out_pix_stride ? out_pix_stride : 2 * c;
  HN_CHECK_ARG(xs >= c && xs % 4 == 0 && as >= c && as % 4 == 0 && ys >= 2 * c && ys % 64 == 0, "bad strides");
  const int c8 = c / 8;
  HN_CHECK_ARG((c8 & (c8 - 1)) == 0 && c8 <= 256, "the carried pass needs c = 32 .. 2048, a power of two (got %d)", c);
  int lg = 0;
  while ((1 << lg) < c8) ++lg;
  const int chunk_px = kCarryUnr * (256 >> lg);
  job.count = lv->count;
  job.relu = relu ? 1 : 0;
  job.c8_log2 = lg;
  job.xs = xs; job.as = as; job.ys = ys;
  job.range_flag = hn::range_flag_ptr();
  job.first_chunk[0] = 0;
  for (int l = 0; l < HN_FCOS_MAX_LEVELS; ++l) {
    const bool on = l < lv->count;
    if (on) {
      HN_CHECK_ARG(lv->x[l] && lv->y16[l] && lv->scale[l] && lv->shift[l] && lv->hw[l] > 0, "level %d: null pointer or hw <= 0", l);
      HN_CHECK_ARG((uintptr_t)lv->x[l] % 16 == 0 && (uintptr_t)lv->y16[l] % 16 == 0 && (uintptr_t)lv->scale[l] % 16 == 0 &&
                       (uintptr_t)lv->shift[l] % 16 == 0, "level %d: tensors must be 16-byte aligned", l);
    }
    const int cpi = on ? hn::cdiv(lv->hw[l], chunk_px) : 1;
    const int64_t next = (int64_t)job.first_chunk[l] + (on ? (int64_t)n * cpi : 0);
    HN_CHECK_ARG(next < ((int64_t)1 << 30), "too many pixels to carry");
    job.hw[l] = on ? lv->hw[l] : 0;
    job.nt[l] = on && (int64_t)n * lv->hw[l] * c * 4 >= ((int64_t)128 << 20) ? 1 : 0;
    job.first_chunk[l + 1] = (int)next;
    job.cpi[l] = cpi;
    magic_u31((unsigned)cpi, job.mg_cpi[l], job.sh_cpi[l]);
    job.x[l] = on ? lv->x[l] : nullptr;
    job.scale[l] = on ? lv->scale[l] : nullptr;
    job.shift[l] = on ? lv->shift[l] : nullptr;
    job.y[l] = on ? (_Float16*)lv->y16[l] : nullptr;
  }
  job.chunks = job.first_chunk[lv->count];
  return HN_OK;
}

}  // namespace

int hn::launch_conv_carry(const void* conv_params, size_t conv_params_bytes, int grid_x, int groups, int terms, int lds_bytes,
                          const void* job, hipStream_t st) {
  HN_CHECK_ARG(conv_params && job && conv_params_bytes == sizeof(ConvParams16), "launch_conv_carry: parameter block mismatch");
  const ConvParams16& p = *static_cast<const ConvParams16*>(conv_params);
  const CarryJob& j = *static_cast<const CarryJob*>(job);
  if (terms == 1) return launch_carry<1>(p, grid_x, groups, lds_bytes, j, st);
  return launch_carry<3>(p, grid_x, groups, lds_bytes, j, st);
}

// hn_conv2d_nhwc_f16x3_grouped + hn_affine_split_f32_levels (affine, per-level pointers, the same stride arguments) on a tensor
// that neither reads nor writes anything this convolution touches, as ONE launch.  Refused -- before anything is launched --
// unless the grouped launch takes the plain row-shared 128 x 128 kernel (hn_conv2d_f16x3_grouped_carry_applies).
extern "C" int hn_conv2d_nhwc_f16x3_grouped_carry(const hn_conv_desc* d, const hn_conv_group* group, const hn_split_levels* lv,
                                                  int relu, int n, int c, int in_pix_stride, int affine_stride,
                                                  int out_pix_stride, void* stream) {
  CarryJob job;
  HN_TRY16(fill_job(lv, relu, n, c, in_pix_stride, affine_stride, out_pix_stride, job));
  if (group)
    for (int l = 0; l < lv->count; ++l)
      for (int g = 0; g < group->count && g < HN_CONV_MAX_GROUP; ++g)
        HN_CHECK_ARG(lv->y16[l] != group->y[g] && lv->y16[l] != group->x16[g] && (const void*)lv->x[l] != group->y[g],
                     "the carried pass must not touch member %d's tensors", g);
  const hn::CarryHook hook = {&job, false};
  return hn::conv_grouped_run(d, group, stream, &hook);
}

extern "C" int hn_conv2d_f16x3_grouped_carry_applies(const hn_conv_desc* d, const hn_conv_group* group) {
  const hn::CarryHook hook = {nullptr, true};
  return hn::conv_grouped_run(d, group, nullptr, &hook) == HN_OK ? 1 : 0;
}
