"""Exact-arithmetic reference of the convolution kernels: operands for which every product a kernel forms and every partial sum, in
any order, is exactly representable in fp32 -- so the tile shape, the summation order, split-K, LDS staging and the MFMA shape
cannot change a bit and a kernel's output must equal an fp64 computation on the CPU bit for bit.  numpy and torch only; nothing
here reads the library.  The split rule and the S32 layout are split_ref's (not restated).

THE OPERAND FAMILIES.  v = a + b with a an integer, 1 <= |a| <= A, or v = 0 exactly (a = b = 0):
  g12   b in {-1, 0, 1} * 2^-12.  hi = fp16(v) = a and lo = fp16(v - hi) = b exactly for A <= 4 (2^-12 is below half an fp16 step
        of every |a| < 8, and the one tie, 1 - 2^-12, goes to the even 1.0; 2^-11 fails: 1 - 2^-11 is an fp16 number).  a != 0
        matters: with a = 0 the hi part would be b.
  g16   A = 1, b in {-1, 0, 1} * 2^-16: an fp16 SUBNORMAL lo part, exact.
  g6    b in {-1, 0, 1} * 2^-6, for the f32 kernel (which forms all four products: multiples of 2^-12).
  int   b = 0: the control (12 significant bits at most: no assumption on the MFMA's internal width is left).
THE MODELS (fp64, exact):  model3 = conv(xa, w) + conv(xb, wa)  -- hi*hi + hi*lo + lo*hi, the f16x3 kernels;  model1 = conv(xa, wa)
(ops.f16_terms(1));  model4 = conv(x, w) (the f32 kernel).  model3 differs from model4 by the lo*lo term, so a kernel that adds a
fourth term fails as well.
THE CONDITION (on the inputs, not a measurement):  S = conv(|x|, |w|) + |bias| + |residual| < LIMIT for every output element, LIMIT
= 2^10 (g12, g6, int: every partial sum is a multiple of 2^-12 below 2^10, 22 significant bits) or 2^6 (g16: multiples of 2^-16).
THE EPILOGUE.  bias and residual sit on the same grid and count in S; ReLU is exact; an fp32 output is the model itself, an S32
output is split_ref.split of it; GroupNorm-on-load tables are scale in {1, -1, 2, -2, 1/2} and an integer shift, with raw inputs
chosen so that the applied value is a family value (so relu(fma(raw, scale, shift)) stays on the grid).
THE EMULATION.  emulate() walks the implicit GEMM in numpy -- rows m -> (img, oy, ox), k tiles of 32 channels with the tap inner
(the order weights.split_f16x3 documents), the three terms, split-K chunks added in z order, the epilogue -- and takes one
deliberate mistake (MUTANTS) so that the bitwise comparison is known to be able to fail.
"""
import types

import numpy as np
import torch

import split_ref as sr

F, H, D = np.float32, np.float16, np.float64
Q = {"g12": 12, "g16": 16, "g6": 6, "int": 0}
LIMIT = {"g12": 2.0 ** 10, "g16": 2.0 ** 6, "g6": 2.0 ** 10, "int": 2.0 ** 10}
SENTINEL32 = F(sr.SENTINEL)

MUTANTS = (
    "lo_hi_dropped_in_last_ktile", "hi_lo_dropped_on_right_border", "fourth_term", "lo_subnormal_flushed",
    "pad_reads_previous_row", "pad_reads_next_image", "bottom_tap_skipped", "dilation_ignored_in_pad_test",
    "stride_origin_off_by_one", "last_m_row_dropped", "cout_tail_duplicated", "relu_before_residual", "relu_cols_rounded_to_8",
    "upsample_ceil", "splitk_last_chunk_dropped", "splitk_chunk_overlap", "slice_stride_ignored", "gn_affine_applied_to_padding",
)

_DEFAULTS = dict(
    kind="f16x3",          # "f16x3" or "f32" (the exact-f32 kernel, model4)
    stride=1, pad=0, dil=1, family="g12", A=2, zeros=0.0, seed=0,
    wseed=None,            # seed of the filter bank and bias where several cases share one (the levels of a thin launch); None: seed
    bias=True,
    res=None,              # None, "f32", "s32" (same size) or "up_f32", "up_s32" (nearest read of a ((oh+1)//2, (ow+1)//2) map)
    relu_cols=0, out_split=False,
    in_wide=None,          # (C of the wider input tensor, first channel): the input is a channel slice
    out_wide=None,         # (C of the wider output tensor, first channel): the output goes into a slice of a sentinel-filled arena
    x_f32=None,            # None: S32 input.  "plain": fp32 input through to_split.  "gn": with the GroupNorm-on-load tables
    tiles=(0,), splitk=False, force_splits=None, terms=3,
    route=None,            # what the library's queries must answer for this case: "igemm", "rs", "halo", "stream"
)


def make_case(name, group, n, h, w, cin, cout, r, s=None, **kw):
    c = dict(_DEFAULTS, name=name, group=group, n=n, h=h, w=w, cin=cin, cout=cout, r=r, s=r if s is None else s)
    unknown = set(kw) - set(_DEFAULTS)
    assert not unknown, unknown
    c.update(kw)
    return types.SimpleNamespace(**c)


def with_family(case, family):
    """the same case on another operand family (the `int` control: same shape, same zero pattern seed)"""
    c = types.SimpleNamespace(**vars(case))
    c.family, c.name = family, f"{case.name}[{family}]"
    if family == "g16":
        c.A = 1
    return c


def out_size(c):
    return ((c.h + 2 * c.pad - c.dil * (c.r - 1) - 1) // c.stride + 1, (c.w + 2 * c.pad - c.dil * (c.s - 1) - 1) // c.stride + 1)


def up_index(i, rh, oh):
    """nearest-neighbour source index of output row / column i of oh from a map of rh"""
    return (i * rh) // oh


def relu_cols(y, cols):
    """ReLU on the first `cols` channels only"""
    y = y.copy()
    y[..., :cols] = np.maximum(y[..., :cols], 0.0)
    return y


def arena(shape_nhw, cw, split):
    """a sentinel-filled output tensor of cw channels: fp32 [N,H,W,cw] or S32 [N,H,W,cw/32,2,32]"""
    if split:
        return np.full(tuple(shape_nhw) + (cw // 32, 2, 32), sr.SENTINEL, H)
    return np.full(tuple(shape_nhw) + (cw,), SENTINEL32, F)


# --------------------------------------------------------------------------------------------------------------------------
# operands
# --------------------------------------------------------------------------------------------------------------------------
def gen(family, shape, rng, A=2, zeros=0.0):
    """-> (v fp32, a fp64, b fp64) with v = a + b exactly, a the integer part (the hi half) and b the lo half"""
    if family == "g16":
        A = 1
    a = rng.integers(1, A + 1, size=shape) * rng.choice(np.array([-1, 1]), size=shape)
    b = rng.integers(-1, 2, size=shape) if family != "int" else np.zeros(shape, np.int64)
    z = rng.random(shape) < zeros
    a = np.where(z, 0, a).astype(D)
    b = np.where(z, 0, b).astype(D) * 2.0 ** -Q[family]
    v = (a + b).astype(F)
    assert (v.astype(D) == a + b).all()
    return v, a, b


GN_SCALES = np.array([1.0, -1.0, 2.0, -2.0, 0.5], F)


def operands(c):
    """every tensor of the case, seeded: x (the APPLIED input, fp32 [N,H,W,Cin]) with its halves xa / xb, xwide (what the input
    tensor holds: x in channels [c0, c0 + Cin)), raw / scale / shift (x_f32 == "gn": xwide = relu(fma(raw, scale, shift))), w with
    wa / wb, bias, res (at its own size)"""
    rng = np.random.default_rng(1000 + c.seed)
    o = types.SimpleNamespace()
    cw, c0 = c.in_wide if c.in_wide else (c.cin, 0)
    o.cw, o.c0 = cw, c0
    target, ta, tb = gen(c.family, (c.n, c.h, c.w, cw), rng, c.A, c.zeros)
    o.raw = o.scale = o.shift = None
    if c.x_f32 == "gn":
        # tables per (image, channel); raw = (target - shift) / scale is exact (a power-of-two scale, an integer shift), so the applied
        # value fma(raw, scale, shift) is the target and the ReLU turns the negative targets into exact zeros
        o.scale = GN_SCALES[rng.integers(0, len(GN_SCALES), size=(c.n, cw))]
        o.shift = rng.integers(-3, 4, size=(c.n, cw)).astype(F)
        raw = (target.astype(D) - o.shift[:, None, None, :]) / o.scale[:, None, None, :].astype(D)
        o.raw = raw.astype(F)
        assert (o.raw.astype(D) == raw).all()
        applied = sr.relu(sr.fma32(o.raw, np.broadcast_to(o.scale[:, None, None, :], raw.shape), np.broadcast_to(o.shift[:, None, None, :], raw.shape)))
        assert (applied == np.maximum(target, 0)).all()
        keep = target > 0
        target, ta, tb = applied, np.where(keep, ta, 0.0), np.where(keep, tb, 0.0)
    elif c.x_f32 == "plain":
        o.raw = target
    o.xwide = target
    o.x, o.xa, o.xb = (np.ascontiguousarray(t[..., c0:c0 + c.cin]) for t in (target, ta, tb))
    wrng = np.random.default_rng(5000 + (c.seed if c.wseed is None else c.wseed))
    o.w, o.wa, o.wb = gen(c.family, (c.cout, c.r, c.s, c.cin), wrng, c.A, c.zeros)
    o.bias = gen(c.family, (c.cout,), wrng, min(c.A, 2))[0] if c.bias else None
    o.res = None
    if c.res:
        oh, ow = out_size(c)
        rh, rw = ((oh + 1) // 2, (ow + 1) // 2) if c.res.startswith("up") else (oh, ow)
        o.res = gen(c.family, (c.n, rh, rw, c.cout), rng, min(c.A, 2))[0]
    return o


# --------------------------------------------------------------------------------------------------------------------------
# the models
# --------------------------------------------------------------------------------------------------------------------------
def conv64(x, w, c):
    """plain fp64 convolution, NHWC x [N,H,W,Cin] with w [Cout,R,S,Cin] -> [N,OH,OW,Cout] (exact on these operands: every
    term is a multiple of 2^-32 and every sum is below 2^10, far inside 53 bits)"""
    wt = torch.from_numpy(np.ascontiguousarray(w, D)).permute(0, 3, 1, 2).contiguous()
    xt = torch.from_numpy(np.ascontiguousarray(x, D))
    outs = []
    for i in range(0, xt.shape[0], 32):
        y = torch.nn.functional.conv2d(xt[i:i + 32].permute(0, 3, 1, 2), wt, None, c.stride, c.pad, c.dil)
        outs.append(y.permute(0, 2, 3, 1).contiguous())
    return torch.cat(outs).numpy()


def model3(o, c):
    return conv64(o.xa, o.w, c) + conv64(o.xb, o.wa, c)


def model1(o, c):
    return conv64(o.xa, o.wa, c)


def model4(o, c):
    return conv64(o.x, o.w, c)


def model(o, c):
    if c.kind == "f32":
        return model4(o, c)
    return model1(o, c) if c.terms == 1 else model3(o, c)


def residual_at_output(o, c):
    """the residual as the epilogue reads it: [N,OH,OW,Cout] fp64 (zeros without one)"""
    oh, ow = out_size(c)
    if o.res is None:
        return np.zeros((c.n, oh, ow, c.cout), D)
    if c.res.startswith("up"):
        iy = up_index(np.arange(oh), o.res.shape[1], oh)
        ix = up_index(np.arange(ow), o.res.shape[2], ow)
        return o.res[:, iy][:, :, ix].astype(D)
    return o.res.astype(D)


def abs_sum(o, c):
    """S, the exactness condition's left side, per output element"""
    s = conv64(np.abs(o.x), np.abs(o.w), c) + np.abs(residual_at_output(o, c))
    return s + (np.abs(o.bias.astype(D)) if o.bias is not None else 0.0)


def finish(y, c):
    """the value array [N,OH,OW,Cout] (fp32, exact) -> the whole output tensor as the kernel leaves it: fp32 or S32, inside the
    sentinel arena when the output is a channel slice"""
    n, oh, ow, cout = y.shape
    cw, c0 = c.out_wide if c.out_wide else (cout, 0)
    out = arena((n, oh, ow), cw, c.out_split)
    if c.out_split:
        hi, lo = sr.split(y)
        out[:, :, :, c0 // 32:(c0 + cout) // 32] = sr.to_s32(hi, lo)
    else:
        out[..., c0:c0 + cout] = y
    return out


def expected_values(c, o=None):
    """the model through the epilogue -> fp32 [N,OH,OW,Cout], asserted exact"""
    o = operands(c) if o is None else o
    y = model(o, c) + (o.bias.astype(D) if o.bias is not None else 0.0) + residual_at_output(o, c)
    y = relu_cols(y, c.relu_cols)
    y32 = y.astype(F)
    assert (y32.astype(D) == y).all(), "the model left fp32: the case breaks the exactness condition"
    return y32 + F(0.0)     # (-0.0 cannot arise from sums of these operands other than as 0 - 0; normalise)


def expected(c, o=None):
    """the bytes the kernel must write: the whole output tensor (arena included)"""
    return finish(expected_values(c, o), c)


def decode(index, c, shape):
    """flat index into the output tensor -> (img, oy, ox, channel of the tensor)"""
    idx = np.unravel_index(index, shape)
    ch = idx[3] * 32 + idx[5] if len(shape) == 6 else idx[3]
    return int(idx[0]), int(idx[1]), int(idx[2]), int(ch), ("lo" if len(shape) == 6 and idx[4] else "hi" if len(shape) == 6 else "f32")


# --------------------------------------------------------------------------------------------------------------------------
# the implicit GEMM's walk, with one deliberate mistake
# --------------------------------------------------------------------------------------------------------------------------
def _flush_subnormal(hv):
    return np.where(np.abs(hv) < H(2.0 ** -14), H(0.0), hv).astype(H)


def emulate(c, o=None, mutant=None, bm=64):
    """the f16x3 implicit GEMM of case c on flat buffers -> the whole output tensor, as expected() gives it"""
    assert mutant is None or mutant in MUTANTS
    assert c.kind == "f16x3"
    o = operands(c) if o is None else o
    oh, ow = out_size(c)
    M, cbs = c.n * oh * ow, c.cin // 32
    # the input as the conversion pass leaves it: hi / lo per channel of the WIDE tensor, flat
    xhi, xlo = sr.split(o.xwide)
    whi, wlo = sr.split(o.w)
    if mutant == "lo_subnormal_flushed":
        xlo, wlo = _flush_subnormal(xlo), _flush_subnormal(wlo)
    xhi, xlo = xhi.reshape(-1).astype(D), xlo.reshape(-1).astype(D)
    whi, wlo = whi.astype(D), wlo.astype(D)
    xs = c.cin if (mutant == "slice_stride_ignored" and c.in_wide) else o.cw
    npix = c.n * c.h * c.w
    m = np.arange(M)
    img, oy, ox = m // (oh * ow), (m // ow) % oh, m % ow
    origin = c.stride - 1 if (mutant == "stride_origin_off_by_one" and c.stride > 1) else 0
    iy0, ix0 = oy * c.stride - c.pad + origin, ox * c.stride - c.pad + origin
    tdil = 1 if mutant == "dilation_ignored_in_pad_test" else c.dil
    ktiles = cbs * c.r * c.s
    splits = c.force_splits if c.force_splits and c.force_splits >= 2 else 1
    kt_per = -(-ktiles // splits)
    splits = -(-ktiles // kt_per)
    planes = np.zeros((splits, M, c.cout), F)
    pad_hi = pad_lo = None
    if mutant == "gn_affine_applied_to_padding" and o.shift is not None:
        pad_hi, pad_lo = sr.split(sr.relu(o.shift))          # what relu(0 * scale + shift) splits into, per (image, channel)
    ch32 = np.arange(32)
    for cb in range(cbs):
        for ky in range(c.r):
            for kx in range(c.s):
                kt = (cb * c.r + ky) * c.s + kx
                zs = [kt // kt_per]
                if mutant == "splitk_last_chunk_dropped" and splits > 1 and zs[0] == splits - 1:
                    continue
                if mutant == "splitk_chunk_overlap" and kt % kt_per == kt_per - 1 and zs[0] + 1 < splits:
                    zs.append(zs[0] + 1)                      # the next chunk starts one tile early
                iy, ix = iy0 + ky * c.dil, ix0 + kx * c.dil
                ty, tx = iy0 + ky * tdil, ix0 + kx * tdil
                ok = (ty >= 0) & (tx < c.w)
                if mutant != "pad_reads_previous_row":
                    ok &= tx >= 0
                if mutant != "pad_reads_next_image":
                    ok &= ty < c.h
                if mutant == "bottom_tap_skipped" and c.r > 1:
                    ok &= ~((oy == oh - 1) & (ky == c.r - 1))
                pix = (img * c.h + iy) * c.w + ix
                idx = pix[:, None] * xs + o.c0 + cb * 32 + ch32[None, :]
                read = ok[:, None] & (pix[:, None] >= 0) & (pix[:, None] < npix) & (idx < xhi.size)
                idx = np.where(read, idx, 0)
                ahi, alo = np.where(read, xhi[idx], 0.0), np.where(read, xlo[idx], 0.0)
                if pad_hi is not None:
                    sel = (~ok)[:, None]
                    ahi = np.where(sel, pad_hi[img][:, o.c0 + cb * 32:o.c0 + cb * 32 + 32].astype(D), ahi)
                    alo = np.where(sel, pad_lo[img][:, o.c0 + cb * 32:o.c0 + cb * 32 + 32].astype(D), alo)
                bhi, blo = whi[:, ky, kx, cb * 32:cb * 32 + 32], wlo[:, ky, kx, cb * 32:cb * 32 + 32]
                t = ahi @ bhi.T
                if c.terms == 3:
                    hl = ahi @ blo.T
                    if mutant == "hi_lo_dropped_on_right_border":
                        hl = np.where((ox == ow - 1)[:, None], 0.0, hl)
                    t = t + hl
                    if not (mutant == "lo_hi_dropped_in_last_ktile" and kt == ktiles - 1):
                        t = t + alo @ bhi.T
                    if mutant == "fourth_term":
                        t = t + alo @ blo.T
                for z in zs:
                    planes[z] = planes[z] + t.astype(F)       # fp32 accumulation, tile after tile
    acc = planes[0]
    for z in range(1, splits):
        acc = acc + planes[z]                                 # the reduction adds the planes in z order
    v = acc + (o.bias if o.bias is not None else F(0.0))
    rc = min(c.cout, -(-c.relu_cols // 8) * 8) if mutant == "relu_cols_rounded_to_8" else c.relu_cols
    if mutant == "relu_before_residual":
        v = relu_cols(v, rc)
    if o.res is not None:
        if c.res.startswith("up"):
            rh, rw = o.res.shape[1:3]
            if mutant == "upsample_ceil":
                ry, rx = np.minimum(-(-(oy * rh) // oh), rh - 1), np.minimum(-(-(ox * rw) // ow), rw - 1)
            else:
                ry, rx = up_index(oy, rh, oh), up_index(ox, rw, ow)
            v = v + o.res[img, ry, rx]
        else:
            v = v + o.res.reshape(M, c.cout)
    if mutant != "relu_before_residual":
        v = relu_cols(v, rc)
    v = (v + F(0.0)).astype(F)
    c8 = c.cout // 8 * 8
    if mutant == "cout_tail_duplicated" and c.cout % 8:
        v[:, c8:] = v[:, c8:c8 + 1]                           # the scalar tail reads its first column for all of them
    rows = M - 1 if (mutant == "last_m_row_dropped" and M % bm == 1) else M
    # the store, on the flat output tensor
    cw, c0 = c.out_wide if c.out_wide else (c.cout, 0)
    out = arena((c.n, oh, ow), cw, c.out_split).reshape(-1)
    dense = mutant == "slice_stride_ignored" and c.out_wide
    if c.out_split:
        hi, lo = sr.split(v)
        ys = 2 * (c.cout if dense else cw)
        off = 2 * c0 + sr.s32_offset(np.arange(rows)[:, None], np.arange(c.cout)[None, :], ys)
        out[off], out[off + 32] = hi[:rows], lo[:rows]
    else:
        ys = c.cout if dense else cw
        out[c0 + np.arange(rows)[:, None] * ys + np.arange(c.cout)[None, :]] = v[:rows]
    return out.reshape(arena((c.n, oh, ow), cw, c.out_split).shape)
