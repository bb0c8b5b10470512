"""The S32 split format and the kernels that make and consume it outside a convolution (csrc/split_ops.hip with the arithmetic of
csrc/affine_split_body.h), as a rule in numpy that is exact to the bit, an emulation of each kernel in the kernel's own walk
over flat buffers, and the emulations with one deliberate mistake each.  numpy only; nothing here reads the library.

THE RULE, operation for operation.
  1. the affine   v = fma(x, scale[img][c], shift[img][c]): ONE fp32 rounding of the exact x*s + t (fma32; proven against
                  fractions.Fraction in test_split_cpu.py).  Without tables v = x, untouched (a -0.0 stays -0.0).
  2. ReLU         IEEE 754-2019 maximum(v, +0): a NaN stays NaN, -0.0 becomes +0.0.
  3. the note     the range flag is raised iff !(|v| <= 65504) for any value written, after the affine and the ReLU: beyond the
                  fp16 range, +-inf and NaN.  Only when the contract is switched on.
  4. the split    hi = fp16(v), round to nearest even with gradual underflow; lo = fp16(v - float(hi)), the difference in fp32.
                  So a finite |v| >= 65520 gives (+-inf, -+inf), +-inf gives (+-inf, NaN) and NaN gives (NaN, NaN).
  5. the layout   channel ch of a pixel sits at  pix*ys + (ch >> 5)*64 + (ch & 31)  halfs, its lo 32 halfs behind; input pixel
                  stride xs, table row stride as, output pixel stride ys >= 2c.
  6. unsplit      float(hi) + float(lo), one fp32 addition.
  7. the pool     3x3, stride 2, pad 1, taps in dy then dx order; per channel the running best starts at -FLT_MAX with the pair
                  (0, 0); an element replaces it when v = float(hi) + float(lo) > best or v is NaN (so of several NaNs the LAST
                  one's pair is copied); taps outside the frame are skipped; the (hi, lo) pair is copied, never re-split.
                  Pairs whose hi is +-inf have no rule.
  8. comparing    same_bits: any two NaNs are equal, -0.0 differs from 0.0.
"""
from fractions import Fraction

import numpy as np

F = np.float32
H = np.float16
FLT_MAX = F(3.4028234663852886e38)
F16_MAX = F(65504.0)
SENTINEL = H(-77.25)

MUTANTS = {
    "affine": ("mul_add", "image0_tables", "table_stride_ignored", "relu_before_affine"),
    "relu": ("relu_launders_nan", "relu_keeps_neg_zero"),
    "conversion": ("hi_truncated", "lo_truncated", "f16_denormals_flushed", "lo_of_unclamped"),
    "layout": ("lo_at_plus_8", "block_stride_32", "tail_pixel_dropped", "second_unrolled_pixel_aliased",
               "level_boundary_off_by_one"),
    "flag": ("flag_ge", "flag_misses_nan", "flag_before_relu"),
    "pool": ("last_tie", "nan_dropped", "pad_reads_zero", "hi_only_compare", "pair_resplit"),
    "unsplit": ("lo_ignored",),
}
ALL_MUTANTS = tuple(m for area in MUTANTS.values() for m in area)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    i = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(i) == b.view(i)) | (np.isnan(a) & np.isnan(b))).all())


def first_difference(a, b):
    """index and values of the first element that same_bits objects to (for assertion messages)"""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    i = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    bad = np.flatnonzero(~((a.view(i) == b.view(i)) | (np.isnan(a) & np.isnan(b))))
    return None if bad.size == 0 else (int(bad[0]), a[bad[0]], b[bad[0]], int(bad.size))


# --------------------------------------------------------------------------------------------------------------------------
# the arithmetic
# --------------------------------------------------------------------------------------------------------------------------
def fma32(x, s, t):
    """fl32(x*s + t) with ONE rounding.  The product of two fp32 values has 48 significant bits: exact in float64.  TwoSum gives the
    float64 sum and its exact error; where the error is not zero the sum is moved to its odd neighbour on the error's side (round
    to odd), and a round-to-odd value of 53 bits rounds to 24 bits (or fewer: fp32 subnormals) as the exact value would."""
    x, s, t = (np.asarray(a, F) for a in (x, s, t))
    with np.errstate(all="ignore"):
        p = x.astype(np.float64) * s.astype(np.float64)
        b = t.astype(np.float64)
        sm = p + b
        bb = sm - p
        err = (p - (sm - bb)) + (b - bb)
        fix = np.isfinite(sm) & np.isfinite(err) & (err != 0) & ((sm.view(np.uint64) & np.uint64(1)) == 0)
        sm = np.where(fix, np.nextafter(sm, np.where(err > 0, np.inf, -np.inf)), sm)
        return sm.astype(F)


def round_fraction_f32(q):
    """an exact rational -> fp32, round to nearest even, gradual underflow, overflow to inf (zero: +0.0)"""
    q = Fraction(q)
    if q == 0:
        return F(0.0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    k = a / quantum
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    r = n * quantum
    out = float("inf") if r >= Fraction(2) ** 128 else float(r)
    return F(out if q > 0 else -out)


def fma_fraction(x, s, t):
    """the same through exact rationals (finite inputs, scalar)"""
    return round_fraction_f32(Fraction(float(x)) * Fraction(float(s)) + Fraction(float(t)))


def relu(v):
    """maximum(v, +0) of IEEE 754-2019: NaN stays, -0.0 -> +0.0"""
    v = np.asarray(v, F)
    return np.where(v > 0, v, np.where(np.isnan(v), v, F(0.0))).astype(F)


def range_bad(v):
    with np.errstate(invalid="ignore"):
        return ~(np.abs(np.asarray(v, F)) <= F16_MAX)


def _f16_toward_zero(v):
    with np.errstate(all="ignore"):
        h = v.astype(H)
        over = np.isfinite(v) & (np.abs(h.astype(F)) > np.abs(v))
        return np.where(over, np.nextafter(h, H(0.0)), h).astype(H)


def _flush(h):
    return np.where(np.abs(h) < H(2.0 ** -14), np.copysign(H(0.0), h), h).astype(H)


def split(v, mutant=None, lo_from=None):
    """fp32 -> (hi, lo) fp16.  lo_from: the value the lo part is taken of (the lo_of_unclamped mutant)"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        hi = _f16_toward_zero(v) if mutant == "hi_truncated" else v.astype(H)
        if mutant == "f16_denormals_flushed":
            hi = _flush(hi)
        d = (v if lo_from is None else np.asarray(lo_from, F)) - hi.astype(F)
        assert d.dtype == F
        lo = _f16_toward_zero(d) if mutant == "lo_truncated" else d.astype(H)
        if mutant == "f16_denormals_flushed":
            lo = _flush(lo)
    return hi, lo


def unsplit(hi, lo, mutant=None):
    with np.errstate(all="ignore"):
        out = hi.astype(F) if mutant == "lo_ignored" else hi.astype(F) + lo.astype(F)
    assert out.dtype == F
    return out


def values(x, s, t, relu_on, mutant=None):
    """steps 1-4 on arrays of equal shape (s, t None: no affine) -> (hi, lo, bad), bad = the range note per element"""
    x = np.asarray(x, F)
    v = x
    if mutant == "relu_before_affine" and relu_on:
        v = relu(v)
    if s is not None:
        if mutant == "mul_add":
            with np.errstate(all="ignore"):
                v = (v * np.asarray(s, F)).astype(F) + np.asarray(t, F)
        else:
            v = fma32(v, s, t)
    pre = v
    if relu_on and mutant != "relu_before_affine":
        if mutant == "relu_launders_nan":
            v = np.where(v > 0, v, F(0.0)).astype(F)
        elif mutant == "relu_keeps_neg_zero":
            v = np.where((v > 0) | np.isnan(v) | ((v == 0) & np.signbit(v)), v, F(0.0)).astype(F)
        else:
            v = relu(v)
    with np.errstate(invalid="ignore"):
        if mutant == "flag_ge":
            bad = ~(np.abs(v) < F16_MAX)
        elif mutant == "flag_misses_nan":
            bad = np.abs(v) > F16_MAX
        elif mutant == "flag_before_relu":
            bad = range_bad(pre)
        else:
            bad = range_bad(v)
    hi, lo = split(v, mutant, lo_from=pre if mutant == "lo_of_unclamped" else None)
    return hi, lo, bad


def rule_apply(x, scale=None, shift=None, relu_on=False):
    """x [N, HW, C] fp32, tables [N, C] or None -> (hi, lo fp16 [N, HW, C], flag bool): the whole pass as steps 1-4"""
    x = np.asarray(x, F)
    assert x.ndim == 3 and (scale is None) == (shift is None)
    s = None if scale is None else np.broadcast_to(np.asarray(scale, F)[:, None, :], x.shape)
    t = None if shift is None else np.broadcast_to(np.asarray(shift, F)[:, None, :], x.shape)
    hi, lo, bad = values(x, s, t, relu_on)
    return hi, lo, bool(bad.any())


# --------------------------------------------------------------------------------------------------------------------------
# the layout
# --------------------------------------------------------------------------------------------------------------------------
def s32_offset(pix, ch, ys, mutant=None):
    """half index of the hi part of channel ch of pixel pix; the lo part is lo_gap() behind"""
    return pix * ys + (ch >> 5) * (32 if mutant == "block_stride_32" else 64) + (ch & 31)


def lo_gap(mutant=None):
    return 8 if mutant == "lo_at_plus_8" else 32


def place(buf, base, hi, lo, ys):
    """write hi, lo [NPIX, C] into the flat fp16 buffer at `base` with pixel stride ys (step 5), in place"""
    npix, c = hi.shape
    off = base + s32_offset(np.arange(npix)[:, None], np.arange(c)[None, :], ys)
    buf[off] = hi
    buf[off + 32] = lo
    return buf


def take(buf, base, npix, c, ys):
    """(hi, lo) [NPIX, C] read from a flat fp16 buffer"""
    off = base + s32_offset(np.arange(npix)[:, None], np.arange(c)[None, :], ys)
    return buf[off], buf[off + 32]


def to_s32(hi, lo):
    """(hi, lo) [..., C] -> the dense S32 array [..., C/32, 2, 32], through place()"""
    lead, c = hi.shape[:-1], hi.shape[-1]
    npix = int(np.prod(lead, dtype=np.int64))
    buf = np.zeros(npix * 2 * c, H)
    place(buf, 0, hi.reshape(npix, c), lo.reshape(npix, c), 2 * c)
    return buf.reshape(lead + (c // 32, 2, 32))


def from_s32(s32):
    """dense S32 array [..., C/32, 2, 32] -> (hi, lo) [..., C]"""
    lead = s32.shape[:-3]
    c = s32.shape[-3] * 32
    return s32[..., 0, :].reshape(lead + (c,)), s32[..., 1, :].reshape(lead + (c,))


# --------------------------------------------------------------------------------------------------------------------------
# the kernels' walks
# --------------------------------------------------------------------------------------------------------------------------
class Flat:
    """the operands of one launch as the library gets them: flat buffers, element offsets and strides"""

    def __init__(self, x, x_off, xs, scale, shift, a_off, a_stride, y, y_off, ys):
        self.x, self.x_off, self.xs = x, x_off, xs
        self.scale, self.shift, self.a_off, self.a_stride = scale, shift, a_off, a_stride
        self.y, self.y_off, self.ys = y, y_off, ys


def _store_pixel(f, img, hw, pix, c, relu_on, mutant, flag, xpix=None):
    """one pixel of one image, all its channel groups (the lanes of a block that share the pixel)"""
    ch = np.arange(c)
    src = f.x_off + (img * hw + (pix if xpix is None else xpix)) * f.xs + ch
    s = t = None
    if f.scale is not None:
        row = 0 if mutant == "image0_tables" else img
        o = f.a_off + row * (c if mutant == "table_stride_ignored" else f.a_stride) + ch
        s, t = f.scale[o], f.shift[o]
    hi, lo, bad = values(f.x[src], s, t, relu_on, mutant)
    dst = f.y_off + s32_offset(img * hw + pix, ch, f.ys, mutant)
    f.y[dst] = hi
    f.y[dst + lo_gap(mutant)] = lo
    flag[0] |= bool(bad.any())


def pow2_grid(n, hw, c):
    """(ppb, gx) of affine_split_pow2_kernel: 256 / (c/8) pixels per block and iteration, ceil(hw / 2 ppb) blocks per image
    capped at ceil(16384 / n)"""
    ppb = 256 // (c // 8)
    return ppb, max(1, min(-(-hw // (2 * ppb)), -(-16384 // n)))


def _walk_pow2(f, img, hw, c, relu_on, mutant, flag, ppb, blocks, unr):
    """the pixel loop of one image over `blocks` blocks: `unr` pixels in flight while pix + (unr - 1) step < hw, then the tail"""
    step = blocks * ppb
    for bx in range(blocks):
        for r in range(ppb):
            pix = bx * ppb + r
            while pix + (unr - 1) * step < hw:
                for u in range(unr):
                    alias = mutant == "second_unrolled_pixel_aliased" and u == 1
                    _store_pixel(f, img, hw, pix + u * step, c, relu_on, mutant, flag, xpix=pix if alias else None)
                pix += unr * step
            while pix < (hw - 1 if mutant == "tail_pixel_dropped" else hw):
                _store_pixel(f, img, hw, pix, c, relu_on, mutant, flag)
                pix += step


def emulate_apply(f, n, hw, c, relu_on, form="pow2", unr=2, gx=None, mutant=None):
    """hn_affine_split_f32 on flat buffers, written in place into f.y -> the range note.  form "pow2": one image per blockIdx.y, a
    lane keeps its channel group; "generic": item i = pixel i / c8, group i % c8.  (Both visit every pixel once, so the order of
    the visits is all that differs; the mutants live in the walk and in values().)  unr = 4 with a gx below pow2_grid()'s: the
    streaming instantiations under a capped grid, the only way their four-deep loop runs (it needs hw > 3 gx ppb)."""
    assert mutant is None or mutant in ALL_MUTANTS
    flag = [False]
    c8 = c // 8
    if form == "pow2":
        assert c8 & (c8 - 1) == 0 and c8 <= 256
        ppb, full = pow2_grid(n, hw, c)
        gx = full if gx is None else gx
        for img in range(n):
            _walk_pow2(f, img, hw, c, relu_on, mutant, flag, ppb, gx, unr)
    else:
        for gpix in range(n * hw - (1 if mutant == "tail_pixel_dropped" else 0)):
            _store_pixel(f, gpix // hw, hw, gpix % hw, c, relu_on, mutant, flag)
    return flag[0]


def level_blocks(n, hws, c):
    """first_block[0 .. count] of affine_split_pow2_levels_kernel"""
    first = [0]
    for hw in hws:
        first.append(first[-1] + pow2_grid(n, hw, c)[1])
    return first


def emulate_levels(fs, n, hws, c, relu_on, mutant=None):
    """hn_affine_split_f32_levels' merged launch: block bx belongs to the LAST level l with bx >= first_block[l]; inside its
    level it is block bx - first_block[l] of first_block[l + 1] - first_block[l]"""
    assert mutant is None or mutant in ALL_MUTANTS
    flag = [False]
    first = level_blocks(n, hws, c)
    ppb = 256 // (c // 8)
    for bx in range(first[-1]):
        lvl = 0
        for l in range(1, len(hws)):
            if (bx > first[l]) if mutant == "level_boundary_off_by_one" else (bx >= first[l]):
                lvl = l
        b0, b1 = first[lvl], first[lvl + 1]
        step = (b1 - b0) * ppb
        for img in range(n):
            for r in range(ppb):
                pix = (bx - b0) * ppb + r
                while pix + step < hws[lvl]:
                    _store_pixel(fs[lvl], img, hws[lvl], pix, c, relu_on, mutant, flag)
                    alias = mutant == "second_unrolled_pixel_aliased"
                    _store_pixel(fs[lvl], img, hws[lvl], pix + step, c, relu_on, mutant, flag, xpix=pix if alias else None)
                    pix += 2 * step
                while pix < (hws[lvl] - 1 if mutant == "tail_pixel_dropped" else hws[lvl]):
                    _store_pixel(fs[lvl], img, hws[lvl], pix, c, relu_on, mutant, flag)
                    pix += step
    return flag[0]


def emulate_unsplit(xbuf, x_off, xs, npix, c, ybuf, y_off, ys, mutant=None):
    """hn_unsplit_f32 on flat buffers: item i = 8 channels of pixel i / c8, written in place into ybuf (fp32)"""
    c8 = c // 8
    e = np.arange(8)
    for i in range(npix * c8):
        pix, ch = i // c8, (i % c8) * 8
        src = x_off + s32_offset(pix, ch + e, xs, mutant)
        ybuf[y_off + pix * ys + ch + e] = unsplit(xbuf[src], xbuf[src + lo_gap(mutant)], mutant)


# --------------------------------------------------------------------------------------------------------------------------
# the pool
# --------------------------------------------------------------------------------------------------------------------------
def pool_out(h, w):
    return (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1


def _pool_window(hi, lo, img, oy, ox, mutant):
    """one output pixel, all channels: step 7"""
    _, h, w, c = hi.shape
    best = np.full(c, -FLT_MAX, F)
    bh, bl = np.zeros(c, H), np.zeros(c, H)
    for dy in range(3):
        iy = 2 * oy - 1 + dy
        for dx in range(3):
            ix = 2 * ox - 1 + dx
            if 0 <= iy < h and 0 <= ix < w:
                th, tl = hi[img, iy, ix], lo[img, iy, ix]
            elif mutant == "pad_reads_zero":
                th, tl = np.zeros(c, H), np.zeros(c, H)
            else:
                continue
            v = th.astype(F) if mutant == "hi_only_compare" else unsplit(th, tl)
            with np.errstate(invalid="ignore"):
                won = (v >= best) if mutant == "last_tie" else (v > best)
            if mutant != "nan_dropped":
                won = won | np.isnan(v)
            best = np.where(won, v, best)
            bh, bl = np.where(won, th, bh), np.where(won, tl, bl)
    if mutant == "pair_resplit":
        bh, bl = split(unsplit(bh, bl))
    return bh, bl


def rule_pool(hi, lo, mutant=None):
    """(hi, lo) [N, H, W, C] -> the pooled pair [N, OH, OW, C]"""
    assert mutant is None or mutant in ALL_MUTANTS
    n, h, w, c = hi.shape
    oh, ow = pool_out(h, w)
    oh_, ol_ = np.zeros((n, oh, ow, c), H), np.zeros((n, oh, ow, c), H)
    for img in range(n):
        for oy in range(oh):
            for ox in range(ow):
                oh_[img, oy, ox], ol_[img, oy, ox] = _pool_window(hi, lo, img, oy, ox, mutant)
    return oh_, ol_


def emulate_pool(xbuf, n, h, w, c, mutant=None):
    """hn_maxpool3x3s2_s32 on a dense flat S32 buffer -> a dense flat S32 buffer: item i = 8 channels (i % c8) of output pixel
    i / c8, decoded x, then y, then image, as the kernel does"""
    assert mutant is None or mutant in ALL_MUTANTS
    oh, ow = pool_out(h, w)
    hi, lo = take(xbuf, 0, n * h * w, c, 2 * c)
    hi, lo = hi.reshape(n, h, w, c), lo.reshape(n, h, w, c)
    out = np.full(n * oh * ow * 2 * c, SENTINEL, H)
    c8 = c // 8
    for i in range(n * oh * ow * c8):
        cc, pix = (i % c8) * 8, i // c8
        ox, oy, img = pix % ow, (pix // ow) % oh, pix // ow // oh
        bh, bl = _pool_window(hi[..., cc:cc + 8], lo[..., cc:cc + 8], img, oy, ox, mutant)
        dst = s32_offset(pix, cc + np.arange(8), 2 * c, mutant)
        out[dst] = bh
        out[dst + lo_gap(mutant)] = bl
    return out
