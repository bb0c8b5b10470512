"""The detector's resize / normalise / pad (fcos_utils/fcos.py:702-709, torchvision GeneralizedRCNNTransform; csrc/fcos_post.hip
fcos_preprocess_kernel, fcos_preprocess_split_kernel, fcos_preprocess_split_tiled_kernel) as a rule in float64, its worst-case
fp32 error bound, an fp32 emulation of the kernels' arithmetic in their order, and that emulation with one deliberate mistake
each.  numpy only; nothing here reads the library.

Layout: images [n, 3, h, w] fp32 -> canvas [n, ph, pw, 4] fp32 (channel 3 zero; zero outside the resized oh x ow rectangle in
the top-left corner), or the stem's split image: fp16 [2 (hi, lo), n, ph + 2b, pw + 2b, 4] with a zero border of b pixels,
hi = fp16(o), lo = fp16(o - float(hi)).
"""
import numpy as np

U = 2.0 ** -24              # unit roundoff of fp32
F = np.float32
D = np.float64
TINY = 2.0 ** -149          # one fp32 subnormal quantum: the floor of every bound (so 0 / 0 does not arise where the rule is 0)
MUTANTS = ("no_half", "no_clamp0", "no_clamp_i1", "scale_inverted", "swap_ohow", "pad_before_normalise", "border_off_by_one",
           "lo_from_rounded")


def fma(a, b, c, stats=None):
    """fmaf(a, b, c) on fp32 arrays: the product of two fp32 numbers is exact in float64 (48 bits), the sum with c is rounded
    once to float64 and once more to fp32.  This double rounding can differ from a true fused multiply-add only where the
    float64 sum is an exact midpoint of two adjacent fp32 numbers while the real sum is not (an exact midpoint goes to even
    either way).  stats['midpoints'] counts the float64 sums that are such midpoints AND inexact (the error term of Knuth's
    TwoSum is not zero); tests/test_pre_cpu.py asserts that no seeded case has one."""
    a, b, c = np.asarray(a), np.asarray(b), np.asarray(c)
    assert a.dtype == F and b.dtype == F and c.dtype == F
    p, c64 = a.astype(D) * b.astype(D), c.astype(D)
    s = p + c64
    r = s.astype(F)
    if stats is not None:
        bb = s - p
        inexact = ((p - (s - bb)) + (c64 - bb)) != 0
        d = s - r.astype(D)
        away = np.where(d > 0, F(np.inf), F(-np.inf)).astype(F)
        gap = np.abs(np.nextafter(r, away).astype(D) - r.astype(D))
        stats["midpoints"] = stats.get("midpoints", 0) + int(np.count_nonzero(inexact & (d != 0) & (2.0 * np.abs(d) == gap)))
    return r


def src_index(in_size, out_size, mutant=None, stats=None):
    """ATen's area_pixel_compute_source_index as the kernels' src_index states it, for dst = 0 .. out_size - 1, all in fp32:
    (i0, i1 int64; l0, l1 fp32).  scale = (float)in / (float)out and real = fmaf(scale, dst + 0.5, -0.5) are PART OF THE
    CONTRACT: a float64 coordinate differs (coordinate_bound)."""
    scale = F(out_size) / F(in_size) if mutant == "scale_inverted" else F(in_size) / F(out_size)
    dst = np.arange(out_size).astype(F)
    if mutant == "no_half":
        real = (np.full_like(dst, scale) * dst).astype(F)
    else:
        real = fma(np.full_like(dst, scale), dst + F(0.5), np.full_like(dst, F(-0.5)), stats)
    if mutant != "no_clamp0":
        real = np.maximum(real, F(0.0))
    i0 = np.minimum(np.floor(real).astype(np.int64), in_size - 1)
    l1 = np.minimum(np.maximum(real - i0.astype(F), F(0.0)), F(1.0)).astype(F)
    i1 = i0 + 1 if mutant == "no_clamp_i1" else np.minimum(i0 + 1, in_size - 1)
    l0 = (F(1.0) - l1).astype(F)
    return i0 % in_size, i1 % in_size, l0, l1        # (% in_size: only a mutant leaves [0, in_size); the kernel would read outside)


def coordinate_bound(in_size, out_size):
    """|fp32 coordinate - float64 coordinate| per dst, BEFORE the clamp at 0: the fp32 one is fl(fl(in / out) * (dst + 0.5) - 0.5)
    with dst + 0.5 exact (dst < 2^23), the division rounded once (relative u) and the fma rounded once (relative u of the
    result, |result| <= s (dst + 0.5) + 0.5).  First order: u s (dst + 0.5) + u (s (dst + 0.5) + 0.5); the factor 1 + 4u holds
    the product of the two."""
    s = float(in_size) / float(out_size)
    d = np.arange(out_size, dtype=D) + 0.5
    return U * (2.0 * s * d + 0.5) * (1.0 + 4.0 * U)


def _norm64(images, mean, std):
    m = np.asarray(mean, F).astype(D).reshape(1, 3, 1, 1)
    s = np.asarray(std, F).astype(D).reshape(1, 3, 1, 1)
    return (images.astype(D) - m) / s


def rule64(images, oh, ow, ph, pw, mean, std):
    """(rule, bound), both [n, ph, pw, 4] float64.

    rule: v = (p - mean) / std in float64 on the fp32 inputs; (i0, i1, l1) per axis from the fp32 coordinate chain (src_index);
    out = (v00 (1 - lx) + v01 lx)(1 - ly) + (v10 (1 - lx) + v11 lx) ly in float64; zero outside oy < oh, ox < ow; channel 3 zero.

    bound: worst-case forward error of the kernels' fp32 chain against that, relative to  S = sum |weight| |v|  over the four
    taps, u = 2^-24, first order:
      * v = fl(fl(p - mean) / std): two roundings, 2u on every tap.
      * l1 = real - i0 is exact: real >= 0 is an fp32 number and i0 = floor(real) (or in - 1 just below it), so the
        difference is a multiple of ulp(real) that is smaller than real, hence an fp32 number.  The rule takes the same l1,
        so nothing of the coordinate chain is an error against it.  l0 = fl(1 - l1): one rounding, u, on the taps weighted
        by l0.
      * bilerp stage 1, r = fma(a, l0, fl(b * l1)): the tap b carries u of the product, both taps carry u of the fma.
        With the rounding of l0 on tap a that is 2u per tap.
      * bilerp stage 2, out = fma(r0, ly0, fl(r1 * ly1)): the same, 2u per tap.
    6u per tap; the seventh u holds every second-order term ((1 + u)^6 - 1 - 6u < 16 u^2).  bound = 7 u S + 2^-149 (one
    subnormal quantum, so that a zero rule with a zero result gives 0 / tiny = 0; the products of the seeded cases are far
    from underflow).  Outside the rectangle and in channel 3 the bound is 0 + 2^-149 with a rule of 0: the result must be 0."""
    n, c, h, w = images.shape
    assert c == 3 and images.dtype == F
    v = _norm64(images, mean, std)
    y0, y1, _, ly = src_index(h, oh)
    x0, x1, _, lx = src_index(w, ow)
    ly, lx = ly.astype(D)[None, None, :, None], lx.astype(D)[None, None, None, :]
    v00, v01 = v[:, :, y0][:, :, :, x0], v[:, :, y0][:, :, :, x1]
    v10, v11 = v[:, :, y1][:, :, :, x0], v[:, :, y1][:, :, :, x1]
    out = (v00 * (1 - lx) + v01 * lx) * (1 - ly) + (v10 * (1 - lx) + v11 * lx) * ly
    s = (np.abs(v00) * (1 - lx) + np.abs(v01) * lx) * (1 - ly) + (np.abs(v10) * (1 - lx) + np.abs(v11) * lx) * ly
    rule = np.zeros((n, ph, pw, 4), D)
    bound = np.full((n, ph, pw, 4), TINY, D)
    rule[:, :oh, :ow, :3] = out.transpose(0, 2, 3, 1)
    bound[:, :oh, :ow, :3] += 7.0 * U * s.transpose(0, 2, 3, 1)
    return rule, bound


def emulate(images, oh, ow, ph, pw, mean, std, mutant=None, stats=None):
    """The kernels' chain in fp32 -> canvas [n, ph, pw, 4] fp32: v = (p - mean) / std (IEEE sub and div), src_index per axis,
    bilerp = fma(r0, wy0, r1 * wy1) with r = fma(a, wx0, b * wx1).  Every operation of the device chain is a correctly rounded
    IEEE operation (the file is built with -ffp-contract=off and the fused ones are explicit fmaf), so the device result equals
    this one bit for bit unless fma()'s double rounding bites (see there)."""
    assert mutant is None or mutant in MUTANTS
    n, c, h, w = images.shape
    assert c == 3 and images.dtype == F
    m = np.asarray(mean, F).reshape(1, 3, 1, 1)
    s = np.asarray(std, F).reshape(1, 3, 1, 1)
    v = ((images - m).astype(F) / s).astype(F)
    eh, ew = (ow, oh) if mutant == "swap_ohow" else (oh, ow)
    eh, ew = min(eh, ph), min(ew, pw)
    y0, y1, wy0, wy1 = src_index(h, eh, mutant, stats)
    x0, x1, wx0, wx1 = src_index(w, ew, mutant, stats)
    shape = (n, 3, eh, ew)
    wy0, wy1 = (np.broadcast_to(t[None, None, :, None], shape) for t in (wy0, wy1))
    wx0, wx1 = (np.broadcast_to(t[None, None, None, :], shape) for t in (wx0, wx1))
    v00, v01 = v[:, :, y0][:, :, :, x0], v[:, :, y0][:, :, :, x1]
    v10, v11 = v[:, :, y1][:, :, :, x0], v[:, :, y1][:, :, :, x1]
    r0 = fma(v00, wx0, (v01 * wx1).astype(F), stats)
    r1 = fma(v10, wx0, (v11 * wx1).astype(F), stats)
    o = fma(r0, wy0, (r1 * wy1).astype(F), stats)
    out = np.zeros((n, ph, pw, 4), F)
    if mutant == "pad_before_normalise":
        out[..., :3] = ((F(0.0) - m) / s).astype(F).reshape(1, 1, 1, 3)
    out[:, :eh, :ew, :3] = o.transpose(0, 2, 3, 1)
    assert out.dtype == F
    return out


def split(canvas, border, mutant=None):
    """fp32 canvas -> the stem's split image fp16 [2, n, ph + 2b, pw + 2b, 4]: hi = fp16(o), lo = fp16(o - float(hi))"""
    assert canvas.dtype == F
    n, ph, pw, _ = canvas.shape
    hi = canvas.astype(np.float16)
    lo = ((hi.astype(F) if mutant == "lo_from_rounded" else canvas) - hi.astype(F)).astype(np.float16)
    out = np.zeros((2, n, ph + 2 * border, pw + 2 * border, 4), np.float16)
    b = border - 1 if mutant == "border_off_by_one" else border
    assert b >= 0, "border_off_by_one needs a border"
    out[0, :, b:b + ph, b:b + pw] = hi
    out[1, :, b:b + ph, b:b + pw] = lo
    return out


def check(out, ref):
    """THE comparison for the fp32 canvas (CPU and GPU tests): |out - rule| <= bound on every element, which outside the resized
    rectangle and in channel 3 means exactly zero; returns max |err| / bound.  ref = (rule, bound) of rule64."""
    want, b = ref
    out = np.asarray(out)
    assert out.shape == want.shape and out.dtype == F, (out.shape, out.dtype)
    assert np.isfinite(out).all(), "non-finite value"
    ratio = np.abs(out.astype(D) - want) / b
    worst = float(ratio.max())
    assert worst <= 1.0, f"|err| / bound = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


def check_split(planes, ref, border):
    """THE comparison for the split image: float(hi) + float(lo) against the rule with the bound widened by what the split
    itself loses: hi = fp16(o) leaves |o - hi| <= 2^-11 |o|, lo = fp16(o - hi) leaves 2^-11 of that, 2^-22 |o|, or half an fp16
    subnormal quantum, 2^-25, where o - hi is below fp16's normal range; |o| <= |rule| + bound.  The zero border has rule 0 and
    bound 2^-149: it must be exactly zero."""
    want, b = ref
    planes = np.asarray(planes)
    n, ph, pw, _ = want.shape
    assert planes.shape == (2, n, ph + 2 * border, pw + 2 * border, 4) and planes.dtype == np.float16, (planes.shape, planes.dtype)
    assert np.isfinite(planes.astype(F)).all(), "non-finite value"
    w2 = np.zeros(planes.shape[1:], D)
    b2 = np.full(planes.shape[1:], TINY, D)
    sl = (slice(None), slice(border, border + ph), slice(border, border + pw))
    w2[sl] = want
    b2[sl] = b + np.where(b > TINY, 2.0 ** -22 * (np.abs(want) + b) + 2.0 ** -25, 0.0)
    ratio = np.abs(planes[0].astype(D) + planes[1].astype(D) - w2) / b2
    worst = float(ratio.max())
    assert worst <= 1.0, f"split |err| / bound = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst
