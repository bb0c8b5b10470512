"""The ResNet stem chain as rules, a worst-case bound, an fp32 emulation and that emulation with one deliberate mistake each.
numpy only; nothing here reads the library.

  stem image   csrc/a2j_ops.hip stem_image_kernel: fp32 [n, h, w, 4] -> fp16 [2 (hi, lo), n, h + 2b, w + 2b, 4], hi = fp16(v),
               lo = fp16(v - hi), zero border.  EXACT: rule_image has no tolerance.
  stem conv    csrc/conv_igemm_f16x3.hip stem16_run / csrc/conv_stem_direct.hip: filter row ky is one 32-deep k tile,
               k = kx * 4 + c over the 8 pixels from bordered pixel (2 oy + ky, 2 ox), zero weights for k >= 28.  rule_conv sums in
               float64 exactly the products the kernel issues, so operand rounding and the dropped lo*lo term are inside the
               rule; what is left is fp32 accumulation and the bias add (check_conv).
  max pooling  3x3 / stride 2 / pad 1, NaN-propagating.  The fused kernel pools fp32 values and splits the maximum; the unfused
               maxpool_s32_kernel (csrc/split_ops.hip) copies the (hi, lo) pair of the first element with the largest hi + lo.
"""
import numpy as np

from pre_ref import TINY, U, split

F, D, H = np.float32, np.float64, np.float16
R, K = 7, 32
FLT_MAX = np.finfo(F).max

# name -> (stage, case of tests/stem_cases.py (or a shape for the stages that take raw data), input kind): where the mutant MUST
# fall outside the bound (conv, fused, pool) or break the exact comparison (image)
MUTANTS = {
    "drop_lo_hi": ("conv", "14x15", "normal"),
    "fp16_accumulate": ("conv", "4x5", "normal"),
    "eighth_tap_nonzero": ("conv", "4x5", "normal"),
    "channel_order": ("conv", "4x5", "depth"),
    "patch_shift_one_pixel": ("conv", "1x1", "normal"),
    "no_phantom_mask": ("fused", "15x17", "edge_heavy"),
    "pool_identity_zero_without_relu": ("pool", (5, 5, 32), "negative"),
    "pool_window_off_by_one": ("fused", "15x17", "normal"),
    "pool_skips_last_row": ("fused", "15x17", "normal"),        # oh = 15 is odd: the last window hangs over the edge
    "border_not_zero": ("image", (2, 5, 7), "nonfinite"),
    "valid_0_becomes_2": ("image", (2, 5, 7), "nonfinite"),
    "nonfinite_not_zeroed": ("image", (2, 5, 7), "nonfinite"),
}


def chain(terms):
    """roundings on the way to one fp32 output: one per issued product (7 filter rows x 32 k x terms) plus the bias add"""
    return R * K * terms + 1


# ---------------------------------------------------------------------------------------------------------------- stem image
def rule_image(x, border, valid=None):
    """(planes fp16 [2, n, h + 2b, w + 2b, 4], valid after the launch or None, range words [4]).  With `valid` (int32 [n]) every
    non-finite pixel is stored as 0 and its image's valid goes 1 -> 2 (0 stays 0); without, it passes through.  Range words
    (hn_common.h range_note_input, noted on the pixel as the caller gave it): word 1 for a finite |v| > 65504, word 2 for a
    non-finite one."""
    x = np.asarray(x)
    assert x.dtype == F and x.ndim == 4 and x.shape[3] == 4
    bad = ~np.isfinite(x)
    words = [0, int(((np.abs(x) > 65504.0) & ~bad).any()), int(bad.any()), 0]
    out_valid = None
    if valid is not None:
        out_valid = np.asarray(valid).astype(np.int32).copy()
        hit = bad.reshape(x.shape[0], -1).any(axis=1)
        out_valid[hit & (out_valid == 1)] = 2
        x = np.where(bad, F(0.0), x)
    with np.errstate(over="ignore", invalid="ignore"):
        planes = split(np.ascontiguousarray(x, F), border)
    return planes, out_valid, words


def emulate_image(x, border, valid=None, mutant=None):
    """The kernel's loop over BORDERED pixels, one image row at a time -> (planes, valid)."""
    x = np.asarray(x)
    n, h, w, _ = x.shape
    hb, wb = h + 2 * border, w + 2 * border
    out = np.zeros((2, n, hb, wb, 4), H)
    if mutant == "border_not_zero":
        out[:] = H(1.0)
    v_out = None if valid is None else np.asarray(valid).astype(np.int32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for img in range(n):
            for yy in range(border, border + h):
                ve = x[img, yy - border].copy()
                if valid is not None:
                    bad = ~(np.abs(ve) <= FLT_MAX)
                    if bad.any():
                        if v_out[img] == 1 or (mutant == "valid_0_becomes_2" and v_out[img] == 0):
                            v_out[img] = 2
                        if mutant != "nonfinite_not_zeroed":
                            ve[bad] = F(0.0)
                hh = ve.astype(H)
                out[0, img, yy, border:border + w] = hh
                out[1, img, yy, border:border + w] = (ve - hh.astype(F)).astype(H)
    return out, v_out


# ------------------------------------------------------------------------------------------------------------------ stem conv
def conv_size(planes):
    _, n, hb, wb, _ = planes.shape
    return n, (hb - R) // 2 + 1, (wb - R) // 2 + 1


def _gather(xp, oys, oxs, mutant=None):
    """im2col of the stem form: [n, len(oys), len(oxs), 7 * 32] with k = ky * 32 + kx * 4 + c, from bordered pixel
    (2 oy + ky, 2 ox + kx), kx = 0 .. 7.  Rows are clamped to the image and 16-byte pieces (pixel pairs) to the row, as the direct
    kernel's patch load clamps them: no conv pixel INSIDE the map ever meets a clamp, the phantom ones (oy = -1, oh; ox = -1, ow)
    do."""
    n, hb, wb, _ = xp.shape
    rows = np.clip(2 * oys[:, None] + np.arange(R)[None], 0, hb - 1)
    if mutant == "patch_shift_one_pixel":
        pix = np.clip(2 * oxs[:, None] + 1 + np.arange(8)[None], 0, wb - 1)
    else:
        piece = np.clip(oxs[:, None] + np.arange(4)[None], 0, wb // 2 - 1)
        pix = (2 * piece[:, :, None] + np.arange(2)).reshape(len(oxs), 8)
    a = xp[:, rows[:, None, :, None], pix[None, :, None, :]]           # [n, OH, OW, 7, 8, 4]
    return a.reshape(n, len(oys), len(oxs), R * K)


def _banks(w16, dtype, mutant=None):
    """w16 [cout, 7, 2, 32] fp16 -> (hi, lo) [cout, 224]"""
    w16 = np.asarray(w16)
    assert w16.dtype == H and w16.shape[1:] == (R, 2, K), w16.shape
    wh, wl = w16[:, :, 0].astype(dtype), w16[:, :, 1].astype(dtype)
    if mutant == "eighth_tap_nonzero":
        wh = wh.copy()
        wh[:, :, 4 * R:] = 0.5
    if mutant == "channel_order":                                      # a bank laid out k = c * 8 + kx
        perm = np.array([(k % 4) * 8 + k // 4 for k in range(K)])
        wh2, wl2 = np.zeros_like(wh), np.zeros_like(wl)
        wh2[:, :, perm], wl2[:, :, perm] = wh, wl
        wh, wl = wh2, wl2
    cout = w16.shape[0]
    return wh.reshape(cout, R * K), wl.reshape(cout, R * K)


def rule_conv(planes, w16, bias, terms=3, relu=False):
    """(rule, S), float64 [n, oh, ow, cout]: the sum of exactly the products the kernel issues -- x_hi w_hi + x_hi w_lo + x_lo w_hi
    for terms = 3, x_hi w_hi alone for terms = 1 -- on the fp16 operands it sees, plus the bias; S = sum |product| + |bias|."""
    assert terms in (1, 3)
    n, oh, ow = conv_size(planes)
    oys, oxs = np.arange(oh), np.arange(ow)
    ah = _gather(np.asarray(planes[0]).astype(D), oys, oxs)
    wh, wl = _banks(w16, D)
    b = np.zeros(wh.shape[0], D) if bias is None else np.asarray(bias).astype(D)
    y = ah @ wh.T
    s = np.abs(ah) @ np.abs(wh).T
    if terms == 3:
        al = _gather(np.asarray(planes[1]).astype(D), oys, oxs)
        y += ah @ wl.T + al @ wh.T
        s += np.abs(ah) @ np.abs(wl).T + np.abs(al) @ np.abs(wh).T
    y, s = y + b, s + np.abs(b)
    return (np.maximum(y, 0.0) if relu else y), s


def check_conv(y32, ref, S, chain_len):
    """max |y - ref| / (chain U S + TINY): the worst-case LINEAR bound of an fp32 sum of `chain_len` - 1 exact products (fp16 x
    fp16 has 22 significant bits) and a bias in ANY order -- every partial sum is bounded by S and rounded at most once per
    addend, relative U = 2^-24 each.  ReLU and the max over a pooling window are 1-Lipschitz, so the bound holds behind them
    with S the window's largest.  A NaN anywhere makes the ratio NaN, which no caller's `<= 1` accepts."""
    y32 = np.asarray(y32)
    assert y32.dtype == F and y32.shape == ref.shape == S.shape, (y32.dtype, y32.shape, ref.shape)
    return float(np.max(np.abs(y32.astype(D) - ref) / (chain_len * U * S + TINY)))


def emulate_conv(planes, w16, bias, terms=3, relu=True, mutant=None, phantom=False):
    """The kernels' chain in fp32: one 32-deep product block per filter row and term, in the kernels' order of terms (x_lo w_hi,
    x_hi w_lo, x_hi w_hi), added to an fp32 accumulator; bias; ReLU.  phantom: the map with a ring of one conv pixel around it
    ([n, oh + 2, ow + 2, cout]), computed from clamped rows / pieces as the fused kernel computes the pixels outside the map."""
    n, oh, ow = conv_size(planes)
    oys, oxs = (np.arange(-1, oh + 1), np.arange(-1, ow + 1)) if phantom else (np.arange(oh), np.arange(ow))
    ah = _gather(np.asarray(planes[0]).astype(D), oys, oxs, mutant)
    al = _gather(np.asarray(planes[1]).astype(D), oys, oxs, mutant)
    wh, wl = _banks(w16, D, mutant)
    acc = np.zeros(ah.shape[:3] + (wh.shape[0],), F)
    acc_t = H if mutant == "fp16_accumulate" else F
    for ky in range(R):
        ks = slice(ky * K, ky * K + K)
        # a 32-deep block of 22-bit products, summed in float64 (a fixed order that does not depend on the array's shape, as a
        # BLAS fp32 product's would) and rounded to fp32 with the accumulator: 21 roundings where the bound allows 673
        blocks = [ah[..., ks] @ wh[:, ks].T]
        if terms == 3:
            blocks = ([] if mutant == "drop_lo_hi" else [al[..., ks] @ wh[:, ks].T]) + [ah[..., ks] @ wl[:, ks].T] + blocks
        for blk in blocks:
            acc = (acc.astype(D) + blk).astype(acc_t).astype(F)
    if bias is not None:
        acc = (acc + np.asarray(bias).astype(F)).astype(F)
    return np.maximum(acc, F(0.0)) if relu else acc


# ---------------------------------------------------------------------------------------------------------------- max pooling
def pool_size(h):
    return (h - 1) // 2 + 1


def _windows(v, fill):
    """the nine taps of the 3x3 / 2 / pad-1 window, in the order (dy, dx): [n, oh, ow, c] each"""
    n, h, w, c = v.shape
    oh, ow = pool_size(h), pool_size(w)
    p = np.full((n, 2 * oh + 1, 2 * ow + 1, c), fill, v.dtype)
    p[:, 1:h + 1, 1:w + 1] = v
    return [p[:, dy:dy + 2 * oh:2, dx:dx + 2 * ow:2] for dy in range(3) for dx in range(3)]


def rule_pool(v):
    """3x3 / stride-2 / pad-1 maximum over float64 or fp32 values [n, h, w, c], -inf padding, NaN-propagating"""
    taps = _windows(np.asarray(v), -np.inf)
    out = taps[0]
    for t in taps[1:]:
        out = np.maximum(out, t)
    return out


def emulate_pool(v, mutant=None):
    """rule_pool in the kernels' terms: the fused kernel starts from 0 (its input is a ReLU's), maxpool_s32_kernel from the lowest
    finite value"""
    v = np.asarray(v)
    if mutant == "pool_skips_last_row":
        v = v.copy()
        v[:, -1] = -np.inf
    if mutant == "pool_window_off_by_one":                # window 2y .. 2y + 2
        n, h, w, c = v.shape
        s = np.full((n, h + 1, w + 1, c), -np.inf, v.dtype)
        s[:, :h - 1, :w - 1] = v[:, 1:, 1:]
        v = s[:, :h, :w]
    out = rule_pool(v)
    return np.maximum(out, v.dtype.type(0)) if mutant == "pool_identity_zero_without_relu" else out


def emulate_fused(planes, w16, bias, terms=3, mutant=None):
    """conv_stem_pool_direct_kernel's values, fp32 [n, poh, pow, cout]: conv + bias + ReLU on the map AND on the ring of phantom
    pixels around it, the phantom ones set to 0, then the maximum from 0."""
    v = emulate_conv(planes, w16, bias, terms, True, mutant, phantom=True)
    if mutant != "no_phantom_mask":
        v[:, 0] = v[:, -1] = 0
        v[:, :, 0] = v[:, :, -1] = 0
    n, oh, ow = conv_size(planes)
    if mutant in ("pool_skips_last_row", "pool_window_off_by_one"):
        return np.maximum(emulate_pool(v[:, 1:-1, 1:-1], mutant), F(0.0))
    # pooling the ring-extended map [oh + 2, ow + 2] without padding = pooling the map with the ring as its padding
    taps = [v[:, dy:dy + 2 * pool_size(oh):2, dx:dx + 2 * pool_size(ow):2] for dy in range(3) for dx in range(3)]
    out = np.zeros_like(taps[0])
    for t in taps:
        out = np.maximum(out, t)
    return out


def rule_fused(planes, w16, bias, terms=3):
    """(rule_pool(relu(rule_conv)), the largest S of each window)"""
    y, s = rule_conv(planes, w16, bias, terms, relu=True)
    return rule_pool(y), rule_pool(s)


# ----------------------------------------------------------------------------------------------------------- the S32 pair forms
def split_f32(v):
    """fp32 -> (hi, lo) fp16: hi = fp16(v), lo = fp16(v - hi)"""
    v = np.asarray(v)
    assert v.dtype == F
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(H)
        return hi, (v - hi.astype(F)).astype(H)


def to_s32(hi, lo):
    """(hi, lo) [n, h, w, c] -> S32 [n, h, w, c / 32, 2, 32]"""
    n, h, w, c = hi.shape
    return np.ascontiguousarray(np.stack([hi.reshape(n, h, w, c // 32, 32), lo.reshape(n, h, w, c // 32, 32)], axis=4))


def from_s32(s):
    """S32 -> (hi, lo) [n, h, w, c]"""
    n, h, w, nb = s.shape[:4]
    return s[:, :, :, :, 0].reshape(n, h, w, nb * 32), s[:, :, :, :, 1].reshape(n, h, w, nb * 32)


def pool_pairs(hi, lo):
    """maxpool_s32_kernel on pairs [n, h, w, c]: v = float(hi) + float(lo) in fp32; scanning the window in (dy, dx) order, a tap
    inside the map replaces the best so far if v > best or v is NaN (best starts at -FLT_MAX with the pair (0, 0)); the winner's
    PAIR is copied."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = hi.astype(F) + lo.astype(F)
    inside = _windows(np.ones(v.shape, bool), False)
    tv, th, tl = _windows(v, F(0.0)), _windows(hi, H(0.0)), _windows(lo, H(0.0))
    best = np.full(tv[0].shape, -FLT_MAX, F)
    bh, bl = np.zeros(best.shape, H), np.zeros(best.shape, H)
    for ok, a, b, c in zip(inside, tv, th, tl):
        with np.errstate(invalid="ignore"):
            take = ok & ((a > best) | np.isnan(a))
        best, bh, bl = np.where(take, a, best), np.where(take, b, bh), np.where(take, c, bl)
    return bh, bl


def equal_sum_pair():
    """Two fp32 numbers one fp32 ulp either side of m = 1 + 2^-11, the midpoint of the adjacent fp16 numbers 1 and 1 + 2^-10:
    below, hi = 1 and v - hi = 2^-11 - 2^-23, which fp16 rounds (a tie, to even) to 2^-11; above, hi = 1 + 2^-10 and lo = -2^-11.
    The pairs (1, +2^-11) and (1 + 2^-10, -2^-11) differ and recombine to the same sum m."""
    m = F(1.0) + F(2.0 ** -11)
    return np.nextafter(m, F(0.0)), np.nextafter(m, F(2.0))
