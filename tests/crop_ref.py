"""The rules of the glue between the detector and the pose network, in numpy, with no torch and no GPU: the padded crop box
(pad_hand_box), the slot walk (hand_slots_kernel; the top-1 crop is its one-slot case), the nearest-resize gather
(hand_crop_gather_kernel; all three in csrc/crop_stage.hip), the joint conversion (convert_one) and the lifter's standardisation (joints2d_standardize_kernel,
lifter_input_gated_kernel).  Integers, crops and the fp32 conversion are stated operation for operation, so a kernel is compared
with them bit for bit; the two float64 references (convert64, standardize64) come with a worst-case bound that is derived here
from the operations and not from anything a kernel returned.

WHERE THE BOX RULE LEAVES PYTHON SLICING, ON PURPOSE.  The reference cuts depth[:, b1 : b3 + 1, b0 : b2 + 1].  For a detection
wholly above or left of the frame, or an inverted one, the padded b2 or b3 is negative, and a negative stop of a Python slice
counts from the far end: the reference would return a crop of almost the whole frame.  Here a negative stop is an empty slice:
`ok` is min(b3 + 1, h) - b1 > 0 and min(b2 + 1, w) - b0 > 0, nothing else, and a box that is not ok is "no hand" (zeros).

Non-finite box coordinates have no rule: the conversion of NaN or inf to int64 is undefined in C++.

NaN.  Arithmetic does not pin a NaN's sign or payload (IEEE 754 leaves both to the implementation), so same_bits() takes any
two NaNs for equal and compares every other value bit by bit (-0.0 differs from 0.0)."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
E32 = 2.0 ** -24            # unit roundoff of fp32: |fl(x) - x| <= E32 |x| in the normal range
ETA32 = 2.0 ** -149         # ... + at most half of this where the result is subnormal
U64 = 2.0 ** -53
PERM = (2, 1, 0, 3)         # the RGBD permutation depth_crop[[2, 1, 0, 3]]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    i = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(i) == b.view(i)) | (np.isnan(a) & np.isnan(b))).all())


# --------------------------------------------------------------------------------------------------------------------------
# the padded box
# --------------------------------------------------------------------------------------------------------------------------
def _trunc64(t):
    """fp32 -> int64 toward zero"""
    return np.trunc(t.astype(np.float64)).astype(np.int64)


def pad_boxes(boxes, w, h, mutant=None):
    """pad_box over an array of boxes [..., 4] -> (int64 [..., 4], ok bool [...])"""
    b = np.asarray(boxes, F).reshape(-1, 4)
    bi = _trunc64(b)                                               # trunc toward zero
    size = np.stack((bi[:, 2] - bi[:, 0], bi[:, 3] - bi[:, 1]), 1)  # (bw, bh), exact in int64
    pad = F(0.4) * size.astype(F)                                  # one rounding: int64 -> fp32; one: the product
    bf = bi.astype(F)
    lo, hi = bf[:, :2] - pad, bf[:, 2:] + pad                      # one rounding each
    if mutant == "fma":       # b - 0.4f * bw contracted: the exact product (53 bits hold it), one rounding at the end
        p64 = np.float64(F(0.4)) * size.astype(F).astype(np.float64)
        lo, hi = (bf[:, :2].astype(np.float64) - p64).astype(F), (bf[:, 2:].astype(np.float64) + p64).astype(F)
    to_int = (lambda t: np.rint(t.astype(np.float64)).astype(np.int64)) if mutant == "round" else _trunc64
    lim = np.array([w, h], np.int64)
    below = hi <= lim.astype(F) if mutant == "le_w" else hi < lim.astype(F)
    o = np.concatenate((np.where(lo > 0, to_int(lo), 0), np.where(below, to_int(hi), lim)), 1)
    cw = np.minimum(o[:, 2] + 1, w) - o[:, 0]
    ch = np.minimum(o[:, 3] + 1, h) - o[:, 1]
    ok = (cw > 0) & (ch > 0)                                       # a negative stop is an empty slice (module docstring)
    o[~ok] = 0
    shape = np.asarray(boxes).shape[:-1]
    return o.reshape(shape + (4,)), ok.reshape(shape)


def pad_box(box_f32, w, h, mutant=None):
    """One detection box (x1, y1, x2, y2) in fp32 and the frame's width and height -> (padded box int64 [4], ok).
    b = trunc(box) toward zero as int64; bw = b2 - b0; pw = float32(0.4) * float32(bw); t0 = float32(b0) - pw, t2 = float32(b2) +
    pw, and the same with bh for t1 and t3: every operation one fp32 rounding, nothing contracted.  Then t > 0 ? trunc(t) : 0
    for the first two and t < w ? trunc(t) : w (t < h ...) for the last two.  ok iff min(b3 + 1, h) - b1 > 0 and
    min(b2 + 1, w) - b0 > 0: a negative stop counts as EMPTY -- this is where the rule departs from Python slicing, on
    purpose (module docstring).  The box is zeroed when ok is false; [0, 0, 0, 0] with ok true is the one-pixel crop at the origin."""
    o, ok = pad_boxes(np.asarray(box_f32, F).reshape(1, 4), w, h, mutant)
    return o[0], bool(ok[0])


def slots(boxes, labels, scores, sides, count, cap, hand_label, k, left_side, w, h, mutant=None):
    """One frame's slots.  boxes [cap, 4] fp32, labels / sides [cap] (sides None: the plain form), scores [cap]: the k-th row with
    label hand_label among the first min(count, cap) rows takes slot k, for k < the number of slots.  A rejected box (pad_box not
    ok) still uses up its rank: its slot is empty.  Empty slots are zero with det_index -1, side -1 and mirror 0; a filled slot has
    side = sides[row] and mirror = 1 iff that is left_side."""
    out = dict(crop_box=np.zeros((k, 4), np.int64), has_hand=np.zeros(k, np.int32), score=np.zeros(k, F),
               det_index=np.full(k, -1, np.int32), side=np.full(k, -1, np.int32), mirror=np.zeros(k, np.int32))
    rows = [r for r in range(max(0, min(int(count), cap))) if labels[r] == hand_label]
    if mutant == "rank_skips_rejected":
        rows = [r for r in rows if pad_box(boxes[r], w, h)[1]]
    for s, r in enumerate(rows[:k]):
        box, ok = pad_box(boxes[r], w, h)
        if not ok:
            continue
        out["crop_box"][s], out["has_hand"][s], out["score"][s], out["det_index"][s] = box, 1, scores[r], r
        if sides is not None:
            out["side"][s], out["mirror"][s] = sides[r], int(sides[r] == left_side)
    return out


# --------------------------------------------------------------------------------------------------------------------------
# the nearest resize
# --------------------------------------------------------------------------------------------------------------------------
def src_index(dst, n_in, n_out, mutant=None):
    """min(floor(float32(dst) * (float32(n_in) / float32(n_out))), n_in - 1): F.interpolate(mode="nearest").  The scale is
    rounded once, the product once.  (The kernels' shortcuts, dst for n_in == n_out and dst >> 1 for n_out == 2 n_in, are this
    rule: the scale is then exactly 1 or 0.5.)"""
    d = np.asarray(dst).astype(F)
    if mutant == "mul_first":
        s = np.floor((d * F(n_in)) / F(n_out)).astype(np.int64)
    elif mutant == "shift_2in1" and n_out == 2 * n_in + 1:
        s = np.asarray(dst).astype(np.int64) >> 1
    else:
        s = np.floor(d * (F(n_in) / F(n_out))).astype(np.int64)
    return s if mutant == "no_clamp" else np.minimum(s, n_in - 1)


def crop_size(box, w, h):
    """(cw, ch) of the clamped inclusive slice"""
    return int(min(box[2] + 1, w) - box[0]), int(min(box[3] + 1, h) - box[1])


def gather(depth, box, has, mirror, out, cpad, reorder, mutant=None):
    """depth [C, H, W] fp32, a padded box -> the crop [out, out, cpad] (NHWC): pixel (oy, ox) is depth[perm(c), b1 + sy, b0 + sx]
    with sy = src_index(oy, ch, out) and sx = src_index(ox, cw, out) -- of out - 1 - ox for a mirrored slot --, channel c of a
    reordered image reads channel [2, 1, 0, 3][c]; channels at and beyond C are zero, and so is all of a slot without a hand."""
    c, h, w = depth.shape
    o = np.zeros((out, out, cpad), F)
    if not has:
        return o
    cw, ch = crop_size(box, w, h)
    ox = np.arange(out)
    sy = int(box[1]) + src_index(ox, ch, out, mutant)
    sx = int(box[0]) + src_index(out - 1 - ox if mirror else ox, cw, out, mutant)
    for k in range(c):
        o[:, :, k] = depth[PERM[k] if reorder else k][sy[:, None], sx[None, :]]
    return o


# --------------------------------------------------------------------------------------------------------------------------
# the joint conversion
# --------------------------------------------------------------------------------------------------------------------------
def _convert(T, kp, box, paras, crop_w, crop_h, clamp_kp, clamp_box, valid, mutant=None):
    kp = np.asarray(kp, F)
    n = kp.shape[0]
    b = np.asarray(box)
    assert b.dtype in (np.int64, np.float32) and b.shape == (n, 4)
    x0, y0, x1, y1 = (b[:, i].astype(T)[:, None] for i in range(4))
    ku, kv, kd = (kp[..., i].astype(T) for i in range(3))
    cw, ch = T(F(crop_w)), T(F(crop_h))
    if clamp_box:             # ros_demo.py as written: x0, y0 to [0, H] and x1, y1 to [0, W] (boxes are never NaN)
        ch_, cw_ = T(clamp_box[0]), T(clamp_box[1])
        x0, y0 = np.minimum(np.maximum(x0, T(0)), ch_), np.minimum(np.maximum(y0, T(0)), ch_)
        x1, y1 = np.minimum(np.maximum(x1, T(0)), cw_), np.minimum(np.maximum(y1, T(0)), cw_)
    if clamp_kp:              # all three to [0, crop_w] (the caller clamps them to [0, 176]); torch.clamp keeps a NaN
        ku, kv, kd = (np.where(np.isnan(t), t, np.minimum(np.maximum(t, T(0)), cw)) for t in (ku, kv, kd))
    with np.errstate(all="ignore"):
        u = ku * (x1 - x0) / cw + x0
        v = kv * (y1 - y0) / (cw if mutant == "crop_w_for_v" else ch) + y0
        img = np.stack((u, v, kd), -1)
        xyz = None
        if paras is not None:
            p = np.asarray(paras, F).astype(T)
            fx, fy, cx, cy = (p[i] for i in range(4)) if p.ndim == 1 else (p[:, i][:, None] for i in range(4))
            xyz = np.stack(((u - cx) * kd / fx * T(1000), (v - cy) * kd / fy * T(1000), kd * T(1000)), -1)
    if valid is not None:
        dead = np.asarray(valid) == 0
        img[dead] = 0
        if xyz is not None:
            xyz[dead] = 0
    return img, xyz, (ku, kv, kd, x0, y0, x1, y1)


def convert32(kp, box, paras, crop_w, crop_h, clamp_kp=False, clamp_box=None, valid=None, mutant=None):
    """convert_one restated, one fp32 rounding per operation in its order: kp [n, J, 3] crop-(u, v, d), box [n, 4] int64 (the
    detector's; converted to fp32 first) or fp32 (the dataset's), paras None, (fx, fy, cx, cy) or one row per sample ->
    (image (u, v, d), camera xyz in mm or None):  u = ku * (x1 - x0) / crop_w + x0, v = kv * (y1 - y0) / crop_h + y0,
    X = (u - cx) * d / fx * 1000, Y likewise, Z = d * 1000.  clamp_box = (H, W): the ros_demo clamp as written there, x0 and y0 to
    [0, H], x1 and y1 to [0, W].  clamp_kp: ku, kv and d to [0, crop_w]; a NaN stays NaN.  Rows with valid == 0 are zeros."""
    img, xyz, _ = _convert(F, kp, box, paras, crop_w, crop_h, clamp_kp, clamp_box, valid, mutant)
    assert img.dtype == F and (xyz is None or xyz.dtype == F)
    return img, xyz


def convert64(kp, box, paras, crop_w, crop_h, clamp_kp=False, clamp_box=None, valid=None):
    """convert32 in float64 (the inputs are the same fp32 / int64 values; the clamps are exact in both)"""
    img, xyz, _ = _convert(np.float64, kp, box, paras, crop_w, crop_h, clamp_kp, clamp_box, valid)
    return img, xyz


def convert_bound(kp, box, paras, crop_w, crop_h, clamp_kp=False, clamp_box=None, valid=None):
    """The worst |convert32 - convert64|, per element -> (bound of image uvd, bound of xyz or None).

    Every fp32 operation returns fl(x) with |fl(x) - x| <= e |x| + eta, e = 2^-24, eta = 2^-149 (the second term only where the
    result is subnormal).  The operands after the clamps are the same numbers in both precisions: the clamps only select, and
    box corners below 2^24 convert to fp32 exactly (asserted).  With q = ku (x1 - x0) / crop_w in exact arithmetic the kernel has
        d^ = (x1 - x0)(1 + d1),  p^ = ku d^ (1 + d2),  q^ = p^ / crop_w (1 + d3),  u^ = (q^ + x0)(1 + d4),   |di| <= e
    so |q^ - q| <= g3 |q| with g3 = (1 + e)^3 - 1, and
        B_u = |u^ - u| <= g3 |q| + e (|q| (1 + g3) + |x0|) + 4 eta.
    v likewise with crop_h; d is copied: bound 0.  Then, each line one more rounding on top of the error it inherits,
        a = u - cx:     B_a = B_u (1 + e) + e |a| + eta
        m = a d:        B_m = |d| B_a (1 + e) + e |m| + eta
        r = m / fx:     B_r = B_m / |fx| (1 + e) + e |r| + eta
        X = 1000 r:     B_X = 1000 B_r (1 + e) + e |X| + eta
        Z = 1000 d:     B_Z = e |Z| + eta
    The exact values on the right are taken from convert64, whose own error (a few 2^-53 relative) is covered by the factor
    1 + 2^-20 on the whole bound.  A non-finite reference has no bound (inf): the comparison then asks for the same class."""
    _, _, (ku, kv, kd, x0, y0, x1, y1) = _convert(np.float64, kp, box, paras, crop_w, crop_h, clamp_kp, clamp_box, None)
    assert max(np.abs(t).max() for t in (x0, y0, x1, y1)) < 2.0 ** 24
    e, eta, slack = E32, ETA32, 1.0 + 2.0 ** -20
    g3 = (1 + e) ** 3 - 1
    cw, ch = float(F(crop_w)), float(F(crop_h))
    with np.errstate(all="ignore"):
        qu, qv = ku * (x1 - x0) / cw, kv * (y1 - y0) / ch
        bu = g3 * np.abs(qu) + e * (np.abs(qu) * (1 + g3) + np.abs(x0)) + 4 * eta
        bv = g3 * np.abs(qv) + e * (np.abs(qv) * (1 + g3) + np.abs(y0)) + 4 * eta
        img = np.stack((bu, bv, np.zeros_like(bu)), -1) * slack
        xyz = None
        if paras is not None:
            p = np.asarray(paras, F).astype(np.float64)
            fx, fy, cx, cy = (p[i] for i in range(4)) if p.ndim == 1 else (p[:, i][:, None] for i in range(4))
            cols = []
            for q, b0, bq, f, c in ((qu, x0, bu, fx, cx), (qv, y0, bv, fy, cy)):
                a = q + b0 - c
                ba = bq * (1 + e) + e * np.abs(a) + eta
                m = a * kd
                bm = np.abs(kd) * ba * (1 + e) + e * np.abs(m) + eta
                r = m / f
                br = bm / np.abs(f) * (1 + e) + e * np.abs(r) + eta
                cols.append(1000 * br * (1 + e) + e * np.abs(1000 * r) + eta)
            cols.append(e * np.abs(1000 * kd) + eta)
            xyz = np.stack(cols, -1) * slack
        img[~np.isfinite(img)] = np.inf
        if xyz is not None:
            xyz[~np.isfinite(xyz)] = np.inf
    if valid is not None:
        dead = np.asarray(valid) == 0
        img[dead] = 0
        if xyz is not None:
            xyz[dead] = 0
    return img, xyz


def bound_ratio(got, want64, bound):
    """max |got - want| / bound over the elements with a finite reference; asserts that the others are of the same class (NaN with
    NaN, +-inf with the same inf) and that an element with bound 0 is equal"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    fin = np.isfinite(want64)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), "NaN differs"
    assert np.array_equal(got[~fin & ~np.isnan(want64)], want64[~fin & ~np.isnan(want64)]), "inf differs"
    err = np.abs(got[fin] - want64[fin])
    b = np.broadcast_to(bound, want64.shape)[fin]
    assert (err[b == 0] == 0).all(), "an element with bound 0 differs"
    return float((err[b > 0] / b[b > 0]).max(initial=0.0))


# --------------------------------------------------------------------------------------------------------------------------
# the lifter's standardisation
# --------------------------------------------------------------------------------------------------------------------------
def standardize64(uv):
    """uv [n, J, 2] fp32 -> (x - mean) / std per row and axis over the J joints, population std, as float64 [n, J, 2].  Mean and
    variance are exact rationals of the fp32 inputs, so the result carries three float64 roundings (the variance, its root, the
    quotient) and nothing that grows with J or with mean / std.  std == 0 gives NaN (0 / 0), as the kernel's division does."""
    uv = np.asarray(uv, F)
    out = np.full(uv.shape, np.nan)
    for i in range(uv.shape[0]):
        for ax in range(2):
            x = [Fraction(float(t)) for t in uv[i, :, ax]] if np.isfinite(uv[i, :, ax]).all() else None
            if x is None:
                continue
            m = sum(x) / len(x)
            a = [t - m for t in x]
            var = sum(t * t for t in a) / len(x)
            if var > 0:
                s = math.sqrt(var)
                out[i, :, ax] = [float(t) / s for t in a]
    return out


def standardize_bound(uv):
    """The worst |kernel - standardize64| per element, for the kernel's scheme: float64 sums in joint order, then ONE fp32
    rounding on store.  With u = 2^-53, X = max |x|, S the true std, z = (x - m) / S:
      * the mean: a sequential sum of J terms and a division, |m^ - m| <= J u X =: dm;       rho := dm / S
      * a^_j = fl(x_j - m^) = a_j + eps_j with |eps_j| <= dm + u |a^_j|.  The vector a^ is a + eps, so by the triangle inequality
        its norm is within (rho + u) relative of |a| = sqrt(J) S; the sum of squares adds at most (J + 1) u relative (with or
        without an fma), the division by J and the root one rounding each:  |S^ - S| <= kappa S, kappa = rho + (J + 4) u
      * the quotient in float64: |a^_j / S^ - z_j| <= (rho + |z_j| (kappa + 2 u)) (1 + 2 kappa) / (1 - kappa), and one more u
      * the store: e |z^|, e = 2^-24
    Together, for kappa < 1/4 (asserted; the factor 2 covers every second-order factor above and standardize64's own three
    roundings):  bound = e |z| + 2 (rho + |z| (kappa + 2 u)) + 2^-149.   Rows with std == 0 or a non-finite joint: inf."""
    uv = np.asarray(uv, F).astype(np.float64)
    j = uv.shape[1]
    z = standardize64(uv)
    with np.errstate(all="ignore"):
        s = uv.std(axis=1, keepdims=True)
        rho = j * U64 * np.abs(uv).max(axis=1, keepdims=True) / s
        kappa = rho + (j + 4) * U64
        b = E32 * np.abs(z) + 2 * (rho + np.abs(z) * (kappa + 2 * U64)) + ETA32
    good = np.isfinite(z)
    assert (np.broadcast_to(kappa, z.shape)[good] < 0.25).all()
    b[~good] = np.inf
    return b


def gate32(uv):
    """lifter_input_gated_kernel's skip rule, fp32 with one rounding per operation: every (u, v) finite, and with lo / hi the
    extremes of an axis, center = (lo + hi) * 0.5, half = 0.5 * (hi - lo), start = center - half, size = (center + half) - start:
    w * h > 0 and x + (w - 1) >= x and y + (h - 1) >= y  ->  bool [n]"""
    uv = np.asarray(uv, F)
    keep = np.isfinite(uv).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        lo, hi = uv.min(axis=1), uv.max(axis=1)
        center, half = (lo + hi) * F(0.5), F(0.5) * (hi - lo)
        start = center - half
        size = (center + half) - start
        keep &= (size[:, 0] * size[:, 1] > 0) & (start[:, 0] + (size[:, 0] - F(1)) >= start[:, 0]) \
            & (start[:, 1] + (size[:, 1] - F(1)) >= start[:, 1])
    return keep
