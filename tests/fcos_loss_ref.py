"""The FCOS criterion (fcos_utils/fcos.py:523-570 the matching, :44-178 the six terms, fcos_utils/utils.py the GIoU loss,
det_utils.py:233-264 encode_single, torchvision's sigmoid_focal_loss; csrc/fcos_loss.hip fcos_loss_kernel + fcos_loss_reduce_kernel)
as a rule, its worst-case fp32 error bound, an fp32 emulation of the two kernels' arithmetic in their order, and that emulation
with one deliberate mistake each.  numpy only; nothing here reads the library.

Layout (what ops.fcos_loss takes): per level l, cls_lr[l] [n, h, w, C + 2], reg_ctr[l] [n, h, w, 5] (relu'd regressions, then the
centre-ness logit) and, with ext, ext[l] [n, h, w, 8] (relu'd (mag, dx, dy), then five contact logits); the points of an image
in anchor order (tests/cand_ref.py).  Targets: gt_boxes [n, G, 4] fp32 ALREADY SCALED to the canvas, gt_labels [n, G] int32,
gt_info [n, G, 5] fp32 = (contactstate, handside, mag, dx, dy), gt_count [n] (clamped to [0, G]; rows beyond it are padding).
Results:
  matched [n, P] int32  index of the point's ground-truth box, -1 for background
  fg      [n]           foreground points
  terms   [n, 6]        per-image SUMS before any factor or division, in the key order: focal(cls), GIoU, centre-ness BCE,
                        focal(hand_lr), focal(hand_contact_state), squared dxdy differences (the last two zero without ext)
  losses  [6]           the batch's dict values, KEYS order (without ext the last two are zero and not in the dict)

The matching is stated in float32, operation for operation as the reference runs it on float32 targets; the terms in float64
on the float32 inputs.  The reference's quirks, restated and not repaired:
  * the "area" that picks among several matching boxes is (y0 - x0) * (y1 - y0), line 563, not the box area;
  * the key 1e8 - area is float32: one ulp at 1e8 is 8, areas closer than that tie, and the first index wins a tie;
  * lower = 0 on the first level, then upper = inf on the last: a one-level table has both;
  * a background point's dxdy target is the row of ground truth 0 (matched.clip(min=0)), and hand_dxdy is a mean over ALL
    n * P * 3 elements, times 10, then divided by the foreground count like the sums;
  * the side and contact targets are (long) of a float: truncation; a negative value is "no column" for that head alone.
An image with count 0 is all background with zero dxdy targets (the drop-in refuses it with ext, as the reference raises).
"""
import numpy as np

import cand_ref as cr

U = 2.0 ** -24
F = np.float32
D = np.float64
TINY = 2.0 ** -126          # a result below the normal range: flushed or denormal, off by this much at most
MAX_GT = 64
KEYS = ("classification", "bbox_regression", "bbox_ctrness", "hand_lr", "hand_contact_state", "hand_dxdy")
MUTANTS = ("alpha_026", "dxdy_no_x10", "dxdy_fg_only", "true_area", "inside_ge", "lower_ge", "divisor_no_max", "last_tie")
ALPHA, SCALE_LR, SCALE_CONTACT, SCALE_DXDY, GIOU_EPS, NORM_EPS = 0.25, 2e-2, 1e-2, 10.0, 1e-7, 1e-12
# additions a value passes through on its way into the chunk's partial sum: the 6 shuffle steps of the wave, the 16 waves of the
# workgroup (the per-thread column sums are part of the chain itself)
DEPTH = 6 + 16


# --------------------------------------------------------------------------------------------------------------------------
# geometry and matching (float32)
# --------------------------------------------------------------------------------------------------------------------------
def flatten(cls_lr, reg_ctr, ext=None):
    cls, reg, sizes = cr.flatten(cls_lr, reg_ctr)
    ex = None
    if ext is not None:
        assert [t.shape[1:3] for t in ext] == list(sizes) and all(t.shape[3] == 8 and t.dtype == F for t in ext)
        ex = np.concatenate([t.reshape(t.shape[0], -1, 8) for t in ext], 1)
    return cls, reg, ex, [tuple(int(v) for v in s) for s in sizes]


def geometry(sizes, strides):
    """per point, the kernel's anchor (cand_ref.boxes32): fp32 centre (cx, cy), size (bw = bh), and the level's first / last flags"""
    lvl, gx, gy, st = cr.grid(sizes, strides)
    half = np.rint((st.astype(F) * F(0.5)).astype(F)).astype(F)
    px, py = (gx * st).astype(F), (gy * st).astype(F)
    ax0, ay0, ax1, ay1 = px - half, py - half, px + half, py + half
    return dict(cx=(F(0.5) * (ax0 + ax1)).astype(F), cy=(F(0.5) * (ay0 + ay1)).astype(F), size=(ax1 - ax0).astype(F),
                first=lvl == 0, last=lvl == len(sizes) - 1)


def match(boxes, count, geo, radius=1.5, mutant=None):
    """fcos.py:531-568 for one image, every operation in float32: boxes [G, 4] -> matched [P] int32"""
    assert boxes.dtype == F and boxes.ndim == 2
    p = geo["cx"].shape[0]
    g = int(min(max(int(count), 0), boxes.shape[0]))
    if g == 0:
        return np.full((p,), -1, np.int32)
    x0, y0, x1, y1 = (boxes[:g, k][None, :] for k in range(4))
    gcx, gcy = (x0 + x1) / F(2), (y0 + y1) / F(2)
    cx, cy, size = geo["cx"][:, None], geo["cy"][:, None], geo["size"][:, None]
    m = np.maximum(np.abs(cx - gcx), np.abs(cy - gcy)) < F(radius) * size
    dist = np.stack([cx - x0, cy - y0, x1 - cx, y1 - cy], -1)
    assert dist.dtype == F
    m &= (dist.min(-1) >= 0) if mutant == "inside_ge" else (dist.min(-1) > 0)
    lower, upper = size * F(4), size * F(8)
    lower = np.where(geo["first"][:, None], F(0), lower)
    upper = np.where(geo["last"][:, None], F(np.inf), upper)
    far = dist.max(-1)
    m &= ((far >= lower) if mutant == "lower_ge" else (far > lower)) & (far < upper)
    area = (x1 - x0) * (y1 - y0) if mutant == "true_area" else (y0 - x0) * (y1 - y0)
    key = F(1e8) - area
    val = np.where(m, key, F(0)).astype(F)
    idx = (g - 1 - val[:, ::-1].argmax(1)) if mutant == "last_tie" else val.argmax(1)
    idx = idx.astype(np.int32)
    idx[val.max(1) < F(1e-5)] = -1
    return idx


def targets(matched, labels, info, count):
    """per point of one image: class, side and contact targets (-1: no column) and the dxdy target [P, 3] fp32"""
    fg = matched >= 0
    m0 = np.maximum(matched, 0)
    if int(count) <= 0:
        none = np.full(matched.shape, -1, np.int64)
        return none, none.copy(), none.copy(), np.zeros(matched.shape + (3,), F)
    cls_t = np.where(fg, labels[m0].astype(np.int64), -1)
    side_t = np.where(fg, np.trunc(info[m0, 1]).astype(np.int64), -1)
    contact_t = np.where(fg, np.trunc(info[m0, 0]).astype(np.int64), -1)
    return cls_t, side_t, contact_t, info[m0, 2:5]


def _match_all(sizes, strides, gt_boxes, gt_count, radius, mutant=None):
    geo = geometry(sizes, strides)
    return geo, np.stack([match(gt_boxes[i], gt_count[i], geo, radius, mutant) for i in range(gt_boxes.shape[0])])


# --------------------------------------------------------------------------------------------------------------------------
# the rule's terms (float64, the reference's formulas as they are written)
# --------------------------------------------------------------------------------------------------------------------------
def _focal_literal(x, t, alpha=ALPHA):
    """torchvision sigmoid_focal_loss(reduction='none'), gamma 2: x [P, K] float64, t [P] target column or -1"""
    y = (np.arange(x.shape[1])[None, :] == t[:, None]).astype(D)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        ce = np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))
    p_t = p * y + (1 - p) * (1 - y)
    return ce * (1 - p_t) ** 2 * (alpha * y + (1 - alpha) * (1 - y))


def _giou_literal(b1, b2, eps=GIOU_EPS):
    x1, y1, x2, y2 = b1.T
    x1g, y1g, x2g, y2g = b2.T
    xk1, yk1, xk2, yk2 = np.maximum(x1, x1g), np.maximum(y1, y1g), np.minimum(x2, x2g), np.minimum(y2, y2g)
    inter = np.where((yk2 > yk1) & (xk2 > xk1), (xk2 - xk1) * (yk2 - yk1), 0.0)
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    iou = inter / (union + eps)
    area_c = (np.maximum(x2, x2g) - np.minimum(x1, x1g)) * (np.maximum(y2, y2g) - np.minimum(y1, y1g))
    return 1 - (iou - (area_c - union) / (area_c + eps))


def rule(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius=1.5):
    """{matched, fg, terms, losses}: the matching in float32, the terms in float64 on the float32 inputs"""
    cls, reg, ex, sizes = flatten(cls_lr, reg_ctr, ext)
    n, p, c = cls.shape[0], cls.shape[1], num_classes
    assert gt_boxes.dtype == F and gt_info.dtype == F and gt_boxes.shape[1] <= MAX_GT
    geo, matched = _match_all(sizes, strides, gt_boxes, gt_count, radius)
    cx, cy, size = (geo[k].astype(D) for k in ("cx", "cy", "size"))
    terms = np.zeros((n, 6))
    for i in range(n):
        m = matched[i]
        fg = m >= 0
        cls_t, side_t, contact_t, dxdy_t = targets(m, gt_labels[i], gt_info[i], gt_count[i])
        x = cls[i].astype(D)
        terms[i, 0] = _focal_literal(x[:, :c], cls_t).sum()
        terms[i, 3] = _focal_literal(x[:, c:c + 2], side_t).sum()
        r = reg[i, fg].astype(D)
        acx, acy, asz = cx[fg], cy[fg], size[fg]
        pred = np.stack([acx - r[:, 0] * asz, acy - r[:, 1] * asz, acx + r[:, 2] * asz, acy + r[:, 3] * asz], -1)
        box = gt_boxes[i, m[fg]].astype(D)
        terms[i, 1] = _giou_literal(pred, box).sum()
        enc = np.stack([acx - box[:, 0], acy - box[:, 1], box[:, 2] - acx, box[:, 3] - acy], -1) / asz[:, None]
        lr_, tb = enc[:, [0, 2]], enc[:, [1, 3]]
        ctr_t = np.sqrt(np.abs((lr_.min(-1) / lr_.max(-1)) * (tb.min(-1) / tb.max(-1))))
        z = r[:, 4]
        terms[i, 2] = (np.maximum(z, 0.0) - z * ctr_t + np.log1p(np.exp(-np.abs(z)))).sum()
        if ex is not None:
            e = ex[i].astype(D)
            terms[i, 4] = _focal_literal(e[:, 3:8], contact_t).sum()
            den = np.maximum(np.sqrt(e[:, 1] ** 2 + e[:, 2] ** 2), NORM_EPS)
            pred3 = np.stack([e[:, 0], 0.1 * (e[:, 1] / den), 0.1 * (e[:, 2] / den)], -1)
            terms[i, 5] = ((pred3 - dxdy_t.astype(D)) ** 2).sum()
    fgs = (matched >= 0).sum(1).astype(np.int64)
    return dict(matched=matched, fg=fgs, terms=terms, losses=_losses(terms, fgs, p))


def _losses(terms, fgs, p, mutant=None):
    """the dict values from the per-image sums (float64)"""
    n = terms.shape[0]
    div = float(fgs.sum()) if mutant == "divisor_no_max" else float(max(1, int(fgs.sum())))
    s = terms.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([s[0] / div, s[1] / div, s[2] / div, s[3] * SCALE_LR / div, s[4] * SCALE_CONTACT / div,
                         (1.0 if mutant == "dxdy_no_x10" else SCALE_DXDY) * (s[5] / (n * p * 3)) / div])


# --------------------------------------------------------------------------------------------------------------------------
# the kernel's chain, written once over two arithmetics: fp32 values (emulate) and float64 values with a running bound
# --------------------------------------------------------------------------------------------------------------------------
class _F32:
    """numpy fp32, one rounding per operation"""
    def inp(self, x): return np.asarray(x, F)
    def const(self, x, like): return np.full(np.shape(like.v if hasattr(like, "v") else like), F(x), F)
    def add(self, a, b): return (a + b).astype(F)
    def sub(self, a, b): return (a - b).astype(F)
    def mul(self, a, b): return (a * b).astype(F)
    def div(self, a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return (a / b).astype(F)
    def max(self, a, b): return np.maximum(a, b)
    def min(self, a, b): return np.minimum(a, b)
    def abs(self, a): return np.abs(a)
    def neg(self, a): return -a
    def sqrt(self, a): return np.sqrt(a).astype(F)
    def exp(self, a):
        with np.errstate(under="ignore"):
            return np.exp(a).astype(F)
    def log1p(self, a): return np.log1p(a).astype(F)
    def where(self, c, a, b): return np.where(c, a, b).astype(F)
    def val(self, a): return a


class _V:
    __slots__ = ("v", "d")
    def __init__(self, v, d): self.v, self.d = v, d


def _rnd(v, d, ulps=1.0):
    return _V(v, d + ulps * U * (np.abs(v) + d) + TINY)


class _Err:
    """float64 values with the worst-case distance of ANY fp32 evaluation of the same chain: "one rounding of v known to d" is
    d + u (|v| + d) (tests/loss_ref.py), + TINY where the result may fall below the normal range; expf, log1pf: 1 ulp = 2 u
    (tests/agg_ref.py's figure for expf); sqrtf, the division: correctly rounded."""
    def inp(self, x):
        x = np.asarray(x, D)
        return _V(x, np.zeros_like(x))
    def const(self, x, like):
        z = np.zeros(np.shape(like.v))
        return _V(z + float(x), z + abs(float(F(x)) - float(x)))
    def add(self, a, b): return _rnd(a.v + b.v, a.d + b.d)
    def sub(self, a, b): return _rnd(a.v - b.v, a.d + b.d)
    def mul(self, a, b): return _rnd(a.v * b.v, np.abs(a.v) * b.d + np.abs(b.v) * a.d + a.d * b.d)
    def div(self, a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            v = a.v / b.v
            room = np.abs(b.v) - b.d
            d = np.where(room > 0, (a.d + np.abs(v) * b.d) / np.where(room > 0, room, 1.0), np.inf)
        return _rnd(v, d)
    def max(self, a, b): return _V(np.maximum(a.v, b.v), np.maximum(a.d, b.d))
    def min(self, a, b): return _V(np.minimum(a.v, b.v), np.maximum(a.d, b.d))
    def abs(self, a): return _V(np.abs(a.v), a.d)
    def neg(self, a): return _V(-a.v, a.d)
    def sqrt(self, a):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.sqrt(a.v)
            d = np.minimum(np.where(a.v > 0, a.d / np.where(a.v > 0, r, 1.0), np.inf), np.sqrt(a.d))
        return _rnd(r, d)
    def exp(self, a):
        with np.errstate(under="ignore"):
            v = np.exp(a.v)
        return _rnd(v, v * np.expm1(a.d), 2.0)
    def log1p(self, a):       # a >= 0: slope 1 / (1 + a) <= 1
        return _rnd(np.log1p(a.v), a.d / (1.0 + np.maximum(a.v - a.d, 0.0)), 2.0)
    def where(self, c, a, b): return _V(np.where(c, a.v, b.v), np.where(c, a.d, b.d))
    def val(self, a): return a.v


def _focal_chain(o, x, t, alpha):
    """[P] per-thread sum over the K columns of alpha_t * softplus(z) * sigmoid(z)^2, z = -x on the target column, x elsewhere
    (the same function as torchvision's ce * (1 - p_t)^2 * alpha_t, without its cancellation)"""
    acc = None
    for k in range(x.shape[1]):
        hit = t == k
        xk = o.inp(x[:, k])
        z = o.where(hit, o.neg(xk), xk)
        e = o.exp(o.neg(o.abs(z)))
        one = o.const(1.0, e)
        sp = o.add(o.max(z, o.const(0.0, e)), o.log1p(e))
        den = o.add(one, e)
        sig = o.where(x[:, k] * np.where(hit, -1, 1) >= 0, o.div(one, den), o.div(e, den))
        a = o.where(hit, o.const(alpha, e), o.const(1.0 - alpha, e))
        v = o.mul(o.mul(sp, o.mul(sig, sig)), a)
        acc = v if acc is None else o.add(acc, v)
    return acc


def _fg_chain(o, reg, box, cx, cy, size):
    """(GIoU loss, centre-ness BCE) of the foreground points: decode, fcos_utils/utils.py, encode_single + BCE-with-logits"""
    r = [o.inp(reg[:, k]) for k in range(5)]
    b = [o.inp(box[:, k]) for k in range(4)]
    acx, acy, sz = o.inp(cx), o.inp(cy), o.inp(size)
    x1, y1 = o.sub(acx, o.mul(r[0], sz)), o.sub(acy, o.mul(r[1], sz))
    x2, y2 = o.add(acx, o.mul(r[2], sz)), o.add(acy, o.mul(r[3], sz))
    zero = o.const(0.0, acx)
    iw = o.max(o.sub(o.min(x2, b[2]), o.max(x1, b[0])), zero)
    ih = o.max(o.sub(o.min(y2, b[3]), o.max(y1, b[1])), zero)
    inter = o.mul(iw, ih)
    union = o.sub(o.add(o.mul(o.sub(x2, x1), o.sub(y2, y1)), o.mul(o.sub(b[2], b[0]), o.sub(b[3], b[1]))), inter)
    eps = o.const(GIOU_EPS, acx)
    iou = o.div(inter, o.add(union, eps))
    area_c = o.mul(o.sub(o.max(x2, b[2]), o.min(x1, b[0])), o.sub(o.max(y2, b[3]), o.min(y1, b[1])))
    miou = o.sub(iou, o.div(o.sub(area_c, union), o.add(area_c, eps)))
    giou = o.sub(o.const(1.0, acx), miou)
    l, t = o.div(o.sub(acx, b[0]), sz), o.div(o.sub(acy, b[1]), sz)
    rr, bb = o.div(o.sub(b[2], acx), sz), o.div(o.sub(b[3], acy), sz)
    tgt = o.sqrt(o.abs(o.mul(o.div(o.min(l, rr), o.max(l, rr)), o.div(o.min(t, bb), o.max(t, bb)))))
    z = r[4]
    bce = o.add(o.sub(o.max(z, zero), o.mul(z, tgt)), o.log1p(o.exp(o.neg(o.abs(z)))))
    return giou, bce


def _dxdy_chain(o, e, tgt):
    """[P] per-thread sum of the three squared differences of (mag, 0.1 dx / max(|(dx, dy)|, 1e-12), 0.1 dy / ...)"""
    mag, dx, dy = (o.inp(e[:, k]) for k in range(3))
    den = o.max(o.sqrt(o.add(o.mul(dx, dx), o.mul(dy, dy))), o.const(NORM_EPS, mag))
    tenth = o.const(0.1, mag)
    pred = (mag, o.mul(tenth, o.div(dx, den)), o.mul(tenth, o.div(dy, den)))
    acc = None
    for k in range(3):
        diff = o.sub(pred[k], o.inp(tgt[:, k]))
        sq = o.mul(diff, diff)
        acc = sq if acc is None else o.add(acc, sq)
    return acc


def _point_values(o, cls, reg, ex, c, geo, m, boxes, labels, info, count, mutant=None):
    """one image: the six per-point values ([P] each, zeros where a term has no share) in the arithmetic o"""
    p = cls.shape[0]
    fg = m >= 0
    cls_t, side_t, contact_t, dxdy_t = targets(m, labels, info, count)
    alpha = 0.26 if mutant == "alpha_026" else ALPHA
    zero = o.inp(np.zeros((p,)))
    out = [_focal_chain(o, cls[:, :c], cls_t, alpha), zero, zero, _focal_chain(o, cls[:, c:c + 2], side_t, alpha), zero, zero]
    if fg.any():
        g, b = _fg_chain(o, reg[fg], boxes[m[fg]], geo["cx"][fg], geo["cy"][fg], geo["size"][fg])
        for k, part in ((1, g), (2, b)):
            full = o.inp(np.zeros((p,)))
            if isinstance(full, _V):
                full.v[fg], full.d[fg] = part.v, part.d
            else:
                full[fg] = part
            out[k] = full
    if ex is not None:
        out[4] = _focal_chain(o, ex[:, 3:8], contact_t, alpha)
        sq = _dxdy_chain(o, ex[:, :3], dxdy_t)
        out[5] = o.where(fg, sq, zero) if mutant == "dxdy_fg_only" else sq
    return out


def bound(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius=1.5):
    """Worst-case forward error of {terms, losses} for ANY fp32 evaluation of the kernels' chain (matched and fg are exact claims):
      * per point, the running bound of _Err through the chain _point_values states, plus the distance of that chain's float64
        value from the rule's (the two are the same function written differently: ~1e-16 relative);
      * the chunk's partial sum: a sequential-sum model with the number of additions a value really passes through, DEPTH
        (adding an exact zero rounds nothing): sum d_i + DEPTH u sum (|v_i| + d_i);
      * the chunk partials are widened and added in float64 (2^-53 per addition, counted), terms rounds the image's sum to fp32
        once, losses = the float64 sums times the factor over the divisor, rounded to fp32 once."""
    cls, reg, ex, sizes = flatten(cls_lr, reg_ctr, ext)
    n, p = cls.shape[:2]
    ref = rule(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius)
    geo = geometry(sizes, strides)
    o = _Err()
    chunks = (p + 1023) // 1024
    ds = np.zeros((n, 6))
    for i in range(n):
        vals = _point_values(o, cls[i], reg[i], ex[i] if ex is not None else None, num_classes, geo, ref["matched"][i],
                             gt_boxes[i], gt_labels[i], gt_info[i], gt_count[i])
        for k, t in enumerate(vals):
            mag = (np.abs(t.v) + t.d).sum()
            ds[i, k] = t.d.sum() + DEPTH * U * mag + chunks * 2.0 ** -53 * mag + abs(t.v.sum() - ref["terms"][i, k])
    d_terms = ds + U * (np.abs(ref["terms"]) + ds)
    div = float(max(1, int(ref["fg"].sum())))
    s = ds.sum(0)
    d_losses = np.array([s[0] / div, s[1] / div, s[2] / div, s[3] * SCALE_LR / div, s[4] * SCALE_CONTACT / div,
                         SCALE_DXDY * (s[5] / (n * p * 3)) / div])
    d_losses = d_losses + U * (np.abs(ref["losses"]) + d_losses) + 8 * 2.0 ** -53 * np.abs(ref["losses"])
    return dict(terms=d_terms, losses=d_losses)


def _chunk_sum(v):
    """[P] fp32 per-point values -> float64 image sum in the kernels' order: xor butterfly over the 64 lanes, the 16 waves in
    order, the chunks in order in float64"""
    p = v.shape[0]
    chunks = (p + 1023) // 1024
    w = np.zeros((chunks * 1024,), F)
    w[:p] = v
    w = w.reshape(chunks, 16, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, :, lane ^ off]).astype(F)
    tot = np.zeros((chunks,), F)
    for k in range(16):
        tot = (tot + w[:, k, 0]).astype(F)
    s = D(0.0)
    for c in range(chunks):
        s = s + D(tot[c])
    return s


def emulate(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius=1.5, mutant=None):
    """The two kernels' arithmetic in numpy fp32, in their order.  (No fma: the library is built with contraction off.)"""
    assert mutant is None or mutant in MUTANTS
    cls, reg, ex, sizes = flatten(cls_lr, reg_ctr, ext)
    n, p = cls.shape[:2]
    geo, matched = _match_all(sizes, strides, gt_boxes, gt_count, radius, mutant)
    o = _F32()
    sums = np.zeros((n, 6), D)
    for i in range(n):
        vals = _point_values(o, cls[i], reg[i], ex[i] if ex is not None else None, num_classes, geo, matched[i], gt_boxes[i],
                             gt_labels[i], gt_info[i], gt_count[i], mutant)
        for k, t in enumerate(vals):
            assert t.dtype == F
            sums[i, k] = _chunk_sum(t)
    fgs = (matched >= 0).sum(1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return dict(matched=matched, fg=fgs, terms=sums.astype(F), losses=_losses(sums, fgs, p, mutant).astype(F))


def mutants():
    """{name: emulate with that one mistake}"""
    return {m: (lambda *a, _m=m, **kw: emulate(*a, mutant=_m, **kw)) for m in MUTANTS}


def check(got, ref, detail=None):
    """THE comparison (CPU and GPU tests): matched and fg equal the rule's; terms and losses are fp32, finite where the rule is,
    and |got - rule| <= bound on every element.  Returns the worst |err| / bound; detail receives it per output."""
    want, b = ref
    assert np.array_equal(np.asarray(got["matched"]), want["matched"]), \
        f"matched: outside the bound (an exact claim): {int((np.asarray(got['matched']) != want['matched']).sum())} points differ"
    assert np.array_equal(np.asarray(got["fg"]).astype(np.int64), want["fg"]), "fg: outside the bound (an exact claim)"
    worst = 0.0
    for key in ("terms", "losses"):
        out = np.asarray(got[key])
        assert out.shape == want[key].shape and out.dtype == F, (key, out.shape, out.dtype)
        assert np.isfinite(out).all(), f"{key}: not finite, outside the bound"
        err = np.abs(out.astype(D) - want[key])
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(err == 0, 0.0, err / b[key])
        ratio = float(q.max())
        if detail is not None:
            detail[key] = ratio
        assert ratio <= 1.0, f"{key}: |err| / bound = {ratio:.3f} at {np.unravel_index(q.argmax(), q.shape)}"
        worst = max(worst, ratio)
    return worst
