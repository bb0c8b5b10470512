"""The FCOS criterion's backward at the detector heads (csrc/fcos_loss.hip fcos_loss_grad_kernel) as a rule
in float64, its worst-case fp32 error bound, an fp32 emulation of the kernel's arithmetic in its order, and that emulation with one
deliberate mistake each.  numpy only; nothing here reads the library.

The differentiated scalar is L = sum_k w_k losses[k] over the six values of tests/fcos_loss_ref.py's rule (KEYS order),
upstream = w ([6]; None = ones, the sum trainval_net_fcos.py:56-57 back-propagates; without ext w[4:] is ignored).  The
gradients are at the tensors as ops.fcos_loss receives them: cls_lr [n, P, C + 2], reg_ctr [n, P, 5] (the four regressions are a
ReLU's OUTPUTS: the gradient is at those outputs, a zero output is not masked) and ext [n, P, 8] (through the normalisation of
(dx, dy)).  The matching is a constant (fcos_loss_ref's `matched`), and so is the batch-wide divisor div = max(1, sum fg).

Coefficients (float64 in the rule; the kernel forms each in double from the fp32 weights and rounds it to fp32 once):
    c0 = w0 / div   c1 = w1 / div   c2 = w2 / div   c3 = w3 0.02 / div   c4 = w4 0.01 / div   c5 = w5 20 / (n P 3 div)

Closed forms, per point:
  * focal columns (classes with c0, sides with c3, contacts with c4): z = -x on the hit column, x elsewhere, alpha_t = 0.25 on the
    hit column, 0.75 elsewhere, e = exp(-|z|), sp = max(z, 0) + log1p(e), sigma = 1 / (1 + e) or e / (1 + e), 1 - sigma the other
    of the two:  f = alpha_t sp sigma^2,  df/dz = alpha_t sigma^2 (sigma + 2 sp (1 - sigma)),  d/dx = -+ that (minus on the hit
    column).  Every factor is positive: no cancellation.
  * centre-ness, foreground only: c2 (sigma(z) - tgt), tgt of encode_single as in the forward.
  * GIoU, foreground only.  x1 = cx - r0 s, y1 = cy - r1 s, x2 = cx + r2 s, y2 = cy + r3 s; I = the intersection, Ap the
    predicted area, U = Ap + Ag - I + eps, Ac the enclosing area, Ace = Ac + eps, loss = 1 - I / U + (Ac - U + eps) / Ace.  For
    an edge v:   dloss/dv = kI dI/dv + kP dAp/dv + kC dAc/dv,   kI = (1 / Ace - 1 / U) - I / U^2,  kP = I / U^2 - 1 / Ace,
    kC = U / Ace^2.  The two quotients' derivatives cancel inside kI and kP.  d/dr = -+ s dloss/dv (minus on x1, y1), times c1.
      dI/dx1 = -hk [x1 > bx0] m,  dI/dx2 = hk [x2 < bx1] m,  dAp/dx1 = -(y2 - y1),  dAc/dx1 = -ch [x1 < bx0], ... where
      wk, hk are the intersection's sides, ch the enclosing box's height, m the reference's mask (wk > 0) & (hk > 0)
      (fcos_utils/utils.py:41-43): no gradient through I without STRICT overlap; [a > b] is 1, 1/2 on a tie, 0: torch.max /
      torch.min of two tensors split the gradient evenly on a tie.
  * dxdy, EVERY point: G_k = c5 (pred_k - tgt_k), pred = (mag, 0.1 dx / den, 0.1 dy / den), den = max(||(dx, dy)||, 1e-12);
    d/dmag = G_0 and, with u = (dx, dy) / den, d/d(dx, dy) = (0.1 / den) (G - u (u . G)); where the norm is below the clamp
    (dx = dy = 0 on a quarter of the seeded points) the norm passes no gradient and d/d(dx, dy) = (0.1 / 1e-12) G: 1e4..1e10,
    finite in fp32, a quirk of the reference that is kept.  The target is fcos_loss_ref.targets' (row 0 on the background,
    zeros in an image without boxes).

Results: {d_cls [n, P, C + 2], d_reg [n, P, 5], d_ext [n, P, 8] or None} in the anchor order (fcos_loss_ref.flatten).
"""
import functools

import numpy as np

import fcos_loss_grad_cases as gc
import fcos_loss_ref as fr

U, F, D, TINY = fr.U, fr.F, fr.D, fr.TINY
KEYS = ("d_cls", "d_reg", "d_ext")
MUTANTS = ("focal_no_sp_term", "hit_sign", "alpha_swapped", "no_x002", "dxdy_no_x10", "dxdy_fg_only", "divisor_no_max",
           "no_enclosing", "bce_no_target", "fmax_intersection", "one_sided_tie")
# the (case, upstream) on which each mutant must fail
MUTANT_CASE = {"focal_no_sp_term": ("edge", 0), "hit_sign": ("edge", 0), "alpha_swapped": ("1pt", 0), "no_x002": ("golden-2", 0),
               "dxdy_no_x10": ("edge", 1), "dxdy_fg_only": ("edge", 0), "divisor_no_max": ("nofg", 0), "no_enclosing": ("golden-2", 1),
               "bce_no_target": ("golden-2", 0), "fmax_intersection": ("g3", 0), "one_sided_tie": ("g3", 0)}
TIE_GUARD = 1e-3


def weights(upstream):
    return np.ones((6,), D) if upstream is None else np.asarray(upstream, D).reshape(6)


def coefficients(upstream, div, n, p, ext, mutant=None):
    """[6] float64"""
    w = weights(upstream)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.array([w[0] / div, w[1] / div, w[2] / div, w[3] * (1.0 if mutant == "no_x002" else fr.SCALE_LR) / div,
                      w[4] * fr.SCALE_CONTACT / div, w[5] * (2.0 if mutant == "dxdy_no_x10" else 2.0 * fr.SCALE_DXDY) / (D(n) * p * 3 * div)])
    if not ext:
        c[4:] = 0.0
    return c


def _setup(cls_lr, reg_ctr, ext, strides, gt_boxes, gt_count, radius, matched):
    cls, reg, ex, sizes = fr.flatten(cls_lr, reg_ctr, ext)
    geo = fr.geometry(sizes, strides)
    if matched is None:
        matched = np.stack([fr.match(gt_boxes[i], gt_count[i], geo, radius) for i in range(cls.shape[0])])
    return cls, reg, ex, geo, matched


# --------------------------------------------------------------------------------------------------------------------------
# the rule (float64 closed forms); magnitude: every product of a cancelling bracket replaced by its absolute value
# --------------------------------------------------------------------------------------------------------------------------
def _focal_grad(x, t, alpha=fr.ALPHA):
    hit = np.arange(x.shape[1])[None, :] == t[:, None]
    z = np.where(hit, -x, x)
    e = np.exp(-np.abs(z))
    sp = np.maximum(z, 0.0) + np.log1p(e)
    den = 1.0 + e
    sig, oms = np.where(z >= 0, 1.0 / den, e / den), np.where(z >= 0, e / den, 1.0 / den)
    d = np.where(hit, alpha, 1.0 - alpha) * sig * sig * (sig + 2.0 * sp * oms)
    return np.where(hit, -d, d)


def _sel(a, b):
    """[a > b]: 1, 1/2 on a tie, 0"""
    return np.where(a > b, 1.0, np.where(a == b, 0.5, 0.0))


def _giou_grad(r, box, cx, cy, s, magnitude=False):
    """d loss / d r [F, 4] (without c1) of the foreground points, float64"""
    x1, y1, x2, y2 = cx - r[:, 0] * s, cy - r[:, 1] * s, cx + r[:, 2] * s, cy + r[:, 3] * s
    bx0, by0, bx1, by1 = box.T
    wk, hk = np.minimum(x2, bx1) - np.maximum(x1, bx0), np.minimum(y2, by1) - np.maximum(y1, by0)
    m = (wk > 0) & (hk > 0)
    inter = np.where(m, wk * hk, 0.0)
    pw, ph = x2 - x1, y2 - y1
    uu = pw * ph + (bx1 - bx0) * (by1 - by0) - inter + fr.GIOU_EPS
    cw, ch = np.maximum(x2, bx1) - np.minimum(x1, bx0), np.maximum(y2, by1) - np.minimum(y1, by0)
    ace = cw * ch + fr.GIOU_EPS
    q = inter / uu ** 2
    if magnitude:
        k_i, k_p = 1.0 / ace + 1.0 / uu + q, q + 1.0 / ace
    else:
        k_i, k_p = (1.0 / ace - 1.0 / uu) - q, q - 1.0 / ace
    k_c = uu / ace ** 2
    ihm, iwm = np.where(m, hk, 0.0), np.where(m, wk, 0.0)
    cols = ((ihm * _sel(x1, bx0), ph, ch * _sel(bx0, x1)), (iwm * _sel(y1, by0), pw, cw * _sel(by0, y1)),
            (ihm * _sel(bx1, x2), ph, ch * _sel(x2, bx1)), (iwm * _sel(by1, y2), pw, cw * _sel(y2, by1)))
    return np.stack([(k_i * a + k_p * b + k_c * c) * s for a, b, c in cols], -1)


def _ctr_target(box, cx, cy, s):
    enc = np.stack([cx - box[:, 0], cy - box[:, 1], box[:, 2] - cx, box[:, 3] - cy], -1) / s[:, None]
    lr_, tb = enc[:, [0, 2]], enc[:, [1, 3]]
    return np.sqrt(np.abs((lr_.min(-1) / lr_.max(-1)) * (tb.min(-1) / tb.max(-1))))


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _dxdy_grad(e, tgt, c5, magnitude=False):
    """[P, 3] at (mag, dx, dy), float64"""
    nrm = np.sqrt(e[:, 1] ** 2 + e[:, 2] ** 2)
    den = np.maximum(nrm, fr.NORM_EPS)
    u = e[:, 1:3] / den[:, None]
    g = c5 * (np.stack([e[:, 0], 0.1 * u[:, 0], 0.1 * u[:, 1]], -1) - tgt)
    if magnitude:
        g = np.abs(c5) * (np.abs(np.stack([e[:, 0], 0.1 * u[:, 0], 0.1 * u[:, 1]], -1)) + np.abs(tgt))
    dot = np.where(nrm < fr.NORM_EPS, 0.0, (np.abs(g[:, 1:] * u) if magnitude else g[:, 1:] * u).sum(-1))
    v = g[:, 1:] + u * dot[:, None] if magnitude else g[:, 1:] - u * dot[:, None]
    return np.concatenate([g[:, :1], (0.1 / den)[:, None] * v], -1)


def rule(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius=1.5, upstream=None,
         magnitude=False, matched=None):
    """{d_cls, d_reg, d_ext} in float64 on the fp32 inputs: the module docstring's closed forms.  magnitude: the size of what each
    element adds up (|products|), which is what a float64 evaluation's own rounding scales with where a bracket cancels."""
    cls, reg, ex, geo, matched = _setup(cls_lr, reg_ctr, ext, strides, gt_boxes, gt_count, radius, matched)
    n, p, c = cls.shape[0], cls.shape[1], num_classes
    div = float(max(1, int((matched >= 0).sum())))
    co = coefficients(upstream, div, n, p, ex is not None)
    if magnitude:
        co = np.abs(co)
    cx, cy, size = (geo[k].astype(D) for k in ("cx", "cy", "size"))
    d_cls, d_reg = np.zeros(cls.shape, D), np.zeros(reg.shape, D)
    d_ext = np.zeros(ex.shape, D) if ex is not None else None
    for i in range(n):
        m = matched[i]
        fg = m >= 0
        cls_t, side_t, contact_t, dxdy_t = fr.targets(m, gt_labels[i], gt_info[i], gt_count[i])
        x = cls[i].astype(D)
        d_cls[i, :, :c] = co[0] * _focal_grad(x[:, :c], cls_t)
        d_cls[i, :, c:] = co[3] * _focal_grad(x[:, c:], side_t)
        r = reg[i, fg].astype(D)
        box = gt_boxes[i, m[fg]].astype(D)
        d_reg[i, fg, :4] = co[1] * _giou_grad(r, box, cx[fg], cy[fg], size[fg], magnitude)
        tgt = _ctr_target(box, cx[fg], cy[fg], size[fg])
        d_reg[i, fg, 4] = co[2] * (_sigmoid(r[:, 4]) + tgt if magnitude else _sigmoid(r[:, 4]) - tgt)
        if ex is not None:
            e = ex[i].astype(D)
            d_ext[i, :, 3:] = co[4] * _focal_grad(e[:, 3:], contact_t)
            d_ext[i, :, :3] = _dxdy_grad(e[:, :3], dxdy_t.astype(D), co[5], magnitude)
    if magnitude:
        d_cls = np.abs(d_cls)
        if d_ext is not None:
            d_ext[..., 3:] = np.abs(d_ext[..., 3:])
    return dict(d_cls=d_cls, d_reg=d_reg, d_ext=d_ext)


# --------------------------------------------------------------------------------------------------------------------------
# the kernel's chain, written once over fcos_loss_ref's two arithmetics: fp32 values (emulate), float64 with a running bound
# --------------------------------------------------------------------------------------------------------------------------
def _focal_grad_chain(o, x, t, coef, mutant=None):
    """[P] per column: the focal derivative times the term's coefficient, the sign flipped on the hit column"""
    alpha = 1.0 - fr.ALPHA if mutant == "alpha_swapped" else fr.ALPHA
    out = []
    for k in range(x.shape[1]):
        hit = t == k
        xk = o.inp(x[:, k])
        z = o.where(hit, o.neg(xk), xk)
        pos = x[:, k] * np.where(hit, -1, 1) >= 0
        e = o.exp(o.neg(o.abs(z)))
        one = o.const(1.0, e)
        sp = o.add(o.max(z, o.const(0.0, e)), o.log1p(e))
        den = o.add(one, e)
        lo, hi = o.div(e, den), o.div(one, den)
        sig, oms = o.where(pos, hi, lo), o.where(pos, lo, hi)
        t2 = o.mul(o.const(2.0, e), o.mul(sp, oms))
        inner = sig if mutant == "focal_no_sp_term" else o.add(sig, t2)
        a = o.where(hit, o.const(alpha, e), o.const(1.0 - alpha, e))
        d = o.mul(o.mul(o.mul(o.mul(sig, sig), inner), a), coef)
        out.append(d if mutant == "hit_sign" else o.where(hit, o.neg(d), d))
    return out


def _selv(o, a, b, one_sided=False):
    """[a > b] on the arithmetic's own values: 1, 1/2 on a tie, 0 (exact numbers)"""
    av, bv = o.val(a), o.val(b)
    s = np.where(av > bv, 1.0, np.where(av == bv, 1.0 if one_sided else 0.5, 0.0))
    return o.inp(s)


def _fg_grad_chain(o, reg, box, cx, cy, size, c1, c2, mutant=None):
    """the foreground points' five d_reg columns: the forward's decode / intersection / union / enclosing box, then the closed form"""
    r = [o.inp(reg[:, k]) for k in range(5)]
    b = [o.inp(box[:, k]) for k in range(4)]
    acx, acy, sz = o.inp(cx), o.inp(cy), o.inp(size)
    x1, y1 = o.sub(acx, o.mul(r[0], sz)), o.sub(acy, o.mul(r[1], sz))
    x2, y2 = o.add(acx, o.mul(r[2], sz)), o.add(acy, o.mul(r[3], sz))
    zero, one = o.const(0.0, acx), o.const(1.0, acx)
    wk, hk = o.sub(o.min(x2, b[2]), o.max(x1, b[0])), o.sub(o.min(y2, b[3]), o.max(y1, b[1]))
    inter = o.mul(o.max(wk, zero), o.max(hk, zero))
    pw, ph = o.sub(x2, x1), o.sub(y2, y1)
    union = o.sub(o.add(o.mul(pw, ph), o.mul(o.sub(b[2], b[0]), o.sub(b[3], b[1]))), inter)
    eps = o.const(fr.GIOU_EPS, acx)
    uu = o.add(union, eps)
    cw, ch = o.sub(o.max(x2, b[2]), o.min(x1, b[0])), o.sub(o.max(y2, b[3]), o.min(y1, b[1]))
    ace = o.add(o.mul(cw, ch), eps)
    ru, ra = o.div(one, uu), o.div(one, ace)
    q = o.div(o.div(inter, uu), uu)
    if mutant == "no_enclosing":
        k_i, k_p, k_c = o.sub(o.neg(ru), q), q, zero
    else:
        k_i, k_p, k_c = o.sub(o.sub(ra, ru), q), o.sub(q, ra), o.mul(o.mul(uu, ra), ra)
    wv, hv = o.val(wk), o.val(hk)
    m = (wv >= 0) & (hv >= 0) if mutant == "fmax_intersection" else (wv > 0) & (hv > 0)
    ihm, iwm = o.where(m, hk, zero), o.where(m, wk, zero)
    one_sided = mutant == "one_sided_tie"
    sel = lambda a_, b_: _selv(o, a_, b_, one_sided)                      # noqa: E731
    sc = o.mul(sz, c1)
    cols = ((ihm, sel(x1, b[0]), ph, ch, sel(b[0], x1)), (iwm, sel(y1, b[1]), pw, cw, sel(b[1], y1)),
            (ihm, sel(b[2], x2), ph, ch, sel(x2, b[2])), (iwm, sel(b[3], y2), pw, cw, sel(y2, b[3])))
    out = []
    for side, s_in, other, enc, s_out in cols:
        t1 = o.mul(k_i, o.mul(side, s_in))
        t2 = o.mul(k_p, other)
        t3 = o.mul(k_c, o.mul(enc, s_out))
        out.append(o.mul(o.add(o.add(t1, t2), t3), sc))
    l, t = o.div(o.sub(acx, b[0]), sz), o.div(o.sub(acy, b[1]), sz)
    rr, bb = o.div(o.sub(b[2], acx), sz), o.div(o.sub(b[3], acy), sz)
    tgt = o.sqrt(o.abs(o.mul(o.div(o.min(l, rr), o.max(l, rr)), o.div(o.min(t, bb), o.max(t, bb)))))
    z = r[4]
    e = o.exp(o.neg(o.abs(z)))
    den = o.add(one, e)
    sig = o.where(reg[:, 4] >= 0, o.div(one, den), o.div(e, den))
    out.append(o.mul(sig if mutant == "bce_no_target" else o.sub(sig, tgt), c2))
    return out


def _dxdy_grad_chain(o, e, tgt, c5):
    """[P] x 3: the gradient at (mag, dx, dy)"""
    mag, dx, dy = (o.inp(e[:, k]) for k in range(3))
    nrm = o.sqrt(o.add(o.mul(dx, dx), o.mul(dy, dy)))
    clamp = o.const(fr.NORM_EPS, mag)
    clamped = o.val(nrm) < o.val(clamp)
    den = o.max(nrm, clamp)
    tenth = o.const(0.1, mag)
    u = (o.div(dx, den), o.div(dy, den))
    pred = (mag, o.mul(tenth, u[0]), o.mul(tenth, u[1]))
    g = [o.mul(o.sub(pred[k], o.inp(tgt[:, k])), c5) for k in range(3)]
    dot = o.where(clamped, o.const(0.0, mag), o.add(o.mul(g[1], u[0]), o.mul(g[2], u[1])))
    rden = o.div(tenth, den)
    return [g[0], o.mul(o.sub(g[1], o.mul(u[0], dot)), rden), o.mul(o.sub(g[2], o.mul(u[1], dot)), rden)]


def _scatter(o, p, fg, part):
    full = o.inp(np.zeros((p,)))
    if isinstance(full, fr._V):
        full.v[fg], full.d[fg] = part.v, part.d
    else:
        full[fg] = part
    return full


def _point_grads(o, cls, reg, ex, c, geo, m, boxes, labels, info, count, co, mutant=None):
    """one image: lists of [P] columns (d_cls: C + 2, d_reg: 5, d_ext: 8 or None) in the arithmetic o"""
    p = cls.shape[0]
    fg = m >= 0
    cls_t, side_t, contact_t, dxdy_t = fr.targets(m, labels, info, count)
    like = o.inp(np.zeros((p,)))
    k = [o.const(v, like) for v in co]
    d_cls = _focal_grad_chain(o, cls[:, :c], cls_t, k[0], mutant) + _focal_grad_chain(o, cls[:, c:c + 2], side_t, k[3], mutant)
    d_reg = [o.inp(np.zeros((p,))) for _ in range(5)]
    if fg.any():
        sub = o.inp(np.zeros((int(fg.sum()),)))
        cols = _fg_grad_chain(o, reg[fg], boxes[m[fg]], geo["cx"][fg], geo["cy"][fg], geo["size"][fg], o.const(co[1], sub),
                              o.const(co[2], sub), mutant)
        d_reg = [_scatter(o, p, fg, col) for col in cols]
    d_ext = None
    if ex is not None:
        g3 = _dxdy_grad_chain(o, ex[:, :3], dxdy_t, k[5])
        if mutant == "dxdy_fg_only":
            g3 = [o.where(fg, g, like) for g in g3]
        d_ext = g3 + _focal_grad_chain(o, ex[:, 3:8], contact_t, k[4], mutant)
    return d_cls, d_reg, d_ext


def _run(o, cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius, upstream, mutant):
    cls, reg, ex, geo, matched = _setup(cls_lr, reg_ctr, ext, strides, gt_boxes, gt_count, radius, None)
    n, p = cls.shape[:2]
    total = int((matched >= 0).sum())
    div = float(total) if mutant == "divisor_no_max" else float(max(1, total))
    w = weights(upstream).astype(F).astype(D)                   # the kernel reads fp32 weights
    co = coefficients(w, div, n, p, ex is not None, mutant)
    return [_point_grads(o, cls[i], reg[i], ex[i] if ex is not None else None, num_classes, geo, matched[i], gt_boxes[i],
                         gt_labels[i], gt_info[i], gt_count[i], co, mutant) for i in range(n)]


def _stack(rows, pick):
    return {key: (None if rows[0][h] is None else np.stack([np.stack([pick(col) for col in img[h]], -1) for img in rows]))
            for h, key in enumerate(KEYS)}


def emulate(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius=1.5, upstream=None,
            mutant=None):
    """The kernel's arithmetic in numpy fp32, in its order (no fma: the file is built with contraction off); the coefficients are
    float64 expressions of the fp32 weights rounded to fp32 once, as the kernel forms them in double."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        rows = _run(fr._F32(), cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius, upstream,
                    mutant)
    out = _stack(rows, lambda col: col)
    assert all(v is None or v.dtype == F for v in out.values())
    return out


def bound(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius=1.5, upstream=None):
    """Worst-case error per gradient element of ANY fp32 evaluation that follows the kernel's chain: fcos_loss_ref._Err's running
    bound ("one rounding of v known to d" is d + u (|v| + d) + 2^-126; expf and log1pf 2 u; division and sqrtf correctly rounded;
    a subtraction's cancellation counted in absolute terms) through the chain _point_grads states, the coefficients as one fp32
    rounding of their float64 value, plus the distance of that chain's float64 value from the rule's closed form (the same function
    written differently).  The selectors (the mask, the ties, the clamp, the foreground) are exact claims: the cases keep every
    smooth point TIE_GUARD away from them and g3 meets them with exactly representable numbers (conditions())."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        rows = _run(fr._Err(), cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius, upstream, None)
    d, v = _stack(rows, lambda col: col.d), _stack(rows, lambda col: col.v)
    want = rule(cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count, radius, upstream)
    return {key: None if d[key] is None else d[key] + np.abs(v[key] - want[key]) + TINY for key in KEYS}


def mutants():
    """{name: emulate with that one mistake}"""
    return {m: (lambda *a, _m=m, **kw: emulate(*a, mutant=_m, **kw)) for m in MUTANTS}


def check(got, ref, detail=None):
    """THE comparison (CPU and GPU tests): every gradient is fp32, finite, and |got - rule| <= bound on every element.  Returns the
    worst |err| / bound; detail receives it per output."""
    want, b = ref
    worst = 0.0
    for key in KEYS:
        if want[key] is None:
            assert got.get(key) is None, key
            continue
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


# --------------------------------------------------------------------------------------------------------------------------
# the cases' conditions and shared references
# --------------------------------------------------------------------------------------------------------------------------
def ties(name):
    """per kind, the points of the case that meet a non-smooth point of the gradient exactly, and `near`: the smallest distance
    of the others from one (box edges, the intersection's sides; the clamp is met by dx = dy = 0 alone and has no near side)"""
    cls_lr, reg_ctr, ext, strides, c, gt_boxes, gt_labels, gt_info, gt_count = gc.args(name)
    cls, reg, ex, geo, matched = _setup(cls_lr, reg_ctr, ext, strides, gt_boxes, gt_count, 1.5, None)
    out = dict(edge=[], apart=[], zero_reg=[], clamp=[], dx0=[], near=np.inf)
    for i in range(cls.shape[0]):
        fg = np.nonzero(matched[i] >= 0)[0]
        r, box = reg[i, fg].astype(D), gt_boxes[i, matched[i, fg]].astype(D)
        cx, cy, s = (geo[k][fg].astype(D) for k in ("cx", "cy", "size"))
        edges = np.stack([cx - r[:, 0] * s, cy - r[:, 1] * s, cx + r[:, 2] * s, cy + r[:, 3] * s], -1) - box
        wk = np.minimum(edges[:, 2] + box[:, 2], box[:, 2]) - np.maximum(edges[:, 0] + box[:, 0], box[:, 0])
        hk = np.minimum(edges[:, 3] + box[:, 3], box[:, 3]) - np.maximum(edges[:, 1] + box[:, 1], box[:, 1])
        sides = np.stack([wk, hk], -1)
        for j, q in enumerate(fg):
            out["edge"] += [(i, int(q))] * int((edges[j] == 0).sum())
            if (sides[j] <= 0).any():
                out["apart"].append((i, int(q)))
            elif (r[j, :4] == 0).any():
                out["zero_reg"].append((i, int(q)))
        rest = np.concatenate([np.abs(edges[edges != 0]), np.abs(sides[sides > 0])])
        out["near"] = min(out["near"], float(rest.min())) if rest.size else out["near"]
        if ex is not None:
            dx, dy = ex[i, :, 1], ex[i, :, 2]
            out["clamp"] += [(i, int(q)) for q in np.nonzero((dx == 0) & (dy == 0))[0]]
            out["dx0"] += [(i, int(q)) for q in np.nonzero((dx == 0) != (dy == 0))[0]]
    return out


def conditions(name):
    """a smooth case keeps its box edges and intersection sides TIE_GUARD away from a tie; g3 meets each tie exactly once"""
    t = ties(name)
    if name == "g3":
        p = gc.G3_POINTS
        assert t["edge"] == [(0, p["TIE"])] and t["apart"] == [(0, p["APART"])] and t["zero_reg"] == [(0, p["ZERO"])], t
        assert t["clamp"] == [(0, p["CLAMP"])] and t["dx0"] == [(0, p["DX0"])], t
    else:
        assert not t["edge"] and not t["apart"] and not t["zero_reg"], (name, t)
    assert t["near"] > TIE_GUARD, (name, t["near"])
    return t


@functools.lru_cache(maxsize=None)
def reference(case):
    """(rule, bound) dicts of the (name, upstream index) case, computed once, read-only"""
    conditions(case[0])
    a, up = gc.args(case[0]), gc.upstream(case)
    out = rule(*a, upstream=up), bound(*a, upstream=up)
    for d in out:
        for t in d.values():
            if t is not None:
                t.setflags(write=False)
    return out
