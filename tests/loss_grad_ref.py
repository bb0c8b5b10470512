"""The A2J criterion's backward at the three heads (csrc/a2j_ops.hip a2j_loss_grad_kernel) as a rule in
float64, its worst-case fp32 error bound, an fp32 emulation of the kernel's arithmetic in its order, that emulation with one
deliberate mistake each, and the cases: the heads and ground truths of tests/loss_cases.py as they are, times two upstream
settings.  numpy only; nothing here reads the library.

The differentiated scalar is  wa * classification + wr * (R * the criterion's regression mean)  of tests/loss_ref.py's rule
(batch [0] and [2]; (wa, wr) = (1, 1) gives total_loss), R = reg_loss_factor, sf = spatial_factor.  Per sample k and joint j, with
w_i the softmax of cls over all fh*fw*16 anchors i, Ea_c = sum w_i anchor_ic, Er_c = sum w_i (anchor_ic + reg_ic),
Ed = sum w_i dep_i, g = gt[k, j] and n = the number of rows with valid != 0:

    ga_c = wa / n / (2J)        * clip(Ea_c - g_c, -1, 1)
    gr_c = wr R sf / n / (2J)   * clip(Er_c - g_c, -1, 1)
    gd   = wr R / n / J         * sign(Ed - g_d)
    d_reg[i, c] = w_i gr_c
    d_dep[i]    = w_i gd
    d_cls[i]    = w_i (sum_c ga_c (anchor_ic - Ea_c) + sum_c gr_c (anchor_ic + reg_ic - Er_c) + gd (dep_i - Ed))

clip is the derivative of the reference's torch.where smooth-L1 (C1: the knee needs no guard); the depth term is the plain L1 the
reference uses, so its derivative is sign.  d E / d cls_i = w_i (x_i - E) for every expectation E = sum w x.
Rows with valid == 0 have zero gradients and are not counted in n; rows with valid == 2 have NaN gradients.
A NaN coordinate c of gt[k, j] (the reference's autograd, pinned by tests/golden/a2j_loss_grad.npz, not repaired): the unselected
branch of torch.where multiplies a zero gradient by the NaN difference, so ga_c and gr_c are NaN: d_reg[:, c] of that joint and the
joint's whole d_cls are NaN, its d_dep and the other coordinate's d_reg are not.  np.clip keeps the NaN, which restates exactly that.

Results: {d_cls [K,fh,fw,16J], d_reg [K,fh,fw,32J], d_dep [K,fh,fw,16J]}, the layouts of the heads (tests/agg_ref.py).
"""
import functools

import numpy as np

import agg_ref as ar
import loss_cases as lc
import loss_ref as lr

A, U, F = ar.A, ar.U, ar.F
KEYS = ("d_cls", "d_reg", "d_dep")
TINY = 2.0 ** -126          # the smallest normal fp32 number
UPSTREAMS = ((1.0, 1.0), (0.7, 1.9))
SIGN_GUARD = 10.0
MUTANTS = ("depth_smooth_l1", "no_clip", "w_times_t", "no_anchor_term", "sf_on_depth", "mean_over_j", "no_reg_factor",
           "valid0_counted", "swap_upstream")
# the (case, upstream) on which each mutant must fail
MUTANT_CASE = {"depth_smooth_l1": ("11x11x21", 0), "no_clip": ("11x11x21", 0), "w_times_t": ("3x5x7", 0),
               "no_anchor_term": ("3x5x7", 0), "sf_on_depth": ("11x11x21-big", 0), "mean_over_j": ("3x5x7", 0),
               "no_reg_factor": ("5x3x6-sf0.1", 0), "valid0_counted": ("3x5x7-valid", 0), "swap_upstream": ("3x5x7", 1)}


def _pack(k, fh, fw, d_cls, d_reg, d_dep):
    """[K, cells, 16, J(, 2)] -> the heads' layouts"""
    return dict(d_cls=d_cls.reshape(k, fh, fw, -1), d_reg=d_reg.reshape(k, fh, fw, -1), d_dep=d_dep.reshape(k, fh, fw, -1))


def _mask_rows(out, v, zero):
    for t in out.values():
        t[v == 0] = zero
        t[v == 2] = np.nan
    return out


def _coefficients(ea, out, g, joints, n, spatial_factor, reg_loss_factor, upstream):
    """float64 (ga [K,J,2], gr [K,J,2], gd [K,J]) and the three scale factors"""
    wa, wr = (np.float64(x) for x in upstream)
    with np.errstate(invalid="ignore", divide="ignore"):
        ca = wa / n / (2 * joints)
        cr = wr * reg_loss_factor * spatial_factor / n / (2 * joints)
        cd = wr * reg_loss_factor / n / joints
        ga = ca * np.clip(ea - g[..., :2], -1.0, 1.0)
        gr = cr * np.clip(out[..., :2] - g[..., :2], -1.0, 1.0)
        gd = cd * np.sign(out[..., 2] - g[..., 2])
    return ga, gr, gd, (ca, cr, cd)


def rule(cls, reg, dep, gt, joints, stride, spatial_factor=0.5, reg_loss_factor=3.0, valid=None, upstream=(1.0, 1.0), magnitude=False):
    """{d_cls, d_reg, d_dep} in float64 (the fp32 inputs widened): the module docstring's closed form.
    magnitude: the same with every product of d_cls's bracket replaced by its absolute value -- the size of what is added up,
    which is what a float64 evaluation's own rounding scales with where the bracket cancels."""
    assert gt.dtype == F and gt.shape == (cls.shape[0], joints, 3)
    k, fh, fw, _ = cls.shape
    v = lr._rows(k, valid)
    w, t, _ = ar._terms(cls, reg, dep, joints, stride)
    anc = ar._anchors(fh, fw, stride)[None, :, :, None, :]
    ea = (w[..., None] * anc).sum(axis=(1, 2))
    out = (w[..., None] * t).sum(axis=(1, 2))
    ga, gr, gd, _ = _coefficients(ea, out, gt.astype(np.float64), joints, np.float64((v != 0).sum()), spatial_factor,
                                  reg_loss_factor, upstream)
    e_, o_ = ea[:, None, None], out[:, None, None]
    m = np.abs if magnitude else (lambda x: x)
    br = (m(ga[:, None, None] * (anc - e_)).sum(-1) + m(gr[:, None, None] * (t[..., :2] - o_[..., :2])).sum(-1)
          + m(gd[:, None, None] * (t[..., 2] - o_[..., 2])))
    if magnitude:
        gr, gd = np.abs(gr), np.abs(gd)
    return _mask_rows(_pack(k, fh, fw, w * br, w[..., None] * gr[:, None, None], w * gd[:, None, None]), v, 0.0)


def _gamma(n):
    """n roundings of a product chain: (1 + u)^n - 1 <= n u / (1 - n u)"""
    return n * U / (1 - n * U)


def _prod(a, da, b, db):
    """fl(a' b') against a b, a' known to da and b' to db: |a| db + |b| da + da db, and the product's own rounding"""
    a, b = np.abs(a), np.abs(b)
    return a * db + b * da + da * db + U * (a + da) * (b + db)


def weight_error(cls, joints):
    """(rho, chain): the relative error of w = e / t is at most rho, to which every w adds the absolute 2^-126.
      * e_i = expf(fl(x_i - m)) carries |x_i - m| u from the rounded subtraction (d/dx e^x = e^x) and 2 u from expf (1 ulp):
        (xmax + 2) u, xmax = max |x_i - m| capped at 104 as in agg_ref.bound;
      * t = the sum of the e_i, all positive, through at most chain = ceil(cells / G) + G + 16 additions: the terms' own
        (xmax + 2) u and chain u;
      * one division: u; 3 u more hold every second-order term, as in agg_ref.bound.
    rho = (2 (xmax + 2) + chain + 4) u.  A term with x_i - m < -87 is a denormal or flushed e_i: an absolute 2^-126 against t >= 1."""
    k, fh, fw, _ = cls.shape
    x = cls.astype(np.float64).reshape(k, fh * fw, A, joints)
    x = x - x.max(axis=(1, 2), keepdims=True)
    _, _, g, _ = ar.geometry(joints)
    chain = -(-(fh * fw) // g) + g + A
    xmax = min(float(np.abs(x).max()), 104.0)
    return (2 * (xmax + 2) + chain + 4) * U, chain


def depth_margin(cls, reg, dep, gt, joints, stride):
    """min over the finite depth differences of |gt_d - Ed| / its own difference bound (inf where none is finite)"""
    out = ar.rule(cls, reg, dep, joints, stride)[..., 2]
    d = out - gt.astype(np.float64)[..., 2]
    b = lr._round(d, ar.bound(cls, reg, dep, joints, stride)[..., 2])
    ok = np.isfinite(d)
    return float((np.abs(d[ok]) / b[ok]).min()) if ok.any() else float("inf")


def bound(cls, reg, dep, gt, joints, stride, spatial_factor=0.5, reg_loss_factor=3.0, valid=None, upstream=(1.0, 1.0)):
    """Worst-case forward error per gradient element of ANY fp32 evaluation that follows the kernel's chains; {d_cls, d_reg, d_dep}.

    With u = 2^-24 and "one rounding of v known to d" meaning d + u (|v| + d) (loss_ref._round):
      * w = e / t: weight_error(): d_w = rho w + 2^-126.
      * the expectations Er (uv), Ed and Ea carry agg_ref.bound: B_r, B_d as it stands, B_a = the same on reg = 0 (loss_ref.bound).
      * the scale factors: wa, wr, R and sf are fp32 roundings of the float64 numbers the rule takes (u relative each), every
        product and division rounds once: ca = wa / n / 2J: 3 roundings; cr = wr R sf / n / 2J: 3 + 2 + 2 = 7; cd = wr R / n / J:
        2 + 1 + 2 = 5; n and 2J are exact.  k roundings: (1 + u)^k - 1 <= k u / (1 - k u).
      * a coefficient's difference E - g: g is fp32 (exact), the subtraction rounds once: d_diff = B + u (|diff| + B).  clip is
        1-Lipschitz, so it moves by at most d_diff; the coefficient's product: _prod.  sign is +-1 exactly where |Ed - g_d| exceeds
        its d_diff (asserted for every case with a factor of SIGN_GUARD, depth_margin()), so gd carries cd's error alone.
      * d_reg = w gr_c and d_dep = w gd: _prod.
      * the bracket of d_cls: five products coefficient * difference.  anchor_c is a small integer (exact); anchor_c - Ea_c and
        dep - Ed round once on an expectation known to B (the cancellation counted in absolute terms: d = B + u (|diff| + B));
        anchor_c + reg_c rounds first (u |anchor + reg|), then the subtraction of Er_c.  Each product: _prod.  The five are added
        in order, each through at most 4 additions: sum d_i + 4 u sum (|v_i| + d_i).  d_cls = w * bracket: _prod.
      * a result below the normal range may be flushed: 2^-126 more on every element.
    Rows with valid == 0 are exact zeros; where the rule has NaN the bound has NaN (check() compares the NaN masks)."""
    k, fh, fw, _ = cls.shape
    v = lr._rows(k, valid)
    w, t, _ = ar._terms(cls, reg, dep, joints, stride)
    anc = ar._anchors(fh, fw, stride)[None, :, :, None, :]
    ea = (w[..., None] * anc).sum(axis=(1, 2))
    out = (w[..., None] * t).sum(axis=(1, 2))
    g = gt.astype(np.float64)
    rho, _ = weight_error(cls, joints)
    d_w = rho * w + TINY
    b_out = ar.bound(cls, reg, dep, joints, stride)
    b_a = ar.bound(cls, np.zeros_like(reg), dep, joints, stride)[..., :2]
    ga, gr, gd, (ca, cr, cd) = _coefficients(ea, out, g, joints, np.float64((v != 0).sum()), spatial_factor, reg_loss_factor, upstream)
    with np.errstate(invalid="ignore"):
        d_ca, d_cr, d_cd = abs(ca) * _gamma(3), abs(cr) * _gamma(7), abs(cd) * _gamma(5)
        d_ga = _prod(ca, d_ca, np.clip(ea - g[..., :2], -1.0, 1.0), lr._round(ea - g[..., :2], b_a))
        d_gr = _prod(cr, d_cr, np.clip(out[..., :2] - g[..., :2], -1.0, 1.0), lr._round(out[..., :2] - g[..., :2], b_out[..., :2]))
        d_gd = d_cd + 0.0 * gd                                     # (NaN where gd is)
        bc = lambda x: x[:, None, None]                            # noqa: E731  [K,J,..] against [K,cells,16,J,..]
        d_reg = _prod(w[..., None], d_w[..., None], bc(gr), bc(d_gr)) + TINY
        d_dep = _prod(w, d_w, bc(gd), bc(d_gd)) + TINY
        diff_a = anc - bc(ea)
        x_r = t[..., :2]
        diff_r = x_r - bc(out[..., :2])
        diff_d = t[..., 2] - bc(out[..., 2])
        terms = [(bc(ga)[..., c], bc(d_ga)[..., c], diff_a[..., c], lr._round(diff_a[..., c], bc(b_a)[..., c])) for c in (0, 1)]
        terms += [(bc(gr)[..., c], bc(d_gr)[..., c], diff_r[..., c],
                   lr._round(diff_r[..., c], U * np.abs(x_r[..., c]) + bc(b_out)[..., c])) for c in (0, 1)]
        terms.append((bc(gd), bc(d_gd), diff_d, lr._round(diff_d, bc(b_out)[..., 2])))
        br = sum(a * b for a, _, b, _ in terms)
        d_terms = [_prod(a, da, b, db) for a, da, b, db in terms]
        d_br = sum(d_terms) + 4 * U * sum(np.abs(a * b) + d for (a, _, b, _), d in zip(terms, d_terms))
        d_cls = _prod(w, d_w, br, d_br) + TINY
    return _mask_rows(_pack(k, fh, fw, d_cls, d_reg, d_dep), v, 0.0)


def _sums_f32(cls, reg, dep, joints, stride):
    """loss_ref._aggregate_f32's running sums before the divisions: fp32 (mj [K,1,J], fin [6,K,J]) in the kernel's order"""
    k, fh, fw, _ = cls.shape
    cells = fh * fw
    _, _, G, _ = ar.geometry(joints)
    c = cls.reshape(k, cells, A, joints)
    r = reg.reshape(k, cells, A, joints, 2)
    d = dep.reshape(k, cells, A, joints)
    mj = c.max(axis=(1, 2))[:, None, :]
    a = np.arange(A)
    p0, p1 = (2 + 4 * (a >> 2)).astype(F), (2 + 4 * (a & 3)).astype(F)
    acc = np.zeros((6, G, k, A, joints), F)
    for p in range(cells):
        hh = p // fw
        ww = p - hh * fw
        e = np.exp((c[:, p] - mj).astype(F)).astype(F)
        a0 = (F(hh * stride) + p0)[None, :, None]
        a1 = (F(ww * stride) + p1)[None, :, None]
        s = acc[:, p % G]
        s[0] += e
        s[1] += e * (a0 + r[:, p, :, :, 0])
        s[2] += e * (a1 + r[:, p, :, :, 1])
        s[3] += e * d[:, p]
        s[4] += e * a0
        s[5] += e * a1
    tot = acc[:, 0].copy()
    for g in range(1, G):
        tot += acc[:, g]
    fin = np.zeros((6, k, joints), F)
    for aa in range(A):
        fin += tot[:, :, aa]
    assert fin.dtype == F and mj.dtype == F
    return mj, fin


def emulate(cls, reg, dep, gt, joints, stride, spatial_factor=0.5, reg_loss_factor=3.0, valid=None, upstream=(1.0, 1.0), mutant=None):
    """The kernel's arithmetic in numpy fp32, in its order: the loss form's maximum and six sums, the owning thread's
    coefficients, then per anchor e = expf(cls - mj), w = e / t, the bracket's five products added in order.  (No fma: numpy rounds
    every product; the kernel's third sweep is built without contraction, its first two as the loss form's.)  Also returns uvd."""
    assert mutant is None or mutant in MUTANTS
    k, fh, fw, _ = cls.shape
    cells = fh * fw
    v = lr._rows(k, valid)
    mj, fin = _sums_f32(cls, reg, dep, joints, stride)
    t = fin[0]
    er0, er1, ed, ea0, ea1 = (fin[q] / t for q in (1, 2, 3, 4, 5))
    wa, wr = (F(x) for x in (upstream[::-1] if mutant == "swap_upstream" else upstream))
    n = F(k if mutant == "valid0_counted" else (v != 0).sum())
    j2 = F(joints if mutant == "mean_over_j" else 2 * joints)
    wrr = wr if mutant == "no_reg_factor" else wr * F(reg_loss_factor)
    with np.errstate(invalid="ignore", divide="ignore"):
        ca = wa / n / j2
        cr = wrr * F(spatial_factor) / n / j2
        cd = (wrr * F(spatial_factor) if mutant == "sf_on_depth" else wrr) / n / F(joints)

        def clip(x):
            return x if mutant == "no_clip" else np.clip(x, F(-1.0), F(1.0))
        ga0, ga1 = ca * clip(ea0 - gt[..., 0]), ca * clip(ea1 - gt[..., 1])
        gr0, gr1 = cr * clip(er0 - gt[..., 0]), cr * clip(er1 - gt[..., 1])
        dd = ed - gt[..., 2]
        gd = cd * (np.clip(dd / F(3.0), F(-1.0), F(1.0)) if mutant == "depth_smooth_l1" else np.sign(dd))
        c = cls.reshape(k, cells, A, joints)
        r = reg.reshape(k, cells, A, joints, 2)
        d = dep.reshape(k, cells, A, joints)
        e = np.exp((c - mj[:, None]).astype(F)).astype(F)
        w = e / t[:, None, None]
        p, a = np.arange(cells), np.arange(A)
        hh = p // fw
        a0 = ((hh * stride).astype(F)[:, None] + (2 + 4 * (a >> 2)).astype(F)[None, :])[None, :, :, None]
        a1 = (((p - hh * fw) * stride).astype(F)[:, None] + (2 + 4 * (a & 3)).astype(F)[None, :])[None, :, :, None]
        bc = lambda x: x[:, None, None]                            # noqa: E731
        zero = F(0.0)
        drop = mutant == "w_times_t"
        b = bc(ga0) * (a0 - (zero if drop else bc(ea0)))
        b = b + bc(ga1) * (a1 - (zero if drop else bc(ea1)))
        if mutant == "no_anchor_term":
            b = np.zeros_like(b)
        b = b + bc(gr0) * ((a0 + r[..., 0]) - (zero if drop else bc(er0)))
        b = b + bc(gr1) * ((a1 + r[..., 1]) - (zero if drop else bc(er1)))
        b = b + bc(gd) * (d - (zero if drop else bc(ed)))
        out = _pack(k, fh, fw, w * b, np.stack([w * bc(gr0), w * bc(gr1)], -1), w * bc(gd))
    assert all(x.dtype == F for x in out.values())
    out = _mask_rows(out, v, F(0.0))
    out["uvd"] = np.stack([er0, er1, ed], -1)
    return out


def mutants():
    """{name: emulate with that one mistake}"""
    return {m: (lambda *a, _m=m, **kw: emulate(*a, mutant=_m, **kw)) for m in MUTANTS}


def check(got, ref, detail=None):
    """THE comparison (CPU and GPU tests): for d_cls, d_reg and d_dep the NaN masks are equal and |got - rule| <= bound on every
    element; returns the worst |err| / bound.  got: fp32 arrays; ref = (rule, bound) dicts; detail receives the ratio per output."""
    want, b = ref
    worst = 0.0
    for key in KEYS:
        out = np.asarray(got[key])
        assert out.shape == want[key].shape and out.dtype == F, (key, out.shape, out.dtype)
        assert np.array_equal(np.isnan(out), np.isnan(want[key])), f"{key}: NaN masks differ"
        err = np.abs(out.astype(np.float64) - want[key])
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(err == 0, 0.0, err / b[key])
        ratio = float(np.nanmax(q)) if not np.isnan(q).all() else 0.0
        if detail is not None:
            detail[key] = ratio
        assert ratio <= 1.0, f"{key}: |err| / bound = {ratio:.3f} at {np.unravel_index(np.nanargmax(q), q.shape)}"
        worst = max(worst, ratio)
    return worst


# ---- the cases: tests/loss_cases.py's fifteen, times UPSTREAMS ----

CASES = tuple((c.name, u) for c in lc.CASES for u in range(len(UPSTREAMS)))


def case_id(case):
    return f"{case[0]}-up{case[1]}"


def kwargs(case):
    """what rule / bound / emulate take behind the heads"""
    return dict(lc.kwargs(case[0]), upstream=UPSTREAMS[case[1]])


def conditions(name):
    """the depth differences keep clear of 0: every finite |gt_d - Ed| exceeds SIGN_GUARD times its own difference bound"""
    kw = lc.kwargs(name)
    margin = depth_margin(*lc.heads(name), kw["gt"], kw["joints"], kw["stride"])
    assert margin > SIGN_GUARD, (name, margin)
    return margin


@functools.lru_cache(maxsize=None)
def reference(case):
    """(rule, bound) dicts of the case, computed once"""
    conditions(case[0])
    kw = kwargs(case)
    out = rule(*lc.heads(case[0]), **kw), bound(*lc.heads(case[0]), **kw)
    for d in out:
        for t in d.values():
            t.setflags(write=False)
    return out
