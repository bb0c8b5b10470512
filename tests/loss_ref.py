"""The A2J criterion (a2j/anchor.py:99-153 A2J_loss.forward, a2j/a2j.py:231-238,318; csrc/a2j_ops.hip a2j_loss_aggregate_kernel
+ a2j_loss_reduce_kernel) as a rule in float64, its worst-case fp32 error bound, an fp32 emulation of the two kernels'
arithmetic in their order, and that emulation with one deliberate mistake each.  numpy only; nothing here reads the library.

Layout: the heads as tests/agg_ref.py states them; gt [K, J, 3] fp32 in crop (coord0, coord1, depth), the coordinates of the
aggregation's output row.  Results (what ops.a2j_loss returns behind the keypoints):
  terms  [K, J, 8] = (La_h, La_w, Lr_h, Lr_w, d, (gt - out)^2 x 3)
  sample [K, 2]    = (anchor_loss, regression_loss)
  batch  [5]       = (classification, the criterion's regression mean, regression * reg_loss_factor, total, rmse)

The reference's quirks, restated and not repaired:
  * the depth term is the plain |gt_d - Ed| (L1): the smooth-L1 with knee 3 of lines 145-149 is computed and never used;
  * spatialFactor multiplies the uv regression mean only, not the depth term and not the anchor loss;
  * both uv means run over the 2 J values of a sample, the depth mean over J;
  * thres and img_shape are unused;
  * a NaN difference fails `diff <= 1`, takes torch.where's second branch (diff - 0.5) and stays NaN;
  * A2JModel multiplies the criterion's regression mean by reg_loss_factor = 3 and adds the anchor mean for total_loss.
valid (the aggregation's flags): rows with 0 are left out of every batch value (divisor = rows with valid != 0; none: 0 / 0 = NaN,
like torch.mean of nothing) and have zero terms; rows with 2 have NaN terms and make the batch values NaN.
"""
import numpy as np

import agg_ref as ar

A, U, F = ar.A, ar.U, ar.F
NT = 8
MUTANTS = ("depth_smooth_l1", "knee3_uv", "sf_on_depth", "no_sf", "mean_over_j", "anchor_from_er", "no_reg_factor",
           "valid0_counted")
KEYS = ("terms", "sample", "batch")


def _sl1(a, knee=1.0):
    """where(a <= knee, 0.5 / knee * a^2, a - 0.5 * knee); NaN takes the second branch"""
    with np.errstate(invalid="ignore"):
        return np.where(a <= knee, 0.5 * (1.0 / knee) * a * a, a - 0.5 * knee)


def expectations(cls, reg, dep, joints, stride):
    """float64 (Ea [K,J,2] = sum w anchor, out [K,J,3] = the aggregation's rule)"""
    w, _, _ = ar._terms(cls, reg, dep, joints, stride)
    fh, fw = cls.shape[1:3]
    ea = (w[..., None] * ar._anchors(fh, fw, stride)[None, :, :, None, :]).sum(axis=(1, 2))
    return ea, ar.rule(cls, reg, dep, joints, stride)


def _rows(k, valid):
    v = np.ones((k,), np.int64) if valid is None else np.asarray(valid).astype(np.int64)
    assert v.shape == (k,) and set(v.tolist()) <= {0, 1, 2}
    return v


def rule(cls, reg, dep, gt, joints, stride, spatial_factor=0.5, reg_loss_factor=3.0, valid=None):
    """{terms, sample, batch} in float64 (the fp32 inputs widened), as a2j/anchor.py:99-153 and a2j/a2j.py:233-238,318 compute them"""
    assert gt.dtype == F and gt.shape == (cls.shape[0], joints, 3)
    k = cls.shape[0]
    v = _rows(k, valid)
    ea, out = expectations(cls, reg, dep, joints, stride)
    g = gt.astype(np.float64)
    terms = np.empty((k, joints, NT))
    terms[..., 0:2] = _sl1(np.abs(g[..., :2] - ea))
    terms[..., 2:4] = _sl1(np.abs(g[..., :2] - out[..., :2]))
    terms[..., 4] = np.abs(g[..., 2] - out[..., 2])
    terms[..., 5:8] = (g - out) ** 2
    terms[v == 0] = 0.0
    terms[v == 2] = np.nan
    sample = np.stack([terms[..., 0:2].mean(axis=(1, 2)),
                       terms[..., 2:4].mean(axis=(1, 2)) * spatial_factor + terms[..., 4].mean(axis=1)], -1)
    use = v != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.float64(use.sum())
        c, r = sample[use, 0].sum() / n, sample[use, 1].sum() / n
        rmse = np.sqrt(terms[use, :, 5:8].sum() / (n * joints * 3))
    return dict(terms=terms, sample=sample, batch=np.array([c, r, r * reg_loss_factor, c + r * reg_loss_factor, rmse]))


def _round(v, d):
    """one more fp32 rounding of a value v known to d: d + u (|v| + d)"""
    return d + U * (np.abs(v) + d)


def _sum(v, d, axis):
    """a sequential fp32 sum of n values v known to d each: every value passes through at most n additions"""
    n = int(np.prod([v.shape[a] for a in (axis if isinstance(axis, tuple) else (axis,))]))
    return v.sum(axis=axis), d.sum(axis=axis) + n * U * (np.abs(v) + d).sum(axis=axis)


def _sqrt_bound(m, dm):
    """|sqrt(m') - sqrt(m)| = |m' - m| / (sqrt(m') + sqrt(m)) <= min(dm / sqrt(m), sqrt(dm)), then sqrtf's own rounding"""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(m)
        return _round(r, np.minimum(np.where(m > 0, dm / r, np.inf), np.sqrt(dm)))


def _rmse_bound(q, dq, joints, use):
    """rmse = sqrt(sum q / (n * J * 3)) from the squared differences q [K, J, 3] known to dq: the sample's 3 J additions, the
    batch's n, the denominator's product (exact below 2^24, counted all the same), the division, the square root"""
    s, ds = _sum(q, dq, (1, 2))
    s, ds = _sum(s[use], ds[use], 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.float64(use.sum()) * joints * 3
        m = s / den
        dm = _round(m, ds / den + U * np.abs(m))
    return _sqrt_bound(m, dm)


def bound(cls, reg, dep, gt, joints, stride, spatial_factor=0.5, reg_loss_factor=3.0, valid=None):
    """Worst-case forward error per output of ANY fp32 evaluation that follows the kernels' chains; {terms, sample, batch}.

    With u = 2^-24, and "one rounding of v known to d" meaning d + u (|v| + d) (the rounding acts on the perturbed value):
      * the expectations Er (uv), Ed and Ea carry agg_ref.bound: B_r, B_d as it stands, and B_a = the same formula with
        t = anchor (agg_ref.bound on reg = 0: it then over-counts one u per term for an addition that is not there).
      * a difference diff = |g - E|: g is fp32 (exact), the subtraction rounds once: d_diff = B + u (|diff| + B).  fabsf is exact.
      * smooth-L1 has slope <= 1 on both sides of a continuous knee, so it moves by at most d_diff whichever side the computed
        value falls on; 0.5 * (a * a) and a - 0.5 each round once (0.5 * is exact): d_L = d_diff + u (L + d_diff).
        The depth term d is the difference itself: d_d = d_diff.
      * a squared difference: |a'^2 - a^2| <= d_diff (2 |a| + d_diff), and the product rounds once: + u (|a| + d_diff)^2.
      * a sequential sum of n values: each value passes through at most n additions: sum d_i + n u sum (|v_i| + d_i)
        (n = 2 J for the two uv sums, J for the depth sum, 3 J for the squared differences, the number of counted rows for the
        batch sums).
      * anchor_loss = sum / (2 J): the divisor is exact, the division rounds once.
      * regression_loss = sum / (2 J) * sf + sum_d / J: two divisions, fl32(sf) against the float64 sf (u relative), the product and
        the addition: one rounding each.
      * batch: sum over the counted rows / n (one rounding); * fl32(reg_loss_factor): two more; total: one more addition.
      * rmse = sqrtf(sum q / (n J 3)): _rmse_bound.
    Rows with valid == 0 are exact zeros, rows with NaN in the rule have a NaN bound (check() compares the NaN masks)."""
    k = cls.shape[0]
    v = _rows(k, valid)
    ref = rule(cls, reg, dep, gt, joints, stride, spatial_factor, reg_loss_factor, valid=None)
    ea, out = expectations(cls, reg, dep, joints, stride)
    g = gt.astype(np.float64)
    b_out = ar.bound(cls, reg, dep, joints, stride)
    b_a = ar.bound(cls, np.zeros_like(reg), dep, joints, stride)[..., :2]
    dt = np.empty((k, joints, NT))
    d_a = _round(g[..., :2] - ea, b_a)
    d_r = _round(g - out, b_out)
    dt[..., 0:2] = _round(ref["terms"][..., 0:2], d_a)
    dt[..., 2:4] = _round(ref["terms"][..., 2:4], d_r[..., :2])
    dt[..., 4] = d_r[..., 2]
    a = np.abs(g - out)
    dt[..., 5:8] = d_r * (2 * a + d_r) + U * (a + d_r) ** 2
    t = ref["terms"].copy()
    t[v == 0], dt[v == 0] = 0.0, 0.0
    t[v == 2], dt[v == 2] = np.nan, np.nan
    sa, dsa = _sum(t[..., 0:2], dt[..., 0:2], (1, 2))
    sr, dsr = _sum(t[..., 2:4], dt[..., 2:4], (1, 2))
    sd, dsd = _sum(t[..., 4], dt[..., 4], 1)
    anchor, d_anchor = sa / (2 * joints), _round(sa / (2 * joints), dsa / (2 * joints))
    mr, d_mr = sr / (2 * joints), _round(sr / (2 * joints), dsr / (2 * joints))
    md, d_md = sd / joints, _round(sd / joints, dsd / joints)
    p = mr * spatial_factor
    d_p = _round(p, d_mr * abs(spatial_factor) + U * np.abs(p))
    d_reg = _round(p + md, d_p + d_md)
    d_sample = np.stack([d_anchor, d_reg], -1)
    use = v != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.float64(use.sum())
        c, dc = _sum(anchor[use], d_anchor[use], 0)
        r, dr = _sum((p + md)[use], d_reg[use], 0)
        c, dc = c / n, _round(c / n, dc / n)
        r, dr = r / n, _round(r / n, dr / n)
        r3 = r * reg_loss_factor
        dr3 = _round(r3, dr * abs(reg_loss_factor) + U * np.abs(r3))
        d_total = _round(c + r3, dc + dr3)
        d_rmse = _rmse_bound(t[..., 5:8], dt[..., 5:8], joints, use)
    return dict(terms=dt, sample=d_sample, batch=np.array([dc, dr, dr3, d_total, d_rmse]))


def rmse_bound_given_out(gt, out):
    """(rmse, bound): sqrt(mean((gt - out)^2)) over all values in float64 from the fp32 keypoints the device RETURNED, and the
    reduction launch's worst-case distance from it: the expectations are exact here (B = 0), the rest as bound() counts it."""
    assert gt.dtype == F and out.dtype == F and gt.shape == out.shape
    diff = gt.astype(np.float64) - out.astype(np.float64)
    d = _round(diff, np.zeros_like(diff))
    a = np.abs(diff)
    dq = d * (2 * a + d) + U * (a + d) ** 2
    return float(np.sqrt((diff ** 2).mean())), float(_rmse_bound(diff ** 2, dq, gt.shape[1], np.ones((gt.shape[0],), bool)))


def _aggregate_f32(cls, reg, dep, joints, stride):
    """agg_ref.emulate with the loss form's two further running sums: fp32 (out [K,J,3], Ea [K,J,2]) in the kernel's order"""
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
    assert fin.dtype == F
    return np.stack([fin[1] / fin[0], fin[2] / fin[0], fin[3] / fin[0]], -1), np.stack([fin[4] / fin[0], fin[5] / fin[0]], -1)


def emulate(cls, reg, dep, gt, joints, stride, spatial_factor=0.5, reg_loss_factor=3.0, valid=None, mutant=None):
    """The two kernels' arithmetic in numpy fp32, in their order: the joint's terms from the divided sums, then per sample the
    joints in order, then the counted samples in order.  (No fma: numpy rounds every product; the bound covers both.)"""
    assert mutant is None or mutant in MUTANTS
    k = cls.shape[0]
    v = _rows(k, valid)
    out, ea = _aggregate_f32(cls, reg, dep, joints, stride)
    if mutant == "anchor_from_er":
        ea = out[..., :2]
    half = F(0.5)

    def sl1(x, knee3=False):
        with np.errstate(invalid="ignore"):
            if knee3:
                return np.where(x <= F(3.0), half * F(1.0 / 3.0) * (x * x), x - F(1.5)).astype(F)
            return np.where(x <= F(1.0), half * (x * x), x - half).astype(F)
    diff = gt - out
    terms = np.empty((k, joints, NT), F)
    terms[..., 0:2] = sl1(np.abs(gt[..., :2] - ea))
    terms[..., 2:4] = sl1(np.abs(diff[..., :2]), knee3=mutant == "knee3_uv")
    terms[..., 4] = sl1(np.abs(diff[..., 2]), knee3=True) if mutant == "depth_smooth_l1" else np.abs(diff[..., 2])
    terms[..., 5:8] = diff * diff
    terms[v == 0] = F(0.0)
    terms[v == 2] = F(np.nan)
    la, lr, ld, sq = (np.zeros((k,), F) for _ in range(4))
    for j in range(joints):
        la = la + terms[:, j, 0]
        la = la + terms[:, j, 1]
        lr = lr + terms[:, j, 2]
        lr = lr + terms[:, j, 3]
        ld = ld + terms[:, j, 4]
        for q in (5, 6, 7):
            sq = sq + terms[:, j, q]
    n_uv = F(joints if mutant == "mean_over_j" else 2 * joints)
    sf = F(1.0) if mutant == "no_sf" else F(spatial_factor)
    anchor = la / n_uv
    if mutant == "sf_on_depth":
        regression = (lr / n_uv + ld / F(joints)) * sf
    else:
        regression = lr / n_uv * sf + ld / F(joints)
    sample = np.stack([anchor, regression], -1)
    ba = br = bq = F(0.0)
    rows = 0
    for i in range(k):
        if v[i] != 0:
            ba, br, bq, rows = ba + anchor[i], br + regression[i], bq + sq[i], rows + 1
    if mutant == "valid0_counted":
        rows = k
    with np.errstate(invalid="ignore", divide="ignore"):
        c, r = ba / F(rows), br / F(rows)
        r3 = r if mutant == "no_reg_factor" else r * F(reg_loss_factor)
        batch = np.array([c, r, r3, c + r3, np.sqrt(bq / (F(rows) * F(joints * 3)))], F)
    assert terms.dtype == F and sample.dtype == F and batch.dtype == F
    return dict(terms=terms, sample=sample, batch=batch, uvd=out)


def mutants():
    """{name: emulate with that one mistake}"""
    return {m: (lambda *a, _m=m, **kw: emulate(*a, mutant=_m, **kw)) for m in MUTANTS}


def check(got, ref, detail=None):
    """THE comparison (CPU and GPU tests): for terms, sample and batch the NaN masks are equal and |got - rule| <= bound on every
    element; returns the worst |err| / bound.  got: {terms, sample, batch} fp32; ref = (rule, bound) dicts; detail: a dict that
    receives the worst ratio per output."""
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
