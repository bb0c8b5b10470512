"""The backward of one FCOS tower layer -- 3x3 / pad 1 convolution -> GroupNorm -> ReLU (csrc/conv3x3_wgrad_f32.hip,
csrc/gn_relu_bwd.hip, ops.conv3x3_dgrad_levels) -- as a rule in float64, the kernels' partition of the
sums (plan functions) and the worst-case fp32 bound of that summation structure.  numpy only; nothing here reads the library.

The rule.  Per level l: a_l [N,h,w,Cin] (the fp32 value float(hi) + float(lo) of the S32 activation), y_l = conv(a_l, W) + b,
g_l = the gradient at relu(GroupNorm(y_l)), both [N,h,w,C]; the forward's fp32 tables scale, shift [N,C] and mean, rstd [N,G];
gamma [C].  With M = h w C / G, per (level, image, group):
    z  = y scale + shift (its sign; the forward's own expression)      gm = g where z > 0, else 0
    xh = (y - mean) rstd        t = gm gamma[c]        s1, s2 = sum_group t, sum_group t xh
    dy = rstd (t - s1 / M - xh s2 / M)       dgamma[c] = sum_{levels, images, pixels} gm xh       dbeta[c] = sum gm
    dW[co,r,s,ci] = sum_{levels, images, q} dy[q,co] a[q + (r - 1, s - 1), ci]       db[co] = sum dy       (zero outside the map)
    dA[p,ci]      = sum_{co,r,s} dy[p - (r - 1, s - 1), co] w[co,r,s,ci]
The tables are taken verbatim (cast up), so a bound covers the kernel's arithmetic only.  Statistics: mean = sum y / M,
rstd = 1 / sqrt(sum y^2 / M - mean^2 + eps), biased variance clamped at 0.

The kernels' structure (what the bounds are derived for), gamma(m) = m u / (1 - m u), u = 2^-24:
  wgrad  The pixels are cut into segments of at most 16 pixels of one row in the order (level, image, row, column);
         `segments per range = ceil(segments / cap)`, cap = clamp(512 / ((Cout / 32) ceil(Cin / 128)), 1, 64).  A dW element is
         one fmaf chain over the pixels of a range (the f32 MFMA is a k-ordered fmaf chain; a = hi + lo is exact; padding pixels
         add an exact zero), then the ranges' partial sums in order: m_W = (most pixels of a range) + ranges - 1 roundings.
         db is a chain of plain additions over the same partition: m_W bounds it too.
  dgrad  the f32 implicit GEMM: one fmaf chain over the 9 Cout terms of an element: m_A = 9 Cout.
  GroupNorm backward  Per 64-pixel chunk and channel, sum gm and sum gm xh are fp32 chains over at most min(hw, 64) terms (each
         thread a strided share, the shares added in thread order: never more additions than terms; absent pixels add exact
         zeros); everything above the chunks is fp64 and contributes less than one fp32 rounding; xh costs two roundings, the
         casts of s1 / M and s2 / M one each, the apply pass five.  Every path has at most m_G = min(hw, 64) + 12 roundings:
         |err| <= gamma(m_G) E with E the rule's expression with every term replaced by its magnitude.
  statistics  per chunk and group an fp32 chain over min(hw, 64) C / G terms (one rounding each for y^2 by fma), then fp64:
         m_S = min(hw, 64) C / G + 4.  |mean err| <= gamma(m_S) sum|y| / M; the variance errs by at most
         dv = gamma(m_S) (sum y^2 / M + 2 |mean| sum|y| / M), rstd by 0.5 rstd^3 dv (1 + 3 rstd^2 dv) + u rstd.
Underflow: a rounding whose result is subnormal errs by at most 2^-150, so every bound adds (roundings) 2^-149.
None of these exceeds the any-order bounds gamma(K + 9) (K the summed pixels), gamma(9 Cout) and gamma(M + 16): the plan
functions assert it, so a bound cannot be widened to hide an error.
"""
import numpy as np

F, D = np.float32, np.float64
U = 2.0 ** -24
SEG, CI_GROUP, WANT_GROUPS, MAX_RANGES, CHUNK = 16, 128, 512, 64, 64
EPS = 1e-5


def gamma(m):
    return m * U / (1.0 - m * U)


def split(a):
    """fp32 [.., C] -> (hi, lo) fp16, the S32 rule: hi = fp16(a), lo = fp16(a - hi)"""
    a = np.asarray(a, F)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(F)).astype(np.float16)
    return hi, lo


def pack_s32(hi, lo):
    """(hi, lo) fp16 [N,h,w,C] -> S32 fp16 [N,h,w,C/32,2,32]"""
    n, h, w, c = hi.shape
    return np.ascontiguousarray(np.stack([hi.reshape(n, h, w, c // 32, 32), lo.reshape(n, h, w, c // 32, 32)], axis=4))


# ---- convolution backward ----
def _conv_sums(a_levels, dys, w, absolute):
    f = np.abs if absolute else (lambda t: t)
    cin, cout = a_levels[0].shape[3], dys[0].shape[3]
    out = {"dW": np.zeros((cout, 3, 3, cin), D), "db": np.zeros((cout,), D)}
    wd = None if w is None else f(np.asarray(w, D))
    for l, (a, dy) in enumerate(zip(a_levels, dys)):
        n, h, wdt, _ = a.shape
        g = f(np.asarray(dy, D))
        ap = np.zeros((n, h + 2, wdt + 2, cin), D)
        ap[:, 1:-1, 1:-1] = f(np.asarray(a, D))
        gp = np.zeros((n, h + 2, wdt + 2, cout), D)
        gp[:, 1:-1, 1:-1] = g
        out["db"] += g.sum((0, 1, 2))
        d_a = np.zeros(a.shape, D)
        for r in range(3):
            for s in range(3):
                out["dW"][:, r, s] += np.einsum("nyxo,nyxi->oi", g, ap[:, r:r + h, s:s + wdt], optimize=True)
                if wd is not None:
                    d_a += gp[:, 2 - r:2 - r + h, 2 - s:2 - s + wdt] @ wd[:, r, s]
        if wd is not None:
            out[f"dA{l}"] = d_a
    return out


def conv_rule(a_levels, dys, w=None):
    """{dW, db, (dA0 .. with w)} in float64"""
    return _conv_sums(a_levels, dys, w, False)


def wgrad_plan(sizes, n, cin, cout):
    """the weight-gradient kernel's partition of the pixels -> (ranges, most pixels of a range, pixels in all)"""
    segs = []
    for h, w in sizes:
        for _ in range(n * h):
            for x0 in range(0, w, SEG):
                segs.append(min(SEG, w - x0))
    groups = (cout // 32) * -(-cin // CI_GROUP)
    cap = 1 if groups >= WANT_GROUPS else min(MAX_RANGES, WANT_GROUPS // groups)
    spr = -(-len(segs) // cap)
    ranges = [sum(segs[i:i + spr]) for i in range(0, len(segs), spr)]
    k = sum(segs)
    assert k == n * sum(h * w for h, w in sizes) and len(ranges) <= MAX_RANGES
    assert max(ranges) + len(ranges) - 1 <= k < k + 9          # never beyond the any-order bound
    return len(ranges), max(ranges), k


def conv_bound(a_levels, dys, w=None):
    """worst-case |err| per element of the kernels' summation structure (module docstring)"""
    mag = _conv_sums(a_levels, dys, w, True)
    cin, cout = a_levels[0].shape[3], dys[0].shape[3]
    ranges, most, k = wgrad_plan([a.shape[1:3] for a in a_levels], a_levels[0].shape[0], cin, cout)
    m_w, m_a = most + ranges - 1, 9 * cout
    assert m_w <= k + 9
    return {key: gamma(m_a if key.startswith("dA") else m_w) * s + (m_a if key.startswith("dA") else m_w) * 2.0 ** -149
            for key, s in mag.items()}


# ---- GroupNorm ----
def _grouped(t, groups):
    n, h, w, c = t.shape
    return t.reshape(n, h * w, groups, c // groups)


def gn_stats(ys, groups, eps=EPS):
    """[(mean [N,G], rstd [N,G])] per level in float64"""
    out = []
    for y in ys:
        t = _grouped(np.asarray(y, D), groups)
        m = t.shape[1] * t.shape[3]
        mean = t.sum((1, 3)) / m
        var = np.maximum((t * t).sum((1, 3)) / m - mean * mean, 0.0)
        out.append((mean, 1.0 / np.sqrt(var + eps)))
    return out


def gn_tables(stats, gamma_, beta):
    """the forward's fold: scale = gamma rstd, shift = beta - mean scale, [N,C] per level (in the dtype of stats)"""
    out = []
    for mean, rstd in stats:
        cpg = gamma_.shape[0] // mean.shape[1]
        scale = np.repeat(rstd, cpg, axis=1) * gamma_[None]
        out.append((scale, beta[None] - np.repeat(mean, cpg, axis=1) * scale))
    return out


def gn_plan(sizes, c, groups):
    """-> ([m_G per level], [m_S per level]): the rounding counts of the GroupNorm backward and of the statistics (module
    docstring), each from its own level's chunk length"""
    cpg = c // groups
    m_g = [min(h * w, CHUNK) + 12 for h, w in sizes]
    m_s = [min(h * w, CHUNK) * cpg + 4 for h, w in sizes]
    for (h, w), mg, ms in zip(sizes, m_g, m_s):
        assert mg <= h * w * cpg + 16 and ms <= h * w * cpg + 16          # never beyond the any-order bound gamma(M + 16)
    return m_g, m_s


def gn_stats_bound(ys, groups, eps=EPS):
    """[(|mean err|, |rstd err|) bounds [N,G]] per level"""
    out = []
    for y, (mean, rstd) in zip(ys, gn_stats(ys, groups, eps)):
        t = _grouped(np.asarray(y, D), groups)
        m = t.shape[1] * t.shape[3]
        m_s = gn_plan([y.shape[1:3]], y.shape[3], groups)[1][0]
        b1, b2 = np.abs(t).sum((1, 3)) / m, (t * t).sum((1, 3)) / m
        dv = gamma(m_s) * (b2 + 2 * np.abs(mean) * b1)
        out.append((gamma(m_s) * b1 + m_s * 2.0 ** -149, 0.5 * rstd ** 3 * dv * (1 + 3 * rstd ** 2 * dv) + U * rstd))
    return out


def z_of(ys, tables):
    """z = y scale + shift per level (float64: the product of two fp32 values is exact there, so the sign is exact)"""
    return [np.asarray(y, D) * np.asarray(sc, D)[:, None, None] + np.asarray(sh, D)[:, None, None] for y, (sc, sh) in zip(ys, tables)]


def _gn_sums(ys, gs, tables, stats, gamma_, groups, absolute):
    f = np.abs if absolute else (lambda t: t)
    c = gamma_.shape[0]
    cpg = c // groups
    gam = f(np.asarray(gamma_, D))
    out = {"dgamma": np.zeros((c,), D), "dbeta": np.zeros((c,), D)}
    for l, (y, g, z, (mean, rstd)) in enumerate(zip(ys, gs, z_of(ys, tables), stats)):
        n, h, w, _ = y.shape
        m = h * w * cpg
        gm = f(np.where(z > 0, np.asarray(g, D), 0.0))
        mean_c = np.repeat(np.asarray(mean, D), cpg, axis=1)[:, None, None]
        rstd_c = np.repeat(np.asarray(rstd, D), cpg, axis=1)[:, None, None]
        xh = f((np.asarray(y, D) - mean_c) * rstd_c)
        t = gm * gam
        s1 = np.repeat(_grouped(t, groups).sum((1, 3)), cpg, axis=1)[:, None, None]
        s2 = np.repeat(_grouped(t * xh, groups).sum((1, 3)), cpg, axis=1)[:, None, None]
        if absolute:
            out[f"dy{l}"] = np.abs(rstd_c) * (t + s1 / m + xh * s2 / m)
        else:
            out[f"dy{l}"] = rstd_c * (t - s1 / m - xh * s2 / m)
        out["dgamma"] += (gm * xh).sum((0, 1, 2))
        out["dbeta"] += gm.sum((0, 1, 2))
    return out


def gn_rule(ys, gs, tables, stats, gamma_, groups):
    """{dy0 .., dgamma, dbeta} in float64; tables = [(scale, shift)], stats = [(mean, rstd)] per level, taken verbatim"""
    return _gn_sums(ys, gs, tables, stats, gamma_, groups, False)


def gn_bound(ys, gs, tables, stats, gamma_, groups):
    """dy of a level: its own m_G; dgamma / dbeta, sums over the levels: the largest level's (it bounds every level's share)"""
    m_g, _ = gn_plan([y.shape[1:3] for y in ys], gamma_.shape[0], groups)
    out = {}
    for k, s in _gn_sums(ys, gs, tables, stats, gamma_, groups, True).items():
        m = m_g[int(k[2:])] if k.startswith("dy") else max(m_g)
        out[k] = gamma(m) * s + m * 2.0 ** -149
    return out


def check(got, reference, detail=None):
    """THE comparison: every output is fp32, finite, and |got - rule| <= bound on every element -> the worst |err| / bound"""
    want, b = reference
    assert set(got) == set(want), (sorted(got), sorted(want))
    worst = 0.0
    for key in sorted(want):
        out = np.asarray(got[key])
        assert out.shape == want[key].shape and out.dtype == F, (key, out.shape, out.dtype)
        assert np.isfinite(out).all(), f"{key}: not finite"
        err = np.abs(out.astype(D) - want[key])
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(err == 0, 0.0, err / b[key])
        ratio = float(q.max())
        if detail is not None:
            detail[key] = ratio
        assert ratio <= 1.0, f"{key}: |err| / bound = {ratio:.3f} at {np.unravel_index(q.argmax(), q.shape)}"
        worst = max(worst, ratio)
    return worst
