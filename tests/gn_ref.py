"""The GroupNorm statistics kernels (csrc/groupnorm.hip) as a rule in float64, their worst-case fp32 error bounds, an emulation
of the two passes in numpy (fp32 partials, fp64 combine), the rows32 partial slab, and the emulations with one deliberate mistake
each.  numpy only; nothing here reads the library.

The kernels turn x [N, HW, C] into per-(image, channel) tables with GroupNorm(x) = x*scale + shift:
    mean, var (biased) per (image, group);  rstd = 1/sqrt(var + eps);  scale = gamma*rstd;  shift = beta - mean*scale.
eps reaches the kernels as a float: the rule uses that fp32 value widened, like every other input.
"""
import numpy as np

U = 2.0 ** -24              # unit roundoff of fp32
U64 = 2.0 ** -53
F = np.float32
ROWS = 64                   # rows per chunk of gn_partial_kernel
MUTANTS = ("drop_last_row", "cnt_no_tail", "next_group", "image0", "straddle_swap")


def _x3(x):
    x = np.asarray(x)
    assert x.dtype == F and x.ndim in (3, 4)
    return x.reshape(x.shape[0], -1, x.shape[-1])


def _moments(x, groups):
    """fp64 mean, E[x^2], E|x| per (image, group)"""
    x = _x3(x).astype(np.float64)
    n, hw, c = x.shape
    xg = x.reshape(n, hw, groups, c // groups)
    return xg.mean(axis=(1, 3)), (xg * xg).mean(axis=(1, 3)), np.abs(xg).mean(axis=(1, 3))


def _tables(mean, var, gamma, beta, eps):
    cpg = gamma.size // mean.shape[1]
    rstd = 1.0 / np.sqrt(var + float(F(eps)))
    scale = gamma.astype(np.float64)[None, :] * np.repeat(rstd, cpg, axis=1)
    shift = beta.astype(np.float64)[None, :] - np.repeat(mean, cpg, axis=1) * scale
    return scale, shift


def rule(x, gamma, beta, groups, eps):
    """-> (scale [N,C], shift [N,C], mean [N,G], var [N,G]) in float64; the variance is the two-pass one (no cancellation)"""
    x3 = _x3(x).astype(np.float64)
    n, hw, c = x3.shape
    xg = x3.reshape(n, hw, groups, c // groups)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    return _tables(mean, var, gamma, beta, eps) + (mean, var)


def chain_affine(c, groups):
    """additions a value passes through in gn_partial_kernel: the thread's ceil(64 / rows_par) rows of 4 elements, then the
    group's rows_par * (cpg / 4) LDS slots"""
    rows_par = 256 // (c // 4)
    return -(-ROWS // rows_par) * 4 + rows_par * (c // groups // 4)


def _propagate(scale, shift, mean, var, gamma, eps, dvar, dmean):
    """(|d scale|, |d shift|) from |d var|, |d mean| per (image, group) and the tables' own fp32 roundings:
      rstd = fl32(1/sqrt(var + eps)):  |d rstd| / rstd <= 0.5 |d var| / (var + eps) + 2u   (first order in d var; u for the cast of
             the fp64 value, the second u holds the second-order terms)
      scale = fl(gamma * rstd):        |d scale| <= |scale| (|d rstd| / rstd + u)
      shift = fl(beta - fl(fl32(mean) * scale)):  |d shift| <= |scale| |d mean| + |mean| |d scale| + 2u |mean scale| + u |shift|
             (the cast of the mean, the product, the subtraction; an fma drops one of them)"""
    cpg = gamma.size // mean.shape[1]
    rep = lambda t: np.repeat(t, cpg, axis=1)
    drstd = 0.5 * dvar / (var + float(F(eps))) + 2 * U
    dscale = np.abs(scale) * (rep(drstd) + U)
    dshift = np.abs(scale) * rep(dmean) + rep(np.abs(mean)) * dscale + 2 * U * np.abs(rep(mean) * scale) + U * np.abs(shift)
    return dscale, dshift


def bound(x, gamma, beta, groups, eps, chain=None):
    """Worst-case error of (scale, shift) from groupnorm_affine, per element.

    gn_partial_kernel adds a chunk's values and squares in fp32; a value passes through  chain  additions (chain_affine), a
    square through one rounding more.  gn_finalize_kernel adds the chunk sums in fp64 (2^-53 per step: nothing at this scale),
    forms mean = s/cnt and var = ss/cnt - mean^2 in fp64.  With u = 2^-24, to first order:
        |d mean|   <= chain u E|x|                 asserted as (chain + 2) u E|x|
        |d E[x^2]| <= (chain + 1) u E[x^2]
        |d var|    <= |d E[x^2]| + 2 |mean| |d mean|,  asserted as  2 (chain + 2) u E[x^2]
    The asserted |d var| is the statement that BOTH terms of E[x^2] - mean^2 are good to (chain + 2) u E[x^2].  The strict
    worst case of the second term is 2 chain u |mean| E|x| <= 2 chain u E[x^2] (every rounding of the sum pushing one way), which
    would make the total (3 chain + 1) u E[x^2]; the form asserted here is the tighter one and therefore the stricter test.
    Relative to var it grows as E[x^2] / var = 1 + (mean/std)^2: that is the kernels' accuracy limit.
    chain: the additions of another producer of the fp32 partials (a conv epilogue's 32-row x 8-channel records: at most 256)."""
    scale, shift, mean, var = rule(x, gamma, beta, groups, eps)
    _, e2, e1 = _moments(x, groups)
    ch = chain_affine(_x3(x).shape[2], groups) if chain is None else chain
    return _propagate(scale, shift, mean, var, gamma, eps, 2 * (ch + 2) * U * e2, (ch + 2) * U * e1)


def _finalize(s, ss, cnt, gamma, beta, eps):
    """gn_finalize*'s tail from fp64 sums [N, G]: fp64 mean / var / rstd, the tables in fp32"""
    cpg = gamma.size // s.shape[1]
    mean = s / cnt
    var = np.maximum(ss / cnt - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + float(F(eps)))).astype(F)
    sc = gamma[None, :] * np.repeat(rstd, cpg, axis=1)
    sh = beta[None, :] - np.repeat(mean.astype(F), cpg, axis=1) * sc
    assert sc.dtype == F and sh.dtype == F
    return sc, sh


def emulate(x, gamma, beta, groups, eps, mutant=None):
    """groupnorm_affine in numpy: per 64-row chunk, thread (rl, col) adds its rows r0 + rl, + rows_par, ... (4 elements each) in
    fp32, the group adds its rows_par x cpg/4 slots in fp32, the chunks are added in fp64.  (Rows past the chunk's end are added
    as zeros: exact.  No fma: numpy rounds the square; the bound covers both.)"""
    assert mutant is None or mutant in MUTANTS
    x = _x3(x)
    n, hw, c = x.shape
    cols, cpg = c // 4, c // groups
    rows_par = 256 // cols
    rp = min(rows_par, ROWS)
    chunks = -(-hw // ROWS)
    xp = np.zeros((n, chunks * ROWS, c), F)
    xp[:, :hw] = x
    if mutant == "drop_last_row":
        xp[:, [min((k + 1) * ROWS, hw) - 1 for k in range(chunks)]] = 0
    xp = xp.reshape(n, chunks, ROWS // rp, rp, cols, 4)
    s = np.zeros((n, chunks, rp, cols), F)
    ss = np.zeros_like(s)
    for i in range(ROWS // rp):
        for e in range(4):
            v = xp[:, :, i, :, :, e]
            s += v
            ss += v * v
    s, ss = (t.reshape(n, chunks, rp, groups, cpg // 4) for t in (s, ss))
    ts = np.zeros((n, chunks, groups), F)
    tss = np.zeros_like(ts)
    for rr in range(rp):
        for q in range(cpg // 4):
            ts += s[:, :, rr, :, q]
            tss += ss[:, :, rr, :, q]
    assert ts.dtype == F
    S, SS = ts.astype(np.float64).sum(axis=1), tss.astype(np.float64).sum(axis=1)
    if mutant == "next_group":
        S, SS = np.roll(S, -1, axis=1), np.roll(SS, -1, axis=1)
    if mutant == "image0" and n > 1:
        S[1], SS[1] = S[0], SS[0]
    cnt = float(chunks * ROWS * cpg if mutant == "cnt_no_tail" else hw * cpg)
    return _finalize(S, SS, cnt, gamma, beta, eps)


def pack_rows32(x, n, hw, c):
    """The rows32 partial slab of x [n*hw, c] (the layout above gn_finalize_rows32_kernel): record (rg, unit) =
    {sum, sumsq} over the unit's 8 channels of the rows of 32-row group rg that belong to image (32 rg) / hw, then the same for
    the next image; float64 sums rounded to fp32.  A second half no row belongs to -- which the kernel must not read -- is NaN."""
    x = np.asarray(x, np.float64).reshape(n * hw, c // 8, 8)
    rgs = -(-n * hw // 32)
    slab = np.full((rgs, c // 8, 4), np.nan)
    img = np.arange(n * hw) // hw
    for rg in range(rgs):
        rows = np.arange(32 * rg, min(32 * rg + 32, n * hw))
        first = (32 * rg) // hw
        for half, im in ((0, first), (2, first + 1)):
            sel = rows[img[rows] == im]
            if len(sel):
                slab[rg, :, half] = x[sel].sum(axis=(0, 2))
                slab[rg, :, half + 1] = (x[sel] ** 2).sum(axis=(0, 2))
    assert not np.isnan(slab[:, :, :2]).any()
    return slab.astype(F).reshape(-1)


def _rows32_sums(slab, n, hw, c, groups, mutant=None):
    """fp64 {sum, sumsq} [N, G] from the slab, reading the halves the kernel reads"""
    units = c // 8
    upg = c // groups // 8
    rec = np.asarray(slab).astype(np.float64).reshape(-1, units, 4)
    s, ss = np.zeros((n, groups)), np.zeros((n, groups))
    for im in range(n):
        for rg in range((im * hw) >> 5, ((im * hw + hw - 1) >> 5) + 1):
            half = 0 if (32 * rg) // hw == im else 2
            if mutant == "straddle_swap":
                half = 2 - half
            r = rec[rg].reshape(groups, upg, 4)
            s[im] += r[:, :, half].sum(axis=1)
            ss[im] += r[:, :, half + 1].sum(axis=1)
    return s, ss


def emulate_rows32(slab, gamma, beta, n, hw, groups, eps, mutant=None):
    """groupnorm_finalize_rows32 in numpy"""
    assert mutant is None or mutant in MUTANTS
    s, ss = _rows32_sums(slab, n, hw, gamma.size, groups, mutant)
    return _finalize(s, ss, float(hw * (gamma.size // groups)), gamma, beta, eps)


def rule_rows32(slab, gamma, beta, n, hw, groups, eps):
    """-> (scale, shift, mean, var, E[x^2]) in float64 FROM THE SLAB: the partials are the kernel's given data"""
    s, ss = _rows32_sums(slab, n, hw, gamma.size, groups)
    cnt = float(hw * (gamma.size // groups))
    mean, e2 = s / cnt, ss / cnt
    var = np.maximum(e2 - mean * mean, 0.0)
    return _tables(mean, var, gamma, beta, eps) + (mean, var, e2)


def bound_rows32(slab, gamma, beta, n, hw, groups, eps):
    """groupnorm_finalize_rows32 against rule_rows32: the partials are data, so what remains is
      * the fp64 combination: items = (row groups of the image) * (units per group) additions for each sum, the division and
        the subtraction: |d var| <= (items + 4) 2^-53 E[x^2], |d mean| <= (items + 2) 2^-53 E|x| (asserted with sqrt(E[x^2]) >= E|x|);
      * the fp32 roundings of _propagate: the cast of rstd, gamma * rstd, the cast of the mean, mean * scale, beta - that."""
    scale, shift, mean, var, e2 = rule_rows32(slab, gamma, beta, n, hw, groups, eps)
    items = (hw // 32 + 2) * (gamma.size // groups // 8)
    return _propagate(scale, shift, mean, var, gamma, eps, (items + 4) * U64 * e2, (items + 2) * U64 * np.sqrt(e2))


def mutants():
    """{name: (emulation with that one mistake, "affine" or "rows32")}"""
    out = {m: ((lambda *a, _m=m: emulate(*a, mutant=_m)), "affine") for m in MUTANTS[:4]}
    out["straddle_swap"] = ((lambda *a: emulate_rows32(*a, mutant="straddle_swap")), "rows32")
    return out


def _compare(scale, shift, want, b):
    worst = 0.0
    for name, got, w, bb in (("scale", scale, want[0], b[0]), ("shift", shift, want[1], b[1])):
        got = np.asarray(got)
        assert got.shape == w.shape and got.dtype == F, (name, got.shape, got.dtype)
        assert np.array_equal(np.isfinite(got), np.isfinite(w)), f"{name}: non-finite masks differ"
        ratio = float((np.abs(got.astype(np.float64) - w) / bb).max())
        assert ratio <= 1.0, f"{name}: |err| / bound = {ratio:.3f}"
        worst = max(worst, ratio)
    return worst


def check(scale, shift, x, gamma, beta, groups, eps, chain=None, ref=None):
    """THE comparison for groupnorm_affine (CPU and GPU tests): non-finite masks equal, |err| <= bound on every element of scale
    and shift; returns the largest |err| / bound.  ref = (rule(...), bound(...)) if the caller keeps them."""
    want, b = ref if ref is not None else (rule(x, gamma, beta, groups, eps), bound(x, gamma, beta, groups, eps, chain))
    return _compare(scale, shift, want, b)


def check_rows32(scale, shift, slab, gamma, beta, n, hw, groups, eps):
    """the same for groupnorm_finalize_rows32, against the slab's own float64 statistics"""
    return _compare(scale, shift, rule_rows32(slab, gamma, beta, n, hw, groups, eps),
                    bound_rows32(slab, gamma, beta, n, hw, groups, eps))
