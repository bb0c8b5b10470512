"""Cases for the tower layers' backward (tests/tower_bwd_ref.py, tests/test_tower_bwd_cpu.py, tests/test_tower_bwd_gpu.py): the
smallest shapes at which the kernels of csrc/conv3x3_wgrad_f32.hip and csrc/gn_relu_bwd.hip can go wrong.  numpy only.

Convolution cases: (n, cin, cout, sizes, options); options: blocks = (first, total) S32 blocks of a wider map that `a` is a slice
of, cols = (first, total) columns of a wider tensor that dy is a slice of.  RANDOM: normal a, dy and w from a fixed seed.
PLANTED: small integers and powers of two, every sum exact in fp32, so the kernel must give the rule's value bit for bit in any
order.  conv_args(name) -> dict(n, cin, cout, sizes, a, hi, lo, dy [levels], w, blocks, cols), computed once, read-only.

GroupNorm cases: (n, c, groups, sizes, options); options: cols = (first, total), masked = the channels of group 0 get beta = -10
(z < 0 everywhere: the group passes no gradient), gamma0 = a channel with gamma = 0 (and beta > 0: its gradient passes),
gzero / gint = planted gradients.  y is normal; where |z| came out below 5e-3 it is moved away, so that the fp32 and the float64
masks agree on every element (asserted at 1e-3 by the CPU test).  gn_args(name) -> dict(n, c, groups, sizes, y, g [levels],
gamma, beta, stats [(mean, rstd)] fp32, tables [(scale, shift)] fp32, cols).
"""
import functools

import numpy as np

import tower_bwd_ref as tr

F, D = np.float32, np.float64

_H, _W = 9, 35   # the planted map: segments 0-15 | 16-31 | 32-34 of every row, one K range each at Cin = Cout = 32
_Q = (4, 17)
CONV_RANDOM = {
    "1x1": (1, 32, 32, [(1, 1)], {}),                                   # one pixel: the eight off-centre taps are exactly 0
    "2x3": (2, 64, 32, [(2, 3)], {}),
    "cross": (3, 32, 64, [(17, 5), (5, 33)], {}),                       # two levels, a row longer than two segments
    "full": (1, 256, 256, [(16, 16)], {}),                              # two ci groups, eight co tiles
    "wide": (1, 256, 512, [(8, 8)], {}),                                # tower0's bank: the plan's cap is 16 ranges
    "slice": (1, 256, 256, [(3, 4)], {"blocks": (8, 16), "cols": (256, 512)}),
    "ranges": (2, 32, 32, [(20, 35)], {}),                              # 120 segments on 64 ranges: two segments per range
}
CONV_PLANTED = {f"hot-{r}{s}": (1, 32, 32, [(_H, _W)], {"hot": [(0, 0, _Q[0], _Q[1], 5, 2.0)], "a_hot": (r, s)})
                for r in range(3) for s in range(3)}
CONV_PLANTED.update({
    # a pair on the two sides of a segment (= K range) boundary
    "pair-range": (1, 32, 32, [(_H, _W)], {"hot": [(0, 0, 4, 15, 3, 2.0), (0, 0, 4, 16, 3, -4.0)]}),
    # ... and of a level boundary: the last pixel of level 0, the first of level 1
    "pair-level": (1, 32, 32, [(3, 4), (2, 2)], {"hot": [(0, 0, 2, 3, 2, 1.0), (1, 0, 0, 0, 2, 8.0)]}),
    "dy-zero": (2, 32, 64, [(9, 12), (3, 3)], {"hot": []}),
})
CONV_CASES = dict(CONV_RANDOM, **CONV_PLANTED)
CONV_NAMES = list(CONV_CASES)

GN_CASES = {
    "1x1": (1, 32, 4, [(1, 1)], {}),
    "2x3": (2, 64, 8, [(2, 3)], {}),
    "cross": (3, 64, 8, [(17, 5), (5, 33)], {}),                        # two and three 64-pixel chunks, the last ones short
    "512": (1, 512, 64, [(6, 8)], {}),
    "slice": (1, 256, 32, [(3, 4)], {"cols": (256, 512)}),
    "masked": (2, 32, 4, [(5, 7)], {"masked": True}),
    "gamma0": (1, 32, 4, [(5, 7), (2, 2)], {"gamma0": 9}),
    "gzero": (2, 64, 8, [(9, 12), (3, 3)], {"gzero": True}),
    "gint": (2, 32, 4, [(9, 12), (3, 3)], {"gint": True}),
}
GN_NAMES = list(GN_CASES)
GN_PLANTED = ("gzero", "gint")


def _freeze(t):
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def conv_args(name):
    n, cin, cout, sizes, opt = CONV_CASES[name]
    rng = np.random.default_rng(9000 + CONV_NAMES.index(name))
    planted = name in CONV_PLANTED
    out = dict(n=n, cin=cin, cout=cout, sizes=sizes, blocks=opt.get("blocks"), cols=opt.get("cols"), planted=planted)
    a, hi, lo, dys = [], [], [], []
    for l, (h, w) in enumerate(sizes):
        if planted:
            raw = rng.integers(-8, 9, (n, h, w, cin)).astype(F)
            if "a_hot" in opt:        # a one-hot activation under tap (r, s) of the one-hot gradient: ONE element of dW
                r, s = opt["a_hot"]
                raw[:] = 0.0
                raw[0, _Q[0] + r - 1, _Q[1] + s - 1, 7] = 3.0
            dy = np.zeros((n, h, w, cout), F)
            for (lv, img, py, px, col, val) in opt["hot"]:
                if lv == l:
                    dy[img, py, px, col] = val
        else:
            raw = rng.standard_normal((n, h, w, cin)).astype(F)
            dy = rng.standard_normal((n, h, w, cout)).astype(F)
        hh, ll = tr.split(raw)
        hi.append(_freeze(hh)); lo.append(_freeze(ll))
        a.append(_freeze(hh.astype(F) + ll.astype(F)))
        dys.append(_freeze(dy))
    if planted:
        wt = (2.0 ** rng.integers(-3, 4, (cout, 3, 3, cin)) * rng.choice([-1.0, 1.0], (cout, 3, 3, cin))).astype(F)
    else:
        wt = (rng.standard_normal((cout, 3, 3, cin)) * 0.05).astype(F)
    out.update(a=a, hi=hi, lo=lo, dy=dys, w=_freeze(wt))
    return out


@functools.lru_cache(maxsize=None)
def conv_reference(name):
    """(rule, bound) of the case with dW, db and dA, computed once, read-only"""
    c = conv_args(name)
    want, b = tr.conv_rule(c["a"], c["dy"], c["w"]), tr.conv_bound(c["a"], c["dy"], c["w"])
    for d in (want, b):
        for t in d.values():
            t.setflags(write=False)
    return want, b


def conv_planted_expected(name):
    """What a planted case must give, written down without the rule: a one-hot dy = v at pixel q, column c gives
    dW[c, r, s, :] = v a[q + (r - 1, s - 1)] (zero outside the map), db[c] = v, dA[q + (r - 1, s - 1)] = v w[c, r, s, :]; several
    one-hots add.  float64."""
    c = conv_args(name)
    opt = CONV_CASES[name][4]
    out = {"dW": np.zeros(c["w"].shape, D), "db": np.zeros((c["cout"],), D)}
    for l, a in enumerate(c["a"]):
        out[f"dA{l}"] = np.zeros(a.shape, D)
    w0 = c["w"].astype(D)
    for (lv, img, qy, qx, col, val) in opt["hot"]:
        a = c["a"][lv].astype(D)
        h, wd = a.shape[1:3]
        out["db"][col] += val
        for r in range(3):
            for s in range(3):
                py, px = qy + r - 1, qx + s - 1
                if 0 <= py < h and 0 <= px < wd:
                    out["dW"][col, r, s] += val * a[img, py, px]
                    out[f"dA{lv}"][img, py, px] += val * w0[col, r, s]
    return out


@functools.lru_cache(maxsize=None)
def gn_args(name, f64_stats=False):
    """f64_stats: the statistics and tables in float64 (what torch's float64 GroupNorm computes) instead of the fp32 tables the
    kernels read; y, g, gamma and beta are the same either way"""
    n, c, groups, sizes, opt = GN_CASES[name]
    rng = np.random.default_rng(9500 + GN_NAMES.index(name))
    cpg = c // groups
    gam = (1.0 + 0.25 * rng.standard_normal(c)).astype(F)
    beta = (0.3 * rng.standard_normal(c)).astype(F)
    if opt.get("masked"):
        beta[:cpg] = -10.0
    if "gamma0" in opt:
        gam[opt["gamma0"]], beta[opt["gamma0"]] = 0.0, 0.5
    ys, gs = [], []
    for h, w in sizes:
        y = (0.7 * rng.standard_normal((n, h, w, c)) + 0.2).astype(F)
        for _ in range(4):     # move y away from the ReLU's kink (a handful of elements: the statistics barely move)
            z = tr.z_of([y], tr.gn_tables(tr.gn_stats([y], groups), gam.astype(D), beta.astype(D)))[0]
            sc = tr.gn_tables(tr.gn_stats([y], groups), gam.astype(D), beta.astype(D))[0][0][:, None, None]
            bad = (np.abs(z) < 5e-3) & (np.abs(sc) > 1e-6)
            if not bad.any():
                break
            y = np.where(bad, y + (np.sign(z) + (z == 0)) * 2e-2 / np.abs(np.where(bad, sc, 1.0)), y).astype(F)
        if opt.get("gzero"):
            g = np.zeros((n, h, w, c), F)
        elif opt.get("gint"):
            g = rng.integers(-4, 5, (n, h, w, c)).astype(F)
        else:
            g = rng.standard_normal((n, h, w, c)).astype(F)
        ys.append(_freeze(y)); gs.append(_freeze(g))
    stats64 = tr.gn_stats(ys, groups)
    if f64_stats:
        stats = stats64
        tables = tr.gn_tables(stats64, gam.astype(D), beta.astype(D))
    else:   # the fp32 tables the kernels read: the fold done in fp32 on the rounded statistics, like the forward's finalize
        stats = [(m.astype(F), r.astype(F)) for m, r in stats64]
        tables = tr.gn_tables(stats, gam, beta)
        assert all(t.dtype == F for pair in tables for t in pair)
    for pair in list(stats) + list(tables):
        for t in pair:
            t.setflags(write=False)
    return dict(n=n, c=c, groups=groups, sizes=sizes, y=ys, g=gs, gamma=_freeze(gam), beta=_freeze(beta), stats=stats,
                tables=tables, cols=opt.get("cols"), masked=bool(opt.get("masked")), gamma0=opt.get("gamma0"))


@functools.lru_cache(maxsize=None)
def gn_reference(name):
    """(rule, bound) of the case on its fp32 tables, computed once, read-only"""
    c = gn_args(name)
    parts = (c["y"], c["g"], c["tables"], c["stats"], c["gamma"], c["groups"])
    want, b = tr.gn_rule(*parts), tr.gn_bound(*parts)
    for d in (want, b):
        for t in d.values():
            t.setflags(write=False)
    return want, b
