"""The backward of the FCOS FPN -- three 3x3 output convolutions, the top-down nearest-neighbour read and three 1x1 laterals
(csrc/conv1x1_wgrad_f32.hip, csrc/upsample_bwd.hip, the reused kernels of tests/tower_bwd_ref.py) -- as a rule
in float64, the kernels' partition of the sums (plan functions) and the worst-case fp32 bound of that summation structure.  numpy
only; nothing here reads the library.

The forward, levels l = 3, 4, 5 (list index 0, 1, 2), c_l [N,h_l,w_l,Cin_l], all activations taken as their fp32 values:
    lat5 = c5 Winner5^T + b     lat_l = c_l Winner_l^T + b + up(lat_{l+1})     P_l = conv3x3(lat_l, Wlayer_l, pad 1) + b
    up(x)[n,o,p] = x[n, floor(o rh / OH), floor(p rw / OW)]      (the kernels' rule, per axis)
The rule, G_l = the gradient at P_l:
    dWlayer_l, dblayer_l = conv_rule of tests/tower_bwd_ref.py on (lat_l, G_l), one level
    D3 = dgrad3x3(G3, Wlayer3)      D4 = dgrad3x3(G4, Wlayer4) + upT(D3)      D5 = dgrad3x3(G5, Wlayer5) + upT(D4)
    upT(D)[n,s,t,c] = sum of D[n,o,p,c] over the o with floor(o rh / OH) = s and the p with floor(p rw / OW) = t
    dWinner_l[co,ci] = sum_q D_l[q,co] c_l[q,ci]      dbinner_l[co] = sum_q D_l[q,co]      dC_l[q,ci] = sum_co D_l[q,co] Winner_l[co,ci]
The S32 rounding of lat_l is passed straight through, as section 9u passes the towers'.

The kernels' structure (what the bounds are derived for), gamma(m) = m u / (1 - m u), u = 2^-24:
  lateral dW, db   The rows (pixels of all images, a flat index) are cut into chunks of 32; `chunks per range = ceil(chunks / cap)`,
         cap = clamp(512 / (ceil(Cout / 64) ceil(Cin / 128)), 1, 64).  A dW element is one fmaf chain over the rows of a range (the
         f32 MFMA is a k-ordered fmaf chain; a = hi + lo is exact; rows past the end add an exact zero), then the ranges' partial
         sums in order: m_W = (most rows of a range) + ranges - 1 roundings.  db is a chain of plain additions over the same
         partition: m_W bounds it too.  Any order of the `rows` products has at most `rows` roundings; every range but the largest
         holds at least one row, so m_W <= rows.
  upT    one chain of additions over the terms of an element in (row, column) order, started from the first term: m_U = terms - 1,
         which is also the any-order count.
  D_l    the f32 implicit GEMM, one fmaf chain over the 9 Cout terms, then the residual upT(D_{l-1}) added in the epilogue:
         m_D = 9 Cout + 1 (the any-order count of 9 Cout products and one more term).
  dC_l   the same kernel as a 1x1 convolution: one fmaf chain over Cout terms, m_C = Cout (the any-order count).
Underflow: a rounding whose result is subnormal errs by at most 2^-150, so every bound adds (roundings) 2^-149.
"""
import numpy as np

import tower_bwd_ref as tr

F, D = np.float32, np.float64
U = tr.U
gamma = tr.gamma
CHUNK, CO_TILE, CI_GROUP, WANT_GROUPS, MAX_RANGES = 32, 64, 128, 512, 64


def _f(absolute):
    return np.abs if absolute else (lambda t: t)


def _bound(m, mag):
    return gamma(m) * mag + m * 2.0 ** -149


# ---- the top-down read and its adjoint ----
def up_index(o_size, r_size):
    """the coarse index every fine index reads: floor(o r / O)"""
    return (np.arange(o_size, dtype=np.int64) * r_size) // o_size


def up_ranges(o_size, r_size):
    """the adjoint kernel's plan for one axis -> [(first, past the last)] per coarse index: ceil(s O / r) <= o < ceil((s + 1) O / r).
    Asserted: r <= O, no range is empty, and the ranges are exactly the sets of the floor rule."""
    assert 0 < r_size <= o_size
    out = [(-(-s * o_size // r_size), min(o_size, -(-(s + 1) * o_size // r_size))) for s in range(r_size)]
    idx = up_index(o_size, r_size)
    for s, (lo, hi) in enumerate(out):
        assert hi > lo and np.array_equal(np.nonzero(idx == s)[0], np.arange(lo, hi))
    return out


def up(x, size):
    """x [N,rh,rw,C] read at the fine size (OH, OW)"""
    return x[:, up_index(size[0], x.shape[1])][:, :, up_index(size[1], x.shape[2])]


def up_t(d, size, absolute=False):
    """upT: d [N,OH,OW,C] -> [N,rh,rw,C] in float64"""
    d = _f(absolute)(np.asarray(d, D))
    rows, cols = up_ranges(d.shape[1], size[0]), up_ranges(d.shape[2], size[1])
    out = np.zeros((d.shape[0], size[0], size[1], d.shape[3]), D)
    for s, (o0, o1) in enumerate(rows):
        for t, (p0, p1) in enumerate(cols):
            out[:, s, t] = d[:, o0:o1, p0:p1].sum((1, 2))
    return out


def up_t_stage(d, size):
    """(rule, bound) of the adjoint kernel on d: per element m_U = terms - 1"""
    rows, cols = up_ranges(d.shape[1], size[0]), up_ranges(d.shape[2], size[1])
    m = np.array([[(o1 - o0) * (p1 - p0) - 1 for p0, p1 in cols] for o0, o1 in rows], D)[None, :, :, None]
    assert m.min() >= 0
    return {"U": up_t(d, size)}, {"U": _bound(m, up_t(d, size, True))}


# ---- the laterals ----
def w1_plan(rows, cin, cout):
    """the 1x1 weight-gradient kernel's partition of the rows -> (ranges, most rows of a range, [rows per range])"""
    assert rows > 0 and cin % 32 == 0 and cout % 32 == 0 and 0 < cin <= 512 and 0 < cout <= 512
    chunks = -(-rows // CHUNK)
    groups = -(-cout // CO_TILE) * -(-cin // CI_GROUP)
    cap = 1 if groups >= WANT_GROUPS else min(MAX_RANGES, WANT_GROUPS // groups)
    cpr = -(-chunks // cap)
    ranges = -(-chunks // cpr)
    sizes = [min(rows, (r + 1) * cpr * CHUNK) - r * cpr * CHUNK for r in range(ranges)]
    assert sum(sizes) == rows and min(sizes) >= 1 and ranges <= MAX_RANGES
    assert max(sizes) + ranges - 1 <= rows          # never beyond the any-order bound
    return ranges, max(sizes), sizes


def w1_ws_bytes(rows, cin, cout):
    ranges = w1_plan(rows, cin, cout)[0]
    return 4 * (ranges * cout * cin + ranges * cout)


def _w1_sums(a, dy, absolute):
    f = _f(absolute)
    a2 = f(np.asarray(a, D)).reshape(-1, a.shape[-1])
    g2 = f(np.asarray(dy, D)).reshape(-1, dy.shape[-1])
    return {"dW": g2.T @ a2, "db": g2.sum(0)}


def w1_rule(a, dy):
    """a [N,h,w,Cin] (the fp32 value of the S32 activation), dy [N,h,w,Cout] -> {dW [Cout,Cin], db [Cout]} in float64"""
    return _w1_sums(a, dy, False)


def w1_stage(a, dy):
    """(rule, bound) of the 1x1 weight-gradient kernel: m_W = most + ranges - 1"""
    rows = int(np.prod(a.shape[:-1]))
    ranges, most, _ = w1_plan(rows, a.shape[-1], dy.shape[-1])
    m = most + ranges - 1
    assert m <= rows
    return w1_rule(a, dy), {k: _bound(m, s) for k, s in _w1_sums(a, dy, True).items()}


def dc_stage(d, w_inner):
    """dC = D Winner (w_inner [Cout,Cin]): (rule, bound), m_C = Cout"""
    m = w_inner.shape[0]
    want = np.asarray(d, D) @ np.asarray(w_inner, D)
    return {"dC": want}, {"dC": _bound(m, np.abs(np.asarray(d, D)) @ np.abs(np.asarray(w_inner, D)))}


# ---- the output convolutions ----
def dgrad3x3(g, w, absolute=False):
    """g [N,h,w,Cout], w [Cout,3,3,Cin] -> dA [N,h,w,Cin] = sum_{co,r,s} g[p - (r - 1, s - 1), co] w[co,r,s,ci], float64"""
    f = _f(absolute)
    n, h, wd, cout = g.shape
    gp = np.zeros((n, h + 2, wd + 2, cout), D)
    gp[:, 1:-1, 1:-1] = f(np.asarray(g, D))
    w64 = f(np.asarray(w, D))
    out = np.zeros((n, h, wd, w.shape[3]), D)
    for r in range(3):
        for s in range(3):
            out += gp[:, 2 - r:2 - r + h, 2 - s:2 - s + wd] @ w64[:, r, s]
    return out


def d_stage(g, w_layer, u=None):
    """D = dgrad3x3(G, Wlayer) (+ U, the residual the launch adds): (rule, bound), m_D = 9 Cout + 1"""
    m = 9 * w_layer.shape[0] + 1
    want, mag = dgrad3x3(g, w_layer), dgrad3x3(g, w_layer, True)
    if u is not None:
        want, mag = want + np.asarray(u, D), mag + np.abs(np.asarray(u, D))
    return {"D": want}, {"D": _bound(m, mag)}


def layer_stage(lat, g):
    """dWlayer, dblayer: the 3x3 weight-gradient kernel on one level (tests/tower_bwd_ref.py)"""
    want, b = tr.conv_rule([lat], [g]), tr.conv_bound([lat], [g])
    return {"dWlayer": want["dW"], "dblayer": want["db"]}, {"dWlayer": b["dW"], "dblayer": b["db"]}


# ---- the whole rule ----
def _fpn_sums(cs, lats, gs, w_inner, w_layer, absolute):
    """cs / lats / gs: per level [N,h,w,C]; w_inner[l] [256,Cin_l]; w_layer[l] [256,3,3,256] -> {dWlayer{l}, dblayer{l}, D{l},
    dWinner{l}, dbinner{l}, dC{l}}; absolute: every term replaced by its magnitude"""
    f = _f(absolute)
    out, prev = {}, None
    for l, (c, lat, g) in enumerate(zip(cs, lats, gs)):
        lay = tr._conv_sums([lat], [g], None, absolute)
        out[f"dWlayer{l}"], out[f"dblayer{l}"] = lay["dW"], lay["db"]
        d = dgrad3x3(g, w_layer[l], absolute)
        if prev is not None:
            d = d + up_t(prev, d.shape[1:3], absolute)
        out[f"D{l}"] = prev = d
        w1 = _w1_sums(c, d, absolute)
        out[f"dWinner{l}"], out[f"dbinner{l}"] = w1["dW"], w1["db"]
        out[f"dC{l}"] = d @ f(np.asarray(w_inner[l], D))
    return out


def fpn_rule(cs, lats, gs, w_inner, w_layer):
    return _fpn_sums(cs, lats, gs, w_inner, w_layer, False)


check = tr.check
