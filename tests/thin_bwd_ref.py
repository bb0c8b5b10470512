"""The backward of the 3x3 / pad 1 head-output convolution (csrc/conv3x3_thin_bwd.hip, ops.conv3x3_thin_backward_levels; DESIGN.md
section 9t) as a rule in float64, and the worst-case fp32 bound of the kernel's summation structure.  numpy only; nothing here
reads the library.

The rule.  One map per level l, a_l [N,h,w,Cin] (the fp32 value float(hi) + float(lo) of the S32 activation), and one or two
members (w [Cout,3,3,Cin], relu_cols, y_l and g_l [N,h,w,Cout]).  gm = g where (column >= relu_cols or y > 0), else 0 -- torch's
ReLU backward on the stored result.  Then, zero outside the map,
    dW[co,r,s,ci] = sum_l sum_n sum_{y,x} gm_l[n,y,x,co] a_l[n,y+r-1,x+s-1,ci]
    db[co]        = sum gm
    dA_l[n,y,x,ci] = sum_members sum_{co,r,s} gm_l[n,y-r+1,x-s+1,co] w[co,r,s,ci]

The kernel's structure (what the bound is derived for).  Pixels are cut into 2 x 32 tiles in the fixed order (level, image, tile
row, tile column); `tiles_per_unit = ceil(tiles / 512)` consecutive tiles form a unit.  A dW element is one FMA chain over the
pixels of a unit in that order (one rounding per pixel: the product is not rounded, a = hi + lo is exact), then the units'
partial sums are added in order: a path of at most m_W = (most pixels of a unit) + units - 1 roundings, so |err| <= gamma(m_W)
sum|terms|, gamma(m) = m u / (1 - m u), u = 2^-24.  db is the same chain of additions (m_W again is an upper bound).  A dA element
is one FMA chain over its 9 x (all members' columns) terms: m_A = 9 * columns.  Underflow: a rounding whose result is subnormal
errs by at most 2^-150 instead, so every bound adds (number of roundings) * 2^-149.  None of this exceeds the any-order bound
gamma(K + 9) sum|terms| with K the number of summed pixels: a unit holds at least one pixel, so m_W <= K (plan() asserts it).
"""
import numpy as np

F, D = np.float32, np.float64
U = 2.0 ** -24
TILE_R, TILE_C, MAX_UNITS = 2, 32, 512


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


def masked(g, y, relu_cols):
    gm = np.array(g, D)
    if relu_cols:
        gm[..., :relu_cols] *= (np.asarray(y)[..., :relu_cols] > 0)
    return gm


def _sums(a_levels, members, absolute):
    """the three sums with every factor as given (absolute: |factor|, the size of what is added up)"""
    f = np.abs if absolute else (lambda t: t)
    cin = a_levels[0].shape[3]
    out = {}
    d_a = [np.zeros(a.shape, D) for a in a_levels]
    for m, (w, relu_cols, ys, gs) in enumerate(members):
        w = f(np.asarray(w, D))
        cout = w.shape[0]
        d_w, d_b = np.zeros((cout, 3, 3, cin), D), np.zeros((cout,), D)
        for l, a in enumerate(a_levels):
            n, h, wd, _ = a.shape
            gm = f(masked(gs[l], ys[l], relu_cols))
            ap = np.zeros((n, h + 2, wd + 2, cin), D)
            ap[:, 1:-1, 1:-1] = f(np.asarray(a, D))
            gp = np.zeros((n, h + 2, wd + 2, cout), D)
            gp[:, 1:-1, 1:-1] = gm
            d_b += gm.sum((0, 1, 2))
            for r in range(3):
                for s in range(3):
                    d_w[:, r, s] += np.einsum("nyxo,nyxi->oi", gm, ap[:, r:r + h, s:s + wd], optimize=True)
                    d_a[l] += gp[:, 2 - r:2 - r + h, 2 - s:2 - s + wd] @ w[:, r, s]
        out[f"dW{m}"], out[f"db{m}"] = d_w, d_b
    for l, t in enumerate(d_a):
        out[f"dA{l}"] = t
    return out


def rule(a_levels, members):
    """{dW0, db0, (dW1, db1,) dA0 .. dA(L-1)} in float64; members = [(w, relu_cols, ys, gs), ...]"""
    return _sums(a_levels, members, False)


def plan(sizes, n):
    """the kernel's partition of the pixels -> (units, most pixels of a unit, pixels in all)"""
    tiles = []
    for h, w in sizes:
        for _ in range(n):
            for ty in range(0, h, TILE_R):
                for tx in range(0, w, TILE_C):
                    tiles.append(min(TILE_R, h - ty) * min(TILE_C, w - tx))
    tpu = -(-len(tiles) // MAX_UNITS)
    units = [sum(tiles[i:i + tpu]) for i in range(0, len(tiles), tpu)]
    k = sum(tiles)
    assert k == n * sum(h * w for h, w in sizes) and len(units) <= MAX_UNITS
    assert max(units) + len(units) - 1 <= k < k + 9          # never beyond the any-order bound
    return len(units), max(units), k


def bound(a_levels, members):
    """worst-case |err| per element of the kernel's summation structure (module docstring)"""
    mag = _sums(a_levels, members, True)
    n = a_levels[0].shape[0]
    units, most, k = plan([a.shape[1:3] for a in a_levels], n)
    m_w = most + units - 1
    m_a = 9 * sum(np.asarray(w).shape[0] for w, _, _, _ in members)
    out = {}
    for key, s in mag.items():
        m = m_a if key.startswith("dA") else m_w
        assert m <= (k + 9 if not key.startswith("dA") else m_a)
        out[key] = gamma(m) * s + m * 2.0 ** -149
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
