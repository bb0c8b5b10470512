"""The A2J aggregation (a2j/anchor.py:57-82 post_process; csrc/a2j_ops.hip a2j_aggregate_kernel) as a rule in float64, its
worst-case fp32 error bound, an fp32 emulation of the kernel's arithmetic in the kernel's order, and that emulation with one
deliberate mistake each.  numpy only; nothing here reads the library.

Layout (what ops.a2j_aggregate takes): cls, dep [K, fh, fw, 16*J], channel = a*J + j; reg [K, fh, fw, 16*J*2], channel =
(a*J + j)*2 + {0: along h, 1: along w}.  Output [K, J, 3] = (sum w (anchor_h + reg_0), sum w (anchor_w + reg_1), sum w dep) with
w the softmax of cls over all fh*fw*16 anchors of the joint and anchor (h, w, a) = (h*stride + 2 + 4*(a>>2), w*stride + 2 + 4*(a&3)).
"""
import numpy as np

A = 16                      # anchors per cell
U = 2.0 ** -24              # unit roundoff of fp32
F = np.float32
MUTANTS = ("swap_p", "swap_hw", "div_fh", "drop_last_cell", "max_per_anchor", "neighbour_channel")


def geometry(joints):
    """launch_aggregate's launch geometry, restated from the joint count alone: (workgroups per crop, joints per workgroup Jw,
    cell groups G, threads)."""
    split = 3 if joints >= 6 else 1
    jw = -(-joints // split)
    aw = A * jw
    g = max(1, min(9, 1024 // aw))
    return split, jw, g, -(-g * aw // 64) * 64


def _anchors(fh, fw, stride):
    """[fh*fw, 16, 2]: cell p = h*fw + w (the NHWC order), anchor a"""
    h, w, a = np.meshgrid(np.arange(fh), np.arange(fw), np.arange(A), indexing="ij")
    return np.stack([h * stride + 2 + 4 * (a >> 2), w * stride + 2 + 4 * (a & 3)], -1).reshape(fh * fw, A, 2).astype(np.float64)


def _terms(cls, reg, dep, joints, stride):
    """fp64 softmax weights w [K, cells, 16, J] and summed quantities t [K, cells, 16, J, 3]; the fp32 inputs widened"""
    k, fh, fw, aj = cls.shape
    assert aj == A * joints and reg.shape == (k, fh, fw, 2 * aj) and dep.shape == cls.shape
    assert cls.dtype == F and reg.dtype == F and dep.dtype == F
    x = cls.astype(np.float64).reshape(k, fh * fw, A, joints)
    x = x - x.max(axis=(1, 2), keepdims=True)
    e = np.exp(x)
    w = e / e.sum(axis=(1, 2), keepdims=True)
    t = np.empty((k, fh * fw, A, joints, 3))
    t[..., :2] = _anchors(fh, fw, stride)[None, :, :, None, :] + reg.astype(np.float64).reshape(k, fh * fw, A, joints, 2)
    t[..., 2] = dep.astype(np.float64).reshape(k, fh * fw, A, joints)
    return w, t, x


def rule(cls, reg, dep, joints, stride):
    w, t, _ = _terms(cls, reg, dep, joints, stride)
    return (w[..., None] * t).sum(axis=(1, 2))


def bound(cls, reg, dep, joints, stride):
    """Worst-case forward error, per output element, of ANY fp32 evaluation that adds in the kernel's chain.

    The kernel computes out = fl(T / S), S = sum e_i, T = sum fl(e_i * t_i), e_i = expf(fl(x_i - m)), m = max x (exact: fmaxf
    does not round), t_i = fl(anchor_i + reg_i) (the anchor itself is a small integer: exact) or dep_i.  With u = 2^-24, to first
    order and relative to  sum w_i |t_i|  (w the exact softmax weight):
      * each e_i carries  |x_i - m| u  from the rounded subtraction in front of expf (d/dx e^x = e^x) and 2 u from expf itself
        (1 ulp); in T the term also carries u for anchor + reg and u for the product.  That is (xmax + 4) u per term of T and no
        more per term of S, and a relative perturbation d of every term moves T / S by at most  d (sum w|t| + |out|) <= 2 d sum w|t|:
        2 (xmax + 4) u.  xmax = max |x_i - m| capped at 104: below -104 expf is 0 in fp32 and the weight is < 7e-46 (see the
        absolute term below).
      * a term of S or T passes through at most  chain = ceil(cells / G) + G + 16  additions: the thread's own cells, the G
        groups, the 16 anchors.  chain * u each for T and S: 2 chain u.
      * the division: u.  The remaining 3 u hold every second-order term: their sum is below (coefficient * u)^2 / u < 1 for
        any coefficient under 4000.
    bound = (2 chain + 2 (xmax + 4) + 4) u sum w_i |t_i|.
    Not in the formula: a term with x_i - m < -87 is a denormal or flushed e_i, an ABSOLUTE error of at most 2^-126 |t_i|
    against the largest term's e = 1.  check() asserts that  2^-126 sum |t_i|  is below a millionth of the bound instead of adding it."""
    w, t, x = _terms(cls, reg, dep, joints, stride)
    cells = w.shape[1]
    _, _, g, _ = geometry(joints)
    chain = -(-cells // g) + g + A
    xmax = min(float(np.abs(x).max()), 104.0)
    swt = (w[..., None] * np.abs(t)).sum(axis=(1, 2))
    b = (2 * chain + 2 * (xmax + 4) + 4) * U * swt
    assert (2.0 ** -126 * np.abs(t).sum(axis=(1, 2)) <= 1e-6 * b).all(), "denormal weights are not negligible in this case"
    return b


def emulate(cls, reg, dep, joints, stride, mutant=None):
    """The kernel's arithmetic in numpy fp32, in its order: thread (g, a, j) adds its cells p = g, g + G, ...; the groups are added
    in order, then the anchors.  (No fma: numpy rounds the product; the bound covers both.)"""
    assert mutant is None or mutant in MUTANTS
    k, fh, fw, aj = cls.shape
    cells = fh * fw
    split, jw, G, _ = geometry(joints)
    c = cls.reshape(k, cells, A, joints)
    r = reg.reshape(k, cells, A, joints, 2)
    d = dep.reshape(k, cells, A, joints)
    if mutant == "neighbour_channel" and joints > 1:      # the last joint of the last workgroup reads channel c - 1
        c, r, d = c.copy(), r.copy(), d.copy()
        c[..., -1], r[..., -1, :], d[..., -1] = c[..., -2], r[..., -2, :], d[..., -2]
    ncell = max(cells - 1, 1) if mutant == "drop_last_cell" else cells
    mj = c[:, :ncell].max(axis=1) if mutant == "max_per_anchor" else c[:, :ncell].max(axis=(1, 2))[:, None, :]   # [K, 16 or 1, J]
    a = np.arange(A)
    p0, p1 = (2 + 4 * (a >> 2)).astype(F), (2 + 4 * (a & 3)).astype(F)
    if mutant == "swap_p":
        p0, p1 = p1, p0
    acc = np.zeros((4, G, k, A, joints), F)
    for p in range(ncell):
        div = fh if mutant == "div_fh" else fw
        hh = p // div
        ww = p - hh * div
        if mutant == "swap_hw":
            hh, ww = ww, hh
        e = np.exp((c[:, p] - mj).astype(F)).astype(F)
        a0 = (F(hh * stride) + p0)[None, :, None]
        a1 = (F(ww * stride) + p1)[None, :, None]
        s = acc[:, p % G]
        s[0] += e
        s[1] += e * (a0 + r[:, p, :, :, 0])
        s[2] += e * (a1 + r[:, p, :, :, 1])
        s[3] += e * d[:, p]
    tot = acc[:, 0].copy()
    for g in range(1, G):
        tot += acc[:, g]
    fin = np.zeros((4, k, joints), F)
    for aa in range(A):
        fin += tot[:, :, aa]
    assert fin.dtype == F
    return np.stack([fin[1] / fin[0], fin[2] / fin[0], fin[3] / fin[0]], -1)


def mutants():
    """{name: emulate with that one mistake}"""
    return {m: (lambda *a, _m=m: emulate(*a, mutant=_m)) for m in MUTANTS}


def check(out, cls, reg, dep, joints, stride, ref=None):
    """THE comparison (CPU and GPU tests): NaN masks equal, |out - rule| <= bound on every element; returns max |err| / bound.
    ref = (rule, bound) computed before, if the caller keeps them."""
    want, b = ref if ref is not None else (rule(cls, reg, dep, joints, stride), bound(cls, reg, dep, joints, stride))
    out = np.asarray(out)
    assert out.shape == want.shape and out.dtype == F, (out.shape, out.dtype)
    assert np.array_equal(np.isnan(out), np.isnan(want)), "NaN masks differ"
    err = np.abs(out.astype(np.float64) - want)
    ratio = float(np.nanmax(err / b))
    assert ratio <= 1.0, f"|err| / bound = {ratio:.3f} at {np.unravel_index(np.nanargmax(err / b), err.shape)}"
    return ratio
