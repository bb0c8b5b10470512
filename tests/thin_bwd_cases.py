"""Cases for the output convolutions' backward (tests/thin_bwd_ref.py, tests/test_thin_bwd_cpu.py, tests/test_thin_bwd_gpu.py): the
smallest shapes at which the kernel of csrc/conv3x3_thin_bwd.hip can go wrong.  numpy only.

A case is (n, cin, sizes, members, options): sizes = the levels' (h, w), members = [(cout, relu_cols), ...] that read the map,
options: dx = (width, channel offset) of the tensor dA is written into, blocks = (first, total) for an S32 input that is a channel
slice of a wider map.  RANDOM: normal a, g and w from a fixed seed; y normal with a fifth of its values exactly 0 (so every case
meets the mask: y == 0 with g != 0 on a ReLU column, y < 0 on a column without).  PLANTED: small integers and powers of two, every
sum exact in fp32, so the kernel must give the rule's value bit for bit in any order (the idiom of tests/conv_exact_cases.py).

args(name) -> dict(n, cin, a [levels] fp32 = float(hi) + float(lo), hi, lo [levels] fp16, members = [(w, relu_cols, ys, gs), ...],
dx, blocks); computed once per case, read-only.
"""
import functools

import numpy as np

import thin_bwd_ref as tr

F = np.float32

RANDOM = {
    # Cin 32 (one block), one member 1 / 0, the 1 x 1 level alone
    "1x1": (1, 32, [(1, 1)], [(1, 0)], {}),
    # Cin 64, 5 / 4, a 2 x 3 level, two images
    "2x3": (2, 64, [(2, 3)], [(5, 4)], {}),
    # exactly one forward tile (eight tiles of the backward's 2 x 32), 8 / 3
    "16x16": (1, 32, [(16, 16)], [(8, 3)], {}),
    # 17 x 5 and 5 x 33 cross a tile row and a 32-pixel run; 16 / 0; three images
    "cross": (3, 32, [(17, 5), (5, 33)], [(16, 0)], {}),
    # the ReLU on every column, 16 / 16
    "relu-all": (1, 64, [(5, 33)], [(16, 16)], {}),
    # three levels, two members on the map (5 + 8 columns)
    "three": (2, 32, [(9, 12), (5, 6), (3, 3)], [(5, 4), (8, 3)], {}),
    # Cin 256, five levels, two members, dA into the cls half of a 512-wide tensor
    "five-256": (1, 256, [(20, 34), (10, 17), (5, 9), (3, 5), (2, 3)], [(5, 4), (8, 3)], {"dx": (512, 0)}),
    # ... and the separate second map (the reg tower's) at channel offset 256 of it
    "second-256": (1, 256, [(10, 17), (5, 9), (3, 5)], [(5, 4)], {"dx": (512, 256)}),
    # a channel-sliced S32 input: blocks 8-15 of a 16-block map
    "slice": (1, 256, [(3, 4)], [(4, 0)], {"blocks": (8, 16)}),
    # more than 512 tiles: two tiles per workgroup (the partition's other path)
    "units": (2, 32, [(72, 352)], [(4, 0)], {}),
}

# one-hot gradients on a 9 x 35 level (tile rows 0-1 | 2-3 | 4-5 | 6-7 | 8, tile columns 0-31 | 32-34): corners, edges, interior
_H, _W = 9, 35
HOT = {"tl": (0, 0), "tr": (0, _W - 1), "bl": (_H - 1, 0), "br": (_H - 1, _W - 1), "top": (0, 17), "bottom": (_H - 1, 17),
       "left": (4, 0), "right": (4, _W - 1), "in": (4, 17)}
PLANTED = {f"hot-{k}": (1, 32, [(_H, _W)], [(3, 0)], {"hot": [(0, 0, y, x, 1, 3.0)]}) for k, (y, x) in HOT.items()}
PLANTED.update({
    # a pair on the two sides of a tile (= workgroup) corner
    "pair-tile": (1, 32, [(_H, _W)], [(3, 0)], {"hot": [(0, 0, 7, 31, 0, 2.0), (0, 0, 8, 32, 0, -4.0)]}),
    # ... and of a level boundary: the last pixel of level 0, the first of level 1
    "pair-level": (1, 32, [(3, 4), (2, 2)], [(3, 0)], {"hot": [(0, 0, 2, 3, 2, 1.0), (1, 0, 0, 0, 2, 8.0)]}),
    # y exactly 0 on the ReLU columns (no gradient), y < 0 on the column without (passes); g non-zero everywhere
    "mask": (1, 32, [(2, 3)], [(5, 4)], {"mask": True}),
    # g all zero: every output element is still written (zeros)
    "gzero": (2, 32, [(9, 12), (3, 3)], [(5, 4), (8, 3)], {"gzero": True}),
})
CASES = dict(RANDOM, **PLANTED)
NAMES = list(CASES)


def _seed(name):
    return 7000 + NAMES.index(name)


def _freeze(t):
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def args(name):
    n, cin, sizes, members, opt = CASES[name]
    rng = np.random.default_rng(_seed(name))
    planted = name in PLANTED
    out = dict(n=n, cin=cin, sizes=sizes, dx=opt.get("dx"), blocks=opt.get("blocks"), planted=planted)
    a, hi, lo = [], [], []
    for h, w in sizes:
        raw = rng.integers(-8, 9, (n, h, w, cin)).astype(F) if planted else rng.standard_normal((n, h, w, cin)).astype(F)
        hh, ll = tr.split(raw)
        hi.append(_freeze(hh)); lo.append(_freeze(ll))
        a.append(_freeze(hh.astype(F) + ll.astype(F)))
    out.update(a=a, hi=hi, lo=lo)
    ms = []
    for m, (cout, relu) in enumerate(members):
        if planted:
            wt = (2.0 ** rng.integers(-3, 4, (cout, 3, 3, cin)) * rng.choice([-1.0, 1.0], (cout, 3, 3, cin))).astype(F)
        else:
            wt = (rng.standard_normal((cout, 3, 3, cin)) * 0.05).astype(F)
        ys, gs = [], []
        for l, (h, w) in enumerate(sizes):
            if planted:
                y = np.ones((n, h, w, cout), F)
                g = np.zeros((n, h, w, cout), F)
                if opt.get("mask"):
                    y[..., :relu], y[..., relu:] = 0.0, -1.0
                    g = rng.integers(1, 5, g.shape).astype(F)
                for (lv, img, py, px, col, val) in opt.get("hot", []):
                    if lv == l and m == 0:
                        g[img, py, px, col] = val
                if not (opt.get("mask") or opt.get("hot") or opt.get("gzero")):
                    raise AssertionError(name)
            else:
                y = rng.standard_normal((n, h, w, cout)).astype(F)
                y[rng.random(y.shape) < 0.2] = 0.0
                g = rng.standard_normal((n, h, w, cout)).astype(F)
            ys.append(_freeze(y)); gs.append(_freeze(g))
        ms.append((_freeze(wt), relu, ys, gs))
    out["members"] = ms
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rule, bound) of the case, computed once, read-only"""
    c = args(name)
    want, b = tr.rule(c["a"], c["members"]), tr.bound(c["a"], c["members"])
    for d in (want, b):
        for t in d.values():
            t.setflags(write=False)
    return want, b


def planted_expected(name):
    """What a planted case must give, written down without the rule: a one-hot g = v at pixel q, column c gives
    dW[c, r, s, :] = v a[q + (r - 1, s - 1)] (zero outside the map), db[c] = v, dA[q + (r - 1, s - 1)] = v w[c, r, s, :]; several
    one-hots add.  mask: only the column without the ReLU passes.  gzero: everything is zero.  float64."""
    c = args(name)
    opt = CASES[name][4]
    out = {}
    for m, (w, _relu, _ys, _gs) in enumerate(c["members"]):
        out[f"dW{m}"], out[f"db{m}"] = np.zeros(w.shape, np.float64), np.zeros((w.shape[0],), np.float64)
    for l, a in enumerate(c["a"]):
        out[f"dA{l}"] = np.zeros(a.shape, np.float64)
    hots = list(opt.get("hot", []))
    if opt.get("mask"):
        g = c["members"][0][3][0]
        hots = [(0, i, y, x, 4, float(g[i, y, x, 4])) for i in range(g.shape[0]) for y in range(g.shape[1]) for x in range(g.shape[2])]
    w0 = c["members"][0][0].astype(np.float64)
    for (lv, img, qy, qx, col, val) in hots:
        a = c["a"][lv].astype(np.float64)
        h, wd = a.shape[1:3]
        out["db0"][col] += val
        for r in range(3):
            for s in range(3):
                py, px = qy + r - 1, qx + s - 1
                if 0 <= py < h and 0 <= px < wd:
                    out["dW0"][col, r, s] += val * a[img, py, px]
                    out[f"dA{lv}"][img, py, px] += val * w0[col, r, s]
    return out
