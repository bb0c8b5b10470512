"""Cases for the FPN's backward (tests/fpn_bwd_ref.py, tests/test_fpn_bwd_cpu.py, tests/test_fpn_bwd_gpu.py): the smallest shapes
at which the kernels of csrc/conv1x1_wgrad_f32.hip and csrc/upsample_bwd.hip can go wrong.  numpy only.

1x1 weight-gradient cases: (n, cin, cout, (h, w), options); options: blocks = (first, total) S32 blocks of a wider map that `a` is a
slice of, cols = (first, total) columns of a wider tensor that dy is a slice of.  RANDOM: normal a, dy and w from a fixed seed.
PLANTED: small integers and powers of two on a 2 x 5 x 8 map at Cin = Cout = 32 (80 rows: ranges of 32, 32 and 16 rows; image 1
starts at row 40), every sum exact in fp32, so the kernel must give the rule's value bit for bit in any order.
w1_args(name) -> dict(n, cin, cout, size, a, hi, lo, dy, w [Cout,Cin], blocks, cols, planted), computed once, read-only.

Adjoint cases: (n, c, (OH, OW), (rh, rw), options); options: cols = (first, total) for the gradient AND the output, ints = planted.
"""
import functools

import numpy as np

import fpn_bwd_ref as fr
import tower_bwd_ref as tr

F, D = np.float32, np.float64

_PH, _PW = 5, 8          # the planted map: rows 0-31 | 32-63 | 64-79 are the three K ranges, image 1 starts at row 40
W1_RANDOM = {
    "1px": (1, 32, 32, (1, 1), {}),
    "odd": (2, 64, 32, (3, 5), {}),
    "c128": (1, 128, 256, (4, 5), {}),                                  # the P3 lateral's bank
    "c512": (1, 512, 256, (3, 3), {}),                                  # P5's: four ci groups
    "slice": (1, 256, 256, (3, 4), {"blocks": (8, 16), "cols": (256, 512)}),
    "ranges": (2, 32, 32, (33, 35), {}),                                # 2310 rows, 73 chunks, two per range: 37 ranges, 6 rows last
}
W1_PLANTED = {
    "hot": (2, 32, 32, (_PH, _PW), {"hot": [(0, 2, 3, 5, 2.0)], "a_hot": (0, 2, 3, 7, 3.0)}),   # ONE element of dW
    "pair-range": (2, 32, 32, (_PH, _PW), {"hot": [(0, 3, 7, 3, 2.0), (0, 4, 0, 3, -4.0)]}),     # rows 31 and 32
    "pair-image": (2, 32, 32, (_PH, _PW), {"hot": [(0, 4, 7, 2, 1.0), (1, 0, 0, 2, 8.0)]}),      # rows 39 and 40
    "dy-zero": (2, 64, 64, (_PH, _PW), {"hot": []}),
}
W1_CASES = dict(W1_RANDOM, **W1_PLANTED)
W1_NAMES = list(W1_CASES)

UP_CASES = {
    "2x": (2, 256, (4, 6), (2, 3), {}),                                 # exact 2x, three blocks of threads
    "5x7": (1, 12, (5, 7), (3, 4), {}),                                 # source counts 2, 2, 1 and 2, 2, 2, 1
    "same": (2, 4, (3, 3), (3, 3), {}),                                 # the identity
    "all": (1, 8, (2, 2), (1, 1), {}),
    "slice": (1, 8, (4, 6), (2, 3), {"cols": (4, 16)}),
    "ints": (2, 8, (5, 7), (3, 4), {"ints": True}),
}
UP_NAMES = list(UP_CASES)

# the whole rule against autograd: (n, (Cin3, Cin4, Cin5), Cout, sizes)
FPN_CASES = {
    "2x": (2, (8, 16, 32), 8, [(8, 12), (4, 6), (2, 3)]),
    "odd": (1, (8, 8, 16), 12, [(5, 7), (3, 4), (2, 2)]),
    "same": (2, (4, 8, 4), 4, [(3, 3), (3, 3), (1, 1)]),
}
FPN_NAMES = list(FPN_CASES)


def _freeze(t):
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def w1_args(name):
    n, cin, cout, (h, w), opt = W1_CASES[name]
    rng = np.random.default_rng(9700 + W1_NAMES.index(name))
    planted = name in W1_PLANTED
    if planted:
        raw = rng.integers(-8, 9, (n, h, w, cin)).astype(F)
        if "a_hot" in opt:
            img, py, px, ch, val = opt["a_hot"]
            raw[:] = 0.0
            raw[img, py, px, ch] = val
        dy = np.zeros((n, h, w, cout), F)
        for (img, py, px, col, val) in opt["hot"]:
            dy[img, py, px, col] = val
        wt = (2.0 ** rng.integers(-3, 4, (cout, cin)) * rng.choice([-1.0, 1.0], (cout, cin))).astype(F)
    else:
        raw = rng.standard_normal((n, h, w, cin)).astype(F)
        dy = rng.standard_normal((n, h, w, cout)).astype(F)
        wt = (rng.standard_normal((cout, cin)) * 0.05).astype(F)
    hi, lo = tr.split(raw)
    return dict(n=n, cin=cin, cout=cout, size=(h, w), rows=n * h * w, a=_freeze(hi.astype(F) + lo.astype(F)), hi=_freeze(hi),
                lo=_freeze(lo), dy=_freeze(dy), w=_freeze(wt), blocks=opt.get("blocks"), cols=opt.get("cols"), planted=planted)


@functools.lru_cache(maxsize=None)
def w1_reference(name):
    """(rule, bound) of the case with dW, db and dC, computed once, read-only"""
    c = w1_args(name)
    want, b = fr.w1_stage(c["a"], c["dy"])
    wc, bc = fr.dc_stage(c["dy"], c["w"])
    want.update(wc); b.update(bc)
    for d in (want, b):
        for t in d.values():
            t.setflags(write=False)
    return want, b


def w1_planted_expected(name):
    """What a planted case must give, written down without the rule: a one-hot dy = v at row q, column c gives dW[c, :] = v a[q, :],
    db[c] = v and dC[q, :] = v w[c, :]; several one-hots add.  float64."""
    c = w1_args(name)
    out = {"dW": np.zeros((c["cout"], c["cin"]), D), "db": np.zeros((c["cout"],), D), "dC": np.zeros(c["a"].shape, D)}
    for (img, py, px, col, val) in W1_CASES[name][4]["hot"]:
        out["dW"][col] += val * c["a"][img, py, px].astype(D)
        out["db"][col] += val
        out["dC"][img, py, px] += val * c["w"][col].astype(D)
    return out


@functools.lru_cache(maxsize=None)
def up_args(name):
    n, ch, (oh, ow), size, opt = UP_CASES[name]
    rng = np.random.default_rng(9800 + UP_NAMES.index(name))
    g = rng.integers(-16, 17, (n, oh, ow, ch)).astype(F) if opt.get("ints") else rng.standard_normal((n, oh, ow, ch)).astype(F)
    return dict(n=n, c=ch, fine=(oh, ow), size=size, g=_freeze(g), cols=opt.get("cols"), planted=bool(opt.get("ints")))


@functools.lru_cache(maxsize=None)
def up_reference(name):
    c = up_args(name)
    want, b = fr.up_t_stage(c["g"], c["size"])
    for d in (want, b):
        for t in d.values():
            t.setflags(write=False)
    return want, b


@functools.lru_cache(maxsize=None)
def fpn_args(name):
    n, cins, cout, sizes = FPN_CASES[name]
    rng = np.random.default_rng(9900 + FPN_NAMES.index(name))
    cs = [_freeze(rng.standard_normal((n, h, w, ci))) for (h, w), ci in zip(sizes, cins)]
    gs = [_freeze(rng.standard_normal((n, h, w, cout))) for h, w in sizes]
    w_inner = [_freeze(rng.standard_normal((cout, ci)) * 0.3) for ci in cins]
    b_inner = [_freeze(rng.standard_normal((cout,))) for _ in cins]
    w_layer = [_freeze(rng.standard_normal((cout, 3, 3, cout)) * 0.2) for _ in cins]
    b_layer = [_freeze(rng.standard_normal((cout,))) for _ in cins]
    return dict(n=n, cins=cins, cout=cout, sizes=sizes, c=cs, g=gs, w_inner=w_inner, b_inner=b_inner, w_layer=w_layer, b_layer=b_layer)
