"""Cases for the FCOS criterion's backward (tests/fcos_loss_grad_ref.py): every case of tests/fcos_loss_cases.py as it is, plus
the handmade `g3`, which holds each non-smooth point of the gradient once with exactly representable values; times two upstream
settings.  tests/golden/make_golden_fcos_loss_grad.py imports g3 from here.

g3: levels 5x7 / 3x4 / 2x2 at strides 8 / 16 / 32, C = 2, ext, two images.  Image 0 has one hand box (8, 4, 46, 30); its nine
foreground points are the level-0 points (16|24|32, 8|16|24).  Seeded heads (regressions |N(0, 1)| * 1.5 + 0.05, the ext
(mag, dx, dy) |N(0, 2^2)| + 0.25: no zero anywhere), then in image 0:
  TIE      point (24, 16): reg[0] = 2.0, so the decoded x1 = 24 - 2 * 8 = 8 is the box's x0: torch.max / torch.min split evenly
  APART    point (16, 8): reg[0] = reg[2] = 0, the decoded box has no width: the reference's mask (strict overlap) is false
  ZERO     point (32, 24): reg[1] = 0 exactly, a ReLU's zero output with overlap left: the gradient at the output is not masked
  CLAMP    point 0: dx = dy = 0, the normalisation's clamp
  DX0      point 1: dx = 0, dy = 1.5
"""
import functools

import numpy as np

import fcos_loss_cases as lc
import fcos_loss_ref as fr

F = np.float32
UPSTREAMS = (None, (0.75, 1.5, 0.0, -1.25, 2.5, 0.625))     # fp32 numbers: six distinct weights, a zero and a negative
G3 = lc.Case("g3", lc.SMALL, (8, 16, 32), 2, 2, True, 20261109, "each non-smooth point of the gradient once",
             (lc._t([(8, 4, 46, 30, 1, (2.0, 1.0, 0.5, 0.06, -0.08))]), lc.G2_TARGETS[0]))
G3_POINTS = {"TIE": 2 * 7 + 3, "APART": 1 * 7 + 2, "ZERO": 3 * 7 + 4, "CLAMP": 0, "DX0": 1}
BY_NAME = dict(lc.BY_NAME, g3=G3)
NAMES = lc.NAMES + ("g3",)
SMOOTH = lc.NAMES
GOLDEN = {"g1": "golden-1", "g2": "golden-2", "g3": "g3"}
CASES = tuple((name, u) for name in NAMES for u in range(len(UPSTREAMS)))


def case_id(case):
    return f"{case[0]}-up{case[1]}"


def g3_heads_flat():
    """(cls [2, 49, 4], reg [2, 49, 5], ex [2, 49, 8]) fp32"""
    cls, reg, ex = lc.heads_flat(G3.seed, G3.n, lc.points(G3), G3.num_classes, True)
    reg[..., :4] += F(0.05)
    rng = np.random.default_rng(G3.seed + 3)
    ex[..., :3] = (np.abs(rng.standard_normal(ex[..., :3].shape)) * 2.0 + 0.25).astype(F)
    reg[0, G3_POINTS["TIE"], 0] = 2.0
    reg[0, G3_POINTS["APART"], 0] = reg[0, G3_POINTS["APART"], 2] = 0.0
    reg[0, G3_POINTS["ZERO"], 1] = 0.0
    ex[0, G3_POINTS["CLAMP"], 1:3] = 0.0
    ex[0, G3_POINTS["DX0"], 1:3] = (0.0, 1.5)
    return cls, reg, ex


@functools.lru_cache(maxsize=None)
def make(name):
    """fcos_loss_cases.make() for its cases; the same tuple for g3, read-only"""
    if name != "g3":
        return lc.make(name)
    cls, reg, ex = g3_heads_flat()
    starts = fr.cr.starts_of(G3.sizes)
    levels = lambda t: [t[:, starts[l]:starts[l + 1]].reshape(G3.n, h, w, t.shape[2]).copy() for l, (h, w) in enumerate(G3.sizes)]
    out = (levels(cls), levels(reg), levels(ex), lc.pad_targets(G3.targets))
    for t in out[0] + out[1] + out[2] + list(out[3]):
        t.setflags(write=False)
    return out


def args(name):
    """the positional arguments of fcos_loss_ref.rule and of fcos_loss_grad_ref.rule / bound / emulate"""
    c = BY_NAME[name]
    cls_lr, reg_ctr, ext, gt = make(name)
    return (cls_lr, reg_ctr, ext, c.strides, c.num_classes) + tuple(gt)


def upstream(case):
    return UPSTREAMS[case[1]]
