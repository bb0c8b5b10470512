"""Seeded head tensors for the candidate and ext-gather tests (tests/cand_ref.py): small level tables at every loop bound of the
candidate kernels (1024-point chunks, the single-workgroup form's 4 x 1024 unroll, more than 64 chunks), planted ties and
overflowing logits.  The generator resamples every point whose decision float64 and fp32 could take differently
(cand_ref.guards) with the case's seed, so no point is left out of any comparison.  Each case's rule is computed once
(reference()) and shared by the tests."""
import functools
from dataclasses import dataclass

import numpy as np

import cand_ref as cr

F = np.float32
WORKLOAD = ((13, 17), (7, 9), (4, 5))      # the workload's three levels (100 x 136, 50 x 68, 25 x 34), scaled down


@dataclass(frozen=True)
class Case:
    name: str
    sizes: tuple
    strides: tuple
    why: str
    n: int = 1
    num_classes: int = 3
    thresh: float = 0.7
    images: tuple = ()        # per image: "mixed" (default) | "none" (nothing passes) | "all" (everything passes)
    special: tuple = ()       # "ties" | "extreme" | "neg-reg"
    cap: int = 0              # 0: the number of points


CASES = (
    Case("workload", WORKLOAD, (8, 16, 32), "the workload's levels and strides, scaled down", n=2),
    Case("one-level", ((9, 11),), (8,), "a single level"),
    Case("five-levels", ((6, 7), (5, 3), (3, 4), (2, 2), (1, 1)), (8, 16, 32, 64, 128), "HN_FCOS_MAX_LEVELS levels", n=2),
    Case("tall", ((19, 5), (3, 2)), (8, 16), "h > w: gy = q / w, not q / h"),
    Case("wide", ((5, 19), (2, 3)), (8, 16), "w > h"),
    Case("odd-strides", ((6, 5), (4, 3), (3, 3)), (5, 7, 1), "half = rint(stride / 2) to even: 2.5 -> 2, 3.5 -> 4, 0.5 -> 0"),
    Case("P1023", ((31, 31), (31, 2)), (8, 16), "one point short of a chunk; level boundary at 961"),
    Case("P1024", ((31, 31), (9, 7)), (8, 16), "exactly one chunk"),
    Case("P1025", ((31, 31), (8, 8)), (8, 16), "one point in the second chunk"),
    Case("P4095", ((63, 63), (14, 9)), (8, 16), "one short of the single-workgroup form's 4 x 1024 round; boundary at 3969"),
    Case("P4096", ((63, 63), (127, 1)), (8, 16), "exactly one round"),
    Case("P4097", ((63, 63), (8, 16)), (8, 16), "one point in the second round"),
    Case("P8193", ((90, 90), (31, 3)), (8, 16), "two rounds and a point; boundary at 8100 inside chunk 7"),
    Case("260x260", ((260, 260),), (8,), "67 600 points = 67 chunks: the scatter kernel's `c += 64` prefix loop runs twice"),
    Case("classes-1", ((5, 7), (3, 4)), (8, 16), "num_classes = 1", n=2, num_classes=1),
    Case("classes-64", ((5, 7), (3, 4)), (8, 16), "num_classes = 64, the most the library takes", n=2, num_classes=64),
    Case("none-all", WORKLOAD, (8, 16, 32), "n = 3: image 1 has no passing point, image 2 only passing points", n=3,
         images=("mixed", "none", "all")),
    Case("thresh-1", WORKLOAD, (8, 16, 32), "thresh = -1: every point passes, scores of 0 included", n=2, thresh=-1.0,
         special=("ties", "extreme")),
    Case("ties", WORKLOAD, (8, 16, 32), "planted exact class ties and side ties on passing points", n=2, special=("ties",)),
    Case("extreme", WORKLOAD, (8, 16, 32), "logits of +-100 and +-88: expf overflows to inf and underflows to 0", n=2,
         special=("extreme",)),
    Case("neg-reg", WORKLOAD, (8, 16, 32), "regressions that are negative and large", n=2, special=("neg-reg",)),
    Case("cap-7", WORKLOAD, (8, 16, 32), "cap below the passing count of images 0 and 2; image 1 keeps nothing", n=3,
         images=("mixed", "none", "all"), cap=7),
)
BY_NAME = {c.name: c for c in CASES}

# the case on which each mutant of cand_ref.mutants() must fail, and the property check() must name
MUTANT_CASE = {"last_tie": ("ties", "label"), "no_sqrt": ("workload", "count"), "gy_by_h": ("tall", "box"),
               "half_unrounded": ("odd-strides", "box"), "level_off_by_one": ("thresh-1", "level"), "side_ge": ("ties", "side"),
               "keep_last": ("cap-7", "point")}


def points(c):
    return sum(h * w for h, w in c.sizes)


def _sample(rng, mode, k, num_classes):
    """(cls_lr rows, ctr) for some points of one image; logits within +-4 so that 1e-3 between two logits is far above fp32's
    resolution of their sigmoids (the slope of sigmoid at 4 is 0.018)"""
    if mode == "none":
        return rng.uniform(-4.0, -2.0, (k, num_classes + 2)), rng.uniform(-4.0, -2.0, k)
    if mode == "all":        # the smallest score is sqrt(sigmoid(2) sigmoid(2)) = 0.88
        x = rng.uniform(2.0, 4.0, (k, num_classes + 2))
        return x, rng.uniform(2.0, 4.0, k)
    return rng.uniform(-4.0, 4.0, (k, num_classes + 2)), rng.uniform(-4.0, 4.0, k)


def _plant(c, cls, reg, planted):
    """planted rows of image 0 (marked in `planted` so that the tests can see they survived the resampling)"""
    C, P = c.num_classes, cls.shape[1]
    rows = iter(range(3, P, max(1, P // 24)))
    def row():
        r = next(rows); planted.append(r); return r
    if "ties" in c.special:
        for a, b in ((1, 2), (0, 2), (0, 1)):             # two classes share the top logit, on a passing point
            r = row(); cls[0, r, :C] = F(-1.0); cls[0, r, a] = cls[0, r, b] = F(3.0); reg[0, r, 4] = F(3.0)
        r = row(); cls[0, r, :C] = F(2.5); reg[0, r, 4] = F(3.5)            # all classes tie
        for v in (0.25, -1.5, 3.0):                      # the two side logits tie, on a passing point
            r = row(); cls[0, r, :C] = F(-1.0); cls[0, r, 0] = F(3.0); reg[0, r, 4] = F(3.0); cls[0, r, C] = cls[0, r, C + 1] = F(v)
    if "extreme" in c.special:
        for big, ctr in ((100.0, 100.0), (88.0, 88.0), (100.0, 2.0), (88.0, 1.0)):      # sigmoid saturates at 1: expf(-100) = 0
            r = row(); cls[0, r, 0] = F(big); reg[0, r, 4] = F(ctr)
        for low, ctr in ((-100.0, 2.0), (-88.0, 3.0), (-100.0, -100.0), (-88.0, -88.0), (2.0, -100.0), (1.0, -88.0)):
            # expf(100) = inf, expf(88) = 1.65e38: the product is 0 or denormal and every class scores the same in fp32, so
            # the classes carry the same logit (the first wins in float64 too)
            r = row(); cls[0, r, :C] = F(low); reg[0, r, 4] = F(ctr)


@functools.lru_cache(maxsize=None)
def make(name):
    """(cls_lr, reg_ctr, planted): per-level read-only fp32 arrays [n, h, w, C + 2] / [n, h, w, 5], and the planted rows"""
    c = BY_NAME[name]
    rng = np.random.default_rng(3000 + [x.name for x in CASES].index(name))
    C, P = c.num_classes, points(c)
    modes = c.images or ("mixed",) * c.n
    cls = np.empty((c.n, P, C + 2), F)
    reg = np.empty((c.n, P, 5), F)
    for i, mode in enumerate(modes):
        a, b = _sample(rng, mode, P, C)
        cls[i], reg[i, :, 4] = a.astype(F), b.astype(F)
    reg[..., :4] = (rng.uniform(-1e4, 1e4, (c.n, P, 4)) if "neg-reg" in c.special else rng.uniform(0.0, 3.0, (c.n, P, 4))).astype(F)
    planted = []
    _plant(c, cls, reg, planted)
    starts = cr.starts_of(c.sizes)
    levels = lambda t: [t[:, starts[l]:starts[l + 1]].reshape(c.n, h, w, t.shape[2]) for l, (h, w) in enumerate(c.sizes)]
    for _ in range(100):
        bad = cr.guards(levels(cls), levels(reg), C, c.thresh)
        if not bad.any():
            break
        for i, mode in enumerate(modes):                   # resample, never exclude
            k = int(bad[i].sum())
            a, b = _sample(rng, mode, k, C)
            cls[i, bad[i]], reg[i, bad[i], 4] = a.astype(F), b.astype(F)
    else:
        raise AssertionError("the guards did not clear")
    out = [t.copy() for t in levels(cls)], [t.copy() for t in levels(reg)]
    for t in out[0] + out[1]:
        t.setflags(write=False)
    return out[0], out[1], tuple(planted)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    cls_lr, reg_ctr, _ = make(name)
    return cr.rule64(cls_lr, reg_ctr, c.strides, c.num_classes, c.thresh, cap=c.cap or None)


# --------------------------------------------------------------------------------------------------------------------------
# ext gather: three levels, 20 points = cap, n = 3 with det_count 0, 1 and cap
# --------------------------------------------------------------------------------------------------------------------------
EXT_SIZES = ((3, 4), (2, 3), (1, 2))
EXT_CAP = 20
EXT_COUNT = (0, 1, EXT_CAP)
EXT_MUTANT_PROPERTY = {"no_clamp": "bound", "last_max": "contact", "keep_point_swapped": "mag"}


@functools.lru_cache(maxsize=None)
def make_ext():
    """(ext per level [3, h, w, 8], point [3, 20], keep [3, 20], count [3]).  Image 2 keeps all 20 points -- the first and the
    last of every level, both sides of every boundary -- through two permutations that are not the identity; image 1 keeps one:
    the first point of level 1 through keep = 5."""
    rng = np.random.default_rng(3900)
    n, cap = 3, EXT_CAP
    flat = np.empty((n, cap, 8), F)
    flat[..., :3] = rng.uniform(0.0, 2.0, (n, cap, 3)).astype(F)          # a ReLU's outputs
    for i in range(n):
        for p in range(cap):                                              # contact logits pairwise equal or >= 1e-3 apart, |x| <= 10
            while True:
                x = rng.uniform(-10.0, 10.0, 5).astype(F)
                g = np.abs(x[:, None].astype(np.float64) - x[None, :])[np.triu_indices(5, 1)]
                if (g >= 1e-3).all():
                    break
            flat[i, p, 3:] = x
    z = F(0.0)
    flat[2, 0, 1:3] = (z, z)                              # dx = dy = 0: the clamp, 0 and not NaN
    flat[2, 1, 1:3] = (z, F(1.25))                        # one of them zero
    flat[2, 11, 1:3] = (F(0.75), z)
    flat[2, 12, 1:3] = (F(1e-20), F(1e-20))               # the squares underflow: 0.1 * d / 1e-12
    flat[2, 17, 1:3] = (F(1e-20), z)
    flat[2, 18, 1:3] = (F(3e-13), F(4e-13))               # norm 5e-13, just below the clamp
    flat[2, 19, 1:3] = (F(3e-12), F(4e-12))               # norm 5e-12, just above it
    flat[1, 12, 1:3] = (z, z)
    flat[2, 5, 3:] = (1.5, 4.0, 4.0, -2.0, 4.0)           # first-max ties: 1, not 2 or 4
    flat[2, 13, 3:] = (-3.0, -3.0, -3.0, -3.0, -3.0)      # all equal: 0
    flat[2, 6, 3:] = (0.5, -1.0, 2.0, 7.0, 7.0)           # 3, not 4
    point = np.stack([rng.permutation(cap) for _ in range(n)]).astype(np.int32)
    keep = np.stack([rng.permutation(cap) for _ in range(n)]).astype(np.int32)
    for perm, at, value in ((keep[1], 0, 5), (point[1], 5, 12)):      # swap, so that both stay permutations
        j = int(np.nonzero(perm == value)[0][0])
        perm[j], perm[at] = perm[at], value
    assert all(sorted(point[i]) == sorted(keep[i]) == list(range(cap)) for i in range(n))
    assert all((point[i] != np.arange(cap)).any() and (keep[i] != np.arange(cap)).any() for i in range(n))
    starts = cr.starts_of(EXT_SIZES)
    ext = [flat[:, starts[l]:starts[l + 1]].reshape(n, h, w, 8).copy() for l, (h, w) in enumerate(EXT_SIZES)]
    count = np.asarray(EXT_COUNT, np.int32)
    for t in ext + [point, keep, count]:
        t.setflags(write=False)
    return ext, point, keep, count


@functools.lru_cache(maxsize=None)
def ext_reference():
    return cr.ext_rule64(*make_ext())


# logits 20 and 30 both have sigmoid == 1.0f: the FIRST of them wins in fp32 (float64 would pick 30)
SATURATED = np.asarray((-2.0, 20.0, 5.0, 30.0, 20.0), F)


@functools.lru_cache(maxsize=None)
def make_saturated():
    """one level of 1 x 2 points, one image, one detection reading point 1"""
    ext = np.zeros((1, 1, 2, 8), F)
    ext[0, 0, 1, :3] = (0.5, 0.3, 0.4)
    ext[0, 0, 1, 3:] = SATURATED
    return [ext], np.asarray([[1, 0]], np.int32), np.asarray([[0, 1]], np.int32), np.asarray([1], np.int32)
