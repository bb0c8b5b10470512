"""Seeded inputs for the GroupNorm statistics tests (tests/gn_ref.py): the shapes at which gn_partial_kernel's reduction tree,
chunk tail and write loop change, each with a ladder of |mean| / std ratios and scales, images and groups that differ (so that
mixing two shows), and a constant tensor; rows32 slabs whose 32-row groups straddle images.  References are computed once."""
import functools
import zlib

import numpy as np

import gn_ref as gr

F = np.float32
EPS = 1e-5

# n, h, w, c, groups
AFFINE = {
    "hw1": (1, 1, 1, 32, 8),
    "hw63": (2, 7, 9, 64, 8),
    "c4": (1, 8, 8, 4, 1),                  # rows_par = 256
    "hw65": (3, 5, 13, 256, 32),            # a one-row tail chunk
    "cpg256": (2, 10, 13, 1024, 4),         # cpg = 256 > 64 lanes, rows_par = 1
    "groups256": (1, 8, 16, 1024, 256),     # cpg = 4
    "hw129": (2, 3, 43, 16, 4),
    "tower": (2, 25, 34, 256, 32),
}
RATIOS = (0, 1, 10, 100)
STDS = (1e-3, 1.0, 1e3)
LADDER = tuple(f"ratio{r}-std{s:g}" for r in RATIOS for s in STDS)
INPUTS = LADDER + ("images", "groups", "constant")

# n, hw, c, groups
ROWS32 = {
    "hw32": (1, 32, 64, 8),
    "hw33": (3, 33, 64, 8),
    "hw36": (5, 36, 64, 4),
    "hw63": (2, 63, 32, 4),
    "hw64": (3, 64, 256, 32),
    "hw130-cpg256": (3, 130, 1024, 4),
}

# the (shape, input) on which each mutant of gn_ref.mutants() must fail
MUTANT_CASE = {"drop_last_row": ("hw65", "ratio1-std1"), "cnt_no_tail": ("hw63", "ratio1-std1"), "next_group": ("hw129", "groups"),
               "image0": ("hw63", "images"), "straddle_swap": "hw33"}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _affine_params(c, rng):
    return (1.0 + 0.2 * rng.standard_normal(c)).astype(F), (0.1 * rng.standard_normal(c)).astype(F)


@functools.lru_cache(maxsize=None)
def make(shape, kind):
    """(x [n,h,w,c], gamma, beta) as read-only fp32 arrays"""
    n, h, w, c, groups = AFFINE[shape]
    rng = _rng("affine", shape, kind)
    gamma, beta = _affine_params(c, rng)
    z = rng.standard_normal((n, h, w, groups, c // groups))
    if kind in LADDER:
        ratio, std = (float(t[len(p):]) for t, p in zip(kind.split("-"), ("ratio", "std")))
        x = (z + ratio) * std
    elif kind == "images":      # image i at 50^i times image 0's scale
        x = (z + 1.0) * (50.0 ** np.arange(n))[:, None, None, None, None]
    elif kind == "groups":      # a different mean per group, neighbours far apart
        x = z + (((np.arange(groups) * 7) % 11 - 5) * 0.7)[None, None, None, :, None]
    else:                       # var = 0, and every partial sum exact
        x = np.full(z.shape, 0.75)
    out = x.reshape(n, h, w, c).astype(F), gamma, beta
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """(rule, bound) of the case, computed once"""
    groups = AFFINE[shape][4]
    x, gamma, beta = make(shape, kind)
    return gr.rule(x, gamma, beta, groups, EPS), gr.bound(x, gamma, beta, groups, EPS)


LIMIT_RATIOS = (0, 10, 100, 1000)


def make_limit(ratio):
    """(x, gamma = 1, beta = 0, groups) at the tower's shape, one image, N(ratio, 1): the inputs of the rstd-limit figures
    (scale IS rstd; run with eps = 0)"""
    _n, h, w, c, groups = AFFINE["tower"]
    z = np.random.default_rng(7).standard_normal((1, h, w, c))
    return (z + ratio).astype(F), np.ones(c, F), np.zeros(c, F), groups


@functools.lru_cache(maxsize=None)
def make_rows32(name, hw_extra=0, poison=True):
    """(slab, x [n*hw, c], gamma, beta): image i at 1 + i times image 0's scale and a mean per group, so that a wrong half or a
    wrong unit shows; hw_extra: a second level of the same n, c for the levels launch"""
    n, hw, c, groups = ROWS32[name]
    hw += hw_extra
    rng = _rng("rows32", name, hw_extra)
    gamma, beta = _affine_params(c, rng)
    z = rng.standard_normal((n, hw, groups, c // groups)) + (((np.arange(groups) * 7) % 11 - 5) * 0.3)[None, None, :, None]
    x = (z * (1.0 + np.arange(n))[:, None, None, None]).reshape(n * hw, c).astype(F)
    slab = gr.pack_rows32(x, n, hw, c)
    if not poison:
        slab = np.nan_to_num(slab, nan=0.0)
    for t in (slab, x, gamma, beta):
        t.setflags(write=False)
    return slab, x, gamma, beta
