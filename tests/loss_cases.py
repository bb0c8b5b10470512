"""Cases of the A2J criterion tests (tests/loss_ref.py): the seeded heads of tests/agg_cases.py at every branch of the launch
geometry, with a ground truth = the float64 rule's keypoint plus a seeded offset: uv offsets from +-{0.25, 0.9, 1.5, 6.0} (both
sides of the smooth-L1 knee at 1), depth offsets from +-{0.01, 0.2} times the case's dep_scale.  Each case's rule and bound are
computed once (reference()) and shared by the tests.

Conditions asserted here (conditions(), run for every case on first use and by tests/test_loss_cpu.py):
  * in every case with at least 4 uv terms, at least a quarter of the Lr terms lie on each side of the knee;
  * no |difference| of a uv term (La or Lr) lies within 1e-3 of the knee, so no term's branch hangs on the last bits."""
import functools
from dataclasses import dataclass

import numpy as np

import agg_cases as ac
import agg_ref as ar
import loss_ref as lr

F = np.float32
UV_OFFSETS = (0.25, 0.9, 1.5, 6.0)
DEPTH_OFFSETS = (0.01, 0.2)
KNEE_GUARD = 1e-3


@dataclass(frozen=True)
class Case:
    name: str
    heads: str                       # the agg_cases case whose heads these are
    why: str
    spatial_factor: float = 0.5
    reg_loss_factor: float = 3.0
    special: str = ""


CASES = tuple(Case(n, n, ac.BY_NAME[n].why) for n in (
    "11x11x21", "11x11x21-peaked-flat", "1x1x1", "3x5x7", "5x3x6", "9x14x5", "1x127x5", "23x31x64", "6x6x63", "4x7x21-stride8",
    "11x11x21-cls30", "11x11x21-big")) + (
    Case("3x5x7-gt-nan", "3x5x7", "one NaN coordinate in gt: its terms, its sample row and every batch value are NaN", special="gt-nan"),
    Case("5x3x6-sf0.1", "5x3x6", "spatial_factor = 0.1 (not an fp32 number) and reg_loss_factor = 2.5", spatial_factor=0.1,
         reg_loss_factor=2.5),
    Case("3x5x7-valid", "3x5x7", "valid = (1, 0, 1): the middle row is left out of the batch values and the divisor", special="valid"),
)
BY_NAME = {c.name: c for c in CASES}

# the case on which each mutant of loss_ref.mutants() must fail
MUTANT_CASE = {"depth_smooth_l1": "11x11x21", "knee3_uv": "11x11x21", "sf_on_depth": "11x11x21-big", "no_sf": "5x3x6-sf0.1",
               "mean_over_j": "3x5x7", "anchor_from_er": "11x11x21", "no_reg_factor": "5x3x6-sf0.1", "valid0_counted": "3x5x7-valid"}


def _balanced(rng, values, n):
    """n draws from +-values with every magnitude as often as the others (to within one), in a seeded order and with seeded signs"""
    mag = np.resize(np.asarray(values, np.float64), n)
    rng.shuffle(mag)
    return mag * rng.choice([-1.0, 1.0], size=n)


def heads(name):
    return ac.make(BY_NAME[name].heads)


def agg(name):
    return ac.BY_NAME[BY_NAME[name].heads]


@functools.lru_cache(maxsize=None)
def make(name):
    """(gt [K,J,3] fp32 read-only, valid [K] int32 or None)"""
    c, a = BY_NAME[name], agg(name)
    out = ac.reference(c.heads)[0]
    for attempt in range(32):      # the first seed of the case's own sequence whose La differences keep clear of the knee too
        rng = np.random.default_rng(7000 + [x.name for x in CASES].index(name) + 100 * attempt)
        off = np.empty((a.k, a.joints, 3))
        off[..., :2] = _balanced(rng, UV_OFFSETS, a.k * a.joints * 2).reshape(a.k, a.joints, 2)
        off[..., 2] = _balanced(rng, DEPTH_OFFSETS, a.k * a.joints).reshape(a.k, a.joints) * a.dep_scale
        gt = (out + off).astype(F)
        if _measure(name, gt)[0] > 2 * KNEE_GUARD:
            break
    if c.special == "gt-nan":
        gt[1, 2, 0] = np.nan
    valid = np.array([1, 0, 1], np.int32) if c.special == "valid" else None
    gt.setflags(write=False)
    conditions(name, gt)
    return gt, valid


def kwargs(name):
    """what rule / bound / emulate take behind the heads"""
    c, a = BY_NAME[name], agg(name)
    gt, valid = make(name)
    return dict(gt=gt, joints=a.joints, stride=a.stride, spatial_factor=c.spatial_factor, reg_loss_factor=c.reg_loss_factor,
                valid=valid)


def _measure(name, gt):
    """(the nearest |uv difference| to the knee, the share of the Lr differences below it), NaN entries aside"""
    a = agg(name)
    ea, out = lr.expectations(*heads(name), a.joints, a.stride)
    g = gt.astype(np.float64)
    d_r = np.abs(g[..., :2] - out[..., :2]).ravel()
    d_a = np.abs(g[..., :2] - ea).ravel()
    d_r, d_a = d_r[~np.isnan(d_r)], d_a[~np.isnan(d_a)]
    return min(np.abs(d_r - 1.0).min(), np.abs(d_a - 1.0).min()), float((d_r <= 1.0).mean()), d_r.size


def conditions(name, gt=None):
    """the two conditions of the module docstring on the case's uv differences"""
    gap, below, count = _measure(name, make(name)[0] if gt is None else gt)
    assert gap > KNEE_GUARD, (name, gap)
    if count >= 4:
        assert 0.25 <= below <= 0.75, (name, below)
    return gap, below


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rule, bound) dicts of the case, computed once"""
    kw = kwargs(name)
    out = lr.rule(*heads(name), **kw), lr.bound(*heads(name), **kw)
    for d in out:
        for t in d.values():
            t.setflags(write=False)
    return out
