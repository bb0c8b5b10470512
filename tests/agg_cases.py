"""Seeded head tensors for the A2J aggregation tests (tests/agg_ref.py): small maps at every branch of launch_aggregate's
geometry.  Each case's rule and bound are computed once (reference()) and shared by the tests."""
import functools
from dataclasses import dataclass

import numpy as np

import agg_ref as ar

F = np.float32


@dataclass(frozen=True)
class Case:
    name: str
    fh: int
    fw: int
    joints: int
    why: str
    k: int = 3
    stride: int = 16
    cls_scale: float = 2.0
    reg_scale: float = 8.0
    dep_scale: float = 1.0
    special: str = ""


CASES = (
    Case("11x11x21", 11, 11, 21, "the model's shape"),
    Case("11x11x21-peaked-flat", 11, 11, 21, "sample 0: one logit +30; sample 1: all logits equal", special="peaked-flat"),
    Case("1x1x1", 1, 1, 1, "one cell, G = 9 with 144 of 192 threads used"),
    Case("3x5x7", 3, 5, 7, "non-square; Jw = 3, the last workgroup has one joint"),
    Case("5x3x6", 5, 3, 6, "transposed; the smallest split case (Jw = 2)"),
    Case("9x14x5", 9, 14, 5, "cells == kBatch*G == 126 exactly; no joint split; 720 -> 768 threads"),
    Case("1x127x5", 1, 127, 5, "one more cell than a batch round, fh = 1"),
    Case("23x31x64", 23, 31, 64, "Jw = 22, G = 2, the last workgroup has 20 joints", k=2),
    Case("7x9x43", 7, 9, 43, "G = 4, 960 threads"),
    Case("6x6x63", 6, 6, 63, "G = 3, 1008 -> 1024 threads"),
    Case("4x7x21-stride8", 4, 7, 21, "the stride argument", stride=8),
    Case("11x11x21-cls30", 11, 11, 21, "differences near expf underflow", cls_scale=30.0),
    Case("11x11x21-big", 11, 11, 21, "magnitude: reg scale 200, dep in mm", reg_scale=200.0, dep_scale=1000.0),
)
BY_NAME = {c.name: c for c in CASES}

# the geometry each case is in the table for, restated from the joint count alone: (split, Jw, G, threads)
GEOMETRY = {"11x11x21": (3, 7, 9, 1024), "1x1x1": (1, 1, 9, 192), "3x5x7": (3, 3, 9, 448), "5x3x6": (3, 2, 9, 320),
            "9x14x5": (1, 5, 9, 768), "1x127x5": (1, 5, 9, 768), "23x31x64": (3, 22, 2, 704), "7x9x43": (3, 15, 4, 960),
            "6x6x63": (3, 21, 3, 1024)}

# the case on which each mutant of agg_ref.mutants() must fail
MUTANT_CASE = {"swap_p": "11x11x21", "swap_hw": "3x5x7", "div_fh": "3x5x7", "drop_last_cell": "1x127x5",
               "max_per_anchor": "11x11x21-peaked-flat", "neighbour_channel": "3x5x7"}


@functools.lru_cache(maxsize=None)
def make(name):
    """(cls, reg, dep) as read-only fp32 numpy arrays in the NHWC head layout"""
    c = BY_NAME[name]
    rng = np.random.default_rng(1000 + [x.name for x in CASES].index(name))
    aj = ar.A * c.joints
    cls = (rng.standard_normal((c.k, c.fh, c.fw, aj)) * c.cls_scale).astype(F)
    reg = (rng.standard_normal((c.k, c.fh, c.fw, 2 * aj)) * c.reg_scale).astype(F)
    dep = ((0.8 + 0.2 * rng.standard_normal((c.k, c.fh, c.fw, aj))) * c.dep_scale).astype(F)
    if c.special == "peaked-flat":
        cls[0, 6, 4, 5 * c.joints:6 * c.joints] += F(30.0)     # cell (6, 4), anchor 5, every joint
        cls[1] = F(0.0)
    for t in (cls, reg, dep):
        t.setflags(write=False)
    return cls, reg, dep


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rule, bound) of the case, computed once"""
    c = BY_NAME[name]
    out = ar.rule(*make(name), c.joints, c.stride), ar.bound(*make(name), c.joints, c.stride)
    for t in out:
        t.setflags(write=False)
    return out
