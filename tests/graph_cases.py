"""The seeded case table of the fused graph convolution (hn_graph_conv_cheby3_f16x3), shared by tests/test_graph_ops_cpu.py
(the arithmetic model on these inputs) and tests/test_graph_ops_gpu.py (the kernel on these inputs), and the cases of feat_interp_add with their bars.  Plain numpy."""
from collections import namedtuple

import numpy as np

from oracle import graph_ref

Case = namedtuple("Case", "v batch fin fout up fi relu bias split")
# fi: None = no residual, "1" = one input feature, "q" = Fout // 4, "eq" = Fout, "2x" = 2 Fout (Fi > Fout)
# A cover of the values below, not their product; every case has its own graph (seed = its index).
#    V  batch Fin  Fout up  Fi    ReLU bias split
FUSED_CASES = [Case(*c) for c in [
    (100, 3, 256, 256, 1, None, 1, 1, 0),
    (100, 3, 256, 256, 2, "eq", 1, 1, 0),
    (100, 1, 256, 256, 1, None, 1, 1, 1),
    (49,  2, 4,   3,   1, None, 0, 1, 0),
    (21,  7, 64,  250, 1, "q",  1, 1, 0),
    (5,   3, 252, 40,  3, "2x", 1, 1, 0),
    (100, 1, 128, 64,  2, "eq", 1, 1, 1),
    (1,   7, 8,   256, 4, "1",  1, 1, 0),
    (1,   3, 36,  17,  1, None, 0, 0, 0),
    (100, 3, 12,  1,   1, None, 0, 1, 0),
    (5,   2, 12,  16,  2, "eq", 1, 0, 0),
    (21,  1, 8,   64,  1, "q",  1, 1, 0),
    (21,  3, 8,   96,  3, None, 1, 1, 1),
    (49,  7, 36,  40,  1, "1",  0, 1, 0),
    (49,  1, 64,  17,  4, "2x", 1, 1, 0),
    (100, 2, 252, 250, 1, "2x", 0, 1, 0),
    (100, 7, 128, 96,  1, "q",  1, 0, 0),
    (21,  2, 256, 3,   1, None, 0, 1, 0),
    (5,   7, 256, 64,  1, "eq", 1, 1, 0),
    (1,   2, 256, 16,  2, None, 1, 1, 0),
    (49,  3, 4,   250, 2, "1",  1, 1, 0),
    (100, 1, 4,   1,   1, None, 0, 0, 0),
    (21,  7, 12,  17,  1, "eq", 1, 1, 0),
    (5,   3, 64,  256, 1, None, 1, 1, 1),
    (49,  2, 128, 40,  2, "q",  0, 0, 0),
    (100, 3, 36,  96,  4, "2x", 1, 1, 0),
    (1,   1, 252, 256, 1, "q",  1, 1, 0),
    (21,  1, 252, 1,   3, "1",  0, 1, 0),
    (49,  7, 8,   3,   1, "eq", 0, 1, 0),
    (100, 2, 64,  64,  3, None, 1, 1, 1),
    (5,   1, 128, 250, 1, None, 1, 1, 0),
    (21,  3, 36,  256, 1, "2x", 1, 1, 0),
    (49,  1, 256, 40,  1, "eq", 1, 1, 0),
    (100, 7, 256, 17,  1, "q",  1, 1, 0),
    (1,   3, 4,   16,  1, "eq", 0, 1, 0),
    (5,   2, 8,   40,  4, None, 1, 1, 0),
    (49,  3, 12,  64,  1, "2x", 1, 0, 1),
    (21,  2, 128, 256, 2, "1",  0, 1, 0),
    (100, 1, 252, 96,  1, "eq", 1, 1, 1),
    (5,   7, 36,  3,   2, None, 0, 1, 0),
]]

# the f16x3 bar of tests/test_conv_gpu.py: |y - fp64| <= F16X3_BAR * max(1, max |fp64|)
F16X3_BAR = 2e-5


def case_id(i):
    c = FUSED_CASES[i]
    return f"{i}-V{c.v}b{c.batch}-{c.fin}to{c.fout}-up{c.up}-fi{c.fi}" + ("-split" if c.split else "")


def residual_width(c):
    return {None: 0, "1": 1, "q": c.fout // 4, "eq": c.fout, "2x": 2 * c.fout}[c.fi]


def fused_inputs(i):
    """Case i -> dict of numpy operands: L (fp32 CSR), x [B,V,Fin], w [Fout, 3 Fin] (k-major columns, N(0, 2 / 3 Fin)),
    bias [Fout] or None, xin [B,V,Fi] or None; all fp32, from the case's own seed."""
    c = FUSED_CASES[i]
    rng = np.random.default_rng(1000 + i)
    fi = residual_width(c)
    return {
        "L": graph_ref.random_graph(c.v, seed=i),
        "x": rng.standard_normal((c.batch, c.v, c.fin)).astype(np.float32),
        "w": (rng.standard_normal((c.fout, 3 * c.fin)) * (2.0 / (3 * c.fin)) ** 0.5).astype(np.float32),
        "bias": rng.standard_normal(c.fout).astype(np.float32) if c.bias else None,
        "xin": rng.standard_normal((c.batch, c.v, fi)).astype(np.float32) if fi else None,
    }


def padded_bank(w, fin):
    """[Fout, 3 Fin] -> [Fout, pad32(3 Fin)] with zero columns behind the basis (the bank the kernel takes)."""
    out = np.zeros((w.shape[0], graph_ref.pad32(3 * fin)), np.float32)
    out[:, :3 * fin] = w
    return out


# feat_interp_add: |out - fp64| <= 1e-5 on N(0, 1) data (the bar of test_graph_ops_match_torch)
INTERP_BAR = 1e-5
# (Fi, Fo, bar): Fi above, below and equal to Fo, one input feature, and ratios that are not exact in fp32.
# Two cases have a bar of their own.  The kernel forms the source index as ATen does, in fp32 (scale = Fi / Fo rounded,
# src = scale (j + 0.5) - 0.5 rounded): with an inexact ratio src is off by about an ulp of its own size (1.5e-5 near 250,
# 3.8e-6 near 62), and the weight's error times the step between two N(0, 1) neighbours (up to ~5 over the 15750 outputs of
# a case) is what the result is off by.  oracle.graph_ref.feat_interp_add_model (that arithmetic in numpy, run on the CPU on
# these very inputs, up 1..4) against fp64:
#     62 -> 250   worst 1.341e-5   bar 4 x = 5.4e-5
#    250 ->  62   worst 4.367e-5   bar 4 x = 1.75e-4
# (24 -> 100: 5.4e-6, within INTERP_BAR; the exact ratios: <= 4.4e-7.)  tests/test_graph_ops_cpu.py asserts these figures.
INTERP_CASES = [(64, 256, INTERP_BAR), (256, 64, INTERP_BAR), (100, 100, INTERP_BAR), (1, 40, INTERP_BAR), (62, 250, 5.4e-5),
                (250, 62, 1.75e-4), (24, 100, INTERP_BAR), (500, 250, INTERP_BAR)]


def interp_inputs(fi, fo):
    """-> [(up, xin [3, 21, fi], y [3, 21, fo])] for up 1..4, fp32 N(0, 1), from the case's own seed."""
    rng = np.random.default_rng(fi * 1000 + fo)
    return [(up, rng.standard_normal((3, 21, fi)).astype(np.float32), rng.standard_normal((3, 21, fo)).astype(np.float32))
            for up in (1, 2, 3, 4)]
