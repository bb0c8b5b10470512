"""Shapes and seeded inputs of the ResNet stem chain (stem_image_kernel -> the stem form of the f16x3 implicit GEMM, or
conv_stem_pool_direct_kernel -> maxpool_s32_kernel) for tests/test_stem_cpu.py and tests/test_stem_gpu.py.  numpy and the
host-side weight packing only; nothing here runs a kernel.

A stem image is (n, ph, pw) with pw even, r = 7, stride = 2, pad = 3: the conv map is oh = (ph - 1) // 2 + 1 rows, the pooled map
poh = (oh - 1) // 2 + 1 rows, and the fused kernel works on 7 x 8 pooled pixels (15 x 17 conv pixels) per workgroup."""
import functools
from collections import namedtuple

import numpy as np
import torch

Case = namedtuple("Case", "name n ph pw why")

CASES = (
    Case("1x1", 1, 2, 2, "image smaller than the filter: every patch row is clamped; a grid of 1 (q = 0, rr = 1 in the remap)"),
    Case("4x5", 2, 7, 10, "even oh, odd ow; less than one patch"),
    Case("14x15", 1, 27, 30, "pooled 7 x 8: exactly one full patch"),
    Case("15x17", 1, 29, 34, "pooled 8 x 9: one pooled row and one pooled column past a patch, 2 x 2 patches; odd oh and ow"),
    Case("17x25", 2, 33, 50, "odd hb = 39: the image's last row is unused by the conv"),
    Case("3x130", 1, 5, 260, "a strip: 9 patches in x only"),
    Case("130x3", 1, 260, 6, "a strip: 10 patches in y only"),
    Case("88x88", 3, 176, 176, "the A2J crop: 7 x 6 patches per image, 126 workgroups (126 & 7 = 6)"),
    Case("15x17x4", 4, 29, 34, "16 workgroups: a multiple of 8, rr = 0 in the remap"),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)
KINDS = ("normal", "depth", "small", "edge_heavy", "all_negative")
# what a kind is fed with: (cin, BN fold, positive weights); `normal` alternates cin 3 / 4 and the fold over the cases
R, STRIDE, PAD, COUT = 7, 2, 3, 64
QR, QC = 7, 8            # pooled pixels per patch of the fused kernel


def geometry(c):
    """(hb, wb, oh, ow, poh, pow, workgroups of the fused kernel)"""
    hb, wb = c.ph + 2 * PAD, c.pw + 2 * PAD
    oh, ow = (c.ph - 1) // 2 + 1, (c.pw - 1) // 2 + 1
    assert oh == (hb - R) // STRIDE + 1 and ow == (wb - R) // STRIDE + 1 and c.pw % 2 == 0
    poh, pow_ = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    return hb, wb, oh, ow, poh, pow_, c.n * (-(-poh // QR)) * (-(-pow_ // QC))


def _seed(name, kind, what):
    return 1000 * NAMES.index(name) + 10 * KINDS.index(kind) + what


def _flavour(name, kind):
    i = NAMES.index(name)
    if kind == "depth":
        return 1, i % 2 == 0
    if kind == "normal":
        return (3, 4)[i % 2], i % 3 != 0
    if kind == "small":
        return 3, i % 2 == 1
    return 4, True       # edge_heavy, all_negative


@functools.lru_cache(maxsize=None)
def image(name, kind):
    """[n, ph, pw, 4] fp32 (read-only)"""
    c = BY_NAME[name]
    g = np.random.default_rng(_seed(name, kind, 1))
    shape = (c.n, c.ph, c.pw, 4)
    if kind == "depth":                          # what pack_depth_nhwc feeds: the crop's depth in channel 0, zeros elsewhere
        x = np.zeros(shape, np.float32)
        x[..., 0] = g.uniform(0.3, 1.3, shape[:3])
    elif kind == "small":                        # hi ~ 1e-2, lo ~ 1e-2 * 2^-12 < 2^-14: every lo part is an fp16 subnormal
        x = (g.standard_normal(shape) * 1e-2).astype(np.float32)
    else:
        x = g.standard_normal(shape).astype(np.float32)
        if kind == "edge_heavy":                 # a phantom conv pixel next to the bottom / right edge would win the pooling
            x = np.abs(x)
            x[:, -2:] *= 50.0
            x[:, :, -2:] *= 50.0
    x = x.astype(np.float32)                     # (channels at or beyond the filter's cin meet zero weights)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def filters(name, kind, cout=COUT):
    """(w16 [cout, 7, 2, 32] fp16, bias [cout] fp32), numpy, read-only: weights.pack_stem_split of a seeded [cout, cin, 7, 7]
    tensor, with a BatchNorm fold (then the bias is its shift) or without (then the bias is seeded beside it)."""
    from hn_amd.weights import pack_stem_split
    cin, fold = _flavour(name, kind)
    g = torch.Generator().manual_seed(_seed(name, kind, 2) + cout)
    w = torch.randn((cout, cin, R, R), generator=g) * 0.1
    if kind in ("edge_heavy", "all_negative"):
        w = w.abs()
    scale = torch.rand((cout,), generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn((cout,), generator=g, dtype=torch.float64) * 0.2
    if kind == "all_negative":
        # |conv| <= max |x| * sum |w| per channel (the split operands recombine to within 2^-21 of these): with a bias below
        # the negative of 1.5 times that, every conv output is < 0
        xmax = float(np.abs(image(name, kind)).max())
        shift = -(1.5 * xmax * (w.double().abs() * (scale.view(-1, 1, 1, 1) if fold else 1.0)).sum(dim=(1, 2, 3)) + 1.0)
    cw = pack_stem_split(w, (scale, shift) if fold else None)
    bias = cw.bias if fold else shift.float()
    w16, bias = cw.w16.numpy().copy(), bias.numpy().copy()
    assert w16.shape == (cout, R, 2, 32) and w16.dtype == np.float16 and bias.dtype == np.float32
    w16.setflags(write=False)
    bias.setflags(write=False)
    return w16, bias
