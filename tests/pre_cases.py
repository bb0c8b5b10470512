"""Seeded frames for the preprocess tests (tests/pre_ref.py): small geometries at every branch of preprocess_run's dispatch
(csrc/fcos_post.hip) and at the limits of the tiled kernel's LDS patch.  Each case's rule and bound are computed once
(reference()) and shared by the tests."""
import functools
from dataclasses import dataclass

import numpy as np

import pre_ref as pr

F = np.float32
MEAN = (0.485, 0.456, 0.406)      # hn_amd.fcos_engine.IMAGE_MEAN / IMAGE_STD
STD = (0.229, 0.224, 0.225)
BORDERS = (0, 1, 3)
TH, TW = 8, 128                   # kPreTH, kPreTW: the tiled kernel's tile of the bordered canvas


@dataclass(frozen=True)
class Case:
    name: str
    geom: tuple            # (h, w, oh, ow, ph, pw)
    form: str              # what fcos_preprocess_split launches: "t8" = tiled <8, 96>, "t16" = tiled <16, 160>, "pp" = per pixel
    why: str
    n: int = 1
    kind: str = "uniform"  # uniform in [0, 1) | const (one value per channel) | corners (one bright pixel in each corner)


CASES = (
    Case("15x219-21x300", (15, 219, 21, 300, 32, 320), "t8", "need_r = 8.0, need_c = 95.71: the last geometry of <8, 96>; 7 x 95 patch", n=3),
    Case("10x186-14x254", (10, 186, 14, 254, 14, 254), "t8", "need_r = 8.0, need_c = 96.0 exactly; no padding; ow ends inside tile 1"),
    Case("5x93-7x127", (5, 93, 7, 127, 8, 128), "t8", "need_c = 96.0; the image's edges lie inside the tiles that hold the border"),
    Case("15x220-21x300", (15, 220, 21, 300, 32, 320), "t16", "need_c = 96.13: one source column more than the row above"),
    Case("16x219-21x300", (16, 219, 21, 300, 32, 320), "t16", "need_r = 8.33: one source row more; an 8-row patch in <16, 160>"),
    Case("13x157-7x127", (13, 157, 7, 127, 8, 128), "t16", "downscale 1.86 / 1.24: need_r = 16.0, need_c = 160.0 exactly; 13 x 157 patch"),
    Case("40x330-33x270", (40, 330, 33, 270, 64, 288), "t16", "downscale 1.21 / 1.22: 11 x 158 patch of 16 x 160", n=3),
    Case("40x330-33x270-corners", (40, 330, 33, 270, 64, 288), "t16", "an index off by one moves a bright corner", kind="corners"),
    Case("26x371-14x300", (26, 371, 14, 300, 32, 320), "pp", "need_c = 160.06: past the patch, the per-pixel kernel", n=2),
    Case("3x2-41x259", (3, 2, 41, 259, 64, 288), "t8", "fewer source pixels than one tile: a 3 x 2 patch"),
    Case("1x1-9x130", (1, 1, 9, 130, 9, 131), "pp", "one source pixel; odd canvas width: per pixel although need_r = 3.8, need_c = 4.0", n=3),
    Case("37x53-97x139", (37, 53, 97, 139, 97, 139), "pp", "odd canvas width at an upscale of <8, 96>'s range", n=3),
    Case("13x157-7x127-odd", (13, 157, 7, 127, 9, 131), "pp", "odd canvas width at a downscale of <16, 160>'s range", n=2),
    Case("64x64-64x64", (64, 64, 64, 64, 64, 64), "t16", "identity: every weight is (1, 0)", n=2),
    Case("30x40-50x66", (30, 40, 50, 66, 64, 96), "t8", "oh < ph and ow < pw with both edges inside tile 0 and row tile 6", n=3),
    Case("30x40-50x66-const", (30, 40, 50, 66, 64, 96), "t8", "a constant image", kind="const"),
    Case("30x40-50x66-corners", (30, 40, 50, 66, 64, 96), "t8", "an index off by one moves a bright corner", kind="corners"),
)
BY_NAME = {c.name: c for c in CASES}

# fcos_preprocess_list: three images of different sizes on one canvas -- upscaled, downscaled, 1 x 1
LIST_GEOM = ((37, 53, 97, 139), (120, 160, 80, 106), (1, 1, 9, 130))
LIST_CANVAS = (128, 160)

# where ATen's CPU bilinear kernel agrees bit for bit with the kernels' order (it picks other code paths at other shapes, so
# no test asserts equality with F.interpolate elsewhere): (h, w, oh, ow)
ATEN_AGREES = ((480, 640, 800, 1066), (120, 160, 80, 106), (37, 53, 97, 139), (9, 300, 8, 130), (2, 3, 8, 128), (64, 64, 64, 64))

# the case on which each mutant of pre_ref.mutants() must fail
MUTANT_CASE = {"no_half": "30x40-50x66", "no_clamp0": "30x40-50x66-corners", "no_clamp_i1": "30x40-50x66-corners",
               "scale_inverted": "40x330-33x270", "swap_ohow": "30x40-50x66", "pad_before_normalise": "30x40-50x66",
               "border_off_by_one": "30x40-50x66-corners", "lo_from_rounded": "30x40-50x66"}


def form_of(h, w, oh, ow, ph, pw, border=3, n=1, generic=False):
    """preprocess_run's dispatch for the dense split form, restated in fp32 as the host computes it"""
    scale_h, scale_w = F(h) / F(oh), F(w) / F(ow)
    need_r = F(TH - 1) * scale_h + F(3.0)
    need_c = F(TW - 1) * scale_w + F(3.0)
    assert need_r.dtype == F and need_c.dtype == F
    if generic or n > 65535 or need_r > F(16.0) or need_c > F(160.0) or (pw + 2 * border) % 2:
        return "pp"
    return "t8" if need_r <= F(8.0) and need_c <= F(96.0) else "t16"


def patch_of(h, w, oh, ow, ph, pw, border):
    """(rows, columns) of the largest source patch any tile of the tiled kernel loads, with the kernel's own index arithmetic"""
    y0, y1, _, _ = pr.src_index(h, oh)
    x0, x1, _, _ = pr.src_index(w, ow)
    rows = cols = 0
    for cy0 in range(0, ph + 2 * border, TH):
        lo, hi = max(cy0 - border, 0), min(cy0 - border + TH, oh) - 1
        if lo <= hi:
            rows = max(rows, int(y1[hi] - y0[lo] + 1))
    for cx0 in range(0, pw + 2 * border, TW):
        lo, hi = max(cx0 - border, 0), min(cx0 - border + TW, ow) - 1
        if lo <= hi:
            cols = max(cols, int(x1[hi] - x0[lo] + 1))
    return rows, cols


def _image(kind, rng, n, h, w):
    if kind == "uniform":
        return rng.random((n, 3, h, w), dtype=F)
    if kind == "const":
        return np.broadcast_to(np.asarray((0.2, 0.5, 0.9), F).reshape(1, 3, 1, 1), (n, 3, h, w)).copy()
    assert kind == "corners"
    x = np.zeros((n, 3, h, w), F)
    x[:, :, 0, 0], x[:, :, 0, -1], x[:, :, -1, 0], x[:, :, -1, -1] = F(1.0), F(0.75), F(0.5), F(0.25)
    return x


@functools.lru_cache(maxsize=None)
def make(name):
    """images [n, 3, h, w] as a read-only fp32 numpy array"""
    c = BY_NAME[name]
    rng = np.random.default_rng(2000 + [x.name for x in CASES].index(name))
    x = _image(c.kind, rng, c.n, c.geom[0], c.geom[1])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rule, bound) of the case's fp32 canvas, computed once"""
    c = BY_NAME[name]
    out = pr.rule64(make(name), *c.geom[2:], MEAN, STD)
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated(name):
    """the fp32 emulation's canvas of the case, computed once"""
    c = BY_NAME[name]
    out = pr.emulate(make(name), *c.geom[2:], MEAN, STD)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_list():
    """the three images of LIST_GEOM, each [3, h, w]"""
    rng = np.random.default_rng(2900)
    out = tuple(rng.random((3, h, w), dtype=F) for h, w, _, _ in LIST_GEOM)
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def list_reference():
    """(rule, bound, emulation) of the list's canvas: every image resized on its own into the top-left corner"""
    ph, pw = LIST_CANVAS
    parts = [(pr.rule64(x[None], oh, ow, ph, pw, MEAN, STD), pr.emulate(x[None], oh, ow, ph, pw, MEAN, STD))
             for x, (_, _, oh, ow) in zip(make_list(), LIST_GEOM)]
    out = (np.concatenate([p[0][0] for p in parts]), np.concatenate([p[0][1] for p in parts]), np.concatenate([p[1] for p in parts]))
    for t in out:
        t.setflags(write=False)
    return out
