"""The table of planted launches that pins the f16x3 range contract at every split producer (the rule: tests/range_ref.py).  The
shapes are those of tests/conv_exact_cases.py (looked up there by name, so the mechanism each one reaches stays the one that table
derives), tests/graph_cases.py's hand-built neighbour tests/range_ref.hand_graph, and tests/pre_cases.py's identity resize.
Importing this file needs numpy only.

  CONV       implicit GEMM under every tile id (ragged 3 x 5 x 7, Cin 64, Cout 96; 1x1 maps of BM - 1, BM, BM + 1 rows), both terms
             modes, the row-shared form, the scalar epilogue, ReLU columns, fp32 and S32 residuals, an output slice
  SPLITK     2 and 7 forced splits, fused reduction (tiles 3, 6, 7, 12) and reduce kernel (1, 2, 4, 8), cancelling partial sums
  COMPOUND   grouped, multi and mixed launches: a plant in the first member, in the last, in the 64-row members of `mixed`
  HALO, STREAM                the direct 3x3 kernel (plain and S32 residual), the streaming 1x1 (the last tile's single pixel)
Every launch carries the words the table claims (`want`); tests/test_range_cpu.py holds them against the rule.
"""
import types

import numpy as np

import conv_exact_cases as cc
import range_ref as rr

F = np.float32
CLEAN, ACT = [0, 0, 0, 0], [1, 0, 0, 0]
INPUT_FINITE, INPUT_NONFINITE = [0, 1, 0, 0], [0, 0, 1, 0]
NEXT, MAX, EPS = rr.NEXT, rr.F16_MAX, rr.EPS
# waves along M of every tile form (csrc/conv_igemm_f16x3.hip, hn_igemm_conv16_run's switch): a wave owns BM / WM rows
TILE_WM = {1: 2, 2: 2, 3: 2, 4: 4, 6: 2, 7: 1, 8: 4, 12: 2}
_BY_NAME = {c.name: c for c in cc.ALL_CASES}


def derive(name, suffix="", **kw):
    """a conv_exact case by name, with epilogue switches of this table"""
    c = types.SimpleNamespace(**vars(_BY_NAME[name]))
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    c.name = name + suffix
    return c


def tile_of(c, tile):
    """(BM, BN, WM) the positions of a launch are derived from; tile 0 (the heuristic's pick): the 64 x 64 form's"""
    t = tile if tile else 3
    return cc.TILE_FORMS[t] + (TILE_WM[t],)


def positions(m, cout, bm, bn, wm):
    rows = sorted(r for r in {0, 1, 15, 16, bm // wm - 1, bm // wm, bm - 1, bm, (m - 1) // bm * bm, m - 1} if 0 <= r < m)
    cols = sorted(c for c in {0, 7, 8, 31, 32, bn - 1, bn, cout - 1} if 0 <= c < cout)
    return rows, cols


def _sign(c, co):
    """+ inside the ReLU columns (a negative value would be turned into 0), - behind them"""
    return 1.0 if co < c.relu_cols else -1.0


def single(c, tile, m, co, ci=None, tag=""):
    """one product of +-65504 moved to the next float by bias[co] = +-2^-8: word 0"""
    s = _sign(c, co)
    ci = (7 * m + 3 * co) % c.cin if ci is None else ci
    return rr.launch(f"{c.name}{tag} tile{tile} plant({m},{co})", c, tile, [rr.plant(m, co, ci, rr.X1, s * rr.W1)], {co: s * EPS},
                     want=ACT, bm=tile_of(c, tile)[0])


def control(c, tile, rows, cols, tag=""):
    """+-65504 exactly at every position at once, no bias: nothing is set"""
    plants = [rr.plant(m, co, 0, rr.X1, _sign(c, co) * rr.W1) for m in rows for co in cols]
    return rr.launch(f"{c.name}{tag} tile{tile} control", c, tile, plants, want=CLEAN, bm=tile_of(c, tile)[0])


def table(c, tile, tag=""):
    """the single-plant launches of every position and the multi-hot control of one (case, tile)"""
    rows, cols = positions(rr.rows_of(c), c.cout, *tile_of(c, tile))
    return [single(c, tile, m, co, tag=tag) for m in rows for co in cols] + [control(c, tile, rows, cols, tag)]


# --------------------------------------------------------------------------------------------------------------------------
# implicit GEMM
# --------------------------------------------------------------------------------------------------------------------------
RAGGED = derive("out_split_96", "[range]", relu_cols=40)                       # 3 x 5 x 7, Cin 64, Cout 96: M = 105
RAGGED_F32 = derive("out_split_96", "[range,f32 out]", relu_cols=40, out_split=False)
RAGGED_RES_F32 = derive("out_split_res_s32_96", "[range,res f32]", res="f32")    # relu_cols = 40
RAGGED_RES_S32 = derive("out_split_res_s32_96", "[range]")
RAGGED_SLICE = derive("out_slice_s32_96", "[range]")                           # channels [32, 128) of a 160-channel tensor


def m_case(rows, tile):
    """the 1 x M map of the exact table with an S32 output (Cout 32: the narrowest one the format has)"""
    return derive(f"m_{rows}_tile{tile}", "[range]", cout=32, out_split=True)


def igemm(tile, terms=3):
    """every launch of the implicit GEMM under one tile id and one terms mode"""
    tag = "" if terms == 3 else "[1 term]"
    c = RAGGED if terms == 3 else derive("out_split_96", "[range]", relu_cols=40, terms=1)
    out = table(c, tile, tag)
    bm = cc.TILE_FORMS[tile][0]
    for m in (bm - 1, bm, bm + 1):
        mc = m_case(m, tile)
        if terms == 1:
            mc.terms = 1
        out += table(mc, tile, tag)
    return out


def relu_launches(tile):
    """-(65504 + 2^-8) in the last ReLU column is stored as 0 and sets nothing; in the column behind it, word 0"""
    c, m = RAGGED, rr.rows_of(RAGGED) - 1
    mk = lambda co, want: rr.launch(f"{c.name} tile{tile} -next in column {co}", c, tile, [rr.plant(m, co, 33, rr.X1, -rr.W1)],
                                    {co: -EPS}, want=want, bm=tile_of(c, tile)[0])
    return [mk(c.relu_cols - 1, CLEAN), mk(c.relu_cols, ACT), mk(0, CLEAN), mk(c.cout - 1, ACT)]


def residual_launches(tile):
    """fp32 residual: a one-hot that carries the value itself; S32 residual: 40000 + 797 * 32 = 65504, 40000 + 798 * 32 = 65536"""
    out = []
    bm = tile_of(RAGGED, tile)[0]
    last = (rr.rows_of(RAGGED) - 1, RAGGED.cout - 1)                           # behind the ReLU columns
    for (m, co) in ((0, 0), last):
        for v, want in ((MAX, CLEAN), (NEXT, ACT), (np.nan, ACT), (np.inf, ACT), (-np.inf, ACT if co >= 40 else CLEAN),
                        (-NEXT, ACT if co >= 40 else CLEAN)):
            out.append(rr.launch(f"{RAGGED_RES_F32.name} tile{tile} res({m},{co}) = {v}", RAGGED_RES_F32, tile, res={(m, co): v},
                                 want=want, bm=bm))
        for xv, want in ((797.0, CLEAN), (798.0, ACT)):
            out.append(rr.launch(f"{RAGGED_RES_S32.name} tile{tile} 40000 + {xv} * 32 at ({m},{co})", RAGGED_RES_S32, tile,
                                 [rr.plant(m, co, 5, xv, rr.W1)], res={(m, co): 40000.0}, want=want, bm=bm))
    return out


def f32_output_launches(tile):
    """the same overflow stored as fp32 is not a converted value: nothing is set"""
    c = RAGGED_F32
    m, co = rr.rows_of(c) - 1, c.cout - 1
    return [rr.launch(f"{c.name} tile{tile} plant({m},{co})", c, tile, [rr.plant(m, co, 9, rr.X1, -rr.W1)], {co: -EPS}, want=CLEAN,
                      bm=tile_of(c, tile)[0])]


def slice_launches(tile):
    """the output is a channel slice of a tensor whose other channels hold NaN: they are not this launch's values"""
    c = RAGGED_SLICE
    m = rr.rows_of(c) - 1
    return [rr.launch(f"{c.name} tile{tile} clean slice in a NaN arena", c, tile, [rr.plant(m, 0, 0), rr.plant(m, c.cout - 1, 0)],
                      want=CLEAN, bm=tile_of(c, tile)[0], out_nan_arena=True),
            rr.launch(f"{c.name} tile{tile} plant in a NaN arena", c, tile, [rr.plant(m, c.cout - 1, 0)], {c.cout - 1: EPS},
                      want=ACT, bm=tile_of(c, tile)[0], out_nan_arena=True)]


RS_CASES = [derive(f"rs_width_{w}", "[range]", out_split=True) for w in (1, 2, 4, 5, 129)]


def row_shared(tile):
    return [l for c in RS_CASES for l in table(c, tile)]


# --------------------------------------------------------------------------------------------------------------------------
# split-K: Cin 96, 3x3 -- 27 k tiles, the block outer and the tap inner: the centre taps of blocks 0 and 2 lie in different chunks
# --------------------------------------------------------------------------------------------------------------------------
def splitk_case(splits, kind):
    return derive(f"splitk{splits}_{kind}", "[range]", out_split=True, relu_cols=32)


def splitk(splits, kind, tile):
    c = splitk_case(splits, kind)
    assert tile in c.tiles and rr.split_of(c, 0)[0] != rr.split_of(c, 64)[0]
    bm, bn, wm = tile_of(c, tile)
    rows, cols = positions(rr.rows_of(c), c.cout, bm, bn, wm)
    out = [single(c, tile, m, co, ci=(0, 37, 95)[(m + co) % 3]) for m in rows for co in cols]
    out.append(control(c, tile, rows, cols))
    m, co = rr.rows_of(c) - 1, c.cout - 1
    for neg, want in ((2050.0, CLEAN), (2048.0, ACT)):        # 2^17 - (2^16 + 64) = 65472; 2^17 - 2^16 = 65536
        out.append(rr.launch(f"{c.name} tile{tile} 2^17 - {neg} * 32", c, tile,
                             [rr.plant(m, co, 3, 4096.0, rr.W1), rr.plant(m, co, 64 + 3, neg, -rr.W1)], want=want, bm=bm))
    return out


# --------------------------------------------------------------------------------------------------------------------------
# compound launches: lists of member launches (one ledger, one block of words)
# --------------------------------------------------------------------------------------------------------------------------
def _members(kind):
    ms = cc.GROUP4[kind]
    return [derive(m.name, "[range]") for m in ms]


def compound(kind):
    """-> [(name, [member launches], want)]: a plant in the first member and in the last (mixed: in every 64-row member too), in
    the fp32-output member of `multi` (nothing is set), and the control with every member multi-hot"""
    ms = _members(kind)
    tile = 1 if kind == "mixed" else 0
    out = []

    def group(name, planted, want):
        ls = []
        for i, c in enumerate(ms):
            if i in planted:
                ls.append(planted[i])
            else:
                ls.append(rr.launch(f"{c.name} quiet", c, tile, want=None, bm=tile_of(c, tile)[0]))
        out.append((f"{kind}: {name}", ls, want))

    small = [i for i, c in enumerate(ms) if 2 * rr.rows_of(c) <= max(rr.rows_of(x) for x in ms)] if kind == "mixed" else []
    for i in sorted({0, len(ms) - 1} | set(small)):
        c = ms[i]
        if not c.out_split:
            continue
        bm, bn, wm = (64, 128, 2) if i in small else tile_of(c, tile)
        rows, cols = positions(rr.rows_of(c), c.cout, bm, bn, wm)
        for m, co in ((rows[0], cols[0]), (rows[-1], cols[-1]), (rows[len(rows) // 2], cols[len(cols) // 2])):
            group(f"member {i} plant({m},{co})", {i: single(c, tile, m, co)}, ACT)
    for i, c in enumerate(ms):
        if not c.out_split:
            m, co = rr.rows_of(c) - 1, c.cout - 1
            group(f"fp32 member {i} plant({m},{co})",
                  {i: rr.launch(f"{c.name} plant", c, tile, [rr.plant(m, co, 1, rr.X1, -rr.W1)], {co: -EPS}, want=CLEAN)}, CLEAN)
    ctl = {}
    for i, c in enumerate(ms):
        bm, bn, wm = (64, 128, 2) if i in small else tile_of(c, tile)
        rows, cols = positions(rr.rows_of(c), c.cout, bm, bn, wm)
        ctl[i] = control(c, tile, rows, cols)
    group("control", ctl, CLEAN)
    return out


# --------------------------------------------------------------------------------------------------------------------------
# halo and stream
# --------------------------------------------------------------------------------------------------------------------------
HALO = [derive("halo_128x17x17_cin32_plain", "[range]"), derive("halo_128x17x17_cin32_s32", "[range]")]
STREAM = derive("stream_up_s32", "[range]")


def halo(c):
    """the direct kernel owns 16 x 16 output tiles of an image: positions on both sides of a tile edge and of an image"""
    hw = c.h * c.w
    rows = sorted({0, 15, 16, 17 * 15 + 16, 17 * 16, hw - 1, hw, rr.rows_of(c) - hw, rr.rows_of(c) - 1})
    cols = [0, 7, 8, 31, 32, 63]
    out = [single(c, 0, m, co) for m in rows for co in cols] + [control(c, 0, rows, cols)]
    if c.res:
        m, co = rr.rows_of(c) - 1, c.cout - 1
        for xv, want in ((797.0, CLEAN), (798.0, ACT)):
            out.append(rr.launch(f"{c.name} 40000 + {xv} * 32", c, 0, [rr.plant(m, co, 5, xv, rr.W1)], res={(m, co): 40000.0}, want=want))
    return out


def stream():
    """m = 66049: the last 128-pixel tile holds one pixel; the up-sampled S32 residual is read at (128, 128) of 129 x 129"""
    c = STREAM
    m_last = rr.rows_of(c) - 1
    assert m_last % 128 == 0
    rows, cols = [0, 127, 128, m_last - 1, m_last], [0, 7, 8, 255]
    out = [single(c, 0, m, co) for m in rows for co in cols] + [control(c, 0, rows, cols)]
    for xv, want in ((797.0, CLEAN), (798.0, ACT)):
        out.append(rr.launch(f"{c.name} 40000 + {xv} * 32 in the last tile", c, 0, [rr.plant(m_last, 255, 5, xv, rr.W1)],
                             res={(m_last, 255): 40000.0}, want=want))
    return out


def every_conv_launch():
    """(for the CPU test) every single-convolution launch of the table"""
    out = []
    for t in cc.ALL_TILES:
        out += igemm(t) + igemm(t, terms=1) + relu_launches(t) + residual_launches(t) + f32_output_launches(t) + slice_launches(t)
        out += row_shared(t)
    for splits in (2, 7):
        for kind, tiles in (("fused", cc.FUSED_REDUCE_TILES), ("reduce_kernel", tuple(t for t in cc.ALL_TILES if t not in cc.FUSED_REDUCE_TILES))):
            for t in tiles:
                out += splitk(splits, kind, t)
    for c in HALO:
        out += halo(c)
    return out + stream()


# --------------------------------------------------------------------------------------------------------------------------
# the lifter's kernels
# --------------------------------------------------------------------------------------------------------------------------
HALF_NEXT = F(float(NEXT) / 2)          # 32752 + 2^-9: twice it is the first float beyond the range, and its fp16 hi is finite


def fused_basis():
    """-> [(name, fin, vertex, value, part that leaves the range or None)] for the fused kernel's in-kernel basis on hand_graph():
    the planted x sits at (sample, vertex, feature) for the first and the last sample and feature"""
    out = []
    for fin in (4, 256):
        out += [
            (f"fin{fin} x = 40000 under L = 2: a1 = 80000", fin, 1, 40000.0, "a1"),
            (f"fin{fin} x = next / 2 under L = 2: a1 = next", fin, 1, float(HALF_NEXT), "a1"),
            (f"fin{fin} x = 32752 under L = 2: a1 = 65504", fin, 1, 32752.0, None),
            (f"fin{fin} x = 40000 two steps up: a2 = 80000", fin, 3, 40000.0, "a2"),
            (f"fin{fin} x = next / 2 two steps up: a2 = next", fin, 3, float(HALF_NEXT), "a2"),
            (f"fin{fin} x = 32752 two steps up: a2 = 65504", fin, 3, 32752.0, None),
            (f"fin{fin} x = next where 2 L L - I has no diagonal: a0", fin, 6, float(NEXT), "a0"),
            (f"fin{fin} x = 65504 where 2 L L - I has no diagonal", fin, 6, 65504.0, None),
            (f"fin{fin} x = -next at an isolated vertex: a0 and a2", fin, 9, -float(NEXT), "a0"),
        ]
    return out
