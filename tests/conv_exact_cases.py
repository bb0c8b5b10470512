"""The case table of the exact-arithmetic convolution tests (tests/conv_exact_ref.py): the smallest shapes at which each mechanism of
the convolution kernels exists.  The trigger of each comes from the code (csrc/conv_igemm_f16x3_plan.h, conv3x3_halo.hip,
conv1x1_stream.hip, conv3x3_thin.hip) and is asserted through the library's own queries by route_of() / assert_route(), so a case
cannot silently take another path.  Importing this file needs numpy only; the queries need the built library (host side only).

  group 1  implicit GEMM, every case under every tile id, splitk off: maps smaller than the filter footprint, images adjacent
           inside one M tile, M and Cout around the tile's BM / BN, strides, dilation, padding forms, filter shapes, the 7x7
           filter that finish_params16 refuses (R*S = 49 > 32: the BUF = false instantiation), the row-shared geometry
  group 2  epilogues on a ragged case (3 x 5 x 7, Cin 64, Cout 40 / 96)
  group 3  split-K through force_splits, k tiles no multiple of the splits, both reductions
  group 4  grouped, multi and mixed launches
  group 5  the halo kernel            group 6  the stream kernel            group 7  the thin kernels, tap and P form
  group 8  the f32 kernel and its tiles                                     group 9  ops.f16_terms(1) against model1
"""
import types

from conv_exact_ref import make_case

# tile id -> (BM, BN) (csrc/conv_igemm_f16x3_plan.h tile_form)
TILE_FORMS = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (128, 32), 6: (64, 128), 7: (32, 64), 8: (256, 64), 12: (64, 64)}
ALL_TILES = tuple(TILE_FORMS)
FUSED_REDUCE_TILES = tuple(t for t, (bm, bn) in TILE_FORMS.items() if bm <= 64 and bn <= 128)     # fused_reduce_form
F32_TILES = (0, 1, 2, 3, 4, 6)
_seed = [0]


def _fam(k):
    """(A, zero share) for a dot product of k terms so that S stays below 2^10 (asserted per case, never assumed): worst case
    (A + 2^-12)^2 k, and for long k the expected k (1 - z)^2 near 500"""
    if k <= 250:
        return 2, 0.0
    if k <= 1000:
        return 1, 0.0
    return 1, round(1.0 - (500.0 / k) ** 0.5, 2)


def _c(name, group, n, h, w, cin, cout, r, s=None, **kw):
    _seed[0] += 1
    k = r * (r if s is None else s) * cin
    a, z = _fam(k)
    if kw.get("family") == "g16":      # S < 2^6: one 32-channel block of a 1x1, or mostly zeros
        a, z = 1, (0.0 if k <= 48 else round(1.0 - (20.0 / k) ** 0.5, 2))
    kw.setdefault("A", a)
    kw.setdefault("zeros", z)
    return make_case(name, group, n, h, w, cin, cout, r, s, seed=_seed[0], **kw)


def _group1():
    cs = []
    T = dict(tiles=ALL_TILES)
    cs += [
        _c("map_1x1_under_3x3", 1, 2, 1, 1, 32, 16, 3, pad=1, **T),           # eight of nine taps are padding
        _c("map_1x2", 1, 1, 1, 2, 32, 16, 3, pad=1, **T),
        _c("map_2x1", 1, 1, 2, 1, 32, 16, 3, pad=1, **T),
        _c("five_images_3x3", 1, 5, 3, 3, 32, 24, 3, pad=1, **T),             # images adjacent inside one M tile
        _c("stride2_6x7", 1, 1, 6, 7, 32, 16, 3, stride=2, pad=1, **T),
        _c("stride2_7x6", 1, 2, 7, 6, 32, 16, 3, stride=2, pad=1, **T),
        _c("stride2_1x1", 1, 2, 5, 7, 32, 16, 1, stride=2, **T),
        _c("dil2_3x3map", 1, 2, 3, 3, 32, 16, 3, pad=2, dil=2, **T),          # footprint 5 >= map
        _c("dil2_5x5map", 1, 1, 5, 5, 32, 16, 3, pad=2, dil=2, **T),
        _c("valid_3x3_on_5x4", 1, 2, 5, 4, 32, 16, 3, pad=0, **T),
        _c("pad2_dil1", 1, 1, 4, 5, 32, 16, 3, pad=2, **T),                   # output larger than input
        _c("filter_1x3", 1, 2, 4, 5, 32, 16, 1, 3, pad=1, **T),
        _c("filter_3x1", 1, 2, 4, 5, 32, 16, 3, 1, pad=1, **T),
        _c("filter_5x5", 1, 1, 4, 6, 32, 16, 5, pad=2, **T),
        _c("filter_7x7_no_descriptors", 1, 2, 5, 6, 32, 24, 7, pad=3, **T),  # R*S = 49 > 32: finish_params16 says no
        _c("g16_1x1", 1, 2, 3, 5, 32, 16, 1, family="g16", **T),              # subnormal lo parts
        _c("g16_3x3", 1, 1, 4, 5, 32, 16, 3, pad=1, family="g16", **T),
        _c("two_blocks_3x3", 1, 2, 3, 4, 64, 16, 3, pad=1, **T),              # two 32-channel blocks: k tile order block outer, tap inner
    ]
    # the row-shared geometry (3x3 / stride 1 / pad 1, whole rows): rs_will_run's spare-slot test is (BM + 1) / W + 1 <= 8 waves - 2
    for wdt, hgt in ((1, 7), (2, 5), (4, 3), (5, 3), (129, 2)):
        cs.append(_c(f"rs_width_{wdt}", 1, 2, hgt, wdt, 32, 32, 3, pad=1, route="rs?", **T))
    for t, (bm, bn) in TILE_FORMS.items():
        for m in (bm - 1, bm, bm + 1):                                         # one 1x1 conv on a 1 x M map
            cs.append(_c(f"m_{m}_tile{t}", 1, 1, 1, m, 32, 8, 1, tiles=(t,)))
        for cout in sorted({1, 5, bn - 8, bn, bn + 8, bn + 1}):                # scalar and vector epilogues, ragged N tile
            cs.append(_c(f"cout_{cout}_tile{t}", 1, 1, 3, 4, 32, cout, 3, pad=1, tiles=(t,), relu_cols=cout))
    return cs


def _group2():
    cs = []
    E = dict(tiles=(0,) + ALL_TILES, pad=1)
    for cout in (40, 96):
        cs += [
            _c(f"no_bias_{cout}", 2, 3, 5, 7, 64, cout, 3, bias=False, **E),
            _c(f"res_f32_{cout}", 2, 3, 5, 7, 64, cout, 3, res="f32", relu_cols=cout, **E),
            _c(f"res_up_f32_{cout}", 2, 3, 5, 7, 64, cout, 3, res="up_f32", **E),                  # from (3, 4) with odd oh, ow
            _c(f"in_slice_{cout}", 2, 3, 5, 7, 64, cout, 3, in_wide=(160, 64), **E),
            _c(f"out_slice_f32_{cout}", 2, 3, 5, 7, 64, cout, 3, out_wide=(cout + 24, 8), relu_cols=cout, **E),
            _c(f"x_f32_plain_{cout}", 2, 3, 5, 7, 64, cout, 3, x_f32="plain", **E),
            _c(f"x_f32_gn_{cout}", 2, 3, 5, 7, 64, cout, 3, x_f32="gn", **E),
        ]
        for rc in sorted({0, 3, 8, cout}):
            cs.append(_c(f"relu_cols_{rc}_of_{cout}", 2, 3, 5, 7, 64, cout, 3, relu_cols=rc, res="f32", **E))
    cs += [
        _c("res_s32_96", 2, 3, 5, 7, 64, 96, 3, res="s32", relu_cols=96, **E),
        _c("res_up_s32_96", 2, 3, 5, 7, 64, 96, 3, res="up_s32", **E),
        _c("out_split_96", 2, 3, 5, 7, 64, 96, 3, out_split=True, relu_cols=96, **E),
        _c("out_split_res_s32_96", 2, 3, 5, 7, 64, 96, 3, out_split=True, res="s32", relu_cols=40, **E),
        _c("out_slice_s32_96", 2, 3, 5, 7, 64, 96, 3, out_split=True, out_wide=(160, 32), **E),
        _c("x_f32_gn_in_slice_96", 2, 3, 5, 7, 64, 96, 3, x_f32="gn", in_wide=(128, 32), **E),
    ]
    return cs


def _group3():
    cs = []
    # Cin 96 with 3x3: 27 k tiles; 2, 4, 7 and 16 splits leave ragged last chunks (14+13, 7+7+7+6, 4x6+3, 2x13+1)
    fused, separate = FUSED_REDUCE_TILES, tuple(t for t in ALL_TILES if t not in FUSED_REDUCE_TILES)      # (3, 6, 7, 12), (1, 2, 4, 8)
    for splits in (2, 4, 7, 16):
        S = dict(pad=1, splitk=True, force_splits=splits)
        cs += [
            _c(f"splitk{splits}_fused", 3, 1, 5, 7, 96, 64, 3, tiles=fused, **S),
            _c(f"splitk{splits}_fused_res_s32out", 3, 1, 5, 7, 96, 64, 3, tiles=fused, res="f32", out_split=True, relu_cols=64, **S),
            _c(f"splitk{splits}_reduce_kernel", 3, 1, 5, 7, 96, 64, 3, tiles=separate, **S),
            _c(f"splitk{splits}_reduce_kernel_res_s32out", 3, 1, 5, 7, 96, 64, 3, tiles=separate, res="s32", out_split=True,
               relu_cols=64, **S),
        ]
    # K = 9216 (288 k tiles) with the sparse A = 1 operands: 7 splits of 42 tiles (the last holds 36)
    cs.append(_c("k9216_sparse", 3, 1, 11, 11, 1024, 32, 3, pad=1, splitk=True, force_splits=7, tiles=(7, 1)))
    return cs


def _group4():
    """compound launches: lists of member cases (each member is also a plain convolution, which is its reference's shape)"""
    G = dict(tiles=(0,), pad=1, bias=True)
    grouped = [_c(f"grouped_{h}x{w}", 4, 2, h, w, 64, 40, 3, relu_cols=24, **G) for h, w in ((7, 9), (2, 1), (1, 1))]
    grouped_s32 = [_c(f"grouped_s32_{h}x{w}", 4, 2, h, w, 64, 64, 3, relu_cols=64, out_split=True, **G) for h, w in ((7, 9), (2, 1), (1, 1))]
    multi = [
        _c("multi_stride2_3x3", 4, 2, 7, 6, 64, 64, 3, stride=2, pad=1, relu_cols=64, out_split=True),
        _c("multi_1x1", 4, 2, 5, 3, 32, 96, 1, out_split=False, res="f32"),
        _c("multi_dilated", 4, 1, 5, 5, 32, 64, 3, pad=2, dil=2, out_split=True, res="s32", relu_cols=64),
    ]
    # the grouped launch that mixed_small_mask splits: 2 x (107 + 27 + 7) tiles of 128 rows x 2 column tiles = 564 on 512 slots, the
    # last round 52 <= 128 full: the members with at most half the rows of the largest take the 64-row form
    mixed = [_c(f"mixed_{i}_{h}x{w}", 4, 1, h, w, 32, 256, 3, relu_cols=256, out_split=True, **G)
             for i in range(2) for h, w in ((100, 136), (50, 68), (25, 34))]
    return dict(grouped=grouped, grouped_s32=grouped_s32, multi=multi, mixed=mixed)


def _group5():
    cs = []
    for n, hw, cins in ((128, 17, (32, 96)), (512, 16, (32,)), (512, 15, (32,))):
        for cin in cins:
            for res in (None, "s32"):
                cs.append(_c(f"halo_{n}x{hw}x{hw}_cin{cin}_{res or 'plain'}", 5, n, hw, hw, cin, 64, 3, pad=1, relu_cols=64,
                             out_split=True, res=res, route="halo", splitk=True))
    return cs


def _group6():
    S = dict(route="stream", splitk=True)
    return [
        _c("stream_plain", 6, 1, 257, 257, 64, 256, 1, **S),                  # m = 66049: the last 128-pixel tile holds one pixel
        _c("stream_up_s32", 6, 1, 257, 257, 128, 256, 1, res="up_s32", out_split=True, **S),     # residual from 129 x 129
        _c("stream_res_f32_relu", 6, 1, 257, 257, 64, 256, 1, res="f32", relu_cols=256, **S),
    ]


THIN_LEVELS = ((1, 2), (2, 1), (1, 167), (167, 1), (7, 9))


def _group7():
    """thin launches: (form, cout, relu_cols, members = one case per level, inputs are channel slices of a 256-channel stack)"""
    out = []
    for form in ("tap", "flat"):
        for cout, rc in ((1, 0), (5, 3), (16, 8)):
            if form == "flat" and cout > 5:
                continue                                                       # (the P form exists for Cout <= 5)
            members = [_c(f"thin_{form}_{cout}_{h}x{w}", 7, 2, h, w, 128, cout, 3, pad=1, relu_cols=rc, in_wide=(256, 128),
                          wseed=700 + cout) for h, w in THIN_LEVELS]
            out.append(types.SimpleNamespace(form=form, cout=cout, relu_cols=rc, members=members, affine=False))
    # the fused GroupNorm apply of the P form (grid-preserving tables): raw fp32 tower outputs, 256 channels, head channels 128..255
    members = [_c(f"thin_affine_{h}x{w}", 7, 8, h, w, 128, 5, 3, pad=1, relu_cols=4, in_wide=(256, 128), x_f32="gn", wseed=777)
               for h, w in ((13, 17), (7, 9))]
    out.append(types.SimpleNamespace(form="flat", cout=5, relu_cols=4, members=members, affine=True))
    return out


def _group8():
    cs = []
    T = dict(kind="f32", family="g6", tiles=F32_TILES)
    for cin in (4, 8, 12, 36):                                                 # the small-C path, chunks per tap
        cs.append(_c(f"f32_cin{cin}", 8, 2, 5, 7, cin, 24, 3, pad=1, relu_cols=10, **T))
    cs += [
        _c("f32_stem_7x7_s2", 8, 2, 13, 10, 4, 64, 7, stride=2, pad=3, relu_cols=64, **T),
        _c("f32_cin64_res", 8, 3, 5, 7, 64, 40, 3, pad=1, res="f32", relu_cols=40, **T),
        _c("f32_cin64_up", 8, 3, 5, 7, 64, 40, 1, res="up_f32", **T),
        _c("f32_gn_on_load", 8, 3, 5, 7, 64, 40, 3, pad=1, x_f32="gn", **T),
        _c("f32_gn_on_load_slice", 8, 2, 4, 3, 32, 33, 3, pad=1, x_f32="gn", in_wide=(96, 32), **T),
        _c("f32_map_1x1", 8, 2, 1, 1, 8, 5, 3, pad=1, **T),
        _c("f32_dil2", 8, 1, 5, 5, 16, 8, 3, pad=2, dil=2, **T),
    ]
    return cs


def _group9():
    T = dict(terms=1, tiles=(0, 1, 3))
    return [
        _c("terms1_five_images_3x3", 9, 5, 3, 3, 32, 24, 3, pad=1, **T),
        _c("terms1_stride2_6x7", 9, 1, 6, 7, 32, 16, 3, stride=2, pad=1, **T),
        _c("terms1_dil2_3x3map", 9, 2, 3, 3, 32, 16, 3, pad=2, dil=2, res="f32", relu_cols=8, **T),
    ]


GROUP1, GROUP2, GROUP3 = _group1(), _group2(), _group3()
GROUP4 = _group4()
GROUP5, GROUP6, GROUP7, GROUP8, GROUP9 = _group5(), _group6(), _group7(), _group8(), _group9()
EMULATED = GROUP1 + GROUP2 + GROUP3                       # what test_conv_exact_cpu.py walks with emulate()
SINGLE = EMULATED + GROUP5 + GROUP6 + GROUP8 + GROUP9     # plain conv2d_nhwc calls
MEMBERS = [m for ms in GROUP4.values() for m in ms] + [m for t in GROUP7 for m in t.members]
ALL_CASES = SINGLE + MEMBERS


# --------------------------------------------------------------------------------------------------------------------------
# the routers, through the library's own queries (host side only)
# --------------------------------------------------------------------------------------------------------------------------
def desc_of(c, tile, ops):
    from conv_exact_ref import out_size
    oh, ow = out_size(c)
    res_mode = 0 if c.res is None else (2 if c.res.startswith("up") else 1)
    rh, rw = ((oh + 1) // 2, (ow + 1) // 2) if res_mode == 2 else (0, 0)
    xs = 0 if not c.in_wide else (2 * c.in_wide[0] if c.kind == "f16x3" else c.in_wide[0])
    d = ops.make_conv_desc(c.n, c.h, c.w, c.cin, c.cout, c.r, c.s, c.stride, c.pad, c.dil, c.relu_cols, res_mode, rh, rw, 0, tile,
                           in_pix_stride=xs)
    d.out_split = 1 if c.out_split else 0
    d.res_split = 1 if c.res in ("s32", "up_s32") else 0
    d.terms = 1 if c.terms == 1 else 0
    d.splitk = (int(c.force_splits) if c.force_splits else 1) if c.splitk else -1
    return d


def route_of(c, tile, ops):
    """which kernel a conv2d_nhwc call of this case runs, from the library's queries: "halo", "stream", "rs" or "igemm", and
    the tile id of the implicit GEMM"""
    import ctypes as C
    lib = ops._lib.load()
    d = desc_of(c, tile, ops)
    picked = lib.hn_conv2d_f16x3_pick_tile(C.byref(d))
    if c.terms != 1 and lib.hn_conv2d_f16x3_uses_halo(C.byref(d), 1 if c.res else 0):
        return "halo", picked
    if lib.hn_conv2d_f16x3_uses_stream(C.byref(d)):
        return "stream", picked
    return ("rs" if lib.hn_conv2d_f16x3_uses_rs(C.byref(d)) else "igemm"), picked


def rs_expected(c, tile):
    """rs_will_run restated for the group-1 row-shared cases: the geometry, no split-K, a tile form that has the row-shared
    instantiation (two-stage 128-row tiles: 128x128, 128x64, 128x32) and (BM + 1) / W + 1 <= waves * 8 - 2 = 30"""
    bm = TILE_FORMS[tile][0]
    return tile in (1, 2, 4) and (bm + 1) // c.w + 1 <= 30


def assert_route(c, tile, ops):
    """the trigger of the case, asserted: a forced tile is the tile that runs; halo / stream cases take their kernel; the row-shared
    cases answer the query both ways; everything else stays on the per-tap implicit GEMM or the row-shared form of the same k order"""
    if c.kind != "f16x3":
        return None
    route, picked = route_of(c, tile, ops)
    if tile:
        assert picked == tile, (c.name, tile, picked)
    if c.route in ("halo", "stream"):
        assert route == c.route, (c.name, route)
    elif c.route == "rs?":
        assert (route == "rs") == rs_expected(c, tile), (c.name, tile, route)
    else:
        assert route in ("igemm", "rs"), (c.name, route)
    return route
