"""The ResNet stem chain on the GPU against tests/stem_ref.py at the shapes of tests/stem_cases.py: stem_image_kernel bit for bit,
the stem form of the f16x3 implicit GEMM and conv_stem_pool_direct_kernel inside the worst-case fp32 accumulation bound of the
float64 rule (and the fused form bit-identical to conv + pooling), maxpool_s32_kernel on maps smaller than its window, the range
contract, the footprint of a NaN pixel and the refusals.  Every reference is computed once per (case, kind) and shared; the
bound ratios are printed."""
import functools

import numpy as np
import pytest
import torch

import stem_cases as sc
import stem_ref as sr
from pre_ref import split

pytestmark = pytest.mark.gpu

F, D, H = np.float32, np.float64, np.float16
NAN16 = 0x7e00


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the cached operands are read-only)


def _bits(t):
    """fp16 tensor / array -> uint16 numpy"""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint16)


def _nan_filled(shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float16)


@functools.lru_cache(maxsize=None)
def _operands(name, kind, cout=sc.COUT):
    """(planes, w16, bias) on the host (fp16, fp16, fp32), read-only"""
    planes = split(sc.image(name, kind), sc.PAD)
    planes.setflags(write=False)
    return (planes,) + sc.filters(name, kind, cout)


@functools.lru_cache(maxsize=None)
def _rule(name, kind, terms=3, cout=sc.COUT):
    """(rule before the ReLU, S) in float64"""
    y, s = sr.rule_conv(*_operands(name, kind, cout), terms)
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s


def _words(block):
    from hn_amd import ops
    return ops.range_check_collect(block).cpu().tolist()


# ---------------------------------------------------------------------------------------------------------------- stem image
def _raw(n, h, w, seed):
    return (np.random.default_rng(seed).standard_normal((n, h, w, 4)) * 3).astype(F)


def _check_image(x, border, valid=None):
    """one launch into a NaN-filled output under a range scope against rule_image: planes in every bit (so every element was
    written), valid, range words"""
    from hn_amd import ops
    n, h, w, _ = x.shape
    want, want_valid, want_words = sr.rule_image(x, border, valid)
    out = _nan_filled((2, n, h + 2 * border, w + 2 * border, 4))
    v = None if valid is None else _dev(np.asarray(valid, np.int32))
    block = torch.zeros((4,), device="cuda", dtype=torch.int32)
    with ops.range_scope(block):
        got = ops.stem_image_nhwc4(_dev(x), border=border, out=out, valid=v)
        words = _words(block)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == want.shape
    g, r = _bits(got), _bits(want)
    nan = np.isnan(want.astype(F))
    assert np.array_equal(np.isnan(got.cpu().numpy().astype(F)), nan)            # (a NaN's payload is not part of the rule)
    assert np.array_equal(g[~nan], r[~nan])
    if valid is not None:
        assert v.cpu().numpy().tolist() == want_valid.tolist()
    assert words == want_words
    return got


@pytest.mark.parametrize("border", [0, 3, 4])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 5, 7), (3, 176, 176)])
def test_stem_image_is_the_exact_split_with_a_zero_border(n, h, w, border):
    x = _raw(n, h, w, 100 + h)
    x.flat[::7] *= F(1e-3)                  # lo parts in fp16's subnormal range too
    got = _check_image(x, border)
    if border:
        b = got.cpu().numpy()
        assert not b[:, :, :border].any() and not b[:, :, -border:].any()
        assert not b[:, :, :, :border].any() and not b[:, :, :, -border:].any()


def test_stem_image_grid_stride_loop_takes_a_second_lap():
    """130 crops of 176 x 176 with a border of 3 are 4 306 120 bordered pixels, more than the grid cap of 16384 x 256 threads:
    the smallest A2J batch whose tail is written by the loop's second lap"""
    n, h, w, border = 130, 176, 176, 3
    assert n * (h + 2 * border) * (w + 2 * border) > 16384 * 256 > (n - 4) * (h + 2 * border) * (w + 2 * border)
    x = np.random.default_rng(130).standard_normal((n, h, w, 4), dtype=F)
    x[n - 1, h - 1, w - 1, 3] = F(-2.5)
    got = _check_image(x, border)
    assert float(got[0, n - 1, h + 2, w + 2, 3]) == -2.5


def test_stem_image_valid_rows_and_non_finite_pixels():
    """valid 1 -> 2 for an image with a NaN / +inf / -inf pixel, 0 stays 0, a clean image keeps its 1; the pixel is stored as 0
    (in images with valid == 0 as well); range word 2 is set.  A finite 3e38 passes: hi = inf, range word 1.  Without `valid`
    the NaN passes through."""
    x = _raw(5, 5, 7, 7)
    x[0, 1, 2, 0] = np.nan                   # valid 0
    x[1, 4, 0, 3], x[1, 0, 6, 1] = np.inf, -np.inf
    x[3, 2, 3, 2] = np.nan
    x[4, 0, 0, 0] = -np.inf                  # valid 0
    for border in (0, 3):
        got = _check_image(x, border, valid=[0, 1, 1, 1, 0])        # -> [0, 2, 1, 2, 0], words [0, 0, 1, 0]
        assert torch.isfinite(got.float()).all()
        assert sr.rule_image(x, border, [0, 1, 1, 1, 0])[1].tolist() == [0, 2, 1, 2, 0]
        got = _check_image(x, border)                                # no valid: NaN and inf pass through
        assert int(torch.isnan(got[0].float()).sum()) == 2 and int(torch.isinf(got[0].float()).sum()) == 3
    big = _raw(2, 3, 4, 8)
    big[1, 2, 1, 1] = F(3e38)
    got = _check_image(big, 3, valid=[1, 1])                         # finite: valid stays 1, word 1 alone
    assert float(got[0, 1, 5, 4, 1]) == float("inf")
    assert sr.rule_image(big, 3, [1, 1])[2] == [0, 1, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ stem conv
def _s32_of(y32):
    """fp32 [n, h, w, c] (numpy) -> the S32 bits of its exact split"""
    return _bits(sr.to_s32(*sr.split_f32(y32)))


def _conv_case(name, kind, cout, relu):
    from hn_amd import ops
    planes, w16, bias = _operands(name, kind, cout)
    x16, w, b = _dev(planes), _dev(w16), _dev(bias)
    y, s = _rule(name, kind, 3, cout)
    got = ops.conv_stem_split(x16, w, b, cout, relu=relu, out_split=False)
    assert tuple(got.shape) == y.shape and got.dtype == torch.float32
    g = got.cpu().numpy()
    ratio = sr.check_conv(g, np.maximum(y, 0.0) if relu else y, s, sr.chain(3))
    s32 = ops.conv_stem_split(x16, w, b, cout, relu=relu, out_split=True)
    assert np.array_equal(_bits(s32), _s32_of(g)), (name, kind, cout, relu)
    return ratio


@pytest.mark.parametrize("name", sc.NAMES)
def test_stem_conv_is_inside_the_fp32_accumulation_bound(name):
    """ops.conv_stem_split, fp32 output, against rule_conv on every kind, with and without the ReLU: |err| <= 673 U S.  The S32
    output of the same call is the exact split of the fp32 one."""
    worst = 0.0
    for kind in sc.KINDS:
        for relu in (True, False):
            ratio = _conv_case(name, kind, sc.COUT, relu)
            print(f"stem conv {name} {kind} relu={int(relu)}: max |err| / bound = {ratio:.4f}")
            assert ratio <= 1.0, (name, kind, relu)
            worst = max(worst, ratio)
    print(f"stem conv {name}: worst {worst:.4f}")


@pytest.mark.parametrize("cout", [32, 64, 128])
@pytest.mark.parametrize("name", ["4x5", "15x17", "17x25"])
def test_stem_conv_column_tiles(name, cout):
    """cout <= 32, <= 64 and above take the 128x32, 128x64 and 128x128 tiles of stem16_run"""
    for kind, relu in (("normal", False), ("depth", True)):
        ratio = _conv_case(name, kind, cout, relu)
        print(f"stem conv {name} {kind} cout={cout} relu={int(relu)}: max |err| / bound = {ratio:.4f}")
        assert ratio <= 1.0, (name, kind, cout)


# ---------------------------------------------------------------------------------------------------------- fused direct kernel
def _fused(name, kind):
    """(pooled S32 of the fused kernel, its values fp32 numpy); the output was NaN-filled"""
    from hn_amd import ops
    c = sc.BY_NAME[name]
    _, _, _, _, poh, pow_, _ = sc.geometry(c)
    planes, w16, bias = _operands(name, kind)
    out = _nan_filled((c.n, poh, pow_, 2, 2, 32))
    got = ops.conv_stem_pool_split(_dev(planes), _dev(w16), _dev(bias), out=out)
    assert got.data_ptr() == out.data_ptr()
    return got, ops.from_split(got).cpu().numpy()


@pytest.mark.parametrize("name", sc.NAMES)
def test_fused_stem_pool_values_planes_and_coverage(name):
    """conv_stem_pool_direct_kernel on every kind: values inside the bound of rule_pool(relu(rule_conv)); planes bit-identical
    to conv_stem_split + maxpool3x3s2_nhwc; every element of a NaN-filled output written; two runs equal; all-negative conv
    outputs pool to planes that are exactly zero.  (The values are read back through from_split, so they carry what the S32
    split itself loses, 2^-22 |v| + 2^-25: the bound is NOT widened for it -- 2^-22 |v| is 1 / 168 of it, and the quantum of a
    subnormal lo shows as the larger ratios of the `small` kind.)"""
    from hn_amd import ops
    for kind in sc.KINDS:
        planes, w16, bias = _operands(name, kind)
        y, s = _rule(name, kind)
        got, values = _fused(name, kind)
        assert not (_bits(got) == NAN16).any() and np.isfinite(values).all()
        ratio = sr.check_conv(values, sr.rule_pool(np.maximum(y, 0.0)), sr.rule_pool(s), sr.chain(3))
        print(f"stem fused {name} {kind}: max |err| / bound = {ratio:.4f}")
        assert ratio <= 1.0, (name, kind)
        unfused = ops.maxpool3x3s2_nhwc(ops.conv_stem_split(_dev(planes), _dev(w16), _dev(bias), sc.COUT, relu=True))
        assert got.shape == unfused.shape and torch.equal(got, unfused), (name, kind)
        again, _ = _fused(name, kind)
        assert torch.equal(got, again)
        if kind == "all_negative":
            assert (y < 0).all() and not _bits(got).any()


@pytest.fixture
def one_term():
    from hn_amd import ops
    old, ops.F16_TERMS = ops.F16_TERMS, 1
    yield
    ops.F16_TERMS = old


@pytest.mark.parametrize("name", sc.NAMES)
def test_fused_stem_pool_with_one_term(name, one_term):
    """ops.F16_TERMS = 1: the hi * hi products alone, against the one-term rule with its own chain of 225"""
    for kind in ("normal", "depth", "small"):
        y, s = _rule(name, kind, 1)
        got, values = _fused(name, kind)
        assert not (_bits(got) == NAN16).any()
        ratio = sr.check_conv(values, sr.rule_pool(np.maximum(y, 0.0)), sr.rule_pool(s), sr.chain(1))
        print(f"stem fused one term {name} {kind}: max |err| / bound = {ratio:.4f}")
        assert ratio <= 1.0, (name, kind)


def test_equal_sum_pairs_fused_and_unfused_planes_differ_values_do_not():
    """The hazard tests/test_stem_cpu.py settles, on the kernels: the bias is one fp32 ulp below 1 + 2^-11 (an fp16 rounding
    midpoint) and one conv pixel, the centre of a pooling window, lies one ulp above it (a single 2^-11 pixel under a 2^-11 centre
    tap adds 2^-22 exactly).  maxpool_s32_kernel keeps the pair of the window's FIRST element, (1, +2^-11); the fused kernel
    splits the maximum, (1 + 2^-10, -2^-11).  Both recombine to 1 + 2^-11: the two forms agree in value, not in planes."""
    from hn_amd import ops
    from hn_amd.weights import pack_stem_split
    below, above = sr.equal_sum_pair()
    w = torch.zeros((64, 1, 7, 7))
    w[:, 0, 3, 3] = 2.0 ** -11
    x = np.zeros((1, 8, 8, 4), F)
    x[0, 4, 4, 0] = 2.0 ** -11                          # the centre tap of conv pixel (2, 2), the centre of pooled (1, 1)'s window
    x16, w16 = _dev(split(x, 3)), pack_stem_split(w).w16.cuda()
    bias = torch.full((64,), float(below), device="cuda")
    conv = ops.conv_stem_split(x16, w16, bias, 64, relu=True, out_split=False).cpu().numpy()
    want = np.full((1, 4, 4, 64), below, F)
    want[0, 2, 2] = above
    assert np.array_equal(conv, want)
    unfused = ops.maxpool3x3s2_nhwc(ops.conv_stem_split(x16, w16, bias, 64, relu=True))
    fused = ops.conv_stem_pool_split(x16, w16, bias)
    assert torch.equal(ops.from_split(unfused), ops.from_split(fused))
    uh, ul = sr.from_s32(unfused.cpu().numpy())
    fh, fl = sr.from_s32(fused.cpu().numpy())
    eh, el = sr.pool_pairs(*sr.split_f32(want))
    assert np.array_equal(uh, eh) and np.array_equal(ul, el)
    sh, sl = sr.split_f32(sr.rule_pool(want))
    assert np.array_equal(fh, sh) and np.array_equal(fl, sl)
    assert (float(uh[0, 1, 1, 0]), float(ul[0, 1, 1, 0])) == (1.0, 2.0 ** -11)
    assert (float(fh[0, 1, 1, 0]), float(fl[0, 1, 1, 0])) == (1.0 + 2.0 ** -10, -2.0 ** -11)
    differ = (uh != fh) | (ul != fl)
    assert differ[0, 1, 1].all() and int(differ.sum()) == 64


# -------------------------------------------------------------------------------------------------------------- range contract
def test_range_contract_of_both_forms():
    """image = 40, weights = 40: 49 x 4 x 1600 = 313 600 per output, beyond the fp16 range.  An fp32 output holds it and notes
    nothing; the S32 output and the fused kernel's pooled S32 map cannot, and raise word 0."""
    from hn_amd import ops
    from hn_amd.weights import pack_stem_split
    x16 = _dev(split(np.full((1, 27, 30, 4), 40.0, F), 3))
    w16 = pack_stem_split(torch.full((64, 4, 7, 7), 40.0)).w16.cuda()
    bias = torch.zeros((64,), device="cuda")
    block = torch.zeros((4,), device="cuda", dtype=torch.int32)
    with ops.range_scope(block):
        y = ops.conv_stem_split(x16, w16, bias, 64, out_split=False)
        assert _words(block) == [0, 0, 0, 0]
        assert float(y.max()) == 49 * 4 * 1600.0
        ops.conv_stem_split(x16, w16, bias, 64, out_split=True)
        assert _words(block) == [1, 0, 0, 0]
        assert _words(block) == [0, 0, 0, 0]            # (collected words are cleared)
        ops.conv_stem_pool_split(x16, w16, bias)
        assert _words(block) == [1, 0, 0, 0]
        small = _dev(split(np.full((1, 27, 30, 4), 0.01, F), 3))
        ops.conv_stem_split(small, w16, bias, 64, out_split=True)
        ops.conv_stem_pool_split(small, w16, bias)
        assert _words(block) == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- NaN footprint
def test_nan_pixel_footprint_is_that_of_an_eight_wide_filter_row():
    """One NaN pixel at bordered (16, 17): the k run of a filter row is 8 pixels wide, so conv pixel (oy, ox) multiplies bordered
    pixels 2 ox .. 2 ox + 7 -- the eighth by a zero weight, and 0 x NaN = NaN.  The conv map is NaN exactly on that 7 x 8
    footprint (ox = 5 .. 8 where a 7 x 7 filter would give 6 .. 8); the pooled maps of the fused and the unfused form are NaN at
    the same positions, which contain the 7 x 7 footprint's and lie inside the 7 x 8 one's.  Pinned, not a defect to fix:
    `valid` and the detector's input check keep non-finite pixels out."""
    from hn_amd import ops
    name, kind = "15x17", "normal"
    _, w16, bias = _operands(name, kind)
    x = sc.image(name, kind).copy()
    x[0, 13, 14, 1] = np.nan
    x16 = ops.stem_image_nhwc4(_dev(x), border=3)
    by, bx = 16, 17
    _, _, oh, ow, poh, pow_, _ = sc.geometry(sc.BY_NAME[name])
    oy, ox = np.arange(oh)[:, None], np.arange(ow)[None, :]
    rows = (2 * oy <= by) & (by <= 2 * oy + 6)
    seven, eight = rows & (2 * ox <= bx) & (bx <= 2 * ox + 6), rows & (2 * ox <= bx) & (bx <= 2 * ox + 7)
    assert int(eight.sum()) == int(seven.sum()) + 4 and eight[5, 5] and not seven[5, 5]
    conv = ops.conv_stem_split(x16, _dev(w16), _dev(bias), 64, relu=True, out_split=False).cpu().numpy()
    for ch in range(64):
        assert np.array_equal(np.isnan(conv[0, :, :, ch]), eight), ch

    def pooled_mask(m):
        return sr.rule_pool(m.astype(F)[None, :, :, None])[0, :, :, 0] > 0

    unfused = ops.from_split(ops.maxpool3x3s2_nhwc(ops.conv_stem_split(x16, _dev(w16), _dev(bias), 64, relu=True))).cpu().numpy()
    fused = ops.from_split(ops.conv_stem_pool_split(x16, _dev(w16), _dev(bias))).cpu().numpy()
    assert np.array_equal(np.isnan(fused), np.isnan(unfused))
    clean = np.isnan(fused)
    assert np.array_equal(fused[~clean], unfused[~clean])
    for ch in range(64):
        got = np.isnan(fused[0, :, :, ch])
        assert (got | ~pooled_mask(seven)).all() and (~got | pooled_mask(eight)).all(), ch


# ------------------------------------------------------------------------------------------------------- maxpool3x3s2 on S32
@pytest.mark.parametrize("c", [32, 96])
def test_maxpool_s32_on_maps_smaller_than_its_window(c):
    """h, w in 1 .. 5 on all-negative data: the result is the true maximum, not 0; a NaN wins; the output planes are the input
    planes of the winning element (pool_pairs), bit for bit."""
    from hn_amd import ops
    for h in range(1, 6):
        for w in range(1, 6):
            g = np.random.default_rng(100 * h + 10 * w + c)
            v = (-np.abs(g.standard_normal((2, h, w, c))) - 0.01).astype(F)
            v[1, h // 2, w // 2, 5] = np.nan
            v[0, h - 1, w - 1, c - 1] = F(-1e-6)                     # the maximum of its windows, in their last tap
            hi, lo = sr.split_f32(v)
            hi[0, 0, 0, 0], lo[0, 0, 0, 0] = H(-1.0), H(2.0 ** -5)   # a pair that is no canonical split: it is copied as it is
            x = _dev(sr.to_s32(hi, lo))
            out = _nan_filled((2, sr.pool_size(h), sr.pool_size(w), c // 32, 2, 32))
            got = ops.maxpool3x3s2_nhwc(x, out=out)
            want = sr.to_s32(*sr.pool_pairs(hi, lo))
            assert tuple(got.shape) == want.shape
            assert np.array_equal(_bits(got), _bits(want)), (h, w)
            values = ops.from_split(got).cpu().numpy()
            rule = sr.rule_pool(hi.astype(F) + lo.astype(F))
            nan = np.isnan(rule)
            assert nan[1, h // 4, w // 4, 5] and np.array_equal(np.isnan(values), nan)
            assert np.array_equal(values[~nan], rule[~nan]) and (values[~nan] < 0).all()


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from hn_amd import ops
    w16 = torch.zeros((64, 7, 2, 32), device="cuda", dtype=torch.float16)
    bias = torch.zeros((128,), device="cuda")
    good = torch.zeros((2, 1, 14, 16, 4), device="cuda", dtype=torch.float16)
    odd = torch.zeros((2, 1, 14, 15, 4), device="cuda", dtype=torch.float16)              # pw = 9
    with pytest.raises(RuntimeError, match="8-pixel k run of the last output column leaves the bordered row"):
        ops.conv_stem_split(odd, w16, bias, 64)
    with pytest.raises(RuntimeError, match="8-pixel k run of the last output column leaves the bordered row"):
        ops.conv_stem_pool_split(odd, w16, bias)
    for cout in (32, 128):
        wc = torch.zeros((cout, 7, 2, 32), device="cuda", dtype=torch.float16)
        with pytest.raises(RuntimeError, match="needs cout = 64, bias, ReLU and an S32 output"):
            ops.conv_stem_pool_split(good, wc, bias, cout=cout)
    with pytest.raises(RuntimeError, match="needs cout = 64, bias, ReLU and an S32 output"):
        ops.conv_stem_pool_split(good, w16, None)
    w8 = torch.zeros((64, 8, 2, 32), device="cuda", dtype=torch.float16)                  # r = 8, pad = 4: the unfused form takes it
    with pytest.raises(RuntimeError, match="written for the 7x7 / stride-2 / pad-3 ResNet stem"):
        ops.conv_stem_pool_split(torch.zeros((2, 1, 16, 16, 4), device="cuda", dtype=torch.float16), w8, bias, r=8)
    for bad in (w16[:32], w16.reshape(64, 7, 64), w16.float(), w16.cpu(), w16.transpose(0, 1)):
        with pytest.raises(ValueError, match="w16 must be the fp16 GPU tensor"):
            ops.conv_stem_split(good, bad, bias, 64)
        with pytest.raises(ValueError, match="w16 must be the fp16 GPU tensor"):
            ops.conv_stem_pool_split(good, bad, bias)
    with pytest.raises(ValueError, match=r"x must be \[N,H,W,4\]"):
        ops.stem_image_nhwc4(torch.zeros((1, 4, 4, 3), device="cuda"))
    with pytest.raises(RuntimeError, match="bad dims"):
        ops.stem_image_nhwc4(torch.zeros((1, 4, 4, 4), device="cuda"), border=5)
    # the accepted calls still run on these operands
    assert tuple(ops.conv_stem_split(good, w16, bias, 64).shape) == (1, 4, 5, 2, 2, 32)
    assert tuple(ops.conv_stem_pool_split(good, w16, bias).shape) == (1, 2, 3, 2, 2, 32)
