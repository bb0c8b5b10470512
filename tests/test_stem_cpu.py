"""The stem chain's rules, bound, emulation and mutants (tests/stem_ref.py) on the host: the float64 rule is torch's conv2d /
max_pool2d on the operands the kernels see; the fp32 emulation is inside the worst-case bound on every case x kind of
tests/stem_cases.py, so the bound is known to hold for the reference path alone before a GPU meets it; every mutant falls outside
on its named case, so the check can fail; weights.pack_stem_split has the layout the rule assumes; and the equal-sum pair
question of the two pooling forms is settled."""
import numpy as np
import pytest
import torch

import stem_cases as sc
import stem_ref as sr
from pre_ref import split

F, D, H = np.float32, np.float64, np.float16


def _planes(name, kind):
    return split(sc.image(name, kind), sc.PAD)


def _torch_conv(xp, bank):
    """conv2d in float64 of a bordered plane [n, hb, wb, 4] with a bank [cout, 224] (k = ky * 32 + kx * 4 + c): a 7 x 8 filter,
    as the kernels' k run is (wb is even, so the 8th tap of the last column is the row's last pixel)"""
    wt = torch.from_numpy(bank.reshape(bank.shape[0], 7, 8, 4)).permute(0, 3, 1, 2)           # [cout, c, ky, kx]
    return torch.nn.functional.conv2d(torch.from_numpy(xp).permute(0, 3, 1, 2), wt, stride=2).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("name,kind", [("4x5", "normal"), ("15x17", "depth"), ("17x25", "small"), ("3x130", "edge_heavy")])
def test_rule_is_torch_conv2d_and_max_pool2d_in_float64(name, kind):
    planes = _planes(name, kind)
    w16, bias = sc.filters(name, kind)
    xh, xl = planes[0].astype(D), planes[1].astype(D)
    wh, wl = (w16[:, :, i].astype(D).reshape(64, 224) for i in (0, 1))
    assert not w16[:, :, :, 28:].any()                       # so the 8-wide row is the 7-wide filter
    for terms in (3, 1):
        y, s = sr.rule_conv(planes, w16, bias, terms)
        if terms == 3:      # conv2d on the recombined operands, less the one product the kernels drop
            want = _torch_conv(xh + xl, wh + wl) - _torch_conv(xl, wl) + bias.astype(D)
        else:
            want = _torch_conv(xh, wh) + bias.astype(D)
        assert np.abs(y - want).max() <= 1e-12 * s.max()
        assert (np.abs(y) <= s).all()
        yr, _ = sr.rule_conv(planes, w16, bias, terms, relu=True)
        assert np.array_equal(yr, np.maximum(y, 0.0))
    pooled = torch.nn.functional.max_pool2d(torch.from_numpy(y).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(sr.rule_pool(y), pooled)
    v = y.copy()
    v[0, 0, 0, 0] = np.nan
    assert np.isnan(sr.rule_pool(v)[0, 0, 0, 0]) and int(np.isnan(sr.rule_pool(v)).sum()) == 1


def test_case_table_has_the_shapes_it_promises():
    g = {c.name: sc.geometry(c) for c in sc.CASES}
    assert g["1x1"][2:] == (1, 1, 1, 1, 1)
    assert g["4x5"][2:6] == (4, 5, 2, 3)
    assert g["14x15"][2:] == (14, 15, 7, 8, 1)
    assert g["15x17"][2:] == (15, 17, 8, 9, 4)
    assert g["17x25"][0] % 2 == 1
    assert g["88x88"][2:] == (88, 88, 44, 44, 126) and 126 & 7 == 6
    assert g["15x17x4"][6] % 8 == 0 and g["15x17x4"][6] >= 16
    assert g["3x130"][6] == 9 and g["130x3"][6] == 10
    lo = split(sc.image("88x88", "small"), 3)[1].astype(D)
    assert np.abs(lo).max() < 2.0 ** -14                     # `small`: every lo part is an fp16 subnormal
    x = sc.image("88x88", "depth")
    assert not x[..., 1:].any() and 0.3 <= x[..., 0].min() and x[..., 0].max() <= 1.3


@pytest.mark.parametrize("name", sc.NAMES)
def test_emulation_is_inside_the_bound_on_every_case_and_kind(name):
    for kind in sc.KINDS:
        planes = _planes(name, kind)
        w16, bias = sc.filters(name, kind)
        for terms in (3, 1):
            y, s = sr.rule_conv(planes, w16, bias, terms)
            r_conv = sr.check_conv(sr.emulate_conv(planes, w16, bias, terms, relu=False), y, s, sr.chain(terms))
            py, ps = sr.rule_fused(planes, w16, bias, terms)
            fused = sr.emulate_fused(planes, w16, bias, terms)
            r_fused = sr.check_conv(fused, py, ps, sr.chain(terms))
            print(f"stem emulation {name} {kind} terms={terms}: conv {r_conv:.4f} fused {r_fused:.4f}")
            assert r_conv <= 1.0 and r_fused <= 1.0
            # the fused form's values ARE the pooled values of the unfused emulation: the phantom ring changes nothing
            unfused = sr.emulate_pool(sr.emulate_conv(planes, w16, bias, terms, relu=True))
            assert np.array_equal(fused, unfused)
            if kind == "all_negative":
                assert (y < 0).all() and not fused.any()


def _pool_data(shape, kind, seed=5):
    h, w, c = shape
    v = np.random.default_rng(seed).standard_normal((2, h, w, c)).astype(F)
    return -np.abs(v) - F(0.01) if kind == "negative" else v


def _image_data(shape, seed=6):
    n, h, w = shape
    x = (np.random.default_rng(seed).standard_normal((n, h, w, 4)) * 3).astype(F)
    x[0, 1, 2, 0], x[0, h - 1, 0, 3], x[1, 0, w - 1, 1] = np.nan, np.inf, -np.inf
    return x


@pytest.mark.parametrize("mutant", sorted(sr.MUTANTS))
def test_every_mutant_is_outside_the_bound_on_its_named_case(mutant):
    stage, case, kind = sr.MUTANTS[mutant]
    if stage in ("conv", "fused"):
        planes = _planes(case, kind)
        w16, bias = sc.filters(case, kind)
        if stage == "conv":
            y, s = sr.rule_conv(planes, w16, bias, 3)
            good, bad = (sr.emulate_conv(planes, w16, bias, 3, relu=False, mutant=m) for m in (None, mutant))
        else:
            y, s = sr.rule_fused(planes, w16, bias, 3)
            good, bad = (sr.emulate_fused(planes, w16, bias, 3, mutant=m) for m in (None, mutant))
        r_good, r_bad = sr.check_conv(good, y, s, sr.chain(3)), sr.check_conv(bad, y, s, sr.chain(3))
        print(f"stem mutant {mutant} on {case} {kind}: {r_bad:.3g} (unmutated {r_good:.3g})")
        assert r_good <= 1.0 and not r_bad <= 1.0
    elif stage == "pool":
        v = _pool_data(case, kind)
        assert np.array_equal(sr.emulate_pool(v), sr.rule_pool(v))
        assert not np.array_equal(sr.emulate_pool(v, mutant), sr.rule_pool(v))
        assert (sr.rule_pool(v) < 0).all()
    else:
        x = _image_data(case)
        valid = np.array([0, 1], np.int32)
        planes, v_out, words = sr.rule_image(x, 3, valid)
        good, bad = (sr.emulate_image(x, 3, valid, m) for m in (None, mutant))
        assert good[0].tobytes() == planes.tobytes() and np.array_equal(good[1], v_out)
        assert bad[0].tobytes() != planes.tobytes() or not np.array_equal(bad[1], v_out)
        assert v_out.tolist() == [0, 2] and words == [0, 0, 1, 0] and np.isfinite(planes.astype(F)).all()


def test_rule_image_range_words_and_passthrough():
    x = _image_data((2, 5, 7))
    planes, v_out, words = sr.rule_image(x, 0)
    assert v_out is None and words == [0, 0, 1, 0]
    assert np.isnan(planes[:, 0, 1, 2, 0].astype(F)).all()                     # hi and lo of the NaN pixel
    assert planes[0, 0, 4, 0, 3] == np.inf and np.isnan(planes[1, 0, 4, 0, 3])  # inf - inf
    big = np.full((1, 1, 1, 4), 3e38, F)
    planes, _, words = sr.rule_image(big, 4)
    assert words == [0, 1, 0, 0] and planes[0, 0, 4, 4, 0] == np.inf and planes.shape == (2, 1, 9, 9, 4)
    assert not planes[:, :, :4].any() and not planes[:, :, :, :4].any()
    assert sr.rule_image(np.full((1, 1, 1, 4), 65504.0, F), 0)[2] == [0, 0, 0, 0]


def test_pack_stem_split_layout():
    from hn_amd.weights import pack_stem_split
    g = torch.Generator().manual_seed(3)
    for cin, r in ((1, 7), (3, 7), (4, 7), (3, 5), (4, 8)):
        w = torch.randn((8, cin, r, r), generator=g)
        scale = torch.rand((8,), generator=g, dtype=torch.float64) + 0.5 + 2.0 ** -30      # not an fp32 number
        shift = torch.randn((8,), generator=g, dtype=torch.float64)
        for bn in (None, (scale, shift)):
            cw = pack_stem_split(w, bn)
            w16 = cw.w16.numpy()
            assert w16.shape == (8, r, 2, 32) and w16.dtype == H
            assert not w16[:, :, :, 4 * r:].any()                                           # zeros for k >= 4 r
            # the fold happens in float64, ONE rounding to fp32, then the split
            f32 = (w.double() * (scale.view(-1, 1, 1, 1) if bn else 1.0)).float().numpy()   # [o, c, ky, kx]
            want = np.zeros((8, r, 8, 4), F)
            want[:, :, :r, :cin] = f32.transpose(0, 2, 3, 1)                                # k = kx * 4 + c
            hi, lo = sr.split_f32(want.reshape(8, r, 32))
            assert np.array_equal(w16[:, :, 0], hi) and np.array_equal(w16[:, :, 1], lo)
            assert (cw.bias is None) if bn is None else torch.equal(cw.bias, shift.float())
            assert (cw.stride, cw.pad) == (2, r // 2)
        folded32 = (w * scale.float().view(-1, 1, 1, 1)).numpy()                            # a fold in fp32 is another bank
        assert not np.array_equal(folded32, (w.double() * scale.view(-1, 1, 1, 1)).float().numpy())
    for shape in ((8, 5, 7, 7), (8, 3, 9, 9), (8, 3, 7, 5)):
        with pytest.raises(ValueError, match="R x R with R <= 8 and Cin <= 4"):
            pack_stem_split(torch.zeros(shape))


def test_equal_sum_pairs_the_two_pooling_forms_agree_in_value_not_in_planes():
    """conv_stem_direct.hip splits max(v); the unfused path splits every v and maxpool_s32_kernel keeps the FIRST pair whose
    recombined sum is largest.  For two fp32 values either side of an fp16 rounding midpoint the pairs differ and the sums are
    equal, so when the smaller value comes first in the window the two forms store different planes that recombine to the same
    fp32 value.  (Downstream the pair's lo part only enters the products x_lo w_hi: the forms then differ by what one dropped
    lo*lo-sized term is worth.)"""
    below, above = sr.equal_sum_pair()
    assert below < above and below.dtype == F
    (h0, l0), (h1, l1) = sr.split_f32(below), sr.split_f32(above)
    assert (float(h0), float(l0)) == (1.0, 2.0 ** -11) and (float(h1), float(l1)) == (1.0 + 2.0 ** -10, -2.0 ** -11)
    assert F(h0) + F(l0) == F(h1) + F(l1) == F(1.0 + 2.0 ** -11)
    v = np.full((1, 3, 3, 32), below, F)          # one window; the larger value in its LAST tap
    v[0, 2, 2] = above
    unfused = sr.pool_pairs(*sr.split_f32(v))
    fused = sr.split_f32(sr.rule_pool(v))
    assert unfused[0].shape == (1, 2, 2, 32)
    at = (0, 1, 1)                                 # the window over rows / columns 1 .. 2 holds both values, `below` first
    assert (float(unfused[0][at][0]), float(unfused[1][at][0])) == (1.0, 2.0 ** -11)
    assert (float(fused[0][at][0]), float(fused[1][at][0])) == (1.0 + 2.0 ** -10, -2.0 ** -11)
    assert np.array_equal(unfused[0].astype(F) + unfused[1].astype(F), fused[0].astype(F) + fused[1].astype(F))
    # with the larger value FIRST the planes agree as well: the order inside the window decides
    v2 = v[:, ::-1, ::-1].copy()
    a, b = sr.pool_pairs(*sr.split_f32(v2)), sr.split_f32(sr.rule_pool(v2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # away from such ties copying the winner's pair IS splitting the maximum
    r = np.random.default_rng(11).standard_normal((2, 9, 7, 32)).astype(F)
    a, b = sr.pool_pairs(*sr.split_f32(r)), sr.split_f32(sr.rule_pool(r))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_s32_layout_helpers_round_trip():
    r = np.random.default_rng(12).standard_normal((2, 3, 4, 96)).astype(F)
    hi, lo = sr.split_f32(r)
    s = sr.to_s32(hi, lo)
    assert s.shape == (2, 3, 4, 3, 2, 32) and np.array_equal(s[1, 2, 3, 2, 1], lo[1, 2, 3, 64:])
    back = sr.from_s32(s)
    assert np.array_equal(back[0], hi) and np.array_equal(back[1], lo)
