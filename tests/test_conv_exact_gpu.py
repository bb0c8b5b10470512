"""Every form of the convolution kernels against the exact-arithmetic reference (tests/conv_exact_ref.py), bit for bit: on the
operand families of that file no summation order, tile shape, split-K plan, LDS staging or MFMA shape can change a bit, so the
kernel output must equal the fp64 model -- the whole output tensor, and the whole sentinel-filled arena where the output is a
channel slice.  No tolerance anywhere.  Every case also runs on the `int` family (small integers, at most 12 significant bits):
the control that separates an indexing mistake from a property of the MFMA's internal accumulation width.  S32 operands are made
on the CPU by the pinned split rule (split_ref), so nothing but the kernel under test runs on the device.  The cases, and the
router trigger each one pins, are tests/conv_exact_cases.py's; test_conv_exact_cpu.py shows that the comparison can fail."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import conv_exact_cases as cc
import conv_exact_ref as cr
import split_ref as sr

pytestmark = pytest.mark.gpu
_FORMS = ("thin_form_flat",)
_cache = {}


@pytest.fixture(autouse=True)
def _kernel_forms_are_reset():
    yield
    if torch.cuda.is_available():
        from hn_amd import ops
        for f in _FORMS:
            ops.set_form(f, False)


def _prepared(c):
    """(operands, expected output tensor) of a case, computed once and left unchanged"""
    if c.name not in _cache:
        o = cr.operands(c)
        s = float(cr.abs_sum(o, c).max())
        assert s < cr.LIMIT[c.family], (c.name, s)
        want = cr.expected(c, o)
        want.setflags(write=False)
        _cache[c.name] = (o, want)
    return _cache[c.name]


def _families(c):
    return (c,) if c.family == "int" else (c, cr.with_family(c, "int"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _s32(v):
    """fp32 [N,H,W,C] -> the S32 tensor on the device, split on the CPU by the rule"""
    return _dev(sr.to_s32(*sr.split(v)))


def _bank(c, o):
    """the filter bank of a case as the front ends take it"""
    from hn_amd.weights import split_f16x3
    w = torch.from_numpy(o.w)
    return NS(w=w.cuda(), bias=None if o.bias is None else _dev(o.bias), w16=split_f16x3(w).cuda() if c.kind == "f16x3" else None,
              stride=c.stride, pad=c.pad, dil=c.dil)


def _same(got, want, c, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (c.name, what, got.shape, want.shape, got.dtype)
    if not sr.same_bits(got, want):
        i, a, b, count = sr.first_difference(got, want)
        pytest.fail(f"{c.name} {what}: {count} of {got.size} elements differ; first at flat {i} = (img, oy, ox, channel, part) "
                    f"{cr.decode(i, c, got.shape)}: kernel {float(a)!r} ({a.view(np.uint16 if a.dtype == np.float16 else np.uint32):#x}), "
                    f"model {float(b)!r} ({b.view(np.uint16 if b.dtype == np.float16 else np.uint32):#x})")


def _input(c, o):
    """-> (x as conv2d_nhwc takes it, in_scale, in_shift)"""
    sl = slice(o.c0, o.c0 + c.cin)
    if c.kind == "f32" or c.x_f32:
        wide = _dev(o.raw if c.x_f32 else o.xwide)
        if c.x_f32 == "gn":
            return wide[..., sl], _dev(o.scale)[:, sl], _dev(o.shift)[:, sl]
        return wide[..., sl], None, None
    return _s32(o.xwide)[:, :, :, o.c0 // 32:(o.c0 + c.cin) // 32], None, None


def _residual(c, o):
    if o.res is None:
        return None
    return _s32(o.res) if c.res.endswith("s32") else _dev(o.res)


def _conv(c, tile):
    """one conv2d_nhwc call of the case -> the whole output tensor (the arena where the output is a slice of one)"""
    from hn_amd import ops
    o, _ = _prepared(c)
    bank = _bank(c, o)
    x, sc, sh = _input(c, o)
    full = out = None
    if c.out_wide:
        oh, ow = cr.out_size(c)
        cw, c0 = c.out_wide
        full = _dev(cr.arena((c.n, oh, ow), cw, c.out_split))
        out = full[:, :, :, c0 // 32:(c0 + c.cout) // 32] if c.out_split else full[..., c0:c0 + c.cout]
    kw = dict(stride=c.stride, pad=c.pad, dil=c.dil, relu_cols=c.relu_cols, residual=_residual(c, o),
              res_upsample=bool(c.res and c.res.startswith("up")), in_scale=sc, in_shift=sh, out=out, tile=tile, w16=bank.w16,
              out_split=c.out_split)
    if c.kind == "f16x3":
        kw.update(splitk=c.splitk, force_splits=c.force_splits)
    if c.terms == 1:
        with ops.f16_terms(1):
            y = ops.conv2d_nhwc(x, bank.w, bank.bias, **kw)
    else:
        y = ops.conv2d_nhwc(x, bank.w, bank.bias, **kw)
    return y if full is None else full


def _check_single(c0, tiles=None):
    from hn_amd import ops
    for c in _families(c0):
        _, want = _prepared(c)
        for tile in (c.tiles if tiles is None else tiles):
            route = cc.assert_route(c, tile, ops)
            _same(_conv(c, tile), want, c, f"tile {tile} ({route})")


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("tile", cc.ALL_TILES)
def test_group1_implicit_gemm_under_every_tile(tile):
    for c in cc.GROUP1:
        if tile in c.tiles:
            _check_single(c, (tile,))


@pytest.mark.parametrize("case", cc.GROUP2, ids=_ids(cc.GROUP2))
def test_group2_epilogues(case):
    _check_single(case)


@pytest.mark.parametrize("case", cc.GROUP3, ids=_ids(cc.GROUP3))
def test_group3_split_k(case):
    """both reductions: the tiles of fused_reduce_form reduce in their last workgroups (the first workspaces of a process get ticket
    counters, and the counters are back at zero afterwards), the others through splitk_reduce_kernel"""
    from hn_amd import ops
    _check_single(case)
    assert ops.tickets_nonzero() == 0


@pytest.mark.parametrize("kind", list(cc.GROUP4), ids=list(cc.GROUP4))
def test_group4_grouped_multi_and_mixed_launches(kind):
    from hn_amd import ops
    members0 = cc.GROUP4[kind]
    for fam in ("own", "int"):
        members = [m if fam == "own" else cr.with_family(m, "int") for m in members0]
        prep = [_prepared(m) for m in members]
        banks = [_bank(m, o) for m, (o, _) in zip(members, prep)]
        xs = [_input(m, o)[0] for m, (o, _) in zip(members, prep)]
        m0 = members[0]
        if kind == "multi":
            fused = []
            outs = ops.conv2d_nhwc_multi([(x, b, dict(relu_cols=m.relu_cols, residual=_residual(m, o), out_split=m.out_split))
                                          for x, b, m, (o, _) in zip(xs, banks, members, prep)], fused=fused)
            assert fused == [True]
        else:
            if kind == "mixed":
                # mixed_small_mask's trigger: more than one round of 128 x 128 tiles on 512 slots, at most three, the last one
                # at most a quarter full -- and the tile the launch picks for all the rows together is 128 x 128
                import ctypes as C
                rows = [m.n * m.h * m.w for m in members]
                total = sum(-(-r // 128) for r in rows) * -(-m0.cout // 128)
                assert 512 < total <= 3 * 512 and 0 < total % 512 <= 128 and min(rows) * 2 <= max(rows)
                d = ops.make_conv_desc(1, sum(rows), 1, m0.cin, m0.cout, 3, 3, 1, 1, 1)
                assert ops._lib.load().hn_conv2d_f16x3_pick_tile(C.byref(d)) == 1
            outs = ops.conv2d_nhwc_grouped(xs, banks, pad=m0.pad, relu_cols=m0.relu_cols, out_split=m0.out_split)
        for m, y, (_, want) in zip(members, outs, prep):
            _same(y, want, m, kind)


@pytest.mark.parametrize("case", cc.GROUP5, ids=_ids(cc.GROUP5))
def test_group5_halo_kernel(case):
    _check_single(case)


@pytest.mark.parametrize("case", cc.GROUP6, ids=_ids(cc.GROUP6))
def test_group6_stream_kernel(case):
    _check_single(case)


@pytest.mark.parametrize("launch", cc.GROUP7, ids=[f"{t.form}_cout{t.cout}{'_affine' if t.affine else ''}" for t in cc.GROUP7])
def test_group7_thin_kernels(launch):
    from hn_amd import ops
    for fam in ("own", "int"):
        members = [m if fam == "own" else cr.with_family(m, "int") for m in launch.members]
        prep = [_prepared(m) for m in members]
        bank = _bank(members[0], prep[0][0])
        assert all((o.w == prep[0][0].w).all() for o, _ in prep)      # one filter bank for all levels (the members share wseed)
        wants = [want for _, want in prep]
        ops.set_form("thin_form_flat", launch.form == "flat")
        try:
            if launch.affine:
                ts = [_dev(o.raw) for o, _ in prep]
                aff = [(_dev(o.scale), _dev(o.shift)) for o, _ in prep]
                assert ops.thin_affine_applies(ts, bank)
                outs = ops.conv3x3_thin_affine_levels(ts, aff, members[0].in_wide[1], bank, relu_cols=launch.relu_cols)
            else:
                xs = [_input(m, o)[0] for m, (o, _) in zip(members, prep)]
                assert ops.thin_uses_flat(xs, bank) == (launch.form == "flat")
                outs = ops.conv3x3_thin_levels(xs, bank, relu_cols=launch.relu_cols)
        finally:
            ops.set_form("thin_form_flat", False)
        for m, y, want in zip(members, outs, wants):
            _same(y, want, m, f"thin {launch.form}")


@pytest.mark.parametrize("case", cc.GROUP8, ids=_ids(cc.GROUP8))
def test_group8_f32_kernel(case):
    _check_single(case)


@pytest.mark.parametrize("case", cc.GROUP9, ids=_ids(cc.GROUP9))
def test_group9_one_term_mode(case):
    """hi*hi only against model1 -- and the same launch with three terms equals model3 and NOT model1: the lo terms are visible
    to this comparison on the device, not only in the emulation"""
    _check_single(case)
    three = NS(**vars(case))
    three.terms, three.name = 3, case.name + "[3 terms]"
    got = _conv(three, 0).cpu().numpy()
    assert sr.same_bits(got, _prepared(three)[1]) and not sr.same_bits(got, _prepared(case)[1])
