"""hn_affine_split_f32, hn_affine_split_f32_levels, hn_unsplit_f32 and hn_maxpool3x3s2_s32 against the rule of tests/split_ref.py
on the cases of tests/split_cases.py, BIT FOR BIT (same_bits: any two NaNs are equal, -0.0 is not 0.0), the range words included;
the streaming instantiations at the one size that reaches them; the implicit-GEMM f16x3 epilogue's S32 store against the split
of its own fp32 output; and the towers' GroupNorm + ReLU end to end inside a bound that is derived, not measured (the measured
ratios: DESIGN.md section 5)."""
import numpy as np
import pytest
import torch

import gn_cases as gc
import split_cases as sc
import split_ref as sr

pytestmark = pytest.mark.gpu

F, H = np.float32, np.float16


def _d(t):
    return torch.from_numpy(np.array(t)).cuda()


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    assert sr.same_bits(got, want), (what, "first difference (index, got, want, count):", sr.first_difference(got, want))


def _device_operands(op, affine):
    """the case's buffers on the device and the launch's views of them -> (x, scale, shift, out, arena)"""
    nb = op.c // 32
    x = _d(op.x_buf).view(op.n, 1, op.hw, op.cw)[..., op.c0:op.c0 + op.c]
    scale = shift = None
    if affine:
        scale, shift = (_d(t).view(op.n, op.aw)[:, op.a0:] for t in (op.sc_buf, op.sh_buf))
    arena = torch.full((op.y_size,), float(sr.SENTINEL), device="cuda", dtype=torch.float16)
    out = arena[sc.GUARD:sc.GUARD + op.n * op.hw * op.ys].view(op.n, 1, op.hw, op.nbw, 2, 32)[:, :, :, op.b0:op.b0 + nb]
    return x, scale, shift, out, arena


def _to_split(ops, op, affine, relu):
    """-> (the whole arena as numpy, the four range words)"""
    x, scale, shift, out, arena = _device_operands(op, affine)
    block = torch.zeros((4,), device="cuda", dtype=torch.int32)
    with ops.range_scope(block):
        got = ops.to_split(x, scale, shift, relu=relu, out=out)
        words = ops.range_check_collect(block).cpu().tolist()
    assert got.data_ptr() == out.data_ptr()
    return arena.cpu().numpy(), words


@pytest.fixture
def forms():
    """(label, switch) of the two kernels; the form switch is process-wide, so it is put back whatever happens"""
    from hn_amd import ops
    yield (("pow2", False), ("generic", True))
    ops.set_form("split_generic", False)


# ---- the apply pass ----
@pytest.mark.parametrize("name", list(sc.APPLY))
def test_apply_pass_is_the_rule_bit_for_bit(name, forms):
    """every variant of the case through the channel-group-stationary kernel and through the generic one (c = 96 and c = 4096 take
    the generic one either way): the whole sentinel-filled arena, so a store outside the output shows, and the range words"""
    from hn_amd import ops
    op = sc.apply_case(name)
    for label, generic in forms:
        ops.set_form("split_generic", generic)
        for affine, relu in sc.variants(name):
            want, flag = sc.apply_expected(name, affine, relu)
            got, words = _to_split(ops, op, affine, relu)
            _assert_bits(got, want, (name, label, affine, relu))
            assert words == [int(flag), 0, 0, 0], (name, label, affine, relu, words)


def test_range_words_are_exactly_the_rule(forms):
    """one special value among harmless ones: [0, 0, 0, 0] at 65504 itself and for the overflow that the ReLU removes, [1, 0, 0,
    0] from nextafter(65504) on -- where the value still splits to a finite pair --, for +-inf and for NaN; and outside a scope no
    word is written"""
    from hn_amd import ops
    for label, generic in forms:
        ops.set_form("split_generic", generic)
        for name, (_v, s, _t, relu, flagged) in sc.FLAGS.items():
            op = sc.flag_case(name)
            want, flag = op.expected(s is not None, relu)
            assert flag == bool(flagged)
            got, words = _to_split(ops, op, s is not None, relu)
            _assert_bits(got, want, (name, label))
            assert words == [flagged, 0, 0, 0], (name, label, words)
    op = sc.flag_case("1e5")
    x, _, _, out, _ = _device_operands(op, False)
    block = torch.zeros((4,), device="cuda", dtype=torch.int32)
    with ops.range_scope(block, on=False):
        ops.to_split(x, out=out)
    assert ops.range_check_collect(block).cpu().tolist() == [0, 0, 0, 0]


# ---- the levels launch ----
@pytest.mark.parametrize("name", list(sc.LEVELS))
def test_levels_launch_is_the_rule_bit_for_bit(name, forms):
    """1, 3 and 5 levels with data and tables of their own (a block sent to the wrong level cannot pass), hw = 1 levels, levels
    whose block ranges meet at every first_block boundary; each level's whole arena against the rule"""
    from hn_amd import ops
    levels = sc.levels_case(name)
    for label, generic in forms:
        ops.set_form("split_generic", generic)
        for relu in (True, False):
            dev = [_device_operands(op, True) for op in levels]
            block = torch.zeros((4,), device="cuda", dtype=torch.int32)
            with ops.range_scope(block):
                ops.to_split_levels([d[0] for d in dev], [(d[1], d[2]) for d in dev], relu=relu, outs=[d[3] for d in dev])
                words = ops.range_check_collect(block).cpu().tolist()
            want = sc.levels_expected(name, relu)
            for l, (d, (w, _flag)) in enumerate(zip(dev, want)):
                _assert_bits(d[4].cpu().numpy(), w, (name, label, relu, "level", l))
            assert words == [int(any(w[1] for w in want)), 0, 0, 0]


# ---- unsplit and the pool ----
@pytest.mark.parametrize("name", list(sc.UNSPLIT))
def test_unsplit_is_one_fp32_addition(name):
    from hn_amd import ops
    u = sc.unsplit_case(name)
    n, h, w = u["shape"]
    nb = u["c"] // 32
    x = _d(u["xbuf"]).view(n, h, w, u["nbw"], 2, 32)[:, :, :, u["b0"]:u["b0"] + nb]
    arena = torch.full((u["y_size"],), float(sc.SENTINEL32), device="cuda")
    out = arena[sc.GUARD:sc.GUARD + u["npix"] * u["ys"]].view(n, h, w, u["cw"])[..., u["c0"]:u["c0"] + u["c"]]
    ops.from_split(x, out=out)
    _assert_bits(arena.cpu().numpy(), u["want"], name)


@pytest.mark.parametrize("name", list(sc.POOL))
def test_pool_copies_the_first_pair_with_the_largest_sum(name):
    """hand-built pairs: all-negative windows on every border, equal sums under different pairs, one NaN and two"""
    from hn_amd import ops
    hi, lo = sc.pool_case(name)
    n, h, w, c = hi.shape
    oh, ow = sr.pool_out(h, w)
    size = n * oh * ow * 2 * c
    arena = torch.full((size + 2 * sc.GUARD,), float(sr.SENTINEL), device="cuda", dtype=torch.float16)
    out = arena[sc.GUARD:sc.GUARD + size].view(n, oh, ow, c // 32, 2, 32)
    ops.maxpool3x3s2_nhwc(_d(sr.to_s32(hi, lo)), out=out)
    want = np.full(size + 2 * sc.GUARD, sr.SENTINEL, H)
    want[sc.GUARD:sc.GUARD + size] = sr.to_s32(*sc.pool_expected(name)).reshape(-1)
    _assert_bits(arena.cpu().numpy(), want, name)


# ---- the streaming instantiations ----
# (n, hw, c): just over the 128 MiB threshold with a pixel tail; above 2^21 pixels, where gx hits its 16384 / n cap; and batch 32 at
# 256 channels with hw > 3 * gx * ppb, the smallest size at which the four-deep loop itself runs (403 MB: three steps of a full grid)
STREAM = {"threshold": (2, 2 ** 19 + 3, 32), "capped": (2, 2 ** 20 + 65, 32), "four-deep": (32, 3 * 512 * 8 + 21, 256)}


@pytest.mark.parametrize("name", list(STREAM))
def test_streaming_instantiations_equal_the_generic_kernel_and_the_rule(name, forms):
    """affine_split_pow2_kernel<true, 2, 4> and <false, 2, 4> run only from 128 MiB of fp32 on: data made on the device, compared
    on the device with the generic kernel (pinned to the rule at the small shapes; here it wraps its grid-stride loop), and the
    first, the last and 4096 interior pixels of every image against the rule on the host"""
    from hn_amd import ops
    n, hw, c = STREAM[name]
    assert ops.split_levels_stream(n, [hw], c) and n * hw * (c // 8) > 16384 * 256
    if name == "threshold":
        assert not ops.split_levels_stream(n, [2 ** 19 - 1], c)
    ppb, gx = sr.pow2_grid(n, hw, c)
    assert (gx == -(-16384 // n)) == (name != "threshold") and (hw > 3 * gx * ppb) == (name == "four-deep")
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    x = torch.randn((n, 1, hw, c), device="cuda", generator=g) * 2
    x *= torch.where(torch.rand((n, 1, hw, c), device="cuda", generator=g) < 1 / 7, 2.0 ** -12, 1.0)
    vals = sc.ladder_values()
    vals = _d(np.resize(vals[np.abs(vals) <= 2052], c))                        # the ladder up to the fp16 midpoints: in range
    x[:, 0, 0], x[:, 0, hw - 1] = vals, vals.flip(0)                           # under every scale below
    rng = np.random.default_rng(12)
    scale = _d(((1.0 + 0.5 * rng.standard_normal((n, c))).clip(-3, 3) * (1 + np.arange(n) % 3)[:, None]).astype(F))
    shift = _d((0.2 * rng.standard_normal((n, c)) - 0.3 * (np.arange(n) % 5)[:, None]).astype(F))
    idx = torch.cat((torch.arange(64), torch.randint(64, hw - 64, (4096,), generator=torch.Generator().manual_seed(13)),
                     torch.arange(hw - 64, hw))).cuda()
    for affine, relu in ((True, True), (False, False)):
        outs = []
        for label, generic in forms[::-1]:
            ops.set_form("split_generic", generic)
            arena = torch.full((2 * sc.GUARD + n * hw * 2 * c,), float(sr.SENTINEL), device="cuda", dtype=torch.float16)
            out = arena[sc.GUARD:sc.GUARD + n * hw * 2 * c].view(n, 1, hw, c // 32, 2, 32)
            block = torch.zeros((4,), device="cuda", dtype=torch.int32)
            with ops.range_scope(block):
                ops.to_split(x, scale if affine else None, shift if affine else None, relu=relu, out=out)
                assert ops.range_check_collect(block).cpu().tolist() == [0, 0, 0, 0], (name, label)
            assert bool((arena[:sc.GUARD] == float(sr.SENTINEL)).all()) and bool((arena[-sc.GUARD:] == float(sr.SENTINEL)).all())
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), (name, affine)      # the bits (no NaN in here)
        xs_ = x[:, 0, idx].cpu().numpy()
        hi, lo, flag = sr.rule_apply(xs_, scale.cpu().numpy() if affine else None, shift.cpu().numpy() if affine else None, relu)
        assert not flag
        _assert_bits(outs[1][:, 0, idx].cpu().numpy(), sr.to_s32(hi, lo), (name, affine, "sampled pixels"))
        del outs, arena, out


# ---- the conv epilogue's S32 store ----
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6, 7, 8])
def test_conv_epilogue_split_store_is_the_split_of_its_fp32_output(tile):
    """The implicit-GEMM f16x3 epilogue computes one fp32 v and only its store depends on out_split: with the tile forced, bias,
    an fp32 residual and a partial relu_cols, the S32 output is split(the fp32 output) bit for bit.  Both calls reach the same
    kernel: 3x3 keeps the 1x1 stream kernel out, a partial relu_cols the halo kernel, splitk=False split-K, and neither the tile
    pick nor the row-shared choice reads out_split -- asserted through the library's own dispatch queries.  Then the flag, on
    outputs that are exactly 65504 and its neighbour (zero filter, so v = bias + residual)."""
    from hn_amd import _lib, ops
    from hn_amd.weights import split_f16x3
    lib = _lib.load()
    n, h, w, cin, cout, relu_cols = 2, 9, 7, 32, 64, 40
    rng = np.random.default_rng(20 + tile)
    x, res = (_d(rng.standard_normal(s).astype(F)) for s in ((n, h, w, cin), (n, h, w, cout)))
    wt = _d((rng.standard_normal((cout, 3, 3, cin)) * (2.0 / (9 * cin)) ** 0.5).astype(F))
    bias = _d((0.1 * rng.standard_normal(cout)).astype(F))
    d = ops.make_conv_desc(n, h, w, cin, cout, 3, 3, 1, 1, 1, relu_cols, 1, tile=tile)
    d.splitk = -1
    sig = []
    for out_split in (0, 1):
        d.out_split = out_split
        sig.append((lib.hn_conv2d_f16x3_pick_tile(d), lib.hn_conv2d_f16x3_uses_halo(d, 1), lib.hn_conv2d_f16x3_uses_stream(d),
                    lib.hn_conv2d_f16x3_uses_rs(d)))
    assert sig[0] == sig[1] and sig[0][:3] == (tile, 0, 0), sig
    xs, w16 = ops.to_split(x), split_f16x3(wt.cpu()).cuda()
    kw = dict(pad=1, relu_cols=relu_cols, residual=res, tile=tile, w16=w16, splitk=False)
    y32 = ops.conv2d_nhwc(xs, wt, bias, **kw)
    y16 = ops.conv2d_nhwc(xs, wt, bias, out_split=True, **kw)
    v = y32.cpu().numpy()
    assert (v[..., relu_cols:] < 0).any() and (v[..., :relu_cols] >= 0).all() and (v[..., :relu_cols] > 0).any()
    _assert_bits(y16.cpu().numpy(), sr.to_s32(*sr.split(v)), ("tile", tile))
    # the flag
    wz = torch.zeros_like(wt)
    wz16 = split_f16x3(wz.cpu()).cuda()
    nxt = float(np.nextafter(F(65504), F(np.inf)))
    for col, value, flagged in ((5, 65504.0, 0), (5, nxt, 1), (50, -65504.0, 0), (50, -nxt, 1), (5, -nxt, 0), (50, float("nan"), 1)):
        b = bias.clone()
        b[col] = value
        r0 = torch.zeros_like(res)
        block = torch.zeros((4,), device="cuda", dtype=torch.int32)
        with ops.range_scope(block):
            y = ops.conv2d_nhwc(xs, wz, b, pad=1, relu_cols=relu_cols, residual=r0, tile=tile, w16=wz16, splitk=False, out_split=True)
            words = ops.range_check_collect(block).cpu().tolist()
        assert words == [flagged, 0, 0, 0], (tile, col, value, words)
        want = np.broadcast_to(b.cpu().numpy(), (n, h, w, cout)).copy()
        want[..., :relu_cols] = sr.relu(want[..., :relu_cols])
        _assert_bits(y.cpu().numpy(), sr.to_s32(*sr.split(want)), ("tile", tile, col, value))


# ---- GroupNorm + ReLU of the towers, end to end ----
@pytest.mark.parametrize("shape", ["hw63", "tower"])
def test_groupnorm_relu_end_to_end_is_inside_the_derived_bound(shape):
    """ops.groupnorm_affine -> ops.to_split(relu=True) -> ops.from_split against torch's float64 relu(group_norm).
    The bound, per element, from the operations and from nothing a kernel returned:  with (ds, dt) gn_ref's worst-case error of the
    tables, v = x*scale + shift exact,
        E  = |x| ds + dt                     the tables' error through x*s + t
        E1 = E + u (|v| + E)                 one fp32 rounding of the fma, u = 2^-24
        B  = E1 + 2^-22 (|v| + E1) + 2^-25   the split: hi and lo carry 22 bits, a subnormal lo is off by half of 2^-24 at most
    ReLU does not increase a difference; the factor 1 + 2^-10 covers the second-order terms and torch's own float64 error."""
    from hn_amd import ops
    n, h, w, c, groups = gc.AFFINE[shape]
    ratios = {}
    for kind in ("ratio1-std1", "ratio10-std1", "groups", "images"):
        x, gamma, beta = gc.make(shape, kind)
        (scale, shift, _mean, _var), (ds, dt) = gc.reference(shape, kind)
        xd = _d(x)
        sc_, sh_ = ops.groupnorm_affine(xd, _d(gamma), _d(beta), groups=groups, eps=gc.EPS)
        got = ops.from_split(ops.to_split(xd, sc_, sh_, relu=True)).cpu().numpy().astype(np.float64)
        x64 = torch.from_numpy(np.array(x)).double().permute(0, 3, 1, 2).contiguous()
        want = torch.relu(torch.nn.functional.group_norm(x64, groups, torch.from_numpy(np.array(gamma)).double(),
                                                         torch.from_numpy(np.array(beta)).double(), eps=float(F(gc.EPS))))
        want = want.permute(0, 2, 3, 1).numpy()
        ax = np.abs(x.astype(np.float64))
        v = np.abs(x.astype(np.float64) * scale[:, None, None, :] + shift[:, None, None, :])
        e = ax * ds[:, None, None, :] + dt[:, None, None, :]
        e1 = e + 2.0 ** -24 * (v + e)
        b = (e1 + 2.0 ** -22 * (v + e1) + 2.0 ** -25) * (1 + 2.0 ** -10)
        assert np.isfinite(got).all() and float(v.max()) < 65504
        ratios[kind] = float((np.abs(got - want) / b).max())
    print(f"gn + relu + split gpu {shape}: |err| / bound " + ", ".join(f"{k} {r:.4f}" for k, r in ratios.items()))
    assert max(ratios.values()) <= 1.0
