"""The f16x3 range contract at every split producer, against the rule of tests/range_ref.py on the planted launches of
tests/range_cases.py: the four flag words as a whole list, read with ops.range_scope / ops.range_check_collect, and the stored output
bit for bit against the closed form (compared on the device).  Every planted operand is an fp16 number and every sum is exact in
fp32, so no summation order, tile shape or split-K plan can move a value across 65504: the words are a function of the table alone.
tests/test_range_cpu.py shows that the table can fail (the mutants of the rule) and that the closed form is conv_exact_ref's fp64
model on the planted operands.  Every convolution launch asserts its route through the library's own queries."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import conv_exact_cases as cc
import conv_exact_ref as cr
import pre_cases as pc
import range_cases as rc
import range_ref as rr
import split_ref as sr

pytestmark = pytest.mark.gpu
F = np.float32
NEXT, MAX = float(rr.NEXT), 65504.0
_state = {}


@pytest.fixture(autouse=True)
def _kernel_forms_are_reset():
    yield
    if torch.cuda.is_available():
        from hn_amd import ops
        for f in ("thin_form_flat", "preprocess_generic"):
            ops.set_form(f, False)


def _words(fn):
    """fn() inside a range scope of its own block -> (fn's result, the four words)"""
    from hn_amd import ops
    block = torch.zeros((4,), device="cuda", dtype=torch.int32)
    with ops.range_scope(block):
        out = fn()
        words = ops.range_check_collect(block).cpu().tolist()
    return out, words


def _same_bits(got, want):
    """two device tensors of one float type: equal bits, or NaN in both"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    ints = torch.int16 if got.dtype == torch.float16 else torch.int32
    return bool(((got.contiguous().view(ints) == want.contiguous().view(ints)) | (got.isnan() & want.isnan())).all())


def _split_dev(v):
    """fp32 [..., C] on the device -> the S32 tensor [..., C/32, 2, 32] of the split rule (hi = fp16(v), lo = fp16(v - hi))"""
    hi = v.half()
    lo = (v - hi.float()).half()
    lead, c = v.shape[:-1], v.shape[-1]
    return torch.stack((hi.view(*lead, c // 32, 32), lo.view(*lead, c // 32, 32)), dim=-2).contiguous()


# --------------------------------------------------------------------------------------------------------------------------
# planted convolution launches
# --------------------------------------------------------------------------------------------------------------------------
def _buffers(c):
    """the zero operands of a case on the device, made once: S32 input, fp32 bank and its split form, bias, residual"""
    key = (c.name, c.cout, c.terms)
    if key not in _state:
        oh, ow = rr.out_size(c)
        b = NS()
        b.x = torch.zeros((c.n, c.h, c.w, c.cin // 32, 2, 32), device="cuda", dtype=torch.float16)
        b.w = torch.zeros((c.cout, c.r, c.s, c.cin), device="cuda")
        b.w16 = torch.zeros((c.cout, (c.cin // 32) * c.r * c.s, 2, 32), device="cuda", dtype=torch.float16)
        b.bias_store = torch.zeros((c.cout + 4,), device="cuda")
        b.bias = b.bias_store[:c.cout] if c.bias else None
        b.res = None
        if c.res:
            rh, rw = ((oh + 1) // 2, (ow + 1) // 2) if rr.upsampled(c) else (oh, ow)
            b.res = (torch.zeros((c.n, rh, rw, c.cout // 32, 2, 32), device="cuda", dtype=torch.float16) if c.res.endswith("s32")
                     else torch.zeros((c.n, rh, rw, c.cout), device="cuda"))
        _state[key] = b
    return _state[key]


def _plant(L, b, on=True, bias=None):
    """write (on) or take back the planted elements of a launch"""
    c = L.case
    bias = b.bias if bias is None else bias
    for p in L.plants:
        img, iy, ix = rr.source_pixel(c, p.m)
        b.x[img, iy, ix, p.ci // 32, 0, p.ci % 32] = float(p.xv) if on else 0.0
        kt = ((p.ci // 32) * c.r + c.r // 2) * c.s + c.s // 2
        b.w16[p.co, kt, 0, p.ci % 32] = float(p.wv) if on else 0.0
        b.w[p.co, c.r // 2, c.s // 2, p.ci] = float(p.wv) if on else 0.0
    for co, v in L.bias.items():
        bias[co] = float(v) if on else 0.0
    if c.res:
        fill = float(L.res_fill)
        assert fill == 0.0
        for (m, co), v in L.res.items():
            r = rr.res_index(c, m)
            flat = b.res.view(-1, c.cout // 32, 2, 32) if c.res.endswith("s32") else b.res.view(-1, c.cout)
            if c.res.endswith("s32"):
                flat[r, co // 32, 0, co % 32] = float(v) if on else fill
            else:
                flat[r, co] = float(v) if on else fill


def _expected_dev(L):
    """the closed form of the launch on the device: the values [M, Cout] it stores"""
    c = L.case
    v = rr.conv_values(L)
    y = torch.zeros((rr.rows_of(c), c.cout), device="cuda")
    for co, (_pre, post) in v.background.items():
        y[:, co] = float(post)
    if v.elems:
        idx = torch.tensor([[m, co] for (m, co) in v.elems], device="cuda")
        y[idx[:, 0], idx[:, 1]] = torch.tensor([float(post) for (_p, _q, post) in v.elems.values()], device="cuda")
    return y


def _check_output(L, got):
    c = L.case
    oh, ow = rr.out_size(c)
    y = _expected_dev(L).view(c.n, oh, ow, c.cout)
    want = _split_dev(y) if c.out_split else y
    assert _same_bits(got, want), (L.name, "the stored output is not the closed form")


def _conv_kwargs(L, b, bias):
    c = L.case
    return dict(stride=c.stride, pad=c.pad, dil=c.dil, relu_cols=c.relu_cols, residual=b.res, res_upsample=rr.upsampled(c), tile=L.tile,
                w16=b.w16, out_split=c.out_split, splitk=c.splitk, force_splits=c.force_splits)


def _run(L, misaligned_bias=False):
    """one conv2d_nhwc call of a planted launch: its route, its words and its whole output"""
    from hn_amd import ops
    c = L.case
    b = _buffers(c)
    route = cc.assert_route(c, L.tile, ops)
    bias = b.bias_store[1:c.cout + 1] if misaligned_bias else b.bias
    _plant(L, b, True, bias)
    try:
        kw = _conv_kwargs(L, b, bias)
        arena = None
        if c.out_wide:
            oh, ow = rr.out_size(c)
            cw, c0 = c.out_wide
            arena = torch.full((c.n, oh, ow, cw // 32, 2, 32), float("nan"), device="cuda", dtype=torch.float16)
            kw["out"] = arena[:, :, :, c0 // 32:(c0 + c.cout) // 32]

        def call():
            if c.terms == 1:
                with ops.f16_terms(1):
                    return ops.conv2d_nhwc(b.x, b.w, bias, **kw)
            return ops.conv2d_nhwc(b.x, b.w, bias, **kw)
        y, words = _words(call)
        assert words == L.want, (L.name, route, words, L.want)
        _check_output(L, y)
        if arena is not None:
            c0 = c.out_wide[1] // 32
            assert bool(arena[:, :, :, :c0].isnan().all()) and bool(arena[:, :, :, c0 + c.cout // 32:].isnan().all()), L.name
    finally:
        _plant(L, b, False, bias)


@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("tile", cc.ALL_TILES)
def test_implicit_gemm_positions_under_every_tile(tile, terms):
    """one launch per (row, channel) position of the ragged 3 x 5 x 7 case and of the 1 x (BM - 1, BM, BM + 1) maps: the product
    +-65504 moved to the next float by the bias sets word 0, and the control with +-65504 at every position at once sets nothing"""
    for L in rc.igemm(tile, terms):
        _run(L)


@pytest.mark.parametrize("tile", cc.ALL_TILES)
def test_implicit_gemm_relu_residuals_fp32_output_and_slices(tile):
    """a value the ReLU removes, fp32 residuals that carry 65504, its neighbour, NaN and +-inf, the S32 residual 40000 under 797 * 32
    and 798 * 32, the same overflow stored as fp32 (not a converted value), and a slice of a tensor whose other channels hold NaN"""
    for L in rc.relu_launches(tile) + rc.residual_launches(tile) + rc.f32_output_launches(tile) + rc.slice_launches(tile):
        _run(L)


@pytest.mark.parametrize("tile", cc.ALL_TILES)
def test_row_shared_form(tile):
    for L in rc.row_shared(tile):
        _run(L)


@pytest.mark.parametrize("tile", cc.ALL_TILES)
def test_scalar_epilogue_with_an_s32_output(tile):
    """The scalar epilogue (csrc/conv_igemm_f16x3_kernel.h, `if (p.out_split) { if (p.range_flag) hn::range_note(...)`) runs where
    fill_params16 clears vec_epi.  An S32 output has Cout % 32 == 0 and a 16-byte aligned pixel stride, so of vec_epi's conditions
    only the alignment of bias (or of an fp32 residual) is left to the caller: the front end checks type and contiguity of the bias
    (ops._req), not its address, so a bias vector that starts 4 bytes into its buffer reaches the scalar epilogue.  No library query
    reports vec_epi; the route is that condition of csrc/conv_igemm_f16x3_plan.h, asserted here on the pointer itself."""
    c = rc.RAGGED
    assert _buffers(c).bias_store[1:].data_ptr() % 16 == 4 and c.cout % 8 == 0
    for L in rc.table(c, tile, "[scalar]") + rc.relu_launches(tile):
        _run(L, misaligned_bias=True)


@pytest.mark.parametrize("splits", [2, 7])
@pytest.mark.parametrize("kind,tile", [("fused", t) for t in cc.FUSED_REDUCE_TILES]
                         + [("reduce_kernel", t) for t in cc.ALL_TILES if t not in cc.FUSED_REDUCE_TILES])
def test_split_k_reductions(kind, tile, splits):
    """epi_finish8 from the fused reduction (tiles 3, 6, 7, 12) and from splitk_reduce_body (1, 2, 4, 8): the positions, the control,
    and two products of 2^17 and -(2^16 + 64) / -2^16 in k tiles of different splits -- the partial sums are far beyond the range,
    the stored 65472 is not, 65536 is; the ticket counters are back at zero"""
    from hn_amd import ops
    for L in rc.splitk(splits, kind, tile):
        _run(L)
    assert ops.tickets_nonzero() == 0


def _bank(b, c):
    return NS(w=b.w, bias=b.bias, w16=b.w16, stride=c.stride, pad=c.pad, dil=c.dil)


@pytest.mark.parametrize("kind", ["grouped_s32", "multi", "mixed"])
def test_grouped_multi_and_mixed_launches(kind):
    """one block of words for the whole launch: a plant in the first member, in the last, in the 64-row members of `mixed`, in the
    fp32-output member of `multi` (nothing is set), and every member multi-hot at exactly +-65504 (nothing is set)"""
    import ctypes as C
    from hn_amd import ops
    for name, members, want in rc.compound(kind):
        bufs = [_buffers(L.case) for L in members]
        assert len({id(b) for b in bufs}) == len(bufs)
        for L, b in zip(members, bufs):
            _plant(L, b, True)
        try:
            m0 = members[0].case
            if kind == "multi":
                fused = []
                items = [(b.x, _bank(b, L.case), dict(relu_cols=L.case.relu_cols, residual=b.res, out_split=L.case.out_split))
                         for L, b in zip(members, bufs)]
                outs, words = _words(lambda: ops.conv2d_nhwc_multi(items, fused=fused))
                assert fused == [True]
            else:
                if kind == "mixed":                    # mixed_small_mask's trigger, as tests/test_conv_exact_gpu.py asserts it
                    rows = [rr.rows_of(L.case) for L in members]
                    total = sum(-(-r // 128) for r in rows) * -(-m0.cout // 128)
                    assert 512 < total <= 3 * 512 and 0 < total % 512 <= 128 and min(rows) * 2 <= max(rows)
                    d = ops.make_conv_desc(1, sum(rows), 1, m0.cin, m0.cout, 3, 3, 1, 1, 1)
                    assert ops._lib.load().hn_conv2d_f16x3_pick_tile(C.byref(d)) == 1
                outs, words = _words(lambda: ops.conv2d_nhwc_grouped([b.x for b in bufs], [_bank(b, L.case) for L, b in zip(members, bufs)],
                                                                     pad=m0.pad, relu_cols=m0.relu_cols, out_split=m0.out_split))
            assert words == want, (name, words)
            for L, y in zip(members, outs):
                _check_output(L, y)
        finally:
            for L, b in zip(members, bufs):
                _plant(L, b, False)


@pytest.mark.parametrize("case", rc.HALO, ids=[c.name for c in rc.HALO])
def test_halo_kernel(case):
    for L in rc.halo(case):
        _run(L)


def test_stream_kernel_last_tile_of_one_pixel():
    for L in rc.stream():
        _run(L)


# --------------------------------------------------------------------------------------------------------------------------
# the carried pass
# --------------------------------------------------------------------------------------------------------------------------
def test_carry_launch_has_one_word_for_both_of_its_halves():
    """a grouped launch with an S32 output that carries a GroupNorm apply pass: a clean convolution with a bad carried value, a
    bad convolution with a clean carried tensor, both clean -- and 65504 against its neighbour in the carried tensor"""
    from hn_amd import ops
    levels = ((9, 13), (5, 7), (4, 8))
    cases = [cr.make_case(f"carry_{h}x{w}", 4, 2, h, w, 32, 128, 3, pad=1, relu_cols=128, out_split=True, bias=True) for h, w in levels]
    bufs = [_buffers(c) for c in cases]
    banks = [_bank(b, c) for b, c in zip(bufs, cases)]
    g = torch.Generator().manual_seed(7)
    carried = [(torch.randn((2, h, w, 64), generator=g) * 3.0).cuda() for h, w in ((5, 7), (3, 4))]
    tabs = [(torch.ones((2, 64), device="cuda"), torch.zeros((2, 64), device="cuda")) for _ in carried]
    dst = [torch.zeros((2, t.shape[1], t.shape[2], 2, 2, 32), device="cuda", dtype=torch.float16) for t in carried]
    kw = dict(pad=1, relu_cols=128, out_split=True, tile=1)
    assert ops.conv2d_nhwc_grouped([b.x for b in bufs], banks, carry_query=True, **kw) is True
    last = rc.single(cases[2], 1, rr.rows_of(cases[2]) - 1, 127)
    quiet = rr.launch("quiet", cases[2], 1, want=None)
    for conv, idx, value, want in ((quiet, None, None, rc.CLEAN), (last, None, None, rc.ACT), (quiet, (1, -1), NEXT, rc.ACT),
                                   (quiet, (1, -1), MAX, rc.CLEAN), (quiet, (0, 0), -NEXT, rc.CLEAN), (quiet, (0, 0), float("nan"), rc.ACT),
                                   (quiet, (0, 5 * 64 + 17), float("-inf"), rc.CLEAN), (quiet, (1, 17), float("inf"), rc.ACT)):
        src = [t.clone() for t in carried]
        if idx is not None:
            src[idx[0]].view(-1)[idx[1]] = value
        _plant(conv, bufs[2], True)
        try:
            outs, words = _words(lambda: ops.conv2d_nhwc_grouped([b.x for b in bufs], banks, carry=(src, tabs, dst, True), **kw))
            assert words == want, (conv.name, idx, value, words)
            _check_output(conv, outs[2])
            ref = ops.to_split_levels(src, tabs, relu=True)
            assert all(_same_bits(d, r) for d, r in zip(dst, ref))
        finally:
            _plant(conv, bufs[2], False)


# --------------------------------------------------------------------------------------------------------------------------
# the thin kernel's fused GroupNorm apply
# --------------------------------------------------------------------------------------------------------------------------
def test_thin_affine_notes_its_slice_and_nothing_else():
    """13 x 17 and 7 x 9 levels, raw fp32 tower outputs of 256 channels, head channels 128..255: a raw value whose applied value
    relu(raw * scale + shift) leaves the range (and a NaN) at the first and the last pixel of channel 128 and of channel 255 sets
    word 0; the same plants in channel 5, outside the slice, set nothing and change no output bit"""
    from hn_amd import ops
    launch = cc.GROUP7[-1]
    assert launch.affine and [(m.h, m.w) for m in launch.members] == [(13, 17), (7, 9)]
    prep = [cr.operands(m) for m in launch.members]
    o0 = prep[0]
    from hn_amd.weights import split_f16x3
    wt = torch.from_numpy(o0.w)
    bank = NS(w=wt.cuda(), bias=torch.from_numpy(o0.bias).cuda(), w16=split_f16x3(wt).cuda())
    aff = [(torch.from_numpy(o.scale).cuda(), torch.from_numpy(o.shift).cuda()) for o in prep]
    ch0 = launch.members[0].in_wide[1]
    ops.set_form("thin_form_flat", True)

    def run(ts):
        assert ops.thin_affine_applies(ts, bank)
        return _words(lambda: ops.conv3x3_thin_affine_levels(ts, aff, ch0, bank, relu_cols=launch.relu_cols))
    clean = [torch.from_numpy(o.raw).cuda() for o in prep]
    base, words = run(clean)
    assert words == rc.CLEAN
    for level in (0, 1):
        n, h, w, cw = clean[level].shape
        for (img, y, x) in ((0, 0, 0), (n - 1, h - 1, w - 1)):
            for ch, inside in ((128, True), (255, True), (5, False)):
                for kind in ("finite", "nan"):
                    ts = [t.clone() for t in clean]
                    # applied = relu(raw * scale + shift): raw = 1e30 with the sign of the scale gives +1e30 or +-2e30
                    s = float(prep[level].scale[img, ch])
                    ts[level][img, y, x, ch] = float("nan") if kind == "nan" else (1e30 if s > 0 else -1e30)
                    outs, words = run(ts)
                    assert words == (rc.ACT if inside else rc.CLEAN), (level, img, y, x, ch, kind, words)
                    if not inside:
                        assert all(_same_bits(a, b) for a, b in zip(outs, base))


# --------------------------------------------------------------------------------------------------------------------------
# the lifter's kernels
# --------------------------------------------------------------------------------------------------------------------------
def _graph():
    from hn_amd import ops
    if "graph" not in _state:
        L = rr.hand_graph()
        _state["graph"] = (L, ops.csr_graph(L, "cuda"), ops.cheby2_graph(L, "cuda"))
    return _state["graph"]


def _zero_bank(fin, fout, bias=None):
    from hn_amd import ops
    k = (3 * fin + 31) // 32 * 32
    w16 = torch.zeros((fout, k // 32, 2, 32), device="cuda", dtype=torch.float16)
    b = torch.zeros((fout,), device="cuda") if bias is None else bias
    return NS(w=torch.zeros((fout, 1, 1, k), device="cuda"), bias=b, w16=w16), NS(w=torch.zeros((fout, 1, 1, k), device="cuda"), bias=b,
                                                                                  w16=w16, w_frag=ops.fragment_order(w16))


@pytest.mark.parametrize("fin", [4, 256])
def test_fused_graph_conv_notes_its_in_kernel_basis(fin):
    """the three parts a0 = x, a1 = L x, a2 = (2 L L - I) x become fp16 pairs inside the kernel whatever the output type: on the
    hand-built graph each part alone leaves the range (x = 40000 under L = 2: a1 = 80000; two steps up: a2; where 2 L L - I has no
    diagonal: a0), with both gather forms (Fin 4: per-lane metadata; Fin 256: wave-uniform), both bank layouts and out_split both
    ways; at exactly 65504 nothing is set.  The bank is zero: where the parts' hi halves stay finite the output is exactly 0"""
    from hn_amd import ops
    L, g, g2 = _graph()
    banks = _zero_bank(fin, 32)
    for name, f, vertex, value, part in rc.fused_basis():
        if f != fin:
            continue
        x = np.zeros((3, L.shape[0], fin), F)                  # 30 rows: two row tiles, the second one partial
        x[0, vertex, 0] = x[2, vertex, fin - 1] = value
        parts = rr.basis_parts(L, x)
        want = [int(any(rr.bad(a).any() for a in parts)), 0, 0, 0]
        assert want == (rc.ACT if part else rc.CLEAN)
        xd = torch.from_numpy(x).cuda()
        for split in (False, True):
            for cw in banks:
                y, words = _words(lambda: ops.graph_conv_cheby3(g, g2, xd, cw, relu=False, out_split=split))
                assert words == want, (name, split, hasattr(cw, "w_frag"), words)
                if all((np.abs(a) < 65520).all() for a in parts):         # every hi half is finite: 0 * hi = 0
                    assert not bool(y.view(torch.int16 if split else torch.int32).any()), name


@pytest.mark.parametrize("up", [1, 2])
def test_fused_graph_conv_s32_epilogue(up):
    """out_split=True: zero bank and zero x, so v = relu(bias) + xin (Fi = Fout: the interpolation is the identity): one bias column
    at the boundary values, an xin one-hot at the positions; both replicated rows of `up` hold split(v), bit for bit"""
    from hn_amd import ops
    L, g, g2 = _graph()
    fin, fout, batch = 8, 64, 3
    v = L.shape[0]
    rows = batch * v
    xd = torch.zeros((batch, v, fin), device="cuda")
    bias = torch.zeros((fout,), device="cuda")
    xin = torch.zeros((batch, v, fout), device="cuda")
    cw = _zero_bank(fin, fout, bias)[1]
    nan = float("nan")

    def check(relu, want, tag):
        y, words = _words(lambda: ops.graph_conv_cheby3(g, g2, xd, cw, relu=relu, xin=xin, up=up, out_split=True))
        assert words == want, (tag, relu, words)
        val = (torch.relu(bias) if relu else bias).view(1, 1, fout) + xin
        val = torch.where(bias.isnan().view(1, 1, fout), torch.full_like(val, nan), val)
        expect = _split_dev(val.repeat_interleave(up, dim=1)).view(batch, v * up, 1, fout // 32, 2, 32)
        assert _same_bits(y, expect), tag
    for col in (0, 31, 32, fout - 1):
        for value, relu, want in ((MAX, True, rc.CLEAN), (NEXT, True, rc.ACT), (-MAX, False, rc.CLEAN), (-NEXT, False, rc.ACT),
                                  (-NEXT, True, rc.CLEAN), (nan, True, rc.ACT), (float("inf"), False, rc.ACT)):
            bias[col] = value
            check(relu, want, ("bias", col, value))
            bias[col] = 0.0
    for row in (0, 15, 16, rows - 1):
        for col in (0, 31, 32, fout - 1):
            for value, want in ((MAX, rc.CLEAN), (-NEXT, rc.ACT), (NEXT, rc.ACT)):
                xin.view(rows, fout)[row, col] = value
                check(True, want, ("xin", row, col, value))       # (the residual is added behind the ReLU: -next stays)
                xin.view(rows, fout)[row, col] = 0.0


def test_cheby3_basis_split_and_pad_split_rows():
    """the layer-by-layer lifter's two split producers: 65504 against its neighbour, NaN and inf at the first and at the last
    element of x0 and of x1, a2 = 2 L x1 - x0 alone out of range, and the zero padding channels; outputs are split(parts)"""
    from hn_amd import ops
    L, g, _ = _graph()
    v, f, b = L.shape[0], 4, 2
    cpad = 32

    def basis(x0, x1):
        out, words = _words(lambda: ops.cheby3_basis_split(g, torch.from_numpy(x0).cuda(), torch.from_numpy(x1).cuda()))
        a0, a1, a2 = rr.basis_split_parts(L, x0, x1)
        full = np.zeros((b, v, cpad), F)
        full[..., :f], full[..., f:2 * f], full[..., 2 * f:3 * f] = a0, a1, a2
        want = [int(rr.bad(full).any()), 0, 0, 0]
        assert sr.same_bits(out.cpu().numpy().reshape(b, v, cpad // 32, 2, 32), sr.to_s32(*sr.split(full))), "basis output"
        return words, want
    zero = np.zeros((b, v, f), F)
    for where in ((0, 0, 0), (b - 1, v - 1, f - 1)):
        for value, flagged in ((MAX, 0), (NEXT, 1), (-NEXT, 1), (np.nan, 1), (np.inf, 1)):
            for which in (0, 1):
                xs = [zero.copy(), zero.copy()]
                xs[which][where] = value
                words, want = basis(*xs)
                assert words == want == [flagged, 0, 0, 0], (where, value, which, words)
    x1 = zero.copy()
    x1[b - 1, 3, f - 1] = 40000.0                              # L[4,3] = 1: a2[4] = 80000 while x0 and x1 stay in range
    words, want = basis(zero, x1)
    assert words == want == rc.ACT
    x1[b - 1, 3, f - 1] = 32752.0
    words, want = basis(zero, x1)
    assert words == want == rc.CLEAN
    # pad_split_rows: [rows, 5] -> 32 channels
    rows, f5 = 7, 5
    for where in ((0, 0), (rows - 1, f5 - 1)):
        for value, flagged in ((MAX, 0), (NEXT, 1), (-NEXT, 1), (np.nan, 1), (-np.inf, 1)):
            x = np.zeros((rows, f5), F)
            x[where] = value
            out, words = _words(lambda: ops.pad_split_rows(torch.from_numpy(x).cuda(), 32))
            assert words == [flagged, 0, 0, 0], (where, value, words)
            full = np.zeros((rows, 32), F)
            full[:, :f5] = x
            assert sr.same_bits(out.cpu().numpy().reshape(rows, 1, 2, 32), sr.to_s32(*sr.split(full)))


def test_pose2mesh_engine_notes_an_overflowing_activation(golden_dir):
    """Pose2MeshEngine inside a range scope, synthetic weights: [0, 0, 0, 0] as they are.  With the first graph convolution's bank
    and bias scaled by a power of two (the bank stays within the fp16 range) its fp32 output -- computed first with oracle/graph_ref
    and asserted beyond 65504 -- is the next launch's basis: word 0.  A second factor puts that activation just beyond the range,
    where its fp16 hi half is still finite.  (Both scenarios also set the word without the basis note: later layers overflow in
    turn and the S32 epilogue in front of fc sees the NaN.  The note itself is pinned by the kernel tests above; this one pins the
    engine's scope and that an overflowing lifter cannot return a clean block of words.)"""
    from hn_amd import ops, synth
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from hn_amd.weights import split_f16x3
    from oracle import graph_ref, pose2mesh_ref
    g = np.load(golden_dir / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    eng = Pose2MeshEngine(sd, graphs, device="cuda")
    pose2d = torch.randn((1, 21, 2), generator=torch.Generator().manual_seed(5)).cuda()
    _, words = _words(lambda: eng.forward(pose2d))
    assert words == rc.CLEAN
    cw, fin_pad, relu = eng.cl[0]
    pose3d = eng.posenet(pose2d.reshape(1, -1)).view(1, 21, 3)
    x = ops.lifter_combine(pose2d, pose3d, fpad=fin_pad).cpu().numpy()
    w = cw.w.cpu().numpy().reshape(cw.w.shape[0], -1)[:, :3 * fin_pad].astype(np.float64)
    bias = cw.bias.cpu().numpy().astype(np.float64)
    L = graphs[-1].tocsr().astype(F)
    top = float(graph_ref.graph_conv_cheby3_ref(L, x, w, bias, relu=relu).max())
    assert 0 < top < 65504
    w0, b0 = cw.w.clone(), cw.bias.clone()
    # a power of two (every product scales exactly), and a factor that puts the largest activation at 65512: beyond the range by
    # six times the f16x3 bar of 2e-5 * 65512 = 1.3, yet below 65520, so its hi half stays finite and nothing downstream is inf
    for scale in (2.0 ** int(np.ceil(np.log2(2 * 65504 / top))), 65512.0 / top):
        cw.w, cw.bias = w0 * scale, b0 * scale
        ws = cw.w.cpu().numpy().reshape(w0.shape[0], -1)[:, :3 * fin_pad].astype(np.float64)
        assert float(np.abs(ws).max()) <= 65504                                # the bank itself stays in range
        top_scaled = float(graph_ref.graph_conv_cheby3_ref(L, x, ws, cw.bias.cpu().numpy().astype(np.float64), relu=relu).max())
        assert top_scaled > 65504 + 1.4, top_scaled                            # the case cannot pass vacuously
        cw.w16 = split_f16x3(cw.w.cpu()).cuda()
        cw.w_frag = ops.fragment_order(cw.w16)
        _, words = _words(lambda: eng.forward(pose2d))
        assert words == rc.ACT, (scale, words)


# --------------------------------------------------------------------------------------------------------------------------
# caller input: the preprocess kernels and stem_image
# --------------------------------------------------------------------------------------------------------------------------
INPUT_VALUES = ((MAX, rc.CLEAN), (NEXT, rc.INPUT_FINITE), (float("inf"), rc.INPUT_NONFINITE), (float("nan"), rc.INPUT_NONFINITE))


@pytest.mark.parametrize("form", ["tiled", "per pixel", "list"])
def test_preprocess_input_words(form):
    """mean 0, std 1 and an identity resize (64 x 64 -> 64 x 64 on a 72 x 80 canvas), so the value IS the pixel: 65504 sets nothing,
    the next float word 1, inf and NaN word 2 -- at the first and at the last pixel; the zero border and the canvas padding are
    silent and stay zero"""
    from hn_amd import ops
    n, h, w, ph, pw, b = 2, 64, 64, 72, 80, 3
    assert pc.form_of(h, w, h, w, ph, pw, b, n) == "t16" and pc.form_of(h, w, h, w, ph, pw, b, n, generic=True) == "pp"
    ops.set_form("preprocess_generic", form == "per pixel")
    mean, std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    for (img, ch, y, x) in ((0, 0, 0, 0), (n - 1, 2, h - 1, w - 1)):
        for value, want in INPUT_VALUES:
            src = torch.zeros((n, 3, h, w), device="cuda")
            src[img, ch, y, x] = value
            if form == "list":
                out, words = _words(lambda: ops.fcos_preprocess_list([src[i] for i in range(n)], [(h, w, h, w)] * n, ph, pw, mean, std,
                                                                     split=True, border=b))
            else:
                out, words = _words(lambda: ops.fcos_preprocess_split(src, h, w, ph, pw, mean, std, border=b))
            assert words == want, (form, img, ch, y, x, value, words)
            inner = torch.zeros_like(out, dtype=torch.bool)
            inner[:, :, b:b + h, b:b + w] = True
            assert not bool(out.masked_fill(inner, 0).view(torch.int16).any())          # border and canvas padding: +0
            if np.isfinite(value):
                hi, lo = sr.split(np.asarray([value], F))
                assert float(out[0, img, b + y, b + x, ch]) == float(hi[0]) and float(out[1, img, b + y, b + x, ch]) == float(lo[0])
                assert int((out.view(torch.int16) != 0).sum()) == (2 if float(lo[0]) else 1)


def test_stem_image_input_words_and_valid():
    """the same three classes of value through stem_image_nhwc4(valid=): a non-finite pixel is stored as 0 and moves valid 1 -> 2
    for its image only; an image with valid == 0 keeps its 0; a finite value beyond the range sets word 1 and is stored as it splits"""
    from hn_amd import ops
    n, h, w, b = 3, 5, 7, 3
    for (img, y, x, ch) in ((0, 0, 0, 0), (1, h - 1, w - 1, 3), (2, h - 1, w - 1, 3)):
        for value, want in INPUT_VALUES:
            src = torch.zeros((n, h, w, 4), device="cuda")
            src[img, y, x, ch] = value
            valid = torch.tensor([1, 1, 0], device="cuda", dtype=torch.int32)
            out, words = _words(lambda: ops.stem_image_nhwc4(src, border=b, valid=valid))
            assert words == want, (img, value, words)
            finite = bool(np.isfinite(value))
            expect = [1, 1, 0]
            if not finite and img != 2:
                expect[img] = 2
            assert valid.cpu().tolist() == expect, (img, value)
            hi, lo = sr.split(np.asarray([value if finite else 0.0], F))
            assert float(out[0, img, b + y, b + x, ch]) == float(hi[0]) and float(out[1, img, b + y, b + x, ch]) == float(lo[0])
            assert int((out.view(torch.int16) != 0).sum()) == (0 if not finite else 2 if float(lo[0]) else 1)
