"""The lifter's graph kernels (csrc/graph_ops.hip) against fp64 (oracle/graph_ref.py) over what their entry points accept:
row lengths on every gather-round boundary and empty rows, dead column tiles, Fi > Fout, up 1..4, graphs smaller than a row
tile, ragged k padding, the grid-stride loops, deep and strided Linear banks -- every output a view into a NaN-filled buffer
that must come back untouched outside the view.

Bars (none of them taken from a kernel's output):
  fused kernel, chain + 1x1 convolution   2e-5 * max(1, max |ref|)       the f16x3 bar of tests/test_conv_gpu.py; the
                                          three-term arithmetic stays under 2.5e-6 of that scale on these inputs and a
                                          dropped cross term misses it by >= 4x (tests/test_graph_ops_cpu.py)
  fused vs chain                          3e-6 * scale                   as test_fused_graph_conv_matches_the_layer_by_layer_form
  spmm / basis                            1e-6 / 2e-6 * scale            as test_graph_ops_match_torch
  feat_interp_add                         1e-5 absolute on N(0, 1) data  as test_graph_ops_match_torch; 62 -> 250 and 250 -> 62
                                          have 4 x the error of the fp32 source index itself (graph_cases.INTERP_CASES)
  linear_rows                             2e-6 * scale * max(1, sqrt(K / 64))   as test_linear_rows_matches_fp64
Every figure is printed (pytest -s) before it is asserted."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from graph_cases import F16X3_BAR, FUSED_CASES, INTERP_BAR, INTERP_CASES, case_id, fused_inputs, interp_inputs, padded_bank
from oracle import graph_ref

pytestmark = pytest.mark.gpu
IDS = [case_id(i) for i in range(len(FUSED_CASES))]
GUARD = 4096          # canary elements in front of and behind every output view (keeps the view 16-byte aligned)


def _canary(numel, dtype=torch.float32):
    """-> (buffer of GUARD + numel + GUARD NaNs, the view of the middle `numel`)"""
    buf = torch.full((numel + 2 * GUARD,), float("nan"), device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + numel]


def _check_canary(buf, what, written=True):
    """Everything outside the view still holds the NaN it was filled with, bit for bit; inside, nothing is NaN (or, for a
    refused call, everything still is)."""
    torch.cuda.synchronize()
    ints = torch.int32 if buf.dtype == torch.float32 else torch.int16
    want = torch.full((1,), float("nan"), dtype=buf.dtype).view(ints).item()
    bits = buf.view(ints)
    numel = buf.numel() - 2 * GUARD
    assert bool((bits[:GUARD] == want).all()) and bool((bits[GUARD + numel:] == want).all()), f"{what}: write outside the output"
    inside = bits[GUARD:GUARD + numel]
    if written:
        assert not bool(torch.isnan(buf[GUARD:GUARD + numel]).any()), f"{what}: NaN (an element never written?) inside the output"
    else:
        assert bool((inside == want).all()), f"{what}: a refused call wrote to the output"


def _report(kernel, case, err, bar):
    print(f"[graph-ops] {kernel:<22} {case:<44} err {err:.3e}  bar {bar:.3e}")
    assert err <= bar, (kernel, case, err, bar)


def _err(got, ref):
    """max |got - ref| over EVERY element, in fp64"""
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max())


def _banks(w, bias, fin):
    """[Fout, 3 Fin] numpy -> the filter bank in the standard layout and the same bank with its MFMA-fragment-order copy"""
    from hn_amd import ops
    from hn_amd.weights import split_f16x3
    wp = torch.from_numpy(padded_bank(w, fin)).view(w.shape[0], 1, 1, -1)
    w16 = split_f16x3(wp).cuda()
    b = None if bias is None else torch.from_numpy(bias).cuda()
    std = types.SimpleNamespace(w=wp.cuda(), bias=b, w16=w16)
    frag = types.SimpleNamespace(w=std.w, bias=b, w16=w16, w_frag=ops.fragment_order(w16))
    return std, frag


def _device_case(i):
    from hn_amd import ops
    c, d = FUSED_CASES[i], fused_inputs(i)
    g, g2 = ops.csr_graph(d["L"], "cuda"), ops.cheby2_graph(d["L"], "cuda")
    x = torch.from_numpy(d["x"]).cuda()
    xin = None if d["xin"] is None else torch.from_numpy(d["xin"]).cuda()
    ref = graph_ref.graph_conv_cheby3_ref(d["L"], d["x"], d["w"], d["bias"], bool(c.relu), d["xin"], c.up)
    return c, d, g, g2, x, xin, ref


def _fused(c, g, g2, x, cw, xin):
    """One launch into a canary buffer -> (fp32 [B, V up, Fout], the buffer)"""
    from hn_amd import ops
    n = c.batch * c.v * c.up * c.fout
    buf, view = _canary(2 * n if c.split else n, torch.float16 if c.split else torch.float32)
    y = ops.graph_conv_cheby3(g, g2, x, cw, relu=bool(c.relu), xin=xin, up=c.up, out_split=bool(c.split), out=view)
    assert y.data_ptr() == view.data_ptr()
    if c.split:
        y = ops.from_split(view.view(c.batch, c.v * c.up, 1, c.fout // 32, 2, 32))
    return y.view(c.batch, c.v * c.up, c.fout), buf


# ---------------------------------------------------------------------------------------------------------------------------
# the fused kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(FUSED_CASES)), ids=IDS)
def test_fused_graph_conv_matches_fp64(i):
    """hn_graph_conv_cheby3_f16x3 vs graph_conv_cheby3_ref, with the standard bank and with ops.fragment_order (bit-identical)."""
    c, d, g, g2, x, xin, ref = _device_case(i)
    std, frag = _banks(d["w"], d["bias"], c.fin)
    y_std, buf_std = _fused(c, g, g2, x, std, xin)
    y_frag, buf_frag = _fused(c, g, g2, x, frag, xin)
    _check_canary(buf_std, IDS[i] + " standard bank")
    _check_canary(buf_frag, IDS[i] + " fragment order")
    scale = max(1.0, float(np.abs(ref).max()))
    _report("graph_conv_cheby3", IDS[i], _err(y_std, ref), F16X3_BAR * scale)
    assert torch.equal(y_std, y_frag), "the two bank layouts give different results"
    assert torch.equal(buf_std.view(torch.int16), buf_frag.view(torch.int16))       # (bit for bit, as stored)


@pytest.mark.parametrize("i", range(len(FUSED_CASES)), ids=IDS)
def test_layer_chain_matches_fp64_and_the_fused_kernel(i):
    """spmm -> basis -> 1x1 convolution -> feat_interp_add on the shapes of the case table: vs fp64 at the f16x3 bar, and the
    fused kernel vs this chain at 3e-6 of the scale (what test_fused_graph_conv_matches_the_layer_by_layer_form asserts on the
    mesh net's own shapes)."""
    from hn_amd import ops
    c, d, g, g2, x, xin, ref = _device_case(i)
    std, _ = _banks(d["w"], d["bias"], c.fin)
    basis = ops.cheby3_basis_split(g, x, ops.spmm_csr(g, x))
    want = ops.conv2d_nhwc(basis, std.w, std.bias, relu=bool(c.relu), w16=std.w16, splitk=False).view(c.batch, c.v, c.fout)
    if xin is not None:
        want = ops.feat_interp_add(xin, want.contiguous(), up=c.up)
    elif c.up > 1:
        want = want.repeat_interleave(c.up, dim=1)          # (the chain has no up-sampling without a residual: a copy)
    got, buf = _fused(c, g, g2, x, std, xin)
    _check_canary(buf, IDS[i])
    scale = max(1.0, float(np.abs(ref).max()))
    _report("chain + conv1x1", IDS[i], _err(want, ref), F16X3_BAR * scale)
    _report("fused vs chain", IDS[i], float((got - want).abs().max()), 3e-6 * max(1.0, want.abs().max().item()))


# ---------------------------------------------------------------------------------------------------------------------------
# the chain's own kernels, through the C ABI (output pointers into canary buffers, Cpad free)
# ---------------------------------------------------------------------------------------------------------------------------
def _ck(status, what):
    from hn_amd import _lib
    _lib.check(status, what)


def _spmm(g, x):
    from hn_amd import _lib, ops
    b, v, f = x.shape
    buf, y = _canary(x.numel())
    _ck(_lib.load().hn_spmm_csr_f32(g.indptr.data_ptr(), g.indices.data_ptr(), g.values.data_ptr(), v, x.data_ptr(), y.data_ptr(),
                                    b, f, ops._stream()), "hn_spmm_csr_f32")
    return y.view(b, v, f), buf


def _basis(g, x0, x1, cpad):
    from hn_amd import _lib, ops
    b, v, f = x0.shape
    buf, out = _canary(b * v * cpad * 2, torch.float16)
    _ck(_lib.load().hn_cheby3_basis_split(g.indptr.data_ptr(), g.indices.data_ptr(), g.values.data_ptr(), v, x0.data_ptr(),
                                          x1.data_ptr(), out.data_ptr(), b, f, cpad, ops._stream()), "hn_cheby3_basis_split")
    return out.view(b, v, 1, cpad // 32, 2, 32), buf


def _interp(xin, y, up):
    from hn_amd import _lib, ops
    b, v, fo = y.shape
    buf, out = _canary(b * v * up * fo)
    _ck(_lib.load().hn_feat_interp_add_f32(xin.data_ptr(), y.data_ptr(), out.data_ptr(), b * v, xin.shape[2], fo, up,
                                           ops._stream()), "hn_feat_interp_add_f32")
    return out.view(b, v * up, fo), buf


def _spmm_and_basis(L, x_np, cpads, tag, chunk=None):
    from hn_amd import ops
    g = ops.csr_graph(L, "cuda")
    x = torch.from_numpy(x_np).cuda()
    b, v, f = x.shape
    y1, buf = _spmm(g, x)
    _check_canary(buf, "spmm " + tag)
    y1_np = y1.cpu().numpy()
    ref = graph_ref.spmm_ref(L, x_np)
    _report("spmm_csr", tag, _err(y1_np, ref), 1e-6 * max(1.0, float(np.abs(ref).max())))
    del ref
    for cpad in cpads:
        out16, buf = _basis(g, x, y1, cpad)
        _check_canary(buf, f"basis {tag} cpad {cpad}")
        got = ops.from_split(out16).view(b, v, cpad).cpu().numpy()
        raw = out16.view(b, v, cpad // 32, 2, 32).cpu().numpy()
        step = chunk or b
        err, scale = 0.0, 1.0
        for b0 in range(0, b, step):          # (fp64 in slices of the batch: the large case is 450 MB of fp64 at once)
            want = graph_ref.basis_ref(L, x_np[b0:b0 + step], y1_np[b0:b0 + step], cpad)
            err = max(err, _err(got[b0:b0 + step, :, :3 * f], want[..., :3 * f]))
            scale = max(scale, float(np.abs(want).max()))
        _report("cheby3_basis_split", f"{tag} cpad {cpad}", err, 2e-6 * scale)
        # the padding channels are exactly zero, hi and lo halves alike
        assert not got[..., 3 * f:].any()
        pad_raw = raw.transpose(0, 1, 3, 2, 4).reshape(b, v, 2, cpad)[..., 3 * f:]
        assert not np.ascontiguousarray(pad_raw).view(np.uint16).any(), "padding halves are not +0"


@pytest.mark.parametrize("f", [4, 24, 100, 256])
def test_spmm_and_basis_match_fp64(f):
    """hn_spmm_csr_f32 and hn_cheby3_basis_split on the random graphs, Cpad = pad32(3 F) and one 32-channel block more."""
    rng = np.random.default_rng(70 + f)
    for v, b in ((1, 7), (5, 3), (21, 2), (49, 1), (100, 3)):
        L = graph_ref.random_graph(v, seed=200 + v)
        x = rng.standard_normal((b, v, f)).astype(np.float32)
        _spmm_and_basis(L, x, (graph_ref.pad32(3 * f), graph_ref.pad32(3 * f) + 32), f"V{v} b{b} F{f}")


@pytest.mark.parametrize("fi,fo,bar", INTERP_CASES, ids=[f"{c[0]}-{c[1]}" for c in INTERP_CASES])
def test_feat_interp_add_matches_fp64(fi, fo, bar):
    """Bars: graph_cases.INTERP_CASES (1e-5; the two inexact ratios with a source index near 62 and 250 have 4 x the error of
    the fp32 arithmetic itself, measured on the CPU)."""
    for up, xin, y in interp_inputs(fi, fo):
        got, buf = _interp(torch.from_numpy(xin).cuda(), torch.from_numpy(y).cuda(), up)
        _check_canary(buf, f"feat_interp_add {fi}->{fo} up {up}")
        _report("feat_interp_add", f"{fi}->{fo} up {up}", _err(got, graph_ref.feat_interp_add_ref(xin, y, up)), bar)


def test_grid_stride_loops_at_batch_64():
    """Batch 64 x 1152 vertices x 256 features: 18432 (spmm, basis) and 73728 (residual) blocks of work on a grid capped at
    8192 -- the chain is the lifter's path above FUSED_MAX_BATCH."""
    rng = np.random.default_rng(64)
    L = graph_ref.random_graph(1152, seed=1152)
    x = rng.standard_normal((64, 1152, 256)).astype(np.float32)
    _spmm_and_basis(L, x, (768,), "V1152 b64 F256", chunk=8)
    xin = rng.standard_normal((64, 1152, 64)).astype(np.float32)
    got, buf = _interp(torch.from_numpy(xin).cuda(), torch.from_numpy(x).cuda(), 1)
    _check_canary(buf, "feat_interp_add b64")
    _report("feat_interp_add", "V1152 b64 64->256", _err(got, graph_ref.feat_interp_add_ref(xin, x, 1)), INTERP_BAR)


# ---------------------------------------------------------------------------------------------------------------------------
# hn_linear_rows_f16x3
# ---------------------------------------------------------------------------------------------------------------------------
def _linear_bar(ref, k):
    return 2e-6 * max(1.0, float(np.abs(ref).max())) * max(1.0, (k / 64) ** 0.5)


@pytest.mark.parametrize("m,k", [(1, 4128), (1, 8192), (1, 16384), (2, 8192), (3, 5120)])
def test_linear_rows_deep_banks_match_fp64(m, k):
    """Banks deeper than one 4096-channel pass (the kernel's `if (k0) request(k0)` branch), up to the 64 KB of staged
    activations the entry point allows; plain, and with the pre-activation affine, residual and output ReLU."""
    from hn_amd import ops
    from hn_amd.pose2mesh_engine import _dense
    rng = np.random.default_rng(m * 100000 + k)
    for n in (1, 7, 64):
        w = (rng.standard_normal((n, k)) * (2.0 / k) ** 0.5).astype(np.float32)
        bias = rng.standard_normal(n).astype(np.float32)
        cw = _dense(torch.from_numpy(w).double(), torch.from_numpy(bias).double(), "cuda")
        x = rng.standard_normal((m, k)).astype(np.float32)
        sc, sh = rng.uniform(0.5, 1.5, k).astype(np.float32), (rng.standard_normal(k) * 0.3).astype(np.float32)
        res = rng.standard_normal((m, n)).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        ref0 = graph_ref.linear_rows_ref(x, w, bias)
        ref1 = graph_ref.linear_rows_ref(x, w, bias, sc, sh, res, True)
        y0 = ops.linear_rows(xd, cw)
        y1 = ops.linear_rows(xd, cw, scale=torch.from_numpy(sc).cuda(), shift=torch.from_numpy(sh).cuda(),
                             residual=torch.from_numpy(res).cuda(), relu=True)
        _report("linear_rows", f"M{m} K{k} N{n} plain", _err(y0, ref0), _linear_bar(ref0, k))
        _report("linear_rows", f"M{m} K{k} N{n} affine+res+relu", _err(y1, ref1), _linear_bar(ref0, k))


@pytest.mark.parametrize("m,k_real,k,n", [(3, 70, 96, 13), (2, 4100, 4128, 7), (4, 42, 64, 64)])
def test_linear_rows_strides(m, k_real, k, n):
    """x_stride > k_real with NaN behind the real columns, res_stride > n with NaN behind the row, y_stride > n with a NaN
    canary between the rows that must survive (the ABI's strides, which ops.linear_rows always passes dense)."""
    from hn_amd import _lib, ops
    from hn_amd.pose2mesh_engine import _dense
    rng = np.random.default_rng(k_real)
    xs, rs, ys = k_real + 5, n + 3, n + 4
    w = (rng.standard_normal((n, k_real)) * (2.0 / k_real) ** 0.5).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    cw = _dense(torch.from_numpy(w).double(), torch.from_numpy(bias).double(), "cuda", cin_pad=k)
    x = rng.standard_normal((m, k_real)).astype(np.float32)
    res = rng.standard_normal((m, n)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, k_real).astype(np.float32), (rng.standard_normal(k_real) * 0.3).astype(np.float32)
    xd = torch.full((m, xs), float("nan"), device="cuda")
    xd[:, :k_real] = torch.from_numpy(x)
    rd = torch.full((m, rs), float("nan"), device="cuda")
    rd[:, :n] = torch.from_numpy(res)
    scd, shd = torch.from_numpy(sc).cuda(), torch.from_numpy(sh).cuda()
    buf, view = _canary(m * ys)
    _ck(_lib.load().hn_linear_rows_f16x3(xd.data_ptr(), m, xs, k_real, scd.data_ptr(), shd.data_ptr(), cw.w16.data_ptr(), k, n,
                                         cw.bias.data_ptr(), rd.data_ptr(), rs, 1, view.data_ptr(), ys, ops._stream()),
        "hn_linear_rows_f16x3")
    torch.cuda.synchronize()
    rows = view.view(m, ys)
    _check_canary(torch.cat([buf[:GUARD], rows[:, :n].reshape(-1), buf[GUARD + m * ys:]]), "linear_rows strided")
    gaps = rows[:, n:].contiguous().view(torch.int32)
    assert bool((gaps == torch.full((1,), float("nan")).view(torch.int32).item()).all()), "write between the rows of y"
    ref = graph_ref.linear_rows_ref(x, w, bias, sc, sh, res, True)
    _report("linear_rows", f"strided M{m} k_real {k_real} K{k} N{n}", _err(rows[:, :n], ref), _linear_bar(ref, k))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: argument checks of the entry points -- an error status and its message, and nothing launched
# ---------------------------------------------------------------------------------------------------------------------------
def _refused(status, match, buf):
    from hn_amd import _lib
    assert status != 0, "the call was accepted"
    msg = (_lib.load().hn_last_error() or b"").decode()
    assert match in msg, (match, msg)
    _check_canary(buf, match, written=False)


def test_graph_conv_refuses_what_it_cannot_run():
    from hn_amd import _lib, ops
    lib = _lib.load()
    L = graph_ref.random_graph(21, seed=1)
    g, g2 = ops.csr_graph(L, "cuda"), ops.cheby2_graph(L, "cuda")
    other = ops.cheby2_graph(graph_ref.random_graph(5, seed=1), "cuda")
    x = torch.randn((1, 21, 260), generator=torch.Generator().manual_seed(0)).cuda()
    w16 = torch.zeros((257, 800 // 32, 2, 32), dtype=torch.float16, device="cuda")        # (large enough for every call below)
    buf, y = _canary(21 * 5 * 260)

    def call(fin=8, fout=16, up=1, split=0, q=g2):
        return lib.hn_graph_conv_cheby3_f16x3(C.byref(ops._csr_struct(g)), C.byref(ops._csr_struct(q)), x.data_ptr(), 1, fin,
                                              w16.data_ptr(), 0, None, fout, 1, None, 0, up, y.data_ptr(), split, ops._stream())

    for kw, match in (({"fin": 6}, "Fin must be"), ({"fin": 260}, "Fin must be"), ({"fout": 0}, "Fout must be"),
                      ({"fout": 257}, "Fout must be"), ({"up": 0}, "up-sampling"), ({"up": 5}, "up-sampling"),
                      ({"fout": 40, "split": 1}, "Fout % 32"), ({"q": other}, "bad graph")):
        _refused(call(**kw), match, buf)
    with pytest.raises(RuntimeError, match="Fout % 32"):        # the same through the wrapper: the library's error, raised
        ops.graph_conv_cheby3(g, g2, x[:, :, :8].contiguous(),
                              types.SimpleNamespace(w=torch.zeros((40, 1, 1, 32), device="cuda"), bias=None, w16=w16),
                              out_split=True, out=y.view(torch.float16)[:21 * 40 * 2])
    _check_canary(buf, "wrapper", written=False)
    assert call() == 0                                           # (the arguments around the refused ones were fine)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y[:21 * 16]).any())


def test_linear_rows_refuses_what_it_cannot_run():
    from hn_amd import _lib, ops
    lib = _lib.load()
    w16 = torch.zeros((2, 8224 // 32, 2, 32), dtype=torch.float16, device="cuda")
    x = torch.zeros((5, 8224), device="cuda")
    buf, y = _canary(5 * 2)

    def call(m, k):
        return lib.hn_linear_rows_f16x3(x.data_ptr(), m, k, k, None, None, w16.data_ptr(), k, 2, None, None, 0, 0, y.data_ptr(), 2,
                                        ops._stream())

    _refused(call(5, 64), "1..4 rows", buf)
    _refused(call(2, 8224), "64 KB", buf)                        # 2 * 8224 * 4 bytes of activations
    _refused(call(4, 4128), "64 KB", buf)
    assert call(2, 8192) == 0                                    # exactly 64 KB is taken
    torch.cuda.synchronize()
    assert bool((y[:4] == 0).all())
