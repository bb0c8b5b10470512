"""The yardstick of tests/test_graph_ops_gpu.py, checked without a GPU: on every input of the fused kernel's case table the
three-term split arithmetic (oracle.graph_ref.graph_conv_model) stays within the f16x3 bar against fp64, and the same arithmetic
with either cross term left out does not -- so the bar passes a correct kernel and can fail a wrong one."""
import numpy as np
import pytest

from graph_cases import F16X3_BAR, FUSED_CASES, INTERP_BAR, INTERP_CASES, case_id, fused_inputs, interp_inputs, residual_width
from oracle import graph_ref

IDS = [case_id(i) for i in range(len(FUSED_CASES))]


def _errors(i):
    c, d = FUSED_CASES[i], fused_inputs(i)
    args = (d["L"], d["x"], d["w"], d["bias"], bool(c.relu), d["xin"], c.up)
    ref = graph_ref.graph_conv_cheby3_ref(*args)
    scale = max(1.0, float(np.abs(ref).max()))
    err = {drop: float(np.abs(graph_ref.graph_conv_model(*args, drop=drop) - ref).max()) / scale for drop in (None, "lo_hi", "hi_lo")}
    return ref, err


@pytest.mark.parametrize("i", range(len(FUSED_CASES)), ids=IDS)
def test_three_term_model_is_within_the_bar_and_two_terms_are_not(i):
    c = FUSED_CASES[i]
    ref, err = _errors(i)
    print(IDS[i], {k: f"{v:.2e}" for k, v in err.items()})
    assert ref.shape == (c.batch, c.v * c.up, c.fout) and np.isfinite(ref).all()
    assert err[None] <= F16X3_BAR, err
    assert err["lo_hi"] > F16X3_BAR and err["hi_lo"] > F16X3_BAR, err


@pytest.mark.parametrize("fi,fo,bar", INTERP_CASES, ids=[f"{c[0]}-{c[1]}" for c in INTERP_CASES])
def test_interp_bars_come_from_the_fp32_arithmetic(fi, fo, bar):
    """feat_interp_add in fp32 as the kernel and ATen compute it (fp32 source index) against fp64 on the GPU test's inputs: within
    the 1e-5 bar where that bar is used, and where a case has a bar of its own, that bar is 4 x this error and no more."""
    err = max(float(np.abs(graph_ref.feat_interp_add_model(xin, y, up).astype(np.float64) - graph_ref.feat_interp_add_ref(xin, y, up)).max())
              for up, xin, y in interp_inputs(fi, fo))
    print(f"feat_interp_add model {fi}->{fo}: {err:.3e}  bar {bar:.3e}")
    if bar == INTERP_BAR:
        assert err <= INTERP_BAR
    else:
        assert err > INTERP_BAR and 4.0 * err <= bar <= 4.05 * err


def test_interp_cases_cover_both_directions_and_one_feature():
    assert any(fi > fo for fi, fo, _ in INTERP_CASES) and any(fi < fo for fi, fo, _ in INTERP_CASES)
    assert any(fi == fo for fi, fo, _ in INTERP_CASES) and any(fi == 1 for fi, fo, _ in INTERP_CASES)
    assert all(bar >= INTERP_BAR for _, _, bar in INTERP_CASES) and sum(bar > INTERP_BAR for _, _, bar in INTERP_CASES) == 2


def test_case_table_covers_what_the_entry_point_accepts():
    cs = FUSED_CASES
    assert {c.fin for c in cs} >= {4, 8, 12, 36, 64, 128, 252, 256}
    assert {c.fout for c in cs} >= {1, 3, 16, 17, 40, 64, 96, 250, 256}
    assert {c.v for c in cs} >= {1, 5, 21, 49, 100} and {c.batch for c in cs} >= {1, 2, 3, 7}
    assert {c.up for c in cs} == {1, 2, 3, 4} and {c.fi for c in cs} == {None, "1", "q", "eq", "2x"}
    assert {c.relu for c in cs} == {0, 1} and {c.bias for c in cs} == {0, 1}
    assert {c.fout for c in cs if c.split} == {c.fout for c in cs if c.fout % 32 == 0} == {64, 96, 256}
    assert any((c.v * c.batch) % 16 for c in cs) and any(c.v < 16 and c.batch * c.v > 2 * c.v for c in cs)
    assert any(residual_width(c) > c.fout for c in cs) and all(residual_width(c) > 0 for c in cs if c.fi)
    assert any(c.split and c.fi and c.up > 1 for c in cs)
    assert 38 <= len(cs) <= 44


def test_random_graph_has_every_listed_row_length_sorted_columns_and_unit_rows():
    assert graph_ref.DEGREES == (0, 1, 4, 5, 8, 9, 16, 17, 40, 7)
    for v in (49, 100, 1152):
        m = graph_ref.random_graph(v, seed=v)
        deg = np.diff(m.indptr)
        assert set(deg.tolist()) == set(graph_ref.DEGREES)
        assert m.dtype == np.float32 and m.indptr.dtype == np.int32 and m.indices.dtype == np.int32
        for r in range(v):
            idx = m.indices[m.indptr[r]:m.indptr[r + 1]]
            assert (np.diff(idx) > 0).all() and (idx >= 0).all() and (idx < v).all()
            if len(idx):
                assert abs(float(np.abs(m.data[m.indptr[r]:m.indptr[r + 1]].astype(np.float64)).sum()) - 1.0) < 1e-6
    for v in (1, 5, 21):                        # small graphs: the lengths are capped at V, never without an entry, empty rows stay
        deg = np.diff(graph_ref.random_graph(v, seed=v).indptr)
        assert 1 <= deg.max() <= v and (deg.min() == 0 or v == 1)
    a, b = graph_ref.random_graph(100, seed=3), graph_ref.random_graph(100, seed=3)
    assert (a != b).nnz == 0 and (a != graph_ref.random_graph(100, seed=4)).nnz > 0


def test_second_order_rows_sit_on_both_sides_of_the_gather_rounds():
    """2 L L - I is gathered eight neighbours a round: rows of at most and of more than 8, 16 and 24 entries all occur (on the
    graphs of the case table taken together and on the 1152-vertex graph of the grid-stride cases), and an empty row of L
    keeps its -1 on the diagonal."""
    lens = np.concatenate([np.diff(graph_ref.cheby2(fused_inputs(i)["L"]).indptr) for i in range(len(FUSED_CASES))])
    big = np.diff(graph_ref.cheby2(graph_ref.random_graph(1152, seed=1152)).indptr)
    for where in (lens, big):
        for lo, hi in ((1, 8), (9, 16), (17, 24), (25, 10 ** 6)):
            assert ((where >= lo) & (where <= hi)).any(), (lo, hi)
    L = graph_ref.random_graph(100, seed=0)
    q = graph_ref.cheby2(L)
    for r in np.nonzero(np.diff(L.indptr) == 0)[0]:
        assert q.indptr[r + 1] - q.indptr[r] == 1 and q.indices[q.indptr[r]] == r and q.data[q.indptr[r]] == -1.0


def test_cheby2_is_the_matrix_the_engine_builds():
    """oracle.graph_ref.cheby2 restates ops.cheby2_graph (fp64 product, one rounding per coefficient): the reference and the
    kernel are given the same second-order coefficients."""
    import torch
    from hn_amd import ops
    for v, seed in ((1, 0), (21, 1), (100, 2)):
        L = graph_ref.random_graph(v, seed)
        g, q = ops.cheby2_graph(L, "cpu"), graph_ref.cheby2(L)
        assert g.v == v and torch.equal(g.indptr, torch.from_numpy(q.indptr.astype(np.int32)))
        assert torch.equal(g.indices, torch.from_numpy(q.indices.astype(np.int32))) and torch.equal(g.values, torch.from_numpy(q.data))
        g1 = ops.csr_graph(L, "cpu")
        assert torch.equal(g1.indices, torch.from_numpy(L.indices)) and torch.equal(g1.values, torch.from_numpy(L.data))


def test_references_agree_with_dense_fp64_and_torch():
    """The fp64 helpers against the definition written densely, and the interpolation against ATen's."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    L = graph_ref.random_graph(21, seed=9)
    d = L.toarray().astype(np.float64)
    x = rng.standard_normal((2, 21, 8)).astype(np.float32)
    w = rng.standard_normal((5, 24)).astype(np.float32)
    bias = rng.standard_normal(5).astype(np.float32)
    xin = rng.standard_normal((2, 21, 3)).astype(np.float32)
    x64 = x.astype(np.float64)
    lx = np.einsum("vu,buf->bvf", d, x64)
    assert np.abs(graph_ref.spmm_ref(L, x) - lx).max() < 1e-14
    q = graph_ref.cheby2(L).toarray().astype(np.float64)
    assert np.abs(q - (2 * d @ d - np.eye(21))).max() < 1e-7          # (one fp32 rounding per coefficient)
    basis = np.concatenate([x64, lx, np.einsum("vu,buf->bvf", q, x64)], axis=2)
    lin = torch.from_numpy(basis @ w.astype(np.float64).T + bias)
    want = torch.relu(lin) + F.interpolate(torch.from_numpy(xin).double(), size=5, mode="linear", align_corners=False)
    want = want.repeat_interleave(3, dim=1).numpy()
    got = graph_ref.graph_conv_cheby3_ref(L, x, w, bias, True, xin, 3)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-12
    b = graph_ref.basis_ref(L, x, lx.astype(np.float32), 64)
    assert b.shape == (2, 21, 64) and np.abs(b[..., 16:24] - (2 * np.einsum("vu,buf->bvf", d, lx.astype(np.float32).astype(np.float64)) - x64)).max() < 1e-14
    assert (b[..., 24:] == 0).all() and (b[..., :8] == x64).all()
    for fi, fo in ((64, 256), (256, 64), (7, 7), (1, 40), (62, 250), (500, 250)):
        a = rng.standard_normal((1, 3, fi)).astype(np.float32)
        y = rng.standard_normal((1, 3, fo)).astype(np.float32)
        t = F.interpolate(torch.from_numpy(a).double(), size=fo, mode="linear", align_corners=False).numpy() + y
        assert np.abs(graph_ref.feat_interp_add_ref(a, y, 2) - np.repeat(t, 2, axis=1)).max() < 1e-12
    xr = rng.standard_normal((2, 40)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, 40), rng.standard_normal(40)
    res = rng.standard_normal((2, 5))
    wl = rng.standard_normal((5, 40))
    want = np.maximum(np.maximum(xr * sc + sh, 0) @ wl.T + bias + res, 0)
    assert np.abs(graph_ref.linear_rows_ref(xr, wl, bias, sc, sh, res, True) - want).max() < 1e-12
