"""The exact-arithmetic convolution reference (tests/conv_exact_ref.py) without a GPU: every case of tests/conv_exact_cases.py keeps
its family's representation claim (weights.split_f16x3 and the S32 rule return exactly the integer and the lo half) and the
exactness condition S < 2^10 (2^6 for subnormal lo parts); the three-term model is the fp64 convolution less the lo*lo term; the
numpy walk of the implicit GEMM equals the model on every group-1 to group-3 case; and every mutant of the walk changes a bit on
some case -- so the bitwise comparison of test_conv_exact_gpu.py is known to be able to fail.  The routers' triggers are asserted
here as well (the library's queries are host code)."""
import numpy as np
import pytest
import torch

import conv_exact_cases as cc
import conv_exact_ref as cr
import split_ref as sr

F, H, D = np.float32, np.float16, np.float64
_ops_cache = {}


def _operands(c):
    if c.name not in _ops_cache:
        _ops_cache[c.name] = cr.operands(c)
    return _ops_cache[c.name]


def test_the_families_split_exactly_and_q11_does_not():
    """(q, A) = (12, 2), (12, 4), (16, 1): hi = a, lo = b under the S32 rule and under weights.split_f16x3; q = 11 fails, as it
    must (2^-11 is a rounding tie at |a| = 1); and a = 0 with b != 0 puts b into the hi half"""
    from hn_amd.weights import split_f16x3
    rng = np.random.default_rng(0)
    for q, A in ((12, 2), (12, 4), (16, 1)):
        a = (rng.integers(1, A + 1, size=(8, 3, 3, 64)) * rng.choice(np.array([-1, 1]), size=(8, 3, 3, 64))).astype(D)
        b = rng.integers(-1, 2, size=a.shape) * 2.0 ** -q
        v = (a + b).astype(F)
        hi, lo = sr.split(v)
        assert (hi.astype(D) == a).all() and (lo.astype(D) == b).all()
        w16 = split_f16x3(torch.from_numpy(v)).numpy()                         # [Cout, (Cin/32) R S, 2, 32], block outer / tap inner
        tiles = lambda t: t.reshape(8, 9, 2, 32).transpose(0, 2, 1, 3).reshape(8, 18, 32)
        assert (w16[:, :, 0].astype(D) == tiles(a)).all() and (w16[:, :, 1].astype(D) == tiles(b)).all()
    one = np.array([1.0 - 2.0 ** -11, -1.0 + 2.0 ** -11], F)
    hi, lo = sr.split(one)
    assert (hi.astype(F) == one).all() and (lo == 0).all()                     # 1 - 2^-11 is an fp16 number itself: hi is not a
    hi, lo = sr.split(np.array([1.0 - 2.0 ** -12, 1.0 + 2.0 ** -12], F))      # ... while at q = 12 the tie below 1 goes to the even 1.0
    assert (hi.astype(D) == 1.0).all() and (lo.astype(D) == np.array([-2.0 ** -12, 2.0 ** -12])).all()
    hi, lo = sr.split(np.array([2.0 ** -12], F))
    assert float(hi[0]) == 2.0 ** -12 and float(lo[0]) == 0.0                  # a = 0: the lo half moved into hi


@pytest.mark.parametrize("family", ["own", "int"])
def test_every_case_keeps_its_representation_claim_and_the_condition(family):
    """x and w split into exactly (a, b); residuals that travel as S32 split exactly; S < LIMIT for every output element"""
    worst = {}
    for c0 in cc.ALL_CASES:
        c = c0 if family == "own" else cr.with_family(c0, "int")
        o = cr.operands(c)
        if c.kind == "f16x3":
            for v, a, b in ((o.x, o.xa, o.xb), (o.w, o.wa, o.wb)):
                hi, lo = sr.split(v)
                assert (hi.astype(D) == a).all() and (lo.astype(D) == b).all(), c.name
            if o.res is not None and c.res.endswith("s32"):
                hi, lo = sr.split(o.res)
                assert (sr.unsplit(hi, lo) == o.res).all(), c.name
        else:
            assert (o.x.astype(D) == o.xa + o.xb).all() and (o.w.astype(D) == o.wa + o.wb).all()
        s = float(cr.abs_sum(o, c).max())
        assert s < cr.LIMIT[c.family], (c.name, s)
        worst[c.group] = max(worst.get(c.group, 0.0), s / cr.LIMIT[c.family])
    print("largest S / limit per group:", {g: round(v, 3) for g, v in sorted(worst.items())})


def test_model3_is_the_fp64_convolution_less_the_lo_lo_term():
    seen = 0.0
    for c in cc.GROUP1[:24] + cc.GROUP2[:6]:
        o = _operands(c)
        lolo = cr.conv64(o.xb, o.wb, c)
        assert (cr.model3(o, c) == cr.model4(o, c) - lolo).all(), c.name
        assert (cr.model1(o, c) == cr.model3(o, c) - cr.conv64(o.xa, o.wb, c) - cr.conv64(o.xb, o.wa, c)).all()
        seen = max(seen, float(np.abs(lolo).max()))
    assert 0.0 < seen < 1e-5          # the fourth term is there, and it is far below any tolerance a test could hold


def test_helpers():
    assert [cr.up_index(i, 3, 5) for i in range(5)] == [0, 0, 1, 1, 2] and [cr.up_index(i, 4, 7) for i in range(7)] == [0, 0, 1, 1, 2, 2, 3]
    y = cr.relu_cols(np.array([[-1.0, -2.0, -3.0]]), 2)
    assert y.tolist() == [[0.0, 0.0, -3.0]]
    a = cr.arena((1, 2, 2), 64, True)
    assert a.shape == (1, 2, 2, 2, 2, 32) and a.dtype == H and (a == sr.SENTINEL).all()
    assert cr.arena((1, 2, 2), 5, False).dtype == F


@pytest.mark.parametrize("group", [1, 2, 3])
def test_the_walk_equals_the_model(group):
    """emulate() without a mutant == expected(), the whole output tensor, on every case of groups 1 to 3"""
    for c in (c for c in cc.EMULATED if c.group == group):
        o = _operands(c)
        want, got = cr.expected(c, o), cr.emulate(c, o)
        assert sr.same_bits(got, want), (c.name, sr.first_difference(got, want))


def test_every_mutant_is_killed():
    """every deliberate mistake of the walk changes at least one bit on at least one case; the table of who kills whom is printed
    (pytest -s) and copied into DESIGN.md.  A mutant nobody kills is a missing case."""
    table = {}
    for c in cc.EMULATED:
        o = _operands(c)
        want = cr.expected(c, o)
        bm = cc.TILE_FORMS[c.tiles[0]][0] if c.tiles[0] else 64
        for mutant in cr.MUTANTS:
            if not sr.same_bits(cr.emulate(c, o, mutant, bm=bm), want):
                table.setdefault(mutant, []).append(c.name)
    for mutant in cr.MUTANTS:
        killers = table.get(mutant, [])
        print(f"{mutant:34s} {len(killers):3d}  {', '.join(killers[:5])}{' ...' if len(killers) > 5 else ''}")
    assert not [m for m in cr.MUTANTS if m not in table]
    # the mistakes that exist at one mechanism only are killed by that mechanism's cases and by nothing else
    assert all(n.startswith("g16") for n in table["lo_subnormal_flushed"])
    assert all("splitk" in n or "k9216" in n for n in table["splitk_last_chunk_dropped"] + table["splitk_chunk_overlap"])
    assert all("stride2" in n for n in table["stride_origin_off_by_one"])
    assert all("dil2" in n for n in table["dilation_ignored_in_pad_test"])
    assert all("gn" in n for n in table["gn_affine_applied_to_padding"])
    assert all("up" in n for n in table["upsample_ceil"])
    assert all("slice" in n for n in table["slice_stride_ignored"])
    assert all(n.startswith("m_") for n in table["last_m_row_dropped"])


def test_the_routers_send_every_case_where_the_table_says():
    """hn_conv2d_f16x3_pick_tile / _uses_rs / _uses_halo / _uses_stream and thin_uses_flat's library query, on the host"""
    import ctypes as C
    from hn_amd import _lib, ops
    lib = _lib.load()
    routes = {}
    for c in cc.SINGLE:
        for tile in c.tiles:
            r = cc.assert_route(c, tile, ops)
            routes[r] = routes.get(r, 0) + 1
    assert routes["halo"] == len(cc.GROUP5) and routes["stream"] == len(cc.GROUP6) and routes["rs"] >= 9
    # the row-shared query answers both ways on the group-1 row-shared cases
    rs = [(c.w, t, cc.route_of(c, t, ops)[0]) for c in cc.GROUP1 if c.route == "rs?" for t in c.tiles]
    assert {r for _, _, r in rs} == {"rs", "igemm"}
    assert all(r == "igemm" for w, _, r in rs if w <= 4) and all(r == "rs" for w, t, r in rs if w >= 5 and t in (1, 2, 4))
    # the 7x7 filter has more taps than the descriptor form's tap table
    assert all(c.r * c.s > 32 for c in cc.GROUP1 if "no_descriptors" in c.name)
    # thin launches: the P form below 64 k pixels only under the form switch; Cout 16 never
    for t in cc.GROUP7:
        lv = _lib.ThinLevels()
        lv.count = len(t.members)
        for i, m in enumerate(t.members):
            lv.h[i], lv.w[i] = m.h, m.w
        n, cin = t.members[0].n, t.members[0].cin
        assert lib.hn_conv3x3_thin_uses_flat(C.byref(lv), n, cin, t.cout) == 0
        ops.set_form("thin_form_flat", True)
        try:
            assert lib.hn_conv3x3_thin_uses_flat(C.byref(lv), n, cin, t.cout) == (1 if t.cout <= 5 else 0)
            if t.affine:
                assert lib.hn_conv3x3_thin_affine_applies(C.byref(lv), n, cin, t.cout) == 1
        finally:
            ops.set_form("thin_form_flat", False)
    # split-K: the k tile count is no multiple of the splits
    for c in cc.GROUP3:
        kt = c.r * c.s * c.cin // 32
        assert kt % c.force_splits and kt % -(-kt // c.force_splits), c.name       # ... and the last chunk is shorter than the others
