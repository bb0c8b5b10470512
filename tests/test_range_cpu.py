"""The range-contract table (tests/range_cases.py) without a GPU: every planted launch is exact (fp16 operands with lo = 0, sums exact
in fp32 -- range_ref asserts it while it evaluates the closed form), the closed form agrees with conv_exact_ref's fp64 model on the
planted operands, the rule gives the words the table claims, and every mutant of the rule changes the words of at least one
launch -- so the comparison of tests/test_range_gpu.py is known to be able to fail.  The routers' triggers are asserted here as
well (the library's queries are host code)."""
import numpy as np
import pytest
import torch

import conv_exact_cases as cc
import conv_exact_ref as cr
import range_cases as rc
import range_ref as rr

F, D = np.float32, np.float64


def _compound_launches():
    return [g for kind in cc.GROUP4 if kind != "grouped" for g in rc.compound(kind)]


def test_the_boundary_values():
    assert float(rr.NEXT) == 65504.0 + 2.0 ** -8 and np.float16(rr.NEXT) == np.float16(65504.0)       # hi stays finite
    assert float(rr.X1) * float(rr.W1) == 65504.0 and float(rc.HALF_NEXT) * 2 == float(rr.NEXT)
    assert rr.fp16_exact([2047, 32, 797, 798, 40000, 4096, 2050, 2048, 32752, np.nan, np.inf]) and not rr.fp16_exact([2049.0])
    assert 2.0 ** 17 - 2050 * 32 == 65472 and 2.0 ** 17 - 2048 * 32 == 65536 and 40000 + 797 * 32 == 65504
    assert rr.bad([65504.0, -65504.0, rr.NEXT, np.nan, np.inf, -np.inf]).tolist() == [False, False, True, True, True, True]
    assert rr.words([rr.entry("input", [rr.NEXT])]) == rc.INPUT_FINITE and rr.words([rr.entry("input", [np.nan])]) == rc.INPUT_NONFINITE
    assert rr.words([rr.entry("input", [np.inf, 3.0e38])]) == [0, 1, 1, 0] and rr.words([rr.entry("input", [65504.0])]) == rc.CLEAN


def test_every_conv_launch_is_exact_and_the_rule_gives_the_claimed_words():
    launches = rc.every_conv_launch()
    assert len({l.name for l in launches}) == len(launches)
    seen = {tuple(w): 0 for w in (rc.CLEAN, rc.ACT)}
    for l in launches:
        got = rr.words(rr.conv_ledger(l))                  # (conv_values asserts the exactness of every operand and sum)
        assert got == l.want, (l.name, got, l.want)
        seen[tuple(got)] += 1
    for name, members, want in _compound_launches():
        got = rr.words([e for l in members for e in rr.conv_ledger(l)])
        assert got == want, (name, got)
        seen[tuple(got)] += 1
    print("launches per claimed words:", seen)
    assert min(seen.values()) > 100


def _agrees(l):
    c = l.case
    o = rr.dense(l)
    y = cr.model(o, c) + (o.bias.astype(D) if o.bias is not None else 0.0) + cr.residual_at_output(o, c)
    y = cr.relu_cols(y, c.relu_cols).reshape(rr.rows_of(c), c.cout)
    want = rr.dense_expected(l).astype(D)
    assert np.array_equal(y, want), (l.name, np.argwhere(y != want)[:4])


def test_the_closed_form_is_conv_exact_refs_model_on_the_planted_operands():
    """every finite launch of the 64 x 64 tile's table, of split-K, one halo and one stream launch, and the compound controls"""
    ls = rc.igemm(3) + rc.relu_launches(3) + rc.residual_launches(3) + rc.f32_output_launches(3) + rc.slice_launches(3) + rc.row_shared(3)
    ls += rc.splitk(2, "fused", 3) + rc.splitk(7, "reduce_kernel", 1)
    ls += [l for l in rc.halo(rc.HALO[1]) if "control" in l.name or "40000" in l.name] + rc.stream()[-3:]
    ls += [l for name, members, _ in _compound_launches() if "control" in name for l in members]
    n = 0
    for l in ls:
        if all(np.isfinite(v) for v in l.res.values()):
            _agrees(l)
            n += 1
    assert n > 300


def test_a_planted_bank_is_what_split_f16x3_makes():
    """the GPU test writes the planted weight straight into the split bank at [co, k tile, hi, channel]: the layout and lo = 0,
    against weights.split_f16x3 (k tiles: block outer, tap inner)"""
    from hn_amd.weights import split_f16x3
    for c, ci in ((rc.RAGGED, 37), (rc.m_case(64, 3), 5), (rc.splitk_case(7, "fused"), 95)):
        w = np.zeros((c.cout, c.r, c.s, c.cin), F)
        w[c.cout - 1, c.r // 2, c.s // 2, ci] = -32.0
        w16 = split_f16x3(torch.from_numpy(w)).numpy()
        want = np.zeros_like(w16)
        want[c.cout - 1, ((ci // 32) * c.r + c.r // 2) * c.s + c.s // 2, 0, ci % 32] = -32.0
        assert np.array_equal(w16, want), c.name


def test_every_mutant_is_caught():
    """each deliberate mistake of the note changes the words of at least one launch; the table of who catches whom is printed"""
    launches = [(l.name, rr.conv_ledger(l), l.want) for l in rc.every_conv_launch()]
    launches += [(name, [e for l in ms for e in rr.conv_ledger(l)], want) for name, ms, want in _compound_launches()]
    launches += [(name, led, want) for name, led, want in _lifter_ledgers()]
    caught = {}
    for name, led, want in launches:
        assert rr.words(led) == want, name
        for mutant in rr.MUTANTS:
            if rr.words(led, mutant) != want:
                caught.setdefault(mutant, []).append(name)
    for mutant in rr.MUTANTS:
        names = caught.get(mutant, [])
        print(f"{mutant:28s} caught by {len(names):5d} launches, first: {names[0] if names else '-'}")
    assert not [m for m in rr.MUTANTS if m not in caught]
    # the mistakes that exist at one mechanism only are caught by that mechanism's launches
    assert all("-next in column" in n or "res(" in n for n in caught["notes_before_relu"])
    assert all("2^17" in n for n in caught["notes_splitk_partials"])
    wants = {name: want for name, _, want in launches}
    assert all(wants[n] == rc.CLEAN for m in ("threshold_ge", "notes_before_relu", "notes_splitk_partials", "notes_neighbour_channels")
               for n in caught[m])                                              # (these mistakes can only add a note)
    assert all(wants[n] == rc.ACT for m in ("blind_to_nan", "skips_last_unit", "skips_last_m_tile_rows", "notes_only_when_out_split")
               for n in caught[m])                                              # (... and these can only lose one)
    assert all("nan" in n for n in caught["blind_to_nan"])
    assert all("NaN arena" in n or "outside" in n for n in caught["notes_neighbour_channels"])
    assert all("fp32 out" in n for n in caught["notes_only_when_out_split"])


def _lifter_ledgers():
    """the fused kernel's basis with both output types, and the values outside a thin launch's channel slice, as ledgers"""
    L = rr.hand_graph()
    out = []
    for name, fin, vertex, value, part in rc.fused_basis():
        x = np.zeros((3, L.shape[0], fin), F)
        x[0, vertex, 0] = x[2, vertex, fin - 1] = value
        parts = rr.basis_parts(L, x)
        flagged = [p for p, a in zip(("a0", "a1", "a2"), parts) if rr.bad(a).any()]
        assert (flagged[:1] == [part]) if part else not flagged, (name, flagged)
        if part in ("a1", "a2"):
            assert flagged == [part], (name, flagged)                       # that part alone
        for split in (False, True):
            led = [rr.entry("operand", a, out_split=split) for a in parts] + [rr.entry("stored" if split else "f32", 0.0)]
            out.append((f"fused basis {name}, {'S32' if split else 'fp32 out'}", led, rc.ACT if part else rc.CLEAN))
    out.append(("thin affine: a plant outside the channel slice", [rr.entry("outside", [np.nan, 1e30]), rr.entry("operand", [1.0])], rc.CLEAN))
    return out


def test_the_hand_graph_isolates_each_basis_part():
    """L and 2 L L - I of the hand-built graph are exact, the first and the last vertex are read by nobody, and each scenario of
    range_cases.fused_basis() drives exactly the part it names out of the range (asserted inside _lifter_ledgers)"""
    L = rr.hand_graph()
    from oracle import graph_ref
    q = graph_ref.cheby2(L).toarray()
    assert q[6, 6] == 0 and q[7, 7] == 0 and q[5, 3] == 2 and q[1, 1] == -1 and not L[:, [0, 8, 9]].toarray().any()
    assert not L[[0, 8, 9]].toarray().any()
    assert len(_lifter_ledgers()) == 2 * len(rc.fused_basis()) + 1
    x0 = np.zeros((1, 10, 4), F)
    x1 = x0.copy()
    x1[0, 3, 2] = 40000.0
    a0, a1, a2 = rr.basis_split_parts(L, x0, x1)
    assert a2[0, 4, 2] == 80000.0 and np.count_nonzero(a2) == 1


def test_the_routers_send_every_launch_where_the_table_says():
    from hn_amd import ops
    seen = set()
    routes = {}
    for l in rc.every_conv_launch():
        key = (l.case.name, l.tile, l.case.terms)
        if key in seen:
            continue
        seen.add(key)
        r = cc.assert_route(l.case, l.tile, ops)
        routes[r] = routes.get(r, 0) + 1
    assert routes["halo"] == 2 and routes["stream"] == 1 and routes["rs"] >= 3 and routes["igemm"] > 50, routes
    for splits in (2, 7):
        for kind in ("fused", "reduce_kernel"):
            c = rc.splitk_case(splits, kind)
            # 27 k tiles in chunks of 14 or 4: the centre taps of blocks 0 and 2 (k tiles 4 and 22) lie in different chunks
            assert rr.split_of(c, 0) == (4 // -(-27 // splits), splits) and rr.split_of(c, 64)[0] == 22 // -(-27 // splits)
            assert rr.split_of(c, 95)[0] == rr.split_of(c, 64)[0] != rr.split_of(c, 0)[0]
