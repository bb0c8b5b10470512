"""The split-format rule (tests/split_ref.py) without a GPU: the exactly rounded fma against fractions.Fraction, the rule against
torch in float64 where torch states the same thing, the layout against a plain reshape, the emulation of every kernel's walk
equal to the rule on every case of tests/split_cases.py, and every mutant failing on its named case -- so the bitwise comparison
of test_split_gpu.py is known to be able to fail."""
import numpy as np
import pytest
import torch

import split_cases as sc
import split_ref as sr

F, H = np.float32, np.float16


# ---- the arithmetic ----
def test_fma32_is_one_rounding_of_the_exact_value():
    """against exact rationals on the ties, the cancellations, results in the fp32 subnormal range and 3000 random triples; the
    unscaled tie (split_cases.TIE) gives 2^30 + 128, the twice-rounded forms 2^30 + 256"""
    x, s, t = (F(v) for v in sc.TIE)
    assert float(sr.fma32(x, s, t)) == 2.0 ** 30 + 128
    assert float(F(np.float64(x) * np.float64(s) + np.float64(t))) == 2.0 ** 30 + 256
    assert float(F(x * s) + t) == 2.0 ** 30 + 256
    rng = np.random.default_rng(5)
    rnd = (rng.standard_normal((3000, 3)) * 2.0 ** rng.integers(-30, 30, size=(3000, 3))).astype(F)
    rnd[1000:2000, 2] = -(rnd[1000:2000, 0] * rnd[1000:2000, 1])                       # cancellation
    rnd[2000:, :2] = (rng.standard_normal((1000, 2)) * 2.0 ** rng.integers(-80, -60, size=(1000, 2))).astype(F)   # subnormal results
    rnd[2000:, 2] = (rng.standard_normal(1000) * 2.0 ** -140).astype(F)
    for tri in (sc.fma_triples(), sc.fma_edge_triples(), rnd):
        got = sr.fma32(tri[:, 0], tri[:, 1], tri[:, 2])
        want = np.array([sr.fma_fraction(*row) for row in tri], F)
        assert (got == want).all(), tri[got != want][:3]          # (value equality: an exact zero's sign is not the rationals' business)
    sub = sr.fma32(rnd[2000:, 0], rnd[2000:, 1], rnd[2000:, 2])
    assert (np.abs(sub) < 2.0 ** -126).mean() > 0.5 and (sub != 0).mean() > 0.5     # the subnormal range was really visited
    # the two-rounding form is wrong on every scaled tie of the cases file, by one fp32 step
    tie = sc.fma_triples()[:9]
    twice = (tie[:, 0].astype(np.float64) * tie[:, 1] + tie[:, 2]).astype(F)
    assert (twice != sr.fma32(tie[:, 0], tie[:, 1], tie[:, 2])).all()
    # non-finite operands and signed zeros go through arithmetic's own rules
    assert np.isnan(sr.fma32(np.inf, 0.0, 1.0)) and np.isnan(sr.fma32(np.inf, 1.0, -np.inf)) and sr.fma32(3e38, 3e38, 0.0) == np.inf
    assert np.signbit(sr.fma32(-0.0, 1.0, -0.0)) and not np.signbit(sr.fma32(-0.0, 1.0, 0.0)) and not np.signbit(sr.fma32(1.0, -1.0, 1.0))


def test_relu_flag_and_split_on_the_ladder():
    """the hand-checked corners of steps 2-4"""
    v = np.array([np.nan, -0.0, 0.0, -1.0, -np.inf, np.inf, 2.0], F)
    assert sr.same_bits(sr.relu(v), np.array([np.nan, 0.0, 0.0, 0.0, 0.0, np.inf, 2.0], F))
    nxt = np.nextafter(F(65504), F(np.inf))
    probe = np.array([65504, nxt, np.nextafter(F(65520), F(0)), 65520, -65504, -nxt, np.inf, -np.inf, np.nan, 0], F)
    assert sr.range_bad(probe).tolist() == [False, True, True, True, False, True, True, True, True, False]
    hi, lo = sr.split(probe)
    with np.errstate(invalid="ignore"):
        want_hi = np.array([65504, 65504, 65504, np.inf, -65504, -65504, np.inf, -np.inf, np.nan, 0], H)
        want_lo = np.array([0, 2.0 ** -8, 16, -np.inf, 0, -2.0 ** -8, np.nan, np.nan, np.nan, 0], H)
    assert sr.same_bits(hi, want_hi) and sr.same_bits(lo, want_lo)
    p = lambda e: 2.0 ** e
    tiny = np.array([p(-24), p(-25), p(-25) * (1 + p(-10)), 1.5 * p(-24), 2.5 * p(-24), p(-14) - p(-25), p(-149), -p(-149), -0.0,
                     2049, 2051, 1 + p(-11), 1 + p(-11) + p(-23)], F)
    hi, lo = sr.split(tiny)
    assert sr.same_bits(hi, np.array([p(-24), 0, p(-24), 2 * p(-24), 2 * p(-24), p(-14), 0, -0.0, -0.0, 2048, 2052, 1, 1 + p(-10)], H))
    # (a remainder of half the smallest fp16 step is a tie and goes to the even zero, keeping its sign)
    assert sr.same_bits(lo, np.array([0, 0, -0.0, -0.0, 0, -0.0, 0, -0.0, 0, 1, -1, p(-11), -p(-11)], H))
    # hi + lo gives the value back wherever 22 bits hold it, and lo's own rounding is the only loss elsewhere
    back = sr.unsplit(hi, lo)
    assert (np.abs(back.astype(np.float64) - tiny) <= 2.0 ** -22 * np.abs(tiny) + 2.0 ** -25).all()
    assert float(back[9]) == 2049 and float(back[10]) == 2051 and float(back[12]) == 1 + p(-11)


@pytest.mark.parametrize("name", ["c32-hw65-n3", "c256-hw9-n3", "c96-hw5-n1", "ladder"])
def test_rule_is_torch_relu_of_the_affine_in_float64(name):
    """where torch states the same thing: unsplit(rule) is relu(x*s + t) in float64 to within one fp32 rounding and the split's
    2^-22 |v| + 2^-25, on every finite in-range element; NaN stays NaN"""
    op = sc.apply_case(name)
    for relu in (True, False):
        hi, lo, _ = sr.rule_apply(op.x, op.scale, op.shift, relu)
        got = sr.unsplit(hi, lo).astype(np.float64)
        xd, sd, td = (torch.from_numpy(np.array(t)).double() for t in (op.x, op.scale, op.shift))
        want = xd * sd[:, None, :] + td[:, None, :]
        want = (torch.relu(want) if relu else want).numpy()
        ok = np.isfinite(want) & (np.abs(want) < 65504)
        assert np.isnan(got[np.isnan(want)]).all() and not np.isnan(got[ok]).any()      # (beyond 65520: (inf, -inf), a NaN sum)
        tol = (2.0 ** -24 + 2.0 ** -22) * np.abs(want) + 2.0 ** -25
        assert (np.abs(got - want)[ok] <= tol[ok]).all(), name


@pytest.mark.parametrize("name", list(sc.POOL))
def test_pool_rule_has_the_value_of_torch_max_pool2d(name):
    """max_pool2d of hi + lo in float64 has the rule's VALUE (which pair is copied is the rule's own business)"""
    hi, lo = sc.pool_case(name)
    oh, ol = sc.pool_expected(name)
    v = torch.from_numpy(sr.unsplit(hi, lo)).double().permute(0, 3, 1, 2)
    want = torch.nn.functional.max_pool2d(v, 3, 2, 1).permute(0, 2, 3, 1).numpy()
    got = sr.unsplit(oh, ol).astype(np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def test_layout_is_a_reshape_of_n_h_w_c32_2_32():
    rng = np.random.default_rng(3)
    for n, hw, c in ((2, 5, 32), (1, 3, 96), (3, 2, 256)):
        hi, lo = sr.split(rng.standard_normal((n, hw, c)).astype(F))
        plain = np.stack((hi.reshape(n, hw, c // 32, 32), lo.reshape(n, hw, c // 32, 32)), axis=3)
        assert sr.same_bits(sr.to_s32(hi, lo), plain)
        back = sr.from_s32(plain)
        assert sr.same_bits(back[0], hi) and sr.same_bits(back[1], lo)
        # a wider pixel stride: the same halfs, further apart, nothing else touched
        ys = 2 * c + 128
        buf = np.full(7 + n * hw * ys, sr.SENTINEL, H)
        sr.place(buf, 7, hi.reshape(-1, c), lo.reshape(-1, c), ys)
        rows = buf[7:].reshape(n * hw, ys)
        assert sr.same_bits(rows[:, :2 * c].reshape(n, hw, c // 32, 2, 32), plain) and (rows[:, 2 * c:] == sr.SENTINEL).all()
        assert (buf[:7] == sr.SENTINEL).all()


# ---- the emulations against the rule ----
def _emulate(kind, name, variant=None, mutant=None, form="pow2"):
    """-> (list of output buffers, flag or None) of the emulation of one case"""
    if kind in ("apply", "flag"):
        op = sc.apply_case(name) if kind == "apply" else sc.flag_case(name)
        affine, relu = variant if kind == "apply" else (sc.FLAGS[name][1] is not None, sc.FLAGS[name][3])
        c8 = op.c // 8
        if c8 & (c8 - 1) or c8 > 256:
            form = "generic"
        f = op.flat(affine)
        flag = sr.emulate_apply(f, op.n, op.hw, op.c, relu, form=form, mutant=mutant)
        return [f.y], flag
    if kind == "levels":
        ops = sc.levels_case(name)
        fs = [op.flat(True) for op in ops]
        flag = sr.emulate_levels(fs, ops[0].n, [op.hw for op in ops], ops[0].c, True, mutant=mutant)
        return [f.y for f in fs], flag
    if kind == "pool":
        hi, lo = sc.pool_case(name)
        n, h, w, c = hi.shape
        return [sr.emulate_pool(sr.to_s32(hi, lo).reshape(-1), n, h, w, c, mutant=mutant)], None
    u = sc.unsplit_case(name)
    y = np.full(u["y_size"], sc.SENTINEL32, F)
    sr.emulate_unsplit(u["xbuf"], u["x_off"], u["xs"], u["npix"], u["c"], y, u["y_off"], u["ys"], mutant=mutant)
    return [y], None


def _expected(kind, name, variant=None):
    if kind == "apply":
        y, flag = sc.apply_expected(name, *variant)
        return [y], flag
    if kind == "flag":
        y, flag = sc.flag_case(name).expected(sc.FLAGS[name][1] is not None, sc.FLAGS[name][3])
        return [y], flag
    if kind == "levels":
        want = sc.levels_expected(name, True)
        return [w[0] for w in want], any(w[1] for w in want)
    if kind == "pool":
        return [sr.to_s32(*sc.pool_expected(name)).reshape(-1)], None
    return [sc.unsplit_case(name)["want"]], None


def _same(got, want):
    return got[1] == want[1] and len(got[0]) == len(want[0]) and all(sr.same_bits(a, b) for a, b in zip(got[0], want[0]))


@pytest.mark.parametrize("name", list(sc.APPLY))
def test_apply_emulation_equals_the_rule(name):
    """both walks (one image per blockIdx.y with two pixels in flight; the flat item loop), every variant, the whole arena"""
    op = sc.apply_case(name)
    c8 = op.c // 8
    for variant in sc.variants(name):
        for form in ("generic",) if (c8 & (c8 - 1) or c8 > 256) else ("pow2", "generic"):
            assert _same(_emulate("apply", name, variant, form=form), _expected("apply", name, variant)), (name, variant, form)
    if op.c == 32 and op.hw >= 127:      # four pixels in flight (the streaming instantiations): with the grid of this size only the
        for gx in (None, 1):             # tail loop runs, with one block per image (a capped grid) the four-deep loop at hw = 193
            f = op.flat(True)
            flag = sr.emulate_apply(f, op.n, op.hw, op.c, True, unr=4, gx=gx)
            assert _same(([f.y], flag), _expected("apply", name, (True, True))), (name, gx)


@pytest.mark.parametrize("name", list(sc.FLAGS))
def test_flag_cases_ask_for_what_their_table_says(name):
    want = _expected("flag", name)
    assert want[1] == bool(sc.FLAGS[name][4]), name
    assert _same(_emulate("flag", name), want)
    assert _same(_emulate("flag", name, form="generic"), want)


def test_the_flagged_value_below_65520_still_splits_finitely():
    y, flag = _expected("flag", "65519.996")
    hi, lo = sr.take(y[0], sc.flag_case("65519.996").y_off, 6, 32, 64)
    assert flag and float(hi[-1, -1]) == 65504 and float(lo[-1, -1]) == 16
    y, flag = _expected("flag", "-1e5-relu")
    hi, lo = sr.take(y[0], sc.flag_case("-1e5-relu").y_off, 6, 32, 64)
    assert not flag and sr.same_bits(hi[-1, -1:], np.zeros(1, H)) and sr.same_bits(lo[-1, -1:], np.zeros(1, H))


@pytest.mark.parametrize("name", list(sc.LEVELS))
def test_levels_emulation_equals_the_rule(name):
    assert _same(_emulate("levels", name), _expected("levels", name)), name
    n, c, hws, _ = sc.LEVELS[name]
    first = sr.level_blocks(n, hws, c)
    assert len(first) == len(hws) + 1 and all(b > a for a, b in zip(first, first[1:]))      # every level owns a block


@pytest.mark.parametrize("name", list(sc.POOL))
def test_pool_emulation_equals_the_rule(name):
    assert _same(_emulate("pool", name), _expected("pool", name)), name


@pytest.mark.parametrize("name", list(sc.UNSPLIT))
def test_unsplit_emulation_equals_the_rule(name):
    assert _same(_emulate("unsplit", name), _expected("unsplit", name)), name


def test_every_mutant_has_a_case():
    assert set(sc.MUTANT_CASE) == set(sr.ALL_MUTANTS)


@pytest.mark.parametrize("mutant", sr.ALL_MUTANTS)
def test_every_mutant_fails_on_its_named_case(mutant):
    kind, name, *rest = sc.MUTANT_CASE[mutant]
    variant = rest[0] if rest else None
    want = _expected(kind, name, variant)
    assert _same(_emulate(kind, name, variant), want), "the unmutated emulation must pass first"
    assert not _same(_emulate(kind, name, variant, mutant=mutant), want), mutant
