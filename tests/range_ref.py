"""The rule of the f16x3 range contract and the planted launches that pin it (tests/range_cases.py holds the table).  numpy only;
nothing here reads the library.

THE RULE.  A launch leaves four words.  Word 0 is set iff at least one value the launch converts to an fp16 hi + lo pair fails
|v| <= 65504 (NaN and +-inf fail it) -- an element stored in the S32 format, or an operand the kernel itself splits for the MFMA
(the basis parts of the fused graph convolution, the thin kernel's fused GroupNorm apply).  Word 1 is set for a finite value of
the CALLER'S INPUT beyond the range and word 2 for a non-finite one (the preprocess kernels and stem_image only).  Word 3 stays 0.
What does not count: a value the epilogue's ReLU turns into 0, a split-K partial sum, anything outside the tensor (neighbour
channels of a channel slice, rows beyond M, the zero border, canvas padding), and a value stored as fp32.

THE LEDGER.  Every planted launch is reduced to a list of entries (kind, values, where they sit): "stored" and "operand" are
converted values, "input" is caller input, "prerelu", "partial", "outside" and "f32" are the values the rule must ignore.
words(ledger) is the rule; words(ledger, mutant) is a deliberate mistake of a kernel's note, so that the table is known to be able
to fail (tests/test_range_cpu.py).

THE PLANTED VALUES are exact: every operand is an fp16 number (lo = 0) and every sum is exact in fp32 -- asserted per launch by
conv_values(), never assumed.  One-hot product: x = 2047 at one element, one weight of +-32 at (co, centre tap, ci): one output
element is +-65504, and bias[co] = 2^-8 moves it to the next float (the rest of the column holds 2^-8).
"""
import types

import numpy as np

F, H, D = np.float32, np.float16, np.float64
F16_MAX = F(65504.0)
NEXT = np.nextafter(F16_MAX, F(np.inf))                 # 65504 + 2^-8: hi = 65504 stays finite, lo = 2^-8
assert float(NEXT) == 65504.0 + 2.0 ** -8
EPS = F(2.0 ** -8)
X1, W1 = F(2047.0), F(32.0)                             # the one-hot product: 2047 * 32 = 65504
MUTANTS = ("notes_before_relu", "notes_splitk_partials", "threshold_ge", "blind_to_nan", "skips_last_unit", "skips_last_m_tile_rows",
           "notes_neighbour_channels", "notes_only_when_out_split")
CONVERTED = ("stored", "operand")
IGNORED = ("prerelu", "partial", "outside", "f32")


def bad(v, mutant=None):
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        if mutant == "threshold_ge":
            return ~(np.abs(v) < F16_MAX)
        if mutant == "blind_to_nan":
            return np.abs(v) > F16_MAX
        return ~(np.abs(v) <= F16_MAX)


def entry(kind, v, rows=None, cols=None, m=None, cout=None, bm=None, out_split=True):
    """one group of values of a launch: rows / cols (arrays shaped like v, or None = not tied to a position), the launch's M, Cout
    and the tile's BM (None: the kernel has no such tiling), and whether the launch's OUTPUT is S32"""
    assert kind in CONVERTED + IGNORED + ("input",), kind
    v = np.atleast_1d(np.asarray(v, F))
    rows = None if rows is None else np.broadcast_to(np.asarray(rows), v.shape)
    cols = None if cols is None else np.broadcast_to(np.asarray(cols), v.shape)
    return types.SimpleNamespace(kind=kind, v=v, rows=rows, cols=cols, m=m, cout=cout, bm=bm, out_split=out_split)


def words(ledger, mutant=None):
    """the four words of a launch; mutant: one deliberate mistake of the note"""
    assert mutant is None or mutant in MUTANTS
    w = [0, 0, 0, 0]
    for e in ledger:
        keep = np.ones(e.v.shape, bool)
        counted = e.kind in CONVERTED
        if mutant == "notes_before_relu":
            counted = counted or e.kind == "prerelu"
        elif mutant == "notes_splitk_partials":
            counted = counted or e.kind == "partial"
        elif mutant == "notes_neighbour_channels":
            counted = counted or e.kind == "outside"
        elif mutant == "notes_only_when_out_split" and e.kind == "operand":
            counted = e.out_split
        elif mutant == "skips_last_unit" and e.kind == "stored" and e.cols is not None:
            keep &= e.cols < (e.cout - 1) // 8 * 8
        elif mutant == "skips_last_m_tile_rows" and e.kind == "stored" and e.rows is not None and e.bm:
            start = (e.m - 1) // e.bm * e.bm
            if start > 0:
                keep &= e.rows < start
        b = bad(e.v, mutant) & keep
        if counted and b.any():
            w[0] = 1
        if e.kind == "input" and b.any():
            with np.errstate(invalid="ignore"):
                finite = np.abs(e.v) <= np.finfo(F).max
            if (b & finite).any():
                w[1] = 1
            if (b & ~finite).any():
                w[2] = 1
    return w


def fp16_exact(v):
    """every finite value is an fp16 number (its lo half is 0); NaN / inf pass (they are planted on purpose)"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        return bool(((v.astype(H).astype(F) == v) | ~np.isfinite(v)).all())


# --------------------------------------------------------------------------------------------------------------------------
# planted convolution launches
# --------------------------------------------------------------------------------------------------------------------------
def plant(m, co, ci=0, xv=X1, wv=W1):
    """x = xv at channel ci of the input pixel under the centre tap of output row m; w = wv at (co, centre tap, ci)"""
    return types.SimpleNamespace(m=int(m), co=int(co), ci=int(ci), xv=F(xv), wv=F(wv))


def launch(name, case, tile=0, plants=(), bias=None, res=None, res_fill=0.0, want=None, bm=None, out_nan_arena=False):
    """case: a conv_exact case (shape, route, epilogue switches).  bias: {co: value} (a bias vector of zeros elsewhere, None: the
    case decides).  res: {(m, co): value} on a residual of res_fill elsewhere (the case's res kind says fp32 or S32).
    want: the words the table claims (checked against the rule on the CPU)."""
    return types.SimpleNamespace(name=name, case=case, tile=tile, plants=list(plants), bias=dict(bias or {}), res=dict(res or {}),
                                 res_fill=F(res_fill), want=want, bm=bm, out_nan_arena=out_nan_arena)


def out_size(c):
    return ((c.h + 2 * c.pad - c.dil * (c.r - 1) - 1) // c.stride + 1, (c.w + 2 * c.pad - c.dil * (c.s - 1) - 1) // c.stride + 1)


def rows_of(c):
    oh, ow = out_size(c)
    return c.n * oh * ow


def source_pixel(c, m):
    """(img, iy, ix) of the input pixel under the centre tap of output row m (asserted inside the image)"""
    oh, ow = out_size(c)
    img, oy, ox = m // (oh * ow), (m // ow) % oh, m % ow
    iy, ix = oy * c.stride - c.pad + (c.r // 2) * c.dil, ox * c.stride - c.pad + (c.s // 2) * c.dil
    assert 0 <= iy < c.h and 0 <= ix < c.w and 0 <= m < rows_of(c), (c.name, m)
    return img, iy, ix


def split_of(c, ci):
    """the split-K chunk of the k tile that holds (centre tap, channel ci): k tiles are block outer, tap inner, and the chunks are
    ceil(ktiles / splits) tiles long (conv_exact_ref.emulate)"""
    ktiles = (c.cin // 32) * c.r * c.s
    splits = c.force_splits if (c.splitk and c.force_splits and c.force_splits >= 2) else 1
    kt_per = -(-ktiles // splits)
    kt = ((ci // 32) * c.r + c.r // 2) * c.s + c.s // 2
    return kt // kt_per, -(-ktiles // kt_per)


def upsampled(c):
    return bool(c.res and c.res.startswith("up"))


def res_index(c, m):
    """row of the residual tensor (at its own size) the epilogue reads for output row m"""
    oh, ow = out_size(c)
    if not upsampled(c):
        return m
    rh, rw = (oh + 1) // 2, (ow + 1) // 2
    img, oy, ox = m // (oh * ow), (m // ow) % oh, m % ow
    return (img * rh + (oy * rh) // oh) * rw + (ox * rw) // ow


def conv_values(L):
    """the closed form of a planted launch -> namespace(elems = {(m, co): (partials per chunk, pre-ReLU value, stored value)},
    background = {co: (pre, stored)} for every other row of a column with a bias; every other element is +0).  A residual plant
    is keyed by the OUTPUT row (with an up-sampled residual the caller plants every output row that reads the same source)."""
    c = L.case
    assert fp16_exact([p.xv for p in L.plants]) and fp16_exact([p.wv for p in L.plants])
    if c.res and c.res.endswith("s32"):
        assert fp16_exact(list(L.res.values()) + [L.res_fill]), "an S32 residual travels as hi with lo = 0"
    nsplit = 1
    acc = {}
    for p in L.plants:
        source_pixel(c, p.m)
        z, nsplit = split_of(c, p.ci)
        acc.setdefault((p.m, p.co), {}).setdefault(z, []).append(D(p.xv) * D(p.wv))
    keys = set(acc) | set(L.res)
    elems = {}
    with np.errstate(all="ignore"):
        for (m, co) in sorted(keys):
            parts = []
            for z in range(nsplit):
                s = sum(acc.get((m, co), {}).get(z, []), D(0.0))
                assert F(s) == s or not np.isfinite(s), (L.name, "a partial sum is not exact in fp32")
                parts.append(F(s))
            v = D(0.0)
            for s in parts:                                                    # the reduction adds the chunks in z order
                v = v + D(s)
                assert D(F(v)) == v or not np.isfinite(v), L.name
            v = v + D(L.bias.get(co, 0.0))
            assert D(F(v)) == v or not np.isfinite(v), L.name
            v = v + D(L.res.get((m, co), L.res_fill if c.res else 0.0))
            assert D(F(v)) == v or not np.isfinite(v), (L.name, "the sum is not exact in fp32")
            pre = F(v)
            elems[(m, co)] = (parts, pre, _relu(pre) if co < c.relu_cols else pre)
        background = {}
        for co in range(c.cout):
            b = D(L.bias.get(co, 0.0)) + D(L.res_fill if c.res else 0.0)
            if b != 0.0:
                assert D(F(b)) == b
                background[co] = (F(b), _relu(F(b)) if co < c.relu_cols else F(b))
    return types.SimpleNamespace(elems=elems, background=background, splits=nsplit)


def _relu(v):
    v = F(v)
    return v if (v > 0 or np.isnan(v)) else F(0.0)


def conv_ledger(L, values=None):
    c = L.case
    v = conv_values(L) if values is None else values
    m, kind = rows_of(c), ("stored" if c.out_split else "f32")
    geom = dict(m=m, cout=c.cout, bm=L.bm, out_split=bool(c.out_split))
    led = []
    for (row, co), (parts, pre, post) in v.elems.items():
        led.append(entry(kind, post, row, co, **geom))
        if c.out_split:                                    # (a launch with an fp32 output has no note that could be misplaced)
            led.append(entry("prerelu", pre, row, co, **geom))
            if v.splits > 1:
                led.append(entry("partial", parts, row, co, **geom))
    for co, (pre, post) in v.background.items():
        led.append(entry(kind, post, None, co, **geom))
        if c.out_split:
            led.append(entry("prerelu", pre, None, co, **geom))
    if L.out_nan_arena:
        led.append(entry("outside", np.nan))
    return led


def dense(L):
    """the launch as dense numpy operands in conv_exact_ref's form (x, xa, xb = 0, w, wa, wb = 0, bias, res) and its dense expected
    values [M, Cout] from the closed form -- for the agreement with conv_exact_ref's fp64 model"""
    c = L.case
    o = types.SimpleNamespace()
    x = np.zeros((c.n, c.h, c.w, c.cin), F)
    w = np.zeros((c.cout, c.r, c.s, c.cin), F)
    for p in L.plants:
        img, iy, ix = source_pixel(c, p.m)
        assert x[img, iy, ix, p.ci] in (0, p.xv) and w[p.co, c.r // 2, c.s // 2, p.ci] in (0, p.wv)
        x[img, iy, ix, p.ci] = p.xv
        w[p.co, c.r // 2, c.s // 2, p.ci] = p.wv
    o.x, o.xa, o.xb, o.w, o.wa, o.wb = x, x.astype(D), np.zeros(x.shape, D), w, w.astype(D), np.zeros(w.shape, D)
    o.xwide, o.cw, o.c0, o.raw, o.scale, o.shift = x, c.cin, 0, None, None, None
    o.bias = None
    if c.bias:
        o.bias = np.zeros(c.cout, F)
        for co, b in L.bias.items():
            o.bias[co] = b
    o.res = None
    if c.res:
        oh, ow = out_size(c)
        rh, rw = ((oh + 1) // 2, (ow + 1) // 2) if upsampled(c) else (oh, ow)
        o.res = np.full((c.n * rh * rw, c.cout), L.res_fill, F)
        for (m, co), r in L.res.items():
            o.res[res_index(c, m), co] = r
        o.res = o.res.reshape(c.n, rh, rw, c.cout)
    return o


def dense_expected(L, values=None):
    """[M, Cout] fp32: what the launch stores, from the closed form"""
    c = L.case
    v = conv_values(L) if values is None else values
    y = np.zeros((rows_of(c), c.cout), F)
    for co, (_pre, post) in v.background.items():
        y[:, co] = post
    for (m, co), (_parts, _pre, post) in v.elems.items():
        y[m, co] = post
    return y


# --------------------------------------------------------------------------------------------------------------------------
# the lifter's kernels: a graph by hand with exactly representable entries
# --------------------------------------------------------------------------------------------------------------------------
def hand_graph():
    """10 vertices.  A: L[2,1] = 2      -> x at 1: a1[2] = 2 x, a2[1] = -x                      (only a1 can leave the range)
                      B: L[4,3] = L[5,4] = 1 -> x at 3: a1[4] = x, a2[5] = 2 x, a2[3] = -x              (only a2)
                      C: L[6,7] = 1, L[7,6] = 1/2 -> x at 6: a1[7] = x / 2, (2 L L - I)[6,6] = [7,7] = 0   (only a0)
    Vertices 0, 8 and 9 have empty rows AND empty columns (the first and the last element of a tensor read by nobody)."""
    import scipy.sparse as sp
    r, c, v = [2, 4, 5, 6, 7], [1, 3, 4, 7, 6], [2.0, 1.0, 1.0, 1.0, 0.5]
    m = sp.csr_matrix((np.asarray(v, F), (r, c)), shape=(10, 10))
    m.sort_indices()
    return m


def basis_parts(L, x):
    """x fp32 [B, V, F] -> (a0, a1, a2) = (x, L x, (2 L L - I) x), fp32, asserted exact (fp64 products of exact entries)"""
    import scipy.sparse as sp
    m = L.astype(D)
    q = (2.0 * (m @ m) - sp.identity(m.shape[0], dtype=D, format="csr")).tocsr()
    b, v, f = x.shape
    flat = x.astype(D).transpose(1, 0, 2).reshape(v, b * f)
    with np.errstate(all="ignore"):
        a1, a2 = m @ flat, q @ flat
        for a in (a1, a2):
            assert ((a.astype(F).astype(D) == a) | ~np.isfinite(a)).all(), "a basis part is not exact in fp32"
    back = lambda a: np.ascontiguousarray(a.reshape(v, b, f).transpose(1, 0, 2)).astype(F)
    return x, back(a1), back(a2)


def basis_split_parts(L, x0, x1):
    """hn_cheby3_basis_split's parts: (x0, x1, 2 L x1 - x0), exact"""
    m = L.astype(D)
    b, v, f = x0.shape
    with np.errstate(all="ignore"):
        lx = (m @ x1.astype(D).transpose(1, 0, 2).reshape(v, b * f)).reshape(v, b, f).transpose(1, 0, 2)
        a2 = 2.0 * lx - x0.astype(D)
        assert ((a2.astype(F).astype(D) == a2) | ~np.isfinite(a2)).all()
    return x0, x1, np.ascontiguousarray(a2).astype(F)
