"""Named inputs for the split-format tests (tests/split_ref.py), each as small as the kernel branch it is meant to reach allows.
The sizes follow from affine_split_pow2_kernel's constants: c8 = c/8 lanes per pixel, ppb = 256/c8 pixels per block and
iteration, gx = ceil(hw / 2 ppb) blocks per image, and the two-deep loop runs while pix + gx*ppb < hw.  Every case carries the
operands as FLAT buffers with offsets and strides -- what the library is handed -- so that the emulation (and a mutant of it)
and the GPU run start from the same bytes; the expectation is computed once per case from the rule."""
import functools
import zlib

import numpy as np

import split_ref as sr

F, H = np.float32, np.float16
GUARD = 64                       # halfs (fp32 buffers: floats) of sentinel before and behind every output
SENTINEL32 = F(-77.25)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ro(*arrays):
    for t in arrays:
        if t is not None:
            t.setflags(write=False)


# --------------------------------------------------------------------------------------------------------------------------
# values
# --------------------------------------------------------------------------------------------------------------------------
def ladder_values():
    """the fp32 values at which a conversion, the ReLU or the range note can go wrong"""
    nx = lambda a, b: float(np.nextafter(F(a), F(b)))
    p = lambda e: 2.0 ** e
    v = [0.0, -0.0, p(-149), -p(-149), p(-127), -p(-130), p(-126),                       # +-0, fp32 subnormals
         p(-24), p(-25), p(-25) * (1 + p(-10)), -p(-25), 1.5 * p(-24), 2.5 * p(-24), -3.5 * p(-24),   # the smallest fp16 steps, ties
         p(-14), p(-14) - p(-24), p(-14) - p(-25), -(p(-14) - p(-25)), p(-14) * (1 + p(-11)),          # subnormal / normal boundary
         0.01, 1e-3, -3e-4, 1.0 / 3.0, 0.75 + p(-20),                                    # lo is an fp16 subnormal
         2049.0, 2051.0, -2049.0, -2051.0, 1 + p(-11), 1 + p(-11) + p(-23), 1 + 3 * p(-11), -(1 + p(-11)),   # fp16 midpoints
         65504.0, nx(65504.0, np.inf), nx(65520.0, 0.0), 65520.0, 1e5, 3e38,             # the top of the range
         -65504.0, nx(-65504.0, -np.inf), -65520.0, -1e5, -3e38,
         np.inf, -np.inf, np.nan]
    return np.array(v, F)


# (x, s, t) whose exact x*s + t lies where two roundings (fp64 then fp32, or product then sum) differ from one, scaled into
# the fp16 range: 8(1 + 2^-23) * (8 - 2^-20) + (2^30 + 128) = 2^30 + 192 - 2^-40, which rounds to 2^30 + 128 and, twice
# rounded, to 2^30 + 256
TIE = (8 * (1 + 2.0 ** -23), 8 - 2.0 ** -20, 2.0 ** 30 + 128)


def fma_triples():
    """[K, 3] fp32: the tie at three scales and both signs, then cancellations t = -fl(x*s) (the result is the product's
    rounding error, which only an fma sees)"""
    out = []
    for k in (-20, -24, -28):
        x, s, t = TIE[0] * 2.0 ** k, TIE[1], TIE[2] * 2.0 ** k
        out += [(x, s, t), (-x, s, -t), (x, -s, -t)]
    for x, s in ((123.456, 234.567), (1234.5678, 0.87654321), (-77.7777, 311.1111), (3.1415927, 2.7182817), (180.5, -181.25),
                 (0.001234, 56789.0), (255.99998, 255.99998)):
        x, s = F(x), F(s)
        out.append((x, s, -(x * s)))
    return np.array(out, F)


def fma_edge_triples():
    """triples for test_split_cpu.py alone (their results split to zeros, or are far out of the fp16 range): the tie unscaled,
    results in the fp32 subnormal range, and the largest finite results"""
    p = lambda e: 2.0 ** e
    out = [TIE, (-TIE[0], TIE[1], -TIE[2])]
    out += [(p(-100) * 1.5, p(-40) * 1.25, p(-149)), (p(-100) * (1 + p(-23)), p(-47) * (1 - p(-24)), -p(-148)),
            (p(-75) * 3, p(-75), 0.0), (p(-75) * (1 + p(-22)), p(-74) * (1 + p(-21)), p(-149)), (p(-126), 0.5, p(-149)),
            (p(-126) * (1 + p(-23)), 0.5, 0.0), (p(-126) * (1 + 3 * p(-23)), 0.5, 0.0), (p(-63), -p(-64) * 1.5, p(-127))]
    out += [(p(64) * 1.9999999, p(63) * 1.9999999, -p(104)), (p(64), p(63) * 1.9999999, p(103))]
    return np.array(out, F)


# --------------------------------------------------------------------------------------------------------------------------
# the apply pass
# --------------------------------------------------------------------------------------------------------------------------
def _apply_shapes():
    out = {}
    for c, hws in ((32, (1, 63, 64, 65, 127, 128, 129, 193)), (256, (1, 7, 8, 9, 17)), (2048, (1, 2, 3)), (96, (1, 5, 43)),
                   (4096, (1, 2))):
        for hw in hws:
            for n in (1, 3):
                out[f"c{c}-hw{hw}-n{n}"] = (n, hw, c, n == 3, "random")
    # the other layout for one shape of each kernel
    out["c32-hw129-n1-wide"] = (1, 129, 32, True, "random")
    out["c256-hw17-n3-dense"] = (3, 17, 256, False, "random")
    out["c96-hw43-n1-wide"] = (1, 43, 96, True, "random")
    out["ladder"] = (2, 3, 64, False, "ladder")
    out["ladder-wide"] = (2, 3, 64, True, "ladder")
    return out


# name -> (n, hw, c, wide, data).  wide: the input is a channel slice of a wider tensor that starts at channel 32, the tables
# have a row stride of c + 32, the output is a block slice of a wider S32 tensor
APPLY = _apply_shapes()
# (affine, relu) runs of a case
VARIANTS = ((True, True), (False, False))
LADDER_VARIANTS = ((True, True), (True, False), (False, True), (False, False))


def variants(name):
    return LADDER_VARIANTS if APPLY[name][4] == "ladder" else VARIANTS


# the range note: one special value among harmless ones -> name: (x, scale, shift, relu, the flag the rule asks for)
_NEXT = float(np.nextafter(F(65504.0), F(np.inf)))
FLAGS = {
    "65504": (65504.0, None, None, True, 0),
    "next-after-65504": (_NEXT, None, None, True, 1),
    "65519.996": (float(np.nextafter(F(65520.0), F(0.0))), None, None, False, 1),     # splits to the finite pair (65504, 16)
    "65520": (65520.0, None, None, True, 1),
    "1e5": (1e5, None, None, False, 1),
    "+inf": (np.inf, None, None, True, 1),
    "-inf": (-np.inf, None, None, False, 1),
    "-inf-relu": (-np.inf, None, None, True, 0),
    "nan": (np.nan, None, None, False, 1),
    "nan-relu": (np.nan, None, None, True, 1),
    "-65504": (-65504.0, None, None, False, 0),
    "-next-after-65504": (-_NEXT, None, None, False, 1),
    "-1e5": (-1e5, None, None, False, 1),
    "-1e5-relu": (-1e5, None, None, True, 0),                                        # the overflow the ReLU removes: +0, no flag
    "affine-65504": (2.0, 32752.0, 0.0, True, 0),
    "affine-next": (2.0, 32752.0, float(np.nextafter(F(65504.0), F(np.inf))) - 65504.0, True, 1),
    "affine-9e4": (300.0, 300.0, 0.0, False, 1),
    "affine--9e4-relu": (-300.0, 300.0, 0.0, True, 0),
    "affine-inf-shift": (1.0, 1.0, np.inf, True, 1),
}
FLAG_SHAPE = (2, 3, 32)


class Operands:
    """one launch: logical arrays (x [n, hw, c], scale / shift [n, c] or None) and the flat buffers they sit in"""

    def __init__(self, n, hw, c, wide, x, scale, shift):
        self.n, self.hw, self.c, self.wide = n, hw, c, wide
        self.x, self.scale, self.shift = x, scale, shift
        nb = c // 32
        self.c0, self.cw = (32, c + 64) if wide else (0, c)
        self.a0, self.aw = (32, c + 32) if wide else (0, c)
        self.b0, self.nbw = (1, nb + 3) if wide else (0, nb)
        rng = _rng("pad", n, hw, c)
        self.x_buf = (rng.standard_normal((n, hw, self.cw)) * 3).astype(F)
        self.x_buf[:, :, self.c0:self.c0 + c] = x
        self.x_buf = self.x_buf.reshape(-1)
        self.xs, self.x_off = self.cw, self.c0
        self.sc_buf = self.sh_buf = None
        if scale is not None:
            self.sc_buf, self.sh_buf = (rng.standard_normal((n, self.aw)).astype(F) for _ in range(2))
            self.sc_buf[:, self.a0:] = scale
            self.sh_buf[:, self.a0:] = shift
            self.sc_buf, self.sh_buf = self.sc_buf.reshape(-1), self.sh_buf.reshape(-1)
        self.a_off, self.a_stride = self.a0, self.aw
        self.ys = 64 * self.nbw
        self.y_off = GUARD + 64 * self.b0
        self.y_size = 2 * GUARD + n * hw * self.ys
        _ro(self.x, self.scale, self.shift, self.x_buf, self.sc_buf, self.sh_buf)

    def flat(self, affine=True):
        """a fresh sentinel-filled arena and the launch's view of it"""
        y = np.full(self.y_size, sr.SENTINEL, H)
        return sr.Flat(self.x_buf, self.x_off, self.xs, self.sc_buf if affine else None, self.sh_buf if affine else None,
                       self.a_off, self.a_stride, y, self.y_off, self.ys)

    def expected(self, affine, relu):
        """(arena, flag) by the rule: steps 1-4 on the logical arrays, step 5 into the sentinel-filled arena"""
        hi, lo, flag = sr.rule_apply(self.x, self.scale if affine else None, self.shift if affine else None, relu)
        y = np.full(self.y_size, sr.SENTINEL, H)
        sr.place(y, self.y_off, hi.reshape(-1, self.c), lo.reshape(-1, self.c), self.ys)
        return y, flag


def _tables(n, c, rng):
    """different per image and per channel, so that a wrong row or channel shows"""
    scale = (1.0 + 0.5 * rng.standard_normal((n, c))) * (1.0 + np.arange(n))[:, None]
    shift = 0.2 * rng.standard_normal((n, c)) - 0.3 * np.arange(n)[:, None]
    return scale.astype(F), shift.astype(F)


def _random_x(n, hw, c, rng):
    """N(0, 2) with every seventh value small enough for an fp16-subnormal hi or lo"""
    x = rng.standard_normal((n, hw, c)) * 2
    small = rng.random((n, hw, c)) < 1.0 / 7.0
    return np.where(small, x * 2.0 ** -rng.integers(8, 20, size=x.shape), x).astype(F)


def _ladder(n, hw, c):
    """channels 0 .. c-17: the ladder values, rolled per image, under power-of-two scales (exact products, so the edges are hit
    with the affine too); the last 16 channels: the fma triples, x in pixel 0 and its fp32 neighbours in pixels 1, 2"""
    vals, tri = ladder_values(), fma_triples()
    assert tri.shape[0] <= 16 and hw == 3
    cl = c - 16
    x = np.zeros((n, hw, c), F)
    scale, shift = np.ones((n, c), F), np.zeros((n, c), F)
    pw = np.array([1, -1, 0.5, 2, 1, -2, 0.25, 1], F)
    for img in range(n):
        x[img, :, :cl] = np.resize(np.roll(vals, 5 * img), hw * cl).reshape(hw, cl)
        scale[img, :cl] = pw[(np.arange(cl) + 3 * img) % 8]
        k = np.roll(np.arange(16), 4 * img) % tri.shape[0]
        x[img, 0, cl:], scale[img, cl:], shift[img, cl:] = tri[k, 0], tri[k, 1], tri[k, 2]
        x[img, 1, cl:] = np.nextafter(tri[k, 0], F(np.inf))
        x[img, 2, cl:] = np.nextafter(tri[k, 0], F(-np.inf))
    return x, scale, shift


@functools.lru_cache(maxsize=None)
def apply_case(name):
    n, hw, c, wide, data = APPLY[name]
    rng = _rng("apply", name)
    if data == "ladder":
        x, scale, shift = _ladder(n, hw, c)
    else:
        x = _random_x(n, hw, c, rng)
        scale, shift = _tables(n, c, rng)
    return Operands(n, hw, c, wide, x, scale, shift)


@functools.lru_cache(maxsize=None)
def apply_expected(name, affine, relu):
    out = apply_case(name).expected(affine, relu)
    _ro(out[0])
    return out


@functools.lru_cache(maxsize=None)
def flag_case(name):
    """harmless data with the special value in the last channel of the last pixel of the last image"""
    v, s, t, _relu, _want = FLAGS[name]
    n, hw, c = FLAG_SHAPE
    rng = _rng("flag", name)
    x = _random_x(n, hw, c, rng)
    x[-1, -1, -1] = v
    scale = shift = None
    if s is not None:
        scale, shift = _tables(n, c, rng)
        scale[-1, -1], shift[-1, -1] = s, t
    return Operands(n, hw, c, False, x, scale, shift)


# --------------------------------------------------------------------------------------------------------------------------
# the levels launch
# --------------------------------------------------------------------------------------------------------------------------
# name -> (n, c, hw per level, wide)
LEVELS = {
    "one-hw1": (1, 32, (1,), False),
    "one-hw129": (2, 256, (129,), False),
    "three": (2, 256, (129, 64, 1), False),
    "three-c32-wide": (3, 32, (129, 64, 1), True),
    "five": (3, 32, (65, 63, 64, 1, 130), False),
    "five-c256": (1, 256, (65, 63, 64, 1, 130), True),
    "five-c2048": (2, 2048, (1, 2, 3, 1, 5), False),
}


@functools.lru_cache(maxsize=None)
def levels_case(name):
    """one Operands per level: data and tables of their own, the same strides"""
    n, c, hws, wide = LEVELS[name]
    out = []
    for l, hw in enumerate(hws):
        rng = _rng("levels", name, l)
        x = _random_x(n, hw, c, rng) + F(l)
        scale, shift = _tables(n, c, rng)
        out.append(Operands(n, hw, c, wide, x, (scale * F(1 + l)).astype(F), shift))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def levels_expected(name, relu):
    out = tuple(op.expected(True, relu) for op in levels_case(name))
    _ro(*(o[0] for o in out))
    return out


# --------------------------------------------------------------------------------------------------------------------------
# the pool and unsplit: hand-built pairs
# --------------------------------------------------------------------------------------------------------------------------
POOL_SIZES = tuple((h, w) for h in range(1, 6) for w in range(1, 6)) + ((7, 6),)
POOL_KINDS = ("random", "negative", "ties", "nan1", "nan2")


def _pool_names():
    out = {}
    for i, (h, w) in enumerate(POOL_SIZES):
        for kind in POOL_KINDS:
            if kind in ("random", "nan1", "nan2") and (h, w) not in ((2, 3), (3, 3), (4, 5), (5, 4), (5, 5), (7, 6)):
                continue
            for c in ((32, 64) if (h, w) == (7, 6) else ((32,) if i % 2 == 0 else (64,))):
                out[f"{kind}-{h}x{w}-c{c}"] = (2 if (h, w) in ((3, 3), (7, 6)) else 1, h, w, c, kind)
    return out


# name -> (n, h, w, c, kind)
POOL = _pool_names()


@functools.lru_cache(maxsize=None)
def pool_case(name):
    """(hi, lo) fp16 [n, h, w, c].
    random    the split of N(0, 1)
    negative  every value below -0.5: a padding tap read as zero, or a best that starts at 0, would win on every border
    ties      EVERY element has the same sum per channel, hv + u/2 with u the fp16 step at hv, as one of three pairs by position:
              the canonical (hv, +u/2), (hv + u, -u/2) and (hv + 2u, -3u/2); the first tap of the scan must be copied
    nan1      random, with (NaN, 0.5) at pixel (1, 1) of every second channel
    nan2      nan1 and a second NaN with the pair (2.0, NaN) at pixel (1, 2): both lie in output (1, 1)'s window"""
    n, h, w, c, kind = POOL[name]
    rng = _rng("pool", name)
    v = rng.standard_normal((n, h, w, c)).astype(F)
    if kind == "negative":
        v = (-np.abs(v) - F(0.5)).astype(F)
    hi, lo = sr.split(v)
    if kind == "ties":
        hv = (2.0 ** (np.arange(c) % 4 - 1)).astype(F)
        u = hv * F(2.0 ** -10)
        form = (np.arange(h)[:, None, None] * 5 + np.arange(w)[None, :, None] * 2 + np.arange(c)[None, None, :] + np.arange(n)[:, None, None, None]) % 3
        hi = (hv + form * u).astype(H)
        lo = ((0.5 - form) * u).astype(H)
        assert sr.same_bits(sr.unsplit(hi, lo), np.broadcast_to((hv + u / 2).astype(F), hi.shape))
    if kind in ("nan1", "nan2"):
        hi, lo = hi.copy(), lo.copy()
        hi[:, 1, 1, ::2], lo[:, 1, 1, ::2] = np.nan, 0.5
        if kind == "nan2":
            hi[:, 1, 2, ::4], lo[:, 1, 2, ::4] = 2.0, np.nan
    hi, lo = np.ascontiguousarray(hi), np.ascontiguousarray(lo)
    _ro(hi, lo)
    return hi, lo


@functools.lru_cache(maxsize=None)
def pool_expected(name):
    out = sr.rule_pool(*pool_case(name))
    _ro(*out)
    return out


# unsplit: pool tensors read dense, and one read as a block slice of a wider S32 tensor and written as a channel slice of a
# wider fp32 tensor -> name: (pool case, strided)
UNSPLIT = {"ties": ("ties-5x5-c32", False), "nan2": ("nan2-7x6-c64", False), "random": ("random-4x5-c64", False),
           "ties-strided": ("ties-4x4-c32", True), "random-strided": ("random-7x6-c32", True)}


@functools.lru_cache(maxsize=None)
def unsplit_case(name):
    """-> dict: the flat S32 input (xbuf, x_off, xs), the output arena's geometry (y_size, y_off, ys), npix, c and the expected
    arena by the rule"""
    pool, strided = UNSPLIT[name]
    hi, lo = pool_case(pool)
    n, h, w, c = hi.shape
    nb, npix = c // 32, n * h * w
    b0, nbw = (2, nb + 3) if strided else (0, nb)
    c0, cw = (32, c + 64) if strided else (0, c)
    xs, ys = 64 * nbw, cw
    xbuf = sr.split(_rng("unsplit", name).standard_normal(npix * xs).astype(F))[0]
    sr.place(xbuf, 64 * b0, hi.reshape(npix, c), lo.reshape(npix, c), xs)
    want = np.full(2 * GUARD + npix * ys, SENTINEL32, F)
    off = GUARD + c0 + np.arange(npix)[:, None] * ys + np.arange(c)[None, :]
    want[off] = sr.unsplit(hi, lo).reshape(npix, c)
    _ro(xbuf, want)
    return dict(xbuf=xbuf, x_off=64 * b0, xs=xs, b0=b0, nbw=nbw, y_size=want.size, y_off=GUARD + c0, ys=ys, c0=c0, cw=cw,
                npix=npix, c=c, shape=(n, h, w), want=want)


# --------------------------------------------------------------------------------------------------------------------------
# where each mutant of split_ref must fail: (kind, case name[, (affine, relu)])
# --------------------------------------------------------------------------------------------------------------------------
MUTANT_CASE = {
    "mul_add": ("apply", "ladder", (True, False)),
    "image0_tables": ("apply", "c256-hw9-n3", (True, True)),
    "table_stride_ignored": ("apply", "c32-hw65-n3", (True, True)),
    "relu_before_affine": ("apply", "c32-hw1-n1", (True, True)),
    "relu_launders_nan": ("flag", "nan-relu"),
    "relu_keeps_neg_zero": ("apply", "ladder", (False, True)),
    "hi_truncated": ("apply", "c32-hw1-n1", (False, False)),
    "lo_truncated": ("apply", "c32-hw1-n1", (False, False)),
    "f16_denormals_flushed": ("apply", "c2048-hw1-n1", (False, False)),
    "lo_of_unclamped": ("apply", "c32-hw1-n1", (True, True)),
    "lo_at_plus_8": ("apply", "c32-hw1-n1", (False, False)),
    "block_stride_32": ("apply", "c256-hw1-n1", (False, False)),
    "tail_pixel_dropped": ("apply", "c32-hw63-n1", (True, True)),
    "second_unrolled_pixel_aliased": ("apply", "c32-hw65-n1", (True, True)),
    "level_boundary_off_by_one": ("levels", "three"),
    "flag_ge": ("flag", "65504"),
    "flag_misses_nan": ("flag", "nan"),
    "flag_before_relu": ("flag", "-1e5-relu"),
    "last_tie": ("pool", "ties-3x3-c32"),
    "nan_dropped": ("pool", "nan1-3x3-c32"),
    "pad_reads_zero": ("pool", "negative-1x1-c32"),
    "hi_only_compare": ("pool", "ties-2x2-c32"),
    "pair_resplit": ("pool", "ties-1x2-c64"),
    "lo_ignored": ("unsplit", "ties"),
}
