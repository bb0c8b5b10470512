"""Seeded inputs of the hand cloud's tests (tests/test_cloud_cpu.py, tests/test_cloud_gpu.py): synthetic silhouettes, mesh depths
and scene depths made here, not a rendered scene, so the kernel and the rule (tests/cloud_ref.py) read identical bytes and no
pixel has to be left out of a comparison."""
import collections
import functools

import numpy as np

import cloud_ref as cr

F = np.float32
# (N, K, H, W, P, stride): a frame smaller than a chunk; odd sizes with P = 1 and stride 3; more than one strip and workgroup at
# stride 1; 16 slots on odd sizes, more than one workgroup per frame and P reached; the live frame
SHAPES = [(1, 1, 5, 7, 4, 1), (2, 3, 33, 65, 1, 3), (2, 2, 48, 64, 64, 1), (3, 16, 203, 301, 4096, 2), (1, 2, 480, 640, 4096, 2)]
BAND = 0.0625              # 2^-4: the edges below are exact
HOLES = (0.0, -0.5, np.nan, np.inf, -np.inf)      # the five kinds of invalid depth

Case = collections.namedtuple("Case", "n k h w points stride band best sil depth paras edges")
# best fp32 [N,H,W]; sil uint8 [N,H,W]; depth fp32 [N,H,W]; paras 4 floats; edges: the pixels (i, r, c, inside) set to the band's edges


def _box(rng, h, w, lo, hi):
    bh, bw = max(1, int(h * rng.uniform(lo, hi))), max(1, int(w * rng.uniform(lo, hi)))
    r0, c0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
    return slice(r0, r0 + bh), slice(c0, c0 + bw)


@functools.lru_cache(maxsize=None)
def case(n, k, h, w, points, stride) -> Case:
    """worked out once per shape, shared, never changed"""
    rng = np.random.default_rng(1000 * h + w + 7 * k)
    sil = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        # slot 0: a blob over most of the frame (it overflows P where P can be reached), the others small, drawn over it; the
        # last slot of the last frame stays empty (where there are three slots or more)
        sil[i, max(0, h // 20):h - h // 20, max(1, w // 20):w - w // 20] = 1
        for kk in range(1, k):
            if i == n - 1 and kk == k - 1 and n * k >= 3:
                continue
            sil[i][_box(rng, h, w, 0.06, 0.2)] = kk + 1
        # bytes that name no slot of this step: K + 1 and 0x7F, with and without the hidden flag
        sil[i][_box(rng, h, w, 0.05, 0.15)] = k + 1
        sil[i][_box(rng, h, w, 0.05, 0.15)] = 0x7F
        sil[i][_box(rng, h, w, 0.03, 0.1)] = 0x80 | (k + 1)
    hidden = (rng.random((n, h, w)) < 0.2) & (sil != 0)
    sil[hidden] |= 0x80
    best = rng.uniform(0.3, 1.2, (n, h, w)).astype(F)
    depth = (best + rng.uniform(-2 * BAND, 2 * BAND, (n, h, w)).astype(F)).astype(F)
    kinds = rng.integers(0, 20 * len(HOLES), (n, h, w))              # a pixel in twenty is a hole, of the five kinds in turn
    for j, value in enumerate(HOLES):
        depth[kinds == j] = F(value)
        depth[0].reshape(-1)[h * w - 1 - 2 * j] = F(value)            # (every kind in the smallest frame too)
    # the band's exact edges on the first four candidates under a valid slot byte: best = 0.5, e = +band (in), the next depth
    # above (out), e = -band (in), the next depth below (out): every e is representable
    who = sil & 0x7F
    rows, cols = np.nonzero((who[0] >= 1) & (who[0] <= k) & (np.arange(h)[:, None] % stride == 0) & (np.arange(w)[None, :] % stride == 0))
    up, down = F(0.5) + F(BAND), F(0.5) - F(BAND)
    values = ((up, True), (np.nextafter(up, F(np.inf)), False), (down, True), (np.nextafter(down, F(0)), False))
    edges = []
    for (r, c), (value, inside) in zip(zip(rows.tolist(), cols.tolist()), values):
        best[0, r, c], depth[0, r, c] = F(0.5), value
        edges.append((0, r, c, inside))
    best[sil == 0] = 0                                                # (as the raster leaves it)
    paras = (0.9 * w + 0.343, 0.95 * w + 0.171, w / 2 - 0.37, h / 2 + 0.21)
    return Case(n, k, h, w, points, stride, BAND, best, sil, depth, paras, tuple(edges))


@functools.lru_cache(maxsize=None)
def expected(n, k, h, w, points, stride, rig_seed=None):
    """cloud_ref on the case (rig_seed: in the rig frame, with rig_cases.extrinsics(n, seed=rig_seed))"""
    c = case(n, k, h, w, points, stride)
    table = None
    if rig_seed is not None:
        import rig_cases as rc
        import rig_ref as rr
        table = rr.table(rc.extrinsics(n, seed=rig_seed))
    return cr.hand_cloud(c.best, c.sil, c.depth, c.paras, k, points, c.band, stride, table)


def census(c: Case):
    """(matches, candidates under a valid slot byte with a valid depth that the band rejects) of the case, counted without the
    rule's own functions where that is cheap"""
    who = (c.sil & 0x7F).astype(int)
    cand = np.zeros(c.sil.shape, bool)
    cand[:, ::c.stride, ::c.stride] = True
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(c.depth) & (c.depth > 0)
        inside = np.abs(c.depth - c.best) <= F(c.band)
    slot = cand & (who >= 1) & (who <= c.k) & valid
    return int((slot & inside).sum()), int((slot & ~inside).sum())


def check_conditions(c: Case, want):
    """what a case must offer before a comparison means anything; a case that misses one fails"""
    total, written = want.count[:, 0], want.count[:, 1]
    matches, rejected = census(c)
    assert matches == int(total.sum())
    truncated, partial = int((total > c.points).sum()), int(((total > 0) & (total < c.points)).sum())
    print(f"case {c.n}x{c.k} {c.h}x{c.w} P={c.points} q={c.stride}: {matches} matches, {rejected} rejected by the band, "
          f"{truncated} slots truncated, {partial} partly filled, {int((total == 0).sum())} empty")
    if c.h >= 48 and c.w >= 64:
        assert matches >= 100 and rejected >= 100, (matches, rejected)
    assert truncated + partial >= 1
    if c.points > 1 and c.n * c.k > 1:       # (one slot cannot be both, and 0 < total < 1 does not exist)
        assert truncated >= 1 and partial >= 1, (truncated, partial)
    else:
        assert truncated >= 1
    if c.n * c.k >= 3:
        assert int((total == 0).sum()) >= 1                           # the empty slot
    assert np.array_equal(written, np.minimum(total, c.points))
    return matches, rejected
