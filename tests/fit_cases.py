"""Seeded inputs of the mesh fit's tests (tests/test_fit_cpu.py, tests/test_fit_gpu.py): mesh depths ray-cast from analytic
ellipsoids (so that normals exist), one slot per ellipsoid with the nearer one drawn over the farther, scene depths from the
same ellipsoids moved by a known small rigid motion plus noise, made here, not a rendered scene, so the kernel and the rule
(tests/fit_ref.py) read identical bytes and no pixel has to be left out of a comparison."""
import collections
import functools

import numpy as np

import fit_ref as fr

F = np.float32
# (N, K, H, W, stride): a frame smaller than a chunk (min_points = 1); odd sizes with stride 3, the empty slot and a slot moved
# beyond a small max_shift; more than one strip and workgroup at stride 1, damp = 0 and the constant-depth patch; 16 slots on
# odd sizes, one of them below min_points; the live frame
SHAPES = [(1, 1, 5, 7, 1), (2, 3, 33, 65, 3), (2, 2, 48, 64, 1), (3, 16, 203, 301, 2), (1, 2, 480, 640, 2)]
VERTICES = (5, 778)
JOINTS = 21
BAND = 0.03125             # 2^-5: the edges below are exact
HOLES = (0.0, -0.5, np.nan, np.inf, -np.inf)      # the five kinds of invalid depth
BACKGROUND = 2.0           # metres: the scene behind the hands
# per shape: min_points, damp, max_shift (metres); max_angle stays the default
PARAMS = {(1, 1, 5, 7, 1): (1, 1e-3, 0.05), (2, 3, 33, 65, 3): (10, 1e-3, 0.01), (2, 2, 48, 64, 1): (30, 0.0, 0.05),
          (3, 16, 203, 301, 2): (30, 1e-3, 0.05), (1, 2, 480, 640, 2): (200, 1e-3, 0.05)}

Case = collections.namedtuple("Case", "n k h w stride band min_points damp max_shift max_angle best sil depth paras xyz_mm meshes edges")
# best fp32 [N,H,W]; sil uint8 [N,H,W]; depth fp32 [N,H,W]; paras 4 floats; xyz_mm fp32 [N*K,21,3]; meshes {V: fp32 [N*K,V,3]};
# edges: the pixels (i, r, c, slot, inside) set to the band's edges


def rotation(rng, angle):
    """a rotation by `angle` radians about a seeded axis, fp64 [3,3] (Rodrigues)"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * (kx @ kx)


def quadric(axes, rot):
    """Q of (p - c)^T Q (p - c) = 1: the ellipsoid with the semi-axes `axes` turned by `rot`"""
    return rot @ np.diag(1.0 / np.asarray(axes, np.float64) ** 2) @ rot.T


def ray_cast(h, w, paras, centre, q):
    """the nearest Z of the ellipsoid (centre, Q) along the ray through every pixel centre (+0.5): fp64 [H,W], nan where the
    ray misses"""
    fx, fy, cx, cy = (float(F(v)) for v in paras)
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = np.stack([(c + 0.5 - cx) / fx, (r + 0.5 - cy) / fy, np.ones((h, w))], axis=-1)
    qa = np.einsum("hwi,ij,hwj->hw", d, q, d)
    qb = d @ (q @ centre)
    qc = centre @ q @ centre - 1.0
    disc = qb * qb - qa * qc
    with np.errstate(invalid="ignore"):
        return np.where(disc > 0, (qb - np.sqrt(np.where(disc > 0, disc, 0))) / qa, np.nan)


def surface_distance(points, centre, q):
    """first-order distance of points fp64 [M,3] to the ellipsoid's surface: f / |grad f| with f = (p - c)^T Q (p - c) - 1"""
    d = np.asarray(points, np.float64) - centre
    g = d @ q
    return (np.einsum("mi,mi->m", g, d) - 1.0) / (2.0 * np.linalg.norm(g, axis=1))


def _box(rng, h, w, lo, hi):
    bh, bw = max(1, int(h * rng.uniform(lo, hi))), max(1, int(w * rng.uniform(lo, hi)))
    r0, c0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
    return slice(r0, r0 + bh), slice(c0, c0 + bw)


@functools.lru_cache(maxsize=None)
def case(n, k, h, w, stride) -> Case:
    """worked out once per shape, shared, never changed"""
    rng = np.random.default_rng(1000 * h + w + 7 * k)
    min_points, damp, max_shift = PARAMS[(n, k, h, w, stride)]
    paras = (0.9 * w + 0.343, 0.95 * w + 0.171, w / 2 - 0.37, h / 2 + 0.21)
    fx = paras[0]
    best = np.zeros((n, h, w), F)
    sil = np.zeros((n, h, w), np.uint8)
    depth = np.full((n, h, w), BACKGROUND, np.float64)
    xyz = np.zeros((n * k, JOINTS, 3), F)
    meshes = {v: np.zeros((n * k, v, 3), F) for v in VERTICES}
    small = min(h, w) < 32
    for i in range(n):
        near = np.full((h, w), np.inf)
        for kk in range(k):
            s = i * k + kk
            # joints and vertices: seeded points about the slot's place (the rule moves whatever it is given)
            z = rng.uniform(0.4, 0.7)
            radius_px = 6.0 if small else rng.uniform(0.3, 0.45) * min(h, w) if h < 48 else rng.uniform(0.2, 0.3) * min(h, w)
            if (n, k, h, w) == (3, 16, 203, 301) and s == 14:
                radius_px = 5.0                                       # the slot below min_points
            lo_r, lo_c = min(radius_px, h / 2), min(radius_px, w / 2)
            row, col = rng.uniform(lo_r, h - lo_r), rng.uniform(lo_c, w - lo_c)
            if kk == 0:
                row, col = h / 2 + rng.uniform(-1, 1), w / 2 + rng.uniform(-1, 1)
            a = radius_px * z / fx
            axes = a * np.array([1.0, rng.uniform(0.55, 0.8), rng.uniform(0.35, 0.5)])
            pose = rotation(rng, rng.uniform(0, np.pi))
            centre = np.array([(col - paras[2]) * z / paras[0], (row - paras[3]) * z / paras[1], z])
            root = centre + rng.uniform(-0.5, 0.5, 3) * a
            xyz[s] = ((centre + rng.uniform(-1, 1, (JOINTS, 3)) * a) * 1000.0).astype(F)
            xyz[s, 0] = (root * 1000.0).astype(F)
            for v in VERTICES:
                pts = centre + rng.uniform(-1, 1, (v, 3)) * a
                meshes[v][s] = (pts * np.array([1.0, -1.0, -1.0])).astype(F)
            empty = i == n - 1 and kk == k - 1 and n * k >= 3          # the last slot of the last frame stays empty
            patch = (n, k, h, w) == (2, 2, 48, 64) and s == 1            # the fronto-parallel constant-depth patch
            # the motion of the measured surface: small, or -- the slot that must exceed max_shift = 0.01 -- 2.5 cm
            far = (n, k, h, w) == (2, 3, 33, 65) and s == 3
            turn = rotation(rng, rng.uniform(0.01, 0.04) * (0.1 if small else 1.0))       # (a small frame's ellipsoid is large)
            shift = rng.normal(size=3)
            shift *= (0.025 if far else rng.uniform(0.001, 0.004)) / np.linalg.norm(shift)
            if empty:
                meshes[VERTICES[0]][s, 0] = (F(-0.0), F(np.nan), F(np.inf))      # (a slot left as it is keeps its bytes)
                continue
            if patch:
                rows, cols = slice(30, 44), slice(40, 60)
                zs = np.full((h, w), np.nan)
                zs[rows, cols] = 0.5
                moved = zs + 2.0 ** -6
            else:
                q0 = quadric(axes, pose)
                zs = ray_cast(h, w, paras, centre, q0)
                moved = ray_cast(h, w, paras, turn @ (centre - root) + root + shift, quadric(axes, turn @ pose))
            with np.errstate(invalid="ignore"):
                front = zs < near
            near[front] = zs[front]
            best[i][front] = zs[front].astype(F)
            sil[i][front] = kk + 1
            depth[i][front] = np.where(np.isnan(moved[front]), BACKGROUND, moved[front] if patch else
                                       moved[front] + rng.normal(0, 0.001, int(front.sum())))
        # bytes that name no slot of this step: K + 1 and 0x7F, with and without the hidden flag (the mesh depth stays)
        if small:
            continue                                                  # (15 candidates: a foreign byte would leave none)
        sil[i][_box(rng, h, w, 0.05, 0.15)] = k + 1
        sil[i][_box(rng, h, w, 0.05, 0.15)] = 0x7F
        sil[i][_box(rng, h, w, 0.03, 0.1)] = 0x80 | (k + 1)
    hidden = (rng.random((n, h, w)) < 0.2) & (sil != 0)
    sil[hidden] |= 0x80
    depth = depth.astype(F)
    kinds = rng.integers(0, 20 * len(HOLES), (n, h, w))               # a pixel in twenty is a hole, of the five kinds in turn
    if (n, k, h, w) == (2, 2, 48, 64):
        kinds[0, 30:44, 40:60] = 10 ** 6                              # (the patch stays whole: its sums are exact)
    for j, value in enumerate(HOLES):
        if not small:
            depth[kinds == j] = F(value)
        depth[0].reshape(-1)[h * w - 1 - 2 * j] = F(value)            # (every kind in the smallest frame too: its last row)
    # the band's exact edges on four matches that are no neighbours of each other: best = 0.5, e = +band (in), the next depth
    # above (out), e = -band (in), the next depth below (out): every e is representable.  A match's own normal is made of its
    # NEIGHBOURS' mesh depths, so the pixel's other conditions stay as they were.
    edges = []
    rows, cols, _t = fr.terms(best[0], sil[0], depth[0], paras, xyz[0, 0], 0, BAND, stride)
    up, down = F(0.5) + F(BAND), F(0.5) - F(BAND)
    values = ((up, True), (np.nextafter(up, F(np.inf)), False), (down, True), (np.nextafter(down, F(0)), False))
    picked = []
    for r, c in () if small else zip(rows.tolist(), cols.tolist()):
        if all(abs(r - pr) + abs(c - pc) > 2 for pr, pc in picked):
            picked.append((r, c))
        if len(picked) == len(values):
            break
    for (r, c), (value, inside) in zip(picked, values):
        best[0, r, c], depth[0, r, c] = F(0.5), value
        edges.append((0, r, c, 0, inside))
    return Case(n, k, h, w, stride, BAND, min_points, damp, max_shift, fr.FIT_MAX_ANGLE, best, sil, depth, paras, xyz, meshes,
                tuple(edges))


def kwargs(c: Case):
    return dict(band=c.band, stride=c.stride, min_points=c.min_points, damp=c.damp, max_shift=c.max_shift, max_angle=c.max_angle)


@functools.lru_cache(maxsize=None)
def expected(n, k, h, w, stride, v=VERTICES[-1]):
    """(fit_ref on the case with meshes of v vertices, the rejected candidates by reason)"""
    c = case(n, k, h, w, stride)
    census = {}
    return fr.mesh_fit(c.best, c.sil, c.depth, c.paras, c.meshes[v], c.xyz_mm, k, census=census, **kwargs(c)), census


def check_conditions(c: Case, want, census):
    """what a case must offer before a comparison means anything; a case that misses one fails"""
    matches, status = want.count[:, 0], want.count[:, 1]
    print(f"case {c.n}x{c.k} {c.h}x{c.w} q={c.stride}: matches per slot {matches.tolist()}, status {status.tolist()}, rejected {census}")
    assert (status == 0).any(), "no slot was fitted"
    assert ((status == 0) | (matches < c.min_points) | (status >= 2)).all() and ((status == 1) == (matches < c.min_points)).all()
    if c.h >= 48:
        rejected = census["neighbour"] + census["band"] + census["grazing"]
        assert int(matches.sum()) >= 100 and rejected >= 100, (int(matches.sum()), rejected)
        assert census["neighbour"] >= 1 and census["band"] >= 1 and census["grazing"] >= 1, census
    if c.n * c.k >= 3:
        assert matches[-1] == 0 and status[-1] == 1                   # the empty slot
    # border pixels reach no sum: every match has its slot's byte on all four neighbours, and lies off the frame's border;
    # counted here without the rule's own masks
    who = (c.sil & 0x7F).astype(int)
    total = 0
    for i in range(c.n):
        for kk in range(c.k):
            rows, cols, t = fr.terms(c.best[i], c.sil[i], c.depth[i], c.paras, c.xyz_mm[i * c.k + kk, 0], kk, c.band, c.stride)
            total += len(rows)
            assert len(rows) == matches[i * c.k + kk]
            if len(rows):
                assert rows.min() >= 1 and rows.max() <= c.h - 2 and cols.min() >= 1 and cols.max() <= c.w - 2
                assert (rows % c.stride == 0).all() and (cols % c.stride == 0).all()
                for dr, dc in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
                    assert (who[i, rows + dr, cols + dc] == kk + 1).all()
                    assert (c.best[i, rows + dr, cols + dc] > 0).all()
                assert np.abs(t).max() < 2 ** 33
    hit = {(i, kk): set(zip(*(a.tolist() for a in fr.terms(c.best[i], c.sil[i], c.depth[i], c.paras, c.xyz_mm[i * c.k + kk, 0], kk,
                                                           c.band, c.stride)[:2]))) for (i, _r, _c, kk, _in) in c.edges}
    assert len(c.edges) == (4 if c.h >= 32 else 0), c.edges       # (a frame of 15 candidates has none to spare)
    for (i, r, col, kk, inside) in c.edges:                           # the band's edges fall where the rule puts them
        assert ((r, col) in hit[(i, kk)]) == inside, (i, r, col, inside)
    return total


def check_statuses():
    """the case set as a whole reaches all four statuses, and status 1 both ways (an empty slot, one below min_points)"""
    seen, starved = set(), False
    for shape in SHAPES:
        want, _census = expected(*shape)
        seen |= set(want.count[:, 1].tolist())
        starved |= bool(((want.count[:, 1] == 1) & (want.count[:, 0] > 0)).any())
    assert seen == {0, 1, 2, 3}, seen
    assert starved
