"""Seeded inputs of the iterated fit's tests (tests/test_refit_cpu.py, tests/test_refit_gpu.py): tessellated ellipsoids
(raster_ref.ellipsoid) as the hand slots' meshes, their first mesh depth and slot byte drawn by the rule itself
(refit_ref.geometry), and scene depths ray-cast analytically (fit_cases.ray_cast) from the same ellipsoids turned and shifted by
a known rigid motion, with depth noise and holes.  Made here, not rendered, so the kernels and the rule read identical bytes."""
import collections
import functools

import numpy as np

import cams_ref
import fit_cases as fc
import fit_ref as fr
import raster_ref as rr
import refit_ref as rf

F = np.float32
RADII = np.array([0.05, 0.08, 0.03])          # raster_ref's hand-sized ellipsoid
JOINTS = 21
BACKGROUND = 2.0
# (N, K, H, W, stride, iterations): one slot on a small frame; two frames of two slots; sixteen slots on odd sizes; the live frame
SHAPES = [(1, 1, 48, 64, 1, 2), (2, 2, 96, 128, 1, 4), (1, 16, 203, 301, 2, 3), (1, 2, 480, 640, 2, 3)]
# per shape: min_points, chosen so that the large slots pass it in every iteration and the small slot of the shape never does
MIN_POINTS = {(1, 1, 48, 64, 1, 2): 100, (2, 2, 96, 128, 1, 4): 60, (1, 16, 203, 301, 2, 3): 40, (1, 2, 480, 640, 2, 3): 200}

Case = collections.namedtuple("Case", "n k h w stride iters min_points best sil depth paras mesh xyz_mm faces lifted truth")
# best fp32 [N,H,W] and sil uint8 [N,H,W]: refit_ref.geometry of the meshes; depth fp32 [N,H,W]; paras 4 floats; mesh fp32
# [N*K,V,3]; xyz_mm fp32 [N*K,21,3]; faces int32 [F,3]; lifted int32 [N*K]; truth: per slot (centre, Q) of the measured surface


def _slot(rng, centre, scale, angle, shift_len, rings, segs):
    """one slot: (mesh fp32 [V,3], faces, xyz_mm fp32 [21,3], (moved centre, Q of the moved surface))"""
    centre, radii = np.asarray(centre, np.float64), RADII * scale
    mesh, faces = rr.ellipsoid(centre, radii, rings=rings, segs=segs)
    xyz = ((centre + rng.uniform(-1, 1, (JOINTS, 3)) * radii) * 1000.0).astype(F)
    xyz[0] = ((centre + np.array([0.0, 0.07 * scale, 0.0])) * 1000.0).astype(F)       # the root: 7 cm below the centre
    turn = fc.rotation(rng, angle)
    shift = rng.normal(size=3)
    shift *= shift_len / np.linalg.norm(shift)
    return mesh, faces, xyz, (centre + shift, fc.quadric(radii, turn))                   # (turned about its own centre)


def scene_depth(rng, h, w, paras, truths, noise=0.001):
    """the nearest of the moved ellipsoids along every pixel's ray, with depth noise; the background elsewhere: fp64 [h,w]"""
    depth = np.full((h, w), np.inf)
    for centre, q in truths:
        z = fc.ray_cast(h, w, paras, centre, q)
        with np.errstate(invalid="ignore"):
            depth = np.where(z < depth, z, depth)
    hit = np.isfinite(depth)
    return np.where(hit, depth + rng.normal(0, noise, (h, w)), BACKGROUND)


def chain_case(seed, h=96, w=128, paras=(123.0, 123.0, 64.0, 48.0)):
    """the CPU recovery through the mesh chain: one 1550-face ellipsoid half a metre away, the measured surface turned by 0.1 rad
    about a seeded axis and shifted by 1.5 cm, 1 mm depth noise, stride 1 -> Case (iters = 4)"""
    rng = np.random.default_rng(seed)
    mesh, faces, xyz, truth = _slot(rng, (0.01, -0.005, 0.5), 1.0, 0.1, 0.015, 25, 31)
    depth = scene_depth(rng, h, w, paras, [truth]).astype(F)
    best, sil = rf.geometry(mesh[None], faces, paras, h, w)
    return Case(1, 1, h, w, 1, 4, fr.FIT_MIN_POINTS, best[None], sil[None], depth[None], paras, mesh[None], xyz[None], faces,
                np.ones(1, np.int32), (truth,))


@functools.lru_cache(maxsize=None)
def case(n, k, h, w, stride, iters) -> Case:
    """worked out once per shape, shared, never changed.  Frame i's slots sit on a grid over the frame at 0.5 m; slot 0 of
    every frame is full-sized for the frame, the LAST slot of the step is not lifted (its mesh is still there), and -- steps
    of three slots or more -- the slot before it is a fifth as large: it stays below min_points in every iteration."""
    rng = np.random.default_rng(1000 * h + w + 7 * k)
    small = h < 64 or k == 16                                             # (a slot covers a few dozen pixels a side)
    rings, segs = (cams_ref.RINGS, cams_ref.SEGS) if small else (25, 31)
    cols = int(np.ceil(np.sqrt(k)))
    rows = (k + cols - 1) // cols
    f = 0.96 * w / cols                                                   # a slot's cell is about w / cols pixels wide
    paras = (f + 0.343, f + 0.171, w / 2 - 0.37, h / 2 + 0.21)
    z = 0.5
    scale = min(1.0, 0.42 * (h / rows) * z / (f * RADII[1]), 0.42 * (w / cols) * z / (f * RADII[0]))
    s_total = n * k
    meshes, xyzs, truths, lifted = [], [], [], np.ones(s_total, np.int32)
    for s in range(s_total):
        kk = s % k
        r, c = divmod(kk, cols)
        u, v = (c + 0.5) * w / cols + rng.uniform(-2, 2), (r + 0.5) * h / rows + rng.uniform(-2, 2)
        centre = ((u - paras[2]) * z / paras[0], (v - paras[3]) * z / paras[1], z + 0.01 * kk)
        tiny = s_total >= 3 and s == s_total - 2
        mesh, faces, xyz, truth = _slot(rng, centre, scale * (0.2 if tiny else 1.0), rng.uniform(0.03, 0.1), rng.uniform(0.003, 0.012),
                                        rings, segs)
        meshes.append(mesh); xyzs.append(xyz); truths.append(truth)
    if s_total >= 2:
        lifted[-1] = 0
    mesh, xyz = np.stack(meshes), np.stack(xyzs)
    best, sil = rf.geometry_frames(mesh, faces, paras, k, h, w, lifted)
    depth = np.stack([scene_depth(rng, h, w, paras, truths[i * k:(i + 1) * k]) for i in range(n)]).astype(F)
    kinds = rng.integers(0, 20 * len(fc.HOLES), (n, h, w))               # a pixel in twenty is a hole, of the five kinds in turn
    for j, value in enumerate(fc.HOLES):
        depth[kinds == j] = F(value)
    return Case(n, k, h, w, stride, iters, MIN_POINTS[(n, k, h, w, stride, iters)], best, sil, depth, paras, mesh, xyz,
                faces.astype(np.int32), lifted, tuple(truths))


def kwargs(c: Case):
    return dict(stride=c.stride, min_points=c.min_points)


@functools.lru_cache(maxsize=None)
def expected(n, k, h, w, stride, iters):
    """refit_ref on the case"""
    c = case(n, k, h, w, stride, iters)
    return rf.mesh_fit_iters(c.best, c.sil, c.depth, c.paras, c.mesh, c.xyz_mm, c.faces, k, iters, lifted=c.lifted, **kwargs(c))


def check_conditions(c: Case, want):
    """what a case must offer before a comparison means anything: a slot fitted in every iteration; and, where the step has the
    slots for it, an unlifted slot (two slots or more) and a lifted slot with a non-zero status in some iteration (three or more)"""
    status, matches = want.trace[:, :, 1], want.trace[:, :, 0]
    print(f"case {c.n}x{c.k} {c.h}x{c.w} q={c.stride} I={c.iters}: matches {matches.tolist()}, status {status.tolist()}, "
          f"cost {want.trace[:, :, 2].tolist()}")
    assert (status == 0).all(axis=1).any(), "no slot was fitted in every iteration"
    s = c.n * c.k
    if s >= 2:
        assert c.lifted[-1] == 0 and (status[-1] != 0).all() and want.mesh[-1].tobytes() == c.mesh[-1].tobytes()
    if s >= 3:
        assert ((status != 0).any(axis=1) & (c.lifted != 0)).any(), "no lifted slot with a non-zero status"
    assert want.trace.shape == (s, c.iters, 3)
