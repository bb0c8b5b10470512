"""The overlay's rule in plain numpy (helper of test_render_cpu.py / test_render_gpu.py; DESIGN.md "The overlay"):

  projection   (X, Y, Z) = (x, -y, -z) of out['mesh']; u = (fx X) / Z + cx, v = (fy Y) / Z + cy in fp32, one rounding per
               operation, intrinsics rounded to fp32 first
  snapping     xi = rint(256 u), yi = rint(256 v); a vertex with non-finite coordinates, Z < 0.05, Z > 100 or
               |xi|, |yi| >= 2^24 rejects every face that uses it; a face of zero doubled area is not drawn
  coverage     int64 edge functions at the sample points (256 col + 128, 256 row + 128), both windings, a sample exactly on
               an edge belongs to the face when the edge is a top or a left edge
  depth        barycentric interpolation of the three Z in float64; the smallest wins, the lower face index on an exact tie
  colour       flat: shade = min(1, 0.3 + 2.4 |n_z| / (|n| pi)), rgb8 = floor(255 shade (1, 1, 0.9) + 0.5)
  image        the face's colour on covered pixels, the frame's own pixel elsewhere
"""
import collections

import numpy as np

SUB, HALF = 256, 128
NEAR, FAR = 0.05, 100.0
BASE = np.array([1.0, 1.0, 0.9])

Raster = collections.namedtuple("Raster", "z1 z2 count face face2")
# z1 / z2 float64 [H,W]: nearest and second-nearest depth (inf where there is none); count int [H,W]: faces covering the
# pixel; face / face2 int [H,W]: index of the nearest / second-nearest face in the concatenated (slot-major) face list, -1
# where there is none


def project(mesh, paras):
    """mesh [V,3] float32 (out['mesh']) -> (xi int64 [V], yi int64 [V], Z float32 [V], ok bool [V])"""
    m = np.asarray(mesh, np.float32)
    fx, fy, cx, cy = (np.float32(p) for p in paras)
    X, Y, Z = m[:, 0], -m[:, 1], -m[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(X) & np.isfinite(Y) & (Z >= np.float32(NEAR)) & (Z <= np.float32(FAR))
        zs = np.where(ok, Z, np.float32(1))
        u = (fx * X) / zs + cx
        v = (fy * Y) / zs + cy
        xs, ys = np.rint(u * np.float32(SUB)), np.rint(v * np.float32(SUB))
        ok = ok & (np.abs(xs) < 2.0 ** 24) & (np.abs(ys) < 2.0 ** 24)
    xi = np.where(ok, xs, 0).astype(np.int64)
    yi = np.where(ok, ys, 0).astype(np.int64)
    return xi, yi, Z, ok


def _edge(ax, ay, bx, by, px, py):
    """Edge a -> b of a face with positive doubled area (clockwise on the screen, y down): (E, sample belongs)."""
    dx, dy = int(bx - ax), int(by - ay)
    e = dx * (py - ay) - dy * (px - ax)
    top_left = dy < 0 or (dy == 0 and dx > 0)
    return e, (e > 0) | ((e == 0) & top_left)


def face_colour(a, b, c):
    """a, b, c: the face's three vertices (any consistent frame with z along the view axis) -> rgb uint8 [3]"""
    n = np.cross(np.asarray(b, np.float64) - np.asarray(a, np.float64), np.asarray(c, np.float64) - np.asarray(a, np.float64))
    length = np.linalg.norm(n)
    l = abs(n[2]) / length if length > 0 else 0.0
    shade = min(1.0, 0.3 + 2.4 * l / np.pi)
    return np.clip(np.floor(255.0 * shade * BASE + 0.5), 0, 255).astype(np.uint8)


def rasterize(meshes, faces, paras, h, w, lifted=None):
    """meshes [K,V,3] float32: the K slots of ONE frame; faces int [F,3]; lifted [K] or None -> (Raster, colours uint8 [K*F,3])"""
    meshes = np.asarray(meshes, np.float32)
    faces = np.asarray(faces, np.int64)
    k, nv, nf = meshes.shape[0], meshes.shape[1], faces.shape[0]
    z1, z2 = np.full((h, w), np.inf), np.full((h, w), np.inf)
    count, face, face2 = np.zeros((h, w), np.int64), np.full((h, w), -1, np.int64), np.full((h, w), -1, np.int64)
    colours = np.zeros((k * nf, 3), np.uint8)
    for s in range(k):
        if lifted is not None and not lifted[s]:
            continue
        xi, yi, z, ok = project(meshes[s], paras)
        for fi, t in enumerate(faces):
            if t.min() < 0 or t.max() >= nv or not ok[t].all():
                continue
            (ax, bx, cx), (ay, by, cy) = (int(q) for q in xi[t]), (int(q) for q in yi[t])
            za, zb, zc = (float(q) for q in z[t])
            area = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay)
            if area == 0:
                continue
            if area < 0:
                bx, by, zb, cx, cy, zc = cx, cy, zc, bx, by, zb
                area = -area
            x0, x1 = max(-((-(min(ax, bx, cx) - HALF)) // SUB), 0), min((max(ax, bx, cx) - HALF) // SUB, w - 1)
            y0, y1 = max(-((-(min(ay, by, cy) - HALF)) // SUB), 0), min((max(ay, by, cy) - HALF) // SUB, h - 1)
            if x0 > x1 or y0 > y1:
                continue
            colours[s * nf + fi] = face_colour(meshes[s, t[0]], meshes[s, t[1]], meshes[s, t[2]])
            px = (np.arange(x0, x1 + 1, dtype=np.int64) * SUB + HALF)[None, :]
            py = (np.arange(y0, y1 + 1, dtype=np.int64) * SUB + HALF)[:, None]
            wa, ia = _edge(bx, by, cx, cy, px, py)
            wb, ib = _edge(cx, cy, ax, ay, px, py)
            wc, ic = _edge(ax, ay, bx, by, px, py)
            ins = ia & ib & ic
            if not ins.any():
                continue
            zz = np.where(ins, (wa * za + wb * zb + wc * zc) / float(area), np.inf)
            win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            o1, o2 = z1[win], z2[win]
            nearer = zz < o1                        # (strict: the lower face index keeps an exact tie)
            face2[win] = np.where(nearer, face[win], np.where(zz < o2, s * nf + fi, face2[win]))
            z2[win] = np.where(nearer, o1, np.minimum(o2, zz))
            z1[win] = np.where(nearer, zz, o1)
            face[win] = np.where(nearer, s * nf + fi, face[win])
            count[win] += ins
    return Raster(z1, z2, count, face, face2), colours


def frame_u8(frame):
    """One frame as RGB uint8 [H,W,3]: from fp32 CHW in 0..1 (rint(255 x)) or from bgr8 HWC."""
    frame = np.asarray(frame)
    if frame.dtype == np.uint8:
        return frame[..., ::-1].copy()
    with np.errstate(all="ignore"):
        q = np.rint(np.float32(255) * frame.astype(np.float32))
    return np.clip(np.nan_to_num(q, nan=0.0), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def composite(raster, colours, frame):
    """image = colour of the nearest face where covered, the frame elsewhere; depth = Z there, 0 elsewhere"""
    covered = raster.face >= 0
    image = frame_u8(frame)
    image[covered] = colours[raster.face[covered]]
    return image, np.where(covered, raster.z1, 0.0), covered


def ambiguous(raster, rel=1e-4):
    """covered pixels whose nearest and second-nearest depth differ by at most `rel` relative (depth fights)"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(raster.z1) & np.isfinite(raster.z2) & ((raster.z2 - raster.z1) <= rel * raster.z1)


def render(meshes, faces, paras, frame, lifted=None):
    """meshes [K,V,3] of one frame -> (image uint8 [H,W,3], depth float64 [H,W], covered bool, ambiguous bool)"""
    f8 = frame_u8(frame)
    h, w = f8.shape[:2]
    ras, colours = rasterize(meshes, faces, paras, h, w, lifted)
    image, depth, covered = composite(ras, colours, frame)
    return image, depth, covered, ambiguous(ras)


def render_candidates(meshes, faces, paras, frame, lifted=None):
    """As render(), plus the image with the SECOND-nearest face's colour where there is one (else the nearest's): what a
    depth fight may legitimately show.  -> (image, image2, covered, ambiguous)"""
    f8 = frame_u8(frame)
    h, w = f8.shape[:2]
    ras, colours = rasterize(meshes, faces, paras, h, w, lifted)
    image, _depth, covered = composite(ras, colours, frame)
    image2 = image.copy()
    second = ras.face2 >= 0
    image2[second] = colours[ras.face2[second]]
    return image, image2, covered, ambiguous(ras)


def ellipsoid(centre, radii, rings=25, segs=31, flip=False):
    """A closed triangle mesh of an ellipsoid in out['mesh'] coordinates (y, z negated): rings * segs + 2 vertices,
    2 * rings * segs faces (25 x 31: 777 vertices, 1550 faces).  centre / radii in the camera frame (Z > 0 in front)."""
    th = np.linspace(0, np.pi, rings + 2)[1:-1]
    ph = np.linspace(0, 2 * np.pi, segs, endpoint=False)
    v = [[0, 0, 1]] + [[np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)] for t in th for p in ph] + [[0, 0, -1]]
    v = np.array(v) * np.asarray(radii, np.float64) + np.asarray(centre, np.float64)
    f = [[0, 1 + s, 1 + (s + 1) % segs] for s in range(segs)]
    for i in range(rings - 1):
        for s in range(segs):
            a, b = 1 + i * segs + s, 1 + i * segs + (s + 1) % segs
            f += [[a, a + segs, b], [b, a + segs, b + segs]]
    last = len(v) - 1
    f += [[last, 1 + (rings - 1) * segs + (s + 1) % segs, 1 + (rings - 1) * segs + s] for s in range(segs)]
    f = np.array(f, np.int32)
    if flip:
        f = f[:, ::-1].copy()
    return (v * np.array([1.0, -1.0, -1.0])).astype(np.float32), f


def frame_bgr8(n, h, w, seed):
    """n seeded noise frames as the camera hands them over: uint8 [n,h,w,3] 'bgr8'"""
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


PARAS = (615.0, 615.0, 320.0, 240.0)


def scenes():
    """The op-level scenes of tests/test_render_gpu.py (tools/bench_render.py measures the depth difference on the same ones):
    name -> (meshes [N,K,V,3], faces [F,3], lifted [N,K] or None, paras, (h, w))"""
    e1, f = ellipsoid((0.02, -0.01, 0.55), (0.05, 0.08, 0.03))
    e2, _ = ellipsoid((0.06, 0.02, 0.56), (0.06, 0.04, 0.04))
    out = {}
    out["one ellipsoid"] = (e1[None, None], f, None, PARAS, (480, 640))
    out["two interpenetrating ellipsoids"] = (np.stack([e1, e2])[None], f, None, PARAS, (480, 640))
    # partly outside a frame whose sides are no multiples of the tile: left / top border crossed, partial tiles right / bottom
    edge, _ = ellipsoid((-0.12, -0.08, 0.5), (0.06, 0.05, 0.04))
    corner, _ = ellipsoid((0.14, 0.09, 0.6), (0.07, 0.07, 0.03))
    out["partly outside the frame"] = (np.stack([edge, corner])[None], f, None, (600.0, 600.0, 150.0, 101.0), (203, 301))
    # two frames; one slot of each not lifted (its vertices are still there: the flag alone decides); the other winding
    out["a slot with lifted = 0"] = (np.stack([np.stack([e1, e2]), np.stack([e2, e1])]), f[:, ::-1].copy(),
                                     np.array([[1, 0], [0, 1]], np.int32), PARAS, (480, 640))
    # three frames, the middle one without any lifted slot (its vertices are still there) between two drawn ones
    out["a whole frame with lifted = 0"] = (np.stack([np.stack([e1, e2])] * 3), f,
                                            np.array([[1, 1], [0, 0], [0, 1]], np.int32), PARAS, (480, 640))
    # degenerate faces (repeated indices; a NaN vertex, 777; a vertex nearer than the near plane, 778), duplicates of the three
    # faces nearest to the camera (exact depth ties: the lower index wins) and of six hidden ones
    vv = np.concatenate([e1, np.array([[np.nan, 0, -0.5], [0.0, 0.0, -0.01]], np.float32)])
    ff = np.concatenate([f, f[-3:], f[:6], np.array([[5, 5, 9], [7, 7, 7], [3, 4, 777], [10, 11, 778], [0, 1, 0]], np.int32)])
    out["degenerate and duplicate faces"] = (vv[None, None], ff.astype(np.int32), None, PARAS, (480, 640))
    # vertices exactly on sample points: a flat square cut along its diagonal, both windings, at Z = 1 with unit intrinsics
    sq = np.array([[x, -y, -1.0] for x, y in ((0.5, 0.5), (20.5, 0.5), (0.5, 12.5), (20.5, 12.5), (30.5, 3.5), (30.5, 20.5))],
                  np.float32)
    out["vertices on sample points"] = (sq[None, None], np.array([[0, 1, 2], [2, 3, 1], [1, 4, 5]], np.int32), None,
                                        (1.0, 1.0, 0.0, 0.0), (24, 40))
    return out
