"""The depth fit iterated, in numpy (csrc/mesh_raster.hip's geometry pass, csrc/mesh_refit.hip,
hn_mesh_geometry_f32 and hn_mesh_fit_iters_f32).  Every fp32 and fp64 operation is rounded on its own, in the order written here,
so the device's outputs can be compared bit for bit.  This file is the specification; it uses tests/raster_ref.py (projection,
snapping, edge functions), tests/fit_ref.py (one Gauss-Newton step) and nothing of the package.

geometry      the raster's nearest Z and slot per pixel.  Projection, snapping, rejection, winding, boxes and coverage are
              raster_ref's; the depth is the kernel's fp32 one:
                z = (((float)wa * za + (float)wb * zb) + (float)wc * zc) * inv_area,   inv_area = 1f / (float)area
              wa, wb, wc the int64 edge values converted to fp32 with round-to-nearest.  Slots ascending, faces ascending, a face
              wins on strict z < best (best starts at FLT_MAX).  depth = best (0: nothing drawn), who = slot + 1 (0: nothing).

mesh_fit_iters  iteration 1: fit_ref.mesh_fit on the given mesh_depth / silhouette.  Iteration t = 2..I: geometry of every
              slot's current mesh (a slot with lifted == 0 is not drawn), then fit_ref.mesh_fit on that depth and byte, the same
              scene depth and camera, the current mesh and joints -- so the lever point is the current root joint --, the same
              parameters and caps.  A slot whose iteration ends with a status other than 0 keeps its bytes for that iteration; it
              is tried again in the next and is still drawn.  No early stop.
              mesh, xyz: after the last iteration.  count, cost: of iteration 1.  trace int64 [slots, I, 3]: (matches, status,
              cost) of every iteration.
compose       rt: the iterations' motions as ONE motion about the original root joint c0 = xyz_mm[s][0] / 1000f, in fp64, scalar
              operations in this order.  R_t, t_t: iteration t's fp32 rt, c_t: its fp32 root joint / 1000f, all taken as doubles.
              The first iteration with status 0: R = R_t, T = t_t (nothing has moved before it, so c_t is c0 and its motion is
              the whole motion: with one iteration rt is fit_ref's, byte for byte).  Every further iteration with status 0:
                u = (c0 + T) - c_t;   T_j <- (((R_t u)_j + c_t_j) + t_t_j) - c0_j;   R <- R_t R,
              (R_t u)_j = (R_t[j][0] u_0 + R_t[j][1] u_1) + R_t[j][2] u_2, every entry of R_t R likewise ((a0 b0 + a1 b1) + a2 b2).
              Then R and T are rounded to fp32.  No iteration with status 0: the identity.
"""
import collections

import numpy as np

import fit_ref
import raster_ref

F = np.float32
FLT_MAX = F(3.402823466e38)
MAX_ITERS = 8

MeshFitIters = collections.namedtuple("MeshFitIters", "mesh xyz rt count cost trace")


def geometry(meshes, faces, paras, h, w, lifted=None):
    """meshes fp32 [K,V,3]: the K slots of ONE frame; faces int [F,3]; lifted [K] or None -> (depth fp32 [h,w], who uint8 [h,w])"""
    meshes = np.asarray(meshes, F)
    faces = np.asarray(faces, np.int64)
    k, nv = meshes.shape[0], meshes.shape[1]
    best = np.full((h, w), FLT_MAX, F)
    who = np.zeros((h, w), np.uint8)
    sub, half = raster_ref.SUB, raster_ref.HALF
    for s in range(k):
        if lifted is not None and not lifted[s]:
            continue
        xi, yi, z, ok = raster_ref.project(meshes[s], paras)
        for t in faces:
            if t.min() < 0 or t.max() >= nv or not ok[t].all():
                continue
            (ax, bx, cx), (ay, by, cy) = (int(q) for q in xi[t]), (int(q) for q in yi[t])
            za, zb, zc = (F(q) for q in z[t])
            area = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay)
            if area == 0:
                continue
            if area < 0:
                bx, by, zb, cx, cy, zc = cx, cy, zc, bx, by, zb
                area = -area
            x0, x1 = max(-((-(min(ax, bx, cx) - half)) // sub), 0), min((max(ax, bx, cx) - half) // sub, w - 1)
            y0, y1 = max(-((-(min(ay, by, cy) - half)) // sub), 0), min((max(ay, by, cy) - half) // sub, h - 1)
            if x0 > x1 or y0 > y1:
                continue
            px = (np.arange(x0, x1 + 1, dtype=np.int64) * sub + half)[None, :]
            py = (np.arange(y0, y1 + 1, dtype=np.int64) * sub + half)[:, None]
            wa, ia = raster_ref._edge(bx, by, cx, cy, px, py)
            wb, ib = raster_ref._edge(cx, cy, ax, ay, px, py)
            wc, ic = raster_ref._edge(ax, ay, bx, by, px, py)
            ins = ia & ib & ic
            if not ins.any():
                continue
            with np.errstate(all="ignore"):
                inv_area = F(1.0) / F(np.int64(area))
                wa, wb, wc = (np.broadcast_to(e, ins.shape).astype(np.int64).astype(F) for e in (wa, wb, wc))
                zz = ((wa * za + wb * zb) + wc * zc) * inv_area
                win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
                nearer = ins & (zz < best[win])
            best[win] = np.where(nearer, zz, best[win])
            who[win] = np.where(nearer, np.uint8(s + 1), who[win])
    return np.where(who != 0, best, F(0)).astype(F), who


def geometry_frames(mesh, faces, paras, k, h, w, lifted=None):
    """mesh fp32 [N*K,V,3]; paras: 4 values or a row per frame [N,4]; lifted [N*K] or None -> (depth [N,h,w], who [N,h,w])"""
    mesh = np.asarray(mesh, F)
    n = mesh.shape[0] // k
    cams = np.asarray(paras, np.float64).astype(F)
    cams = np.tile(cams, (n, 1)) if cams.ndim == 1 else cams
    depth, who = np.empty((n, h, w), F), np.empty((n, h, w), np.uint8)
    for i in range(n):
        lif = None if lifted is None else np.asarray(lifted).reshape(-1)[i * k:(i + 1) * k]
        depth[i], who[i] = geometry(mesh[i * k:(i + 1) * k], faces, cams[i], h, w, lif)
    return depth, who


def compose(c0, steps):
    """c0: the original root joint (3 fp32, metres); steps: (status, rt fp32 [12], c fp32 [3]) of every iteration -> rt fp32 [12]"""
    c0 = [float(v) for v in c0]
    big_r, big_t, moved = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], False
    for status, rt, c in steps:
        if status != 0:
            continue
        r, t, c = [float(v) for v in rt[:9]], [float(v) for v in rt[9:]], [float(v) for v in c]
        if not moved:
            big_r, big_t, moved = r, t, True
            continue
        u = [(c0[j] + big_t[j]) - c[j] for j in range(3)]
        new_t = [((((r[3 * j] * u[0] + r[3 * j + 1] * u[1]) + r[3 * j + 2] * u[2]) + c[j]) + t[j]) - c0[j] for j in range(3)]
        big_r = [(r[3 * i] * big_r[j] + r[3 * i + 1] * big_r[3 + j]) + r[3 * i + 2] * big_r[6 + j] for i in range(3) for j in range(3)]
        big_t = new_t
    with np.errstate(all="ignore"):
        return np.array(big_r + big_t, np.float64).astype(F)


def mesh_fit_iters(best, sil, depth, paras, mesh, xyz_mm, faces, k, iters, lifted=None, band=fit_ref.FIT_BAND,
                   stride=fit_ref.FIT_STRIDE, min_points=fit_ref.FIT_MIN_POINTS, damp=fit_ref.FIT_DAMP,
                   max_shift=fit_ref.FIT_MAX_SHIFT, max_angle=fit_ref.FIT_MAX_ANGLE, states=None) -> MeshFitIters:
    """best fp32 [N,H,W], sil uint8 [N,H,W], depth fp32 [N,H,W] (or [N,1,H,W]), paras: 4 values or [N,4], mesh fp32 [N*K,V,3],
    xyz_mm fp32 [N*K,J,3], faces int [F,3], lifted [N*K] or None -> MeshFitIters.  states: a list that receives every
    iteration's fit_ref.MeshFit."""
    assert 1 <= iters <= MAX_ITERS
    sil = np.asarray(sil, np.uint8)
    n, h, w = sil.shape
    mesh, xyz_mm = np.asarray(mesh, F), np.asarray(xyz_mm, F)
    slots = mesh.shape[0]
    cur_mesh, cur_xyz, cur_best, cur_sil = mesh, xyz_mm, np.asarray(best, F), sil
    trace = np.empty((slots, iters, 3), np.int64)
    steps = [[] for _ in range(slots)]
    first = None
    for t in range(iters):
        if t:
            cur_best, cur_sil = geometry_frames(cur_mesh, faces, paras, k, h, w, lifted)
        got = fit_ref.mesh_fit(cur_best, cur_sil, depth, paras, cur_mesh, cur_xyz, k, band, stride, min_points, damp, max_shift,
                               max_angle)
        if states is not None:
            states.append(got)
        first = got if first is None else first
        trace[:, t, 0], trace[:, t, 1], trace[:, t, 2] = got.count[:, 0], got.count[:, 1], got.cost
        with np.errstate(all="ignore"):
            for s in range(slots):
                steps[s].append((int(got.count[s, 1]), got.rt[s], cur_xyz[s, 0] / fit_ref.KILO))
        cur_mesh, cur_xyz = got.mesh, got.xyz
    with np.errstate(all="ignore"):
        rt = np.stack([compose(xyz_mm[s, 0] / fit_ref.KILO, steps[s]) for s in range(slots)])
    return MeshFitIters(cur_mesh, cur_xyz, rt, first.count, first.cost, trace)
