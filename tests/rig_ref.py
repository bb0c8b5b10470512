"""The rig frame of a multi-camera live step in numpy float32 (csrc/rig_ops.hip, hn_rig_fuse_f32): the
per-slot transform into the caller's rig frame, the greedy association of slots across cameras and the score-weighted fusion.
Every operation is one fp32 operation rounded on its own, in the order written here (explicit loops where the order of a sum
matters), so the device's outputs can be compared bit for bit.  This file is the specification; nothing of the package is
imported."""
import collections

import numpy as np

F = np.float32
RIG_RADIUS = 0.08          # metres; a starting value, not tuned on this model
MAX_SLOTS = 256

RigFused = collections.namedtuple("RigFused", "rig_xyz rig_mesh rig_hand rig_count rig_views rig_seed fused_xyz fused_mesh")


def table(extrinsics):
    """[N,3,4] or [N,4,4] camera -> rig rows as the device keeps them: fp32 [N,12] = the rows of [R | t], rounded once"""
    e = np.asarray(extrinsics, np.float64)
    return np.ascontiguousarray(e[:, :3, :].astype(F).reshape(e.shape[0], 12))


def transform(row, c):
    """row: fp32 [12] = [R | t] row-major; c: fp32 [..., 3] camera-frame points (metres) -> fp32 [..., 3] in the rig frame:
    out[r] = ((R[r][0] * c.x + R[r][1] * c.y) + R[r][2] * c.z) + t[r], four roundings after the three products"""
    m = np.asarray(row, F).reshape(3, 4)
    c = np.asarray(c, F)
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    out = np.empty(c.shape, F)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[..., r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


def centres(rig_xyz):
    """[S,J,3] -> [S,3]: the joints summed one after the other, then one divide by J"""
    s, j, _ = rig_xyz.shape
    acc = rig_xyz[:, 0].copy()
    with np.errstate(all="ignore"):
        for i in range(1, j):
            acc = acc + rig_xyz[:, i]
        return acc / F(j)


def associate(centre, lifted, k, radius=RIG_RADIUS, side=None):
    """centre fp32 [S,3], lifted [S] (== 1 takes part), k slots per camera, side [S] or None (None: no side gate) ->
    (group int32 [S], count, views int32 [S], seed int32 [S]); greedy, frame-major, distances to the SEED's centre"""
    s = centre.shape[0]
    n = s // k
    r2 = F(radius) * F(radius)
    group = np.full((s,), -1, np.int32)
    views, seed = np.zeros((s,), np.int32), np.full((s,), -1, np.int32)
    count = 0
    with np.errstate(all="ignore"):
        for a in range(s):
            if lifted[a] != 1 or group[a] != -1:
                continue
            g = count
            count += 1
            group[a], seed[g], views[g] = g, a, 1
            for i in range(a // k + 1, n):
                best, best_d2 = -1, None
                for kk in range(k):
                    t = i * k + kk
                    if lifted[t] != 1 or group[t] != -1 or (side is not None and side[t] != side[a]):
                        continue
                    d = centre[t] - centre[a]
                    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    if d2 <= r2 and (best < 0 or d2 < best_d2):           # (NaN fails both; a tie keeps the lower k)
                        best, best_d2 = t, d2
                if best >= 0:
                    group[best] = g
                    views[g] += 1
    return group, count, views, seed


def fuse_points(points, group, count, score):
    """points fp32 [S,P,3] in the rig frame, group [S], score fp32 [S] -> fp32 [S,P,3]: row g = the rig hand's members, one
    member copied, several averaged with their scores: (sum w * x) / (sum w), both sums in member (slot) order"""
    out = np.zeros(points.shape, F)
    with np.errstate(all="ignore"):
        for g in range(count):
            members = [m for m in range(points.shape[0]) if group[m] == g]
            if len(members) == 1:
                out[g] = points[members[0]]
                continue
            w = F(score[members[0]])
            acc, wsum = w * points[members[0]], w
            for m in members[1:]:
                w = F(score[m])
                acc = acc + w * points[m]
                wsum = wsum + w
            out[g] = acc / wsum
    return out


def rig_fuse(xyz_mm, mesh, has_hand, lifted, score, ext_table, k, radius=RIG_RADIUS, side=None) -> RigFused:
    """xyz_mm fp32 [S,J,3] (camera frame, millimetres), mesh fp32 [S,V,3] (the final mesh: metres, (x, -y, -z) of the camera
    frame), has_hand / lifted int [S], score fp32 [S], ext_table fp32 [N,12], S = N * k, side int [S] or None -> the eight
    outputs of hn_rig_fuse_f32, shaped per slot ([N,k,...]) and per rig hand ([S,...])."""
    xyz_mm, mesh = np.asarray(xyz_mm, F), np.asarray(mesh, F)
    s, j, _ = xyz_mm.shape
    v = mesh.shape[1]
    n = s // k
    assert n * k == s and ext_table.shape == (n, 12) and s <= MAX_SLOTS
    has_hand, lifted = np.asarray(has_hand).reshape(s), np.asarray(lifted).reshape(s).astype(np.int32)
    score = np.asarray(score, F).reshape(s)
    rig_xyz, rig_mesh = np.zeros((s, j, 3), F), np.zeros((s, v, 3), F)
    flip = np.array([1, -1, -1], F)
    with np.errstate(all="ignore"):
        for a in range(s):
            if has_hand[a] == 1:
                rig_xyz[a] = transform(ext_table[a // k], xyz_mm[a] / F(1000))
            if lifted[a] == 1:
                rig_mesh[a] = transform(ext_table[a // k], mesh[a] * flip)          # (x, -y, -z): exact
    group, count, views, seed = associate(centres(rig_xyz), lifted, k, radius, None if side is None else np.asarray(side).reshape(s))
    return RigFused(rig_xyz.reshape(n, k, j, 3), rig_mesh.reshape(n, k, v, 3), group.reshape(n, k), int(count), views, seed,
                    fuse_points(rig_xyz, group, count, score), fuse_points(rig_mesh, group, count, score))
