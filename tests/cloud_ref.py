"""Each hand's depth pixels as a compact 3-D point cloud, in numpy float32 (csrc/hand_cloud.hip,
hn_hand_cloud_f32).  Every operation is one fp32 operation rounded on its own, in the order written here, and the matches of a
slot are taken in row-major order (np.nonzero's), so the device's outputs can be compared bit for bit.  This file is the
specification; nothing of the package is imported.

Per frame i: best [H,W] (the raster's out_depth: the nearest mesh Z, 0 where nothing was drawn), sil [H,W] (the silhouette
byte), D [H,W] (the scene depth, metres), the camera row (fx, fy, cx, cy) and optionally the extrinsics row [R | t].

  candidate   pixel (r, c) with r % stride == 0 and c % stride == 0
  match       a candidate matches slot k of its frame when (sil & 0x7F) == k + 1 with k < K (the hidden flag 0x80 is ignored; a
              byte naming a slot >= K matches nothing), D is valid (finite and > 0) and fabsf(e) <= band, e = D - best
  point       x = (((float)c + 0.5) - cx) * D / fx   (subtract, multiply, divide), y likewise with r, cy, fy, z = D: the camera
              frame of xyz_mm (x right, y down, z forward), metres, the pixel centre at +0.5 -- the raster's sample point
  rig mode    out[r] = ((R[r][0] * x + R[r][1] * y) + R[r][2] * z) + t[r] with the frame's row (tests/rig_ref.py transform)
  order       slot s = i * K + k receives its matches in row-major order (r ascending, then c); the first min(total, P) go to
              cloud[s][0..], the rows from there to P are zeros
  count       cloud_count[s] = (total matches, rows written), int32
  resid       cloud_resid[s] = sum over ALL matches of (int32)rint(e * 1e6), int64: micrometres
"""
import collections

import numpy as np

F = np.float32
CLOUD_POINTS = 4096        # rows per slot
CLOUD_BAND = 0.03          # metres; a starting value, not tuned on this model
CLOUD_STRIDE = 2           # every second row and column; a starting value, not tuned on this model
HALF, MICRO = F(0.5), F(1e6)

HandCloud = collections.namedtuple("HandCloud", "cloud count resid")
# cloud fp32 [N*K,P,3]; count int32 [N*K,2]; resid int64 [N*K]


def valid_depth(d):
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def residual(depth, best):
    """e = D - best, one fp32 subtraction"""
    with np.errstate(all="ignore"):
        return np.asarray(depth, F) - np.asarray(best, F)


def matches(best, sil, depth, k, band=CLOUD_BAND, stride=CLOUD_STRIDE):
    """best fp32 [H,W], sil uint8 [H,W], depth fp32 [H,W] of ONE frame -> int [H,W]: the slot a pixel matches, -1 for none"""
    best, sil, depth = np.asarray(best, F), np.asarray(sil, np.uint8), np.asarray(depth, F)
    h, w = sil.shape
    who = (sil & 0x7F).astype(np.int64)
    e = residual(depth, best)
    with np.errstate(invalid="ignore"):
        ok = (who >= 1) & (who <= k) & valid_depth(depth) & (np.abs(e) <= F(band))
    cand = np.zeros((h, w), bool)
    cand[::stride, ::stride] = True
    return np.where(ok & cand, who - 1, -1)


def point(r, c, d, paras):
    """the camera-frame points of the pixels (r, c) with depths d (scalars or arrays of one shape): fp32 [..., 3]"""
    fx, fy, cx, cy = (F(v) for v in paras)
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        x = ((np.asarray(c).astype(F) + HALF) - cx) * d / fx
        y = ((np.asarray(r).astype(F) + HALF) - cy) * d / fy
    return np.stack([x, y, d], axis=-1).astype(F)


def to_rig(row, p):
    """9i's transform of points fp32 [..., 3] (tests/rig_ref.py transform, the same operation order)"""
    m = np.asarray(row, F).reshape(3, 4)
    p = np.asarray(p, F)
    out = np.empty(p.shape, F)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[..., r] = ((m[r, 0] * p[..., 0] + m[r, 1] * p[..., 1]) + m[r, 2] * p[..., 2]) + m[r, 3]
    return out


def micrometres(e):
    """(int32)rint(e * 1e6) of fp32 residuals"""
    with np.errstate(all="ignore"):
        return np.rint(np.asarray(e, F) * MICRO).astype(np.int32)


def hand_cloud(best, sil, depth, paras, k, points=CLOUD_POINTS, band=CLOUD_BAND, stride=CLOUD_STRIDE, ext_table=None) -> HandCloud:
    """best fp32 [N,H,W], sil uint8 [N,H,W], depth fp32 [N,H,W] (or [N,1,H,W]), paras: 4 values or a row per frame [N,4],
    ext_table: fp32 [N,12] or None (the camera frame) -> HandCloud"""
    best, sil = np.asarray(best, F), np.asarray(sil, np.uint8)
    n, h, w = sil.shape
    depth = np.asarray(depth, F).reshape(n, h, w)
    cams = np.asarray(paras, np.float64).astype(F)
    cams = np.tile(cams, (n, 1)) if cams.ndim == 1 else cams
    assert cams.shape == (n, 4) and points >= 1 and stride >= 1 and 1 <= k <= 16
    cloud = np.zeros((n * k, points, 3), F)
    count = np.zeros((n * k, 2), np.int32)
    resid = np.zeros((n * k,), np.int64)
    for i in range(n):
        slot = matches(best[i], sil[i], depth[i], k, band, stride)
        um = micrometres(residual(depth[i], best[i]))
        for kk in range(k):
            s = i * k + kk
            rows, cols = np.nonzero(slot == kk)                       # (np.nonzero walks in row-major order: r, then c)
            total = len(rows)
            written = min(total, points)
            rows, cols = rows[:written], cols[:written]               # the first in that order are kept
            p = point(rows, cols, depth[i, rows, cols], cams[i])
            cloud[s, :written] = p if ext_table is None else to_rig(ext_table[i], p)
            count[s] = (total, written)
            resid[s] = sum(int(v) for v in um[slot == kk])            # (integers: any order)
    return HandCloud(cloud, count, resid)
