"""Each hand's mesh fitted to its measured depth: one Gauss-Newton step of projective point-to-plane alignment per hand slot, in
numpy (csrc/mesh_fit.hip, hn_mesh_fit_f32).  Every fp32 and fp64 operation is rounded on its own, in the
order written here, the sums are integers (their order does not matter), so the device's outputs can be compared bit for bit.
This file is the specification; nothing of the package is imported.

Per frame i: best [H,W] (the raster's out_depth: the nearest mesh Z, 0 where nothing was drawn), sil [H,W] (the silhouette
byte), D [H,W] (the scene depth, metres), the camera row (fx, fy, cx, cy).  Per slot s = i * K + k: mesh[s] [V,3] (the mesh the
raster drew: metres, the OpenGL convention (x, -y, -z) of the camera point) and xyz_mm[s] [J,3] (camera millimetres, x right,
y down, z forward).

  P(r, c, z)  ((((float)c + 0.5) - cx) * z / fx, (((float)r + 0.5) - cy) * z / fy, z): tests/cloud_ref.py's point
  candidate   pixel (r, c) with 1 <= r <= H - 2, 1 <= c <= W - 2, r % stride == 0 and c % stride == 0
  match       of slot k < K: who = sil & 0x7F == k + 1 at the pixel and at its four neighbours (r, c +- 1), (r +- 1, c), best > 0
              at all five, D valid (finite and > 0), fabsf(D - best) <= band, and the conditions of the next four lines
  normal      gx = P(r, c+1, best) - P(r, c-1, best), gy = P(r+1, c, best) - P(r-1, c, best) (best: at that neighbour);
              n = gx x gy, len = sqrtf((nx nx + ny ny) + nz nz) finite and > 0, n = n / len, fabsf(nz) >= FIT_MIN_COS
  lever       c0 = xyz_mm[s][0] / 1000f, p = P(r, c, best), d = p - c0 with every fabsf(d_j) <= FIT_REACH, m = d x n,
              J = (nx, ny, nz, mx, my, mz)
  residual    rho = (nx ex + ny ey) + nz ez with e = P(r, c, D) - p; fabsf(rho) <= 1
  sums        int64, every term (int64)rint(x * 2^30) of ONE fp32 product x: A[j][k] += J_j J_k (j <= k), b[j] += J_j rho,
              cost += rho rho, npts += 1
  solve       fp64: A / 2^30, b / 2^30, A[j][j] += damp * npts (j < 3) or (damp * npts) * FIT_ARM^2 (j >= 3), Cholesky L L^T in
              index order (a pivot fails when it is not > 0), forward and back substitution: x = (t, w)
  status      1: npts < min_points (no solve); 2: a pivot failed or x is not finite; 3: t.t > max_shift^2 or a.a > tan^2(max_angle
              / 2) with a = w / 2; 0: fitted
  rotation    Cayley: R = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), fp64, then R and t rounded to fp32
  apply       fp32, camera point x: x' = (((R_r0 d0 + R_r1 d1) + R_r2 d2) + c0_r) + t_r with d = x - c0; a mesh vertex goes
              through (x, -y, -z) in and out, a joint through / 1000f in and * 1000f out; status != 0: R = I, t = 0 and the
              mesh and the joints are byte copies
"""
import collections
import math

import numpy as np

F = np.float32
FIT_BAND = 0.03            # metres between the measured depth and the mesh Z; a starting value, not tuned on this model
FIT_STRIDE = 2             # every second row and column; a starting value, not tuned on this model
FIT_MIN_POINTS = 200       # fewer matches: no fit; a starting value, not tuned on this model
FIT_DAMP = 1e-3            # Levenberg damping per match; a starting value, not tuned on this model
FIT_MAX_SHIFT = 0.05       # metres: a larger step is refused; a starting value, not tuned on this model
FIT_MAX_ANGLE = 0.35       # radians: a larger step is refused; a starting value, not tuned on this model
FIT_MIN_COS = F(0.2)       # pixels seen at a steeper grazing angle carry no usable normal
FIT_REACH = F(1.0)         # a hand's surface lies within a metre of its wrist: this bounds the sums
FIT_ARM = 0.1              # metres: the lever arm that puts the rotation damping on the translation's scale
HALF, KILO, Q30 = F(0.5), F(1000.0), F(2.0 ** 30)
TERMS = 29                 # 21 of A (j <= k, row by row), 6 of b, the cost, the count
PAIRS = tuple((j, k) for j in range(6) for k in range(j, 6))

MeshFit = collections.namedtuple("MeshFit", "mesh xyz rt count cost")
# mesh fp32 [N*K,V,3]; xyz fp32 [N*K,J,3]; rt fp32 [N*K,12]; count int32 [N*K,2] (matches, status); cost int64 [N*K]


def caps(max_shift=FIT_MAX_SHIFT, max_angle=FIT_MAX_ANGLE):
    """the two caps as the doubles the kernel and the rule take: max_shift^2 and tan^2(max_angle / 2)"""
    half = math.tan(float(max_angle) / 2.0)
    return float(max_shift) * float(max_shift), half * half


def valid_depth(d):
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def point(r, c, z, paras):
    """P(r, c, z): three fp32 arrays (tests/cloud_ref.py's point, the same operation order)"""
    fx, fy, cx, cy = (F(v) for v in paras)
    z = np.asarray(z, F)
    with np.errstate(all="ignore"):
        x = ((np.asarray(c).astype(F) + HALF) - cx) * z / fx
        y = ((np.asarray(r).astype(F) + HALF) - cy) * z / fy
    return x, y, z


def cross(a, b):
    """a x b, each component two products and one subtraction"""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def q30(x):
    """(int64)rint(x * 2^30) of fp32 values"""
    return np.rint(np.asarray(x, F) * Q30).astype(np.int64)


def terms(best, sil, depth, paras, root_mm, kk, band=FIT_BAND, stride=FIT_STRIDE, count=None):
    """ONE frame, slot kk: best fp32 [H,W], sil uint8 [H,W], depth fp32 [H,W], root_mm = xyz_mm[s][0] -> (rows, cols, T) of
    the matches in row-major order, T int64 [matches, 29] their terms.  count: a dict that receives the candidates under the
    slot's byte that were rejected, by reason."""
    best, sil, depth = np.asarray(best, F), np.asarray(sil, np.uint8), np.asarray(depth, F)
    h, w = sil.shape
    if h < 3 or w < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, TERMS), np.int64)
    who = sil & 0x7F
    rr, cc = np.meshgrid(np.arange(1, h - 1), np.arange(1, w - 1), indexing="ij")
    at = lambda a, dr=0, dc=0: a[1 + dr:h - 1 + dr, 1 + dc:w - 1 + dc]  # noqa: E731
    with np.errstate(all="ignore"):
        cand = (rr % stride == 0) & (cc % stride == 0) & (at(who) == kk + 1)
        near = np.ones_like(cand)
        for dr, dc in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            near &= (at(who, dr, dc) == kk + 1) & (at(best, dr, dc) > 0)
        near &= at(best) > 0
        d_here, b_here = at(depth), at(best)
        e = d_here - b_here
        inside = valid_depth(d_here) & (np.abs(e) <= F(band))
        px = point(rr, cc + 1, at(best, 0, 1), paras), point(rr, cc - 1, at(best, 0, -1), paras)
        py = point(rr + 1, cc, at(best, 1, 0), paras), point(rr - 1, cc, at(best, -1, 0), paras)
        gx = tuple(a - b for a, b in zip(*px))
        gy = tuple(a - b for a, b in zip(*py))
        n = cross(gx, gy)
        length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        has_normal = np.isfinite(length) & (length > 0)
        n = tuple(v / length for v in n)
        facing = has_normal & (np.abs(n[2]) >= FIT_MIN_COS)
        c0 = np.asarray(root_mm, F) / KILO
        p = point(rr, cc, b_here, paras)
        d = tuple(p[j] - c0[j] for j in range(3))
        reach = (np.abs(d[0]) <= FIT_REACH) & (np.abs(d[1]) <= FIT_REACH) & (np.abs(d[2]) <= FIT_REACH)
        m = cross(d, n)
        q = point(rr, cc, d_here, paras)
        ev = tuple(q[j] - p[j] for j in range(3))
        rho = (n[0] * ev[0] + n[1] * ev[1]) + n[2] * ev[2]
        small = np.abs(rho) <= F(1.0)
        hit = cand & near & inside & facing & reach & small
        if count is not None:
            for name, mask in (("neighbour", cand & ~near), ("band", cand & near & ~inside), ("grazing", cand & near & inside & ~facing),
                               ("other", cand & near & inside & facing & ~(reach & small))):
                count[name] = count.get(name, 0) + int(mask.sum())
        rows, cols = np.nonzero(hit)
        jac = [v[rows, cols].astype(F) for v in n + m]
        rho = rho[rows, cols].astype(F)
        out = np.empty((len(rows), TERMS), np.int64)
        for a, (j, k) in enumerate(PAIRS):
            out[:, a] = q30(jac[j] * jac[k])
        for j in range(6):
            out[:, 21 + j] = q30(jac[j] * rho)
        out[:, 27] = q30(rho * rho)
        out[:, 28] = 1
    return rows + 1, cols + 1, out


def cholesky_solve(a, b):
    """a: 6 x 6 nested lists of Python floats (the upper triangle is read), b: 6 floats -> x (6 floats), or None when a pivot is
    not > 0.  Scalar fp64 operations, one by one, in index order."""
    low = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = a[j][j]
        for k in range(j):
            s = s - low[j][k] * low[j][k]
        if not s > 0.0:
            return None
        low[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = a[j][i]
            for k in range(j):
                s = s - low[i][k] * low[j][k]
            low[i][j] = s / low[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - low[i][k] * y[k]
        y[i] = s / low[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - low[k][i] * x[k]
        x[i] = s / low[i][i]
    return x


def cayley(a):
    """the rotation of the Cayley vector a (3 Python floats): nine fp64 values, row-major, from + - * / only"""
    a0, a1, a2 = a
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    u, den = 1.0 - aa, 1.0 + aa
    return [(u + (2.0 * a0) * a0) / den, ((2.0 * a0) * a1 - 2.0 * a2) / den, ((2.0 * a0) * a2 + 2.0 * a1) / den,
            ((2.0 * a1) * a0 + 2.0 * a2) / den, (u + (2.0 * a1) * a1) / den, ((2.0 * a1) * a2 - 2.0 * a0) / den,
            ((2.0 * a2) * a0 - 2.0 * a1) / den, ((2.0 * a2) * a1 + 2.0 * a0) / den, (u + (2.0 * a2) * a2) / den]


def solve(sums, min_points=FIT_MIN_POINTS, damp=FIT_DAMP, shift2=None, tan2=None):
    """sums: the 29 integers of a slot -> (status, rt): rt fp32 [12] = R row-major, then t"""
    if shift2 is None or tan2 is None:
        shift2, tan2 = caps()
    identity = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)
    npts = int(sums[28])
    if npts < min_points:
        return 1, identity
    a = [[0.0] * 6 for _ in range(6)]
    for t, (j, k) in enumerate(PAIRS):
        a[j][k] = a[k][j] = float(int(sums[t])) / 1073741824.0
    b = [float(int(sums[21 + j])) / 1073741824.0 for j in range(6)]
    lam = float(damp) * float(npts)
    for j in range(3):
        a[j][j] = a[j][j] + lam
    for j in range(3, 6):
        a[j][j] = a[j][j] + lam * (FIT_ARM * FIT_ARM)
    x = cholesky_solve(a, b)
    if x is None or not all(math.isfinite(v) for v in x):
        return 2, identity
    t = x[:3]
    half = [x[3] * 0.5, x[4] * 0.5, x[5] * 0.5]
    tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    aa = (half[0] * half[0] + half[1] * half[1]) + half[2] * half[2]
    if tt > shift2 or aa > tan2:
        return 3, identity
    with np.errstate(all="ignore"):
        return 0, np.array(cayley(half) + t, np.float64).astype(F)


def move(x, rt, c0):
    """fp32 camera points x [..., 3] moved by rt about c0"""
    x, out = np.asarray(x, F), np.empty(np.shape(x), F)
    with np.errstate(all="ignore"):
        d = [x[..., j] - c0[j] for j in range(3)]
        for r in range(3):
            out[..., r] = (((rt[3 * r] * d[0] + rt[3 * r + 1] * d[1]) + rt[3 * r + 2] * d[2]) + c0[r]) + rt[9 + r]
    return out


def apply(mesh, xyz_mm, status, rt):
    """one slot: mesh fp32 [V,3] (x, -y, -z), xyz_mm fp32 [J,3] -> the moved pair; status != 0: byte copies"""
    mesh, xyz_mm = np.asarray(mesh, F), np.asarray(xyz_mm, F)
    if status != 0:
        return mesh.copy(), xyz_mm.copy()
    flip = np.array([1, -1, -1], F)
    with np.errstate(all="ignore"):
        c0 = xyz_mm[0] / KILO
        return move(mesh * flip, rt, c0) * flip, move(xyz_mm / KILO, rt, c0) * KILO


def mesh_fit(best, sil, depth, paras, mesh, xyz_mm, k, band=FIT_BAND, stride=FIT_STRIDE, min_points=FIT_MIN_POINTS, damp=FIT_DAMP,
             max_shift=FIT_MAX_SHIFT, max_angle=FIT_MAX_ANGLE, census=None) -> MeshFit:
    """best fp32 [N,H,W], sil uint8 [N,H,W], depth fp32 [N,H,W] (or [N,1,H,W]), paras: 4 values or a row per frame [N,4],
    mesh fp32 [N*K,V,3], xyz_mm fp32 [N*K,J,3] -> MeshFit.  census: a dict that receives the rejected candidates by reason."""
    best, sil = np.asarray(best, F), np.asarray(sil, np.uint8)
    n, h, w = sil.shape
    depth = np.asarray(depth, F).reshape(n, h, w)
    cams = np.asarray(paras, np.float64).astype(F)
    cams = np.tile(cams, (n, 1)) if cams.ndim == 1 else cams
    mesh, xyz_mm = np.asarray(mesh, F), np.asarray(xyz_mm, F)
    assert cams.shape == (n, 4) and stride >= 1 and 1 <= k <= 16 and mesh.shape[0] == xyz_mm.shape[0] == n * k
    shift2, tan2 = caps(max_shift, max_angle)
    out = MeshFit(np.empty_like(mesh), np.empty_like(xyz_mm), np.empty((n * k, 12), F), np.empty((n * k, 2), np.int32),
                  np.empty((n * k,), np.int64))
    for i in range(n):
        for kk in range(k):
            s = i * k + kk
            _rows, _cols, t = terms(best[i], sil[i], depth[i], cams[i], xyz_mm[s, 0], kk, band, stride, census)
            sums = [int(v) for v in t.sum(axis=0)] if len(t) else [0] * TERMS       # (integers: any order)
            status, rt = solve(sums, min_points, damp, shift2, tan2)
            out.mesh[s], out.xyz[s] = apply(mesh[s], xyz_mm[s], status, rt)
            out.rt[s], out.count[s], out.cost[s] = rt, (sums[28], status), sums[27]
    return out
