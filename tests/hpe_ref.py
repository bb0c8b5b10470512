"""The hand-pose evaluator's tables, accumulated as integers: MPJPE, PCK and AUC for the absolute, the root-relative and the
Procrustes-aligned error, in numpy fp64 (csrc/hpe_metrics.hip, hn_hpe_accumulate_f32).  It restates what the
DexYCB toolkit's HPEEvaluator.evaluate feeds its three EvalUtil accumulators (dex_ycb_toolkit/hpe_eval.py:198-218,
freihand/utils/eval_util.py, freihand/eval.py:72-95 align_w_scale).  Every fp64 operation is rounded on its own, in the order
written here, reductions over the joints are sequential loops in joint order and the accumulated state is integer, so the device's
outputs can be compared bit for bit and any order of the samples, any split into batches, gives the same bytes.  This file is
the specification; nothing of the package is imported.

Inputs: pred, gt fp32 [S,J,3] in millimetres (widened exactly to fp64), valid int32 [S] or None, thresholds fp64 [T],
non-decreasing.

  fed         a sample is fed when valid != 0 (or valid is None) and each of its 2 J 3 values is finite and below 2^20 in
              magnitude; every other sample is SKIPPED: it is counted in n[1] and adds nothing else.  (The evaluator skips the
              samples whose annotation is all -1, hpe_eval.py:79; here the caller says so through `valid`.)
  dist(a, b)  sqrt((dx dx + dy dy) + dz dz) with d = a - b: what np.sqrt(np.sum(np.square(diff), axis=1)) computes for 3 columns
  ab          dist(gt_j, pred_j)
  rr          dist(gt_j - gt_0, pred_j - pred_0): d = (gt_j - gt_0) - (pred_j - pred_0), as the evaluator feeds it
  pa          dist(gt_j, aligned_j) with aligned = align_w_scale(gt, pred), A = gt, B = pred:
    means     t1 = (((0 + A_0) + A_1) + ...) / J per coordinate, t2 of B likewise
    centre    A'_j = A_j - t1, B'_j = B_j - t2
    norms     s1 = sqrt(sum) + 1e-8 with sum = (((0 + A'_00 A'_00) + A'_01 A'_01) + A'_02 A'_02) + A'_10 A'_10 ..., joint by
              joint, coordinate by coordinate; s2 of B' likewise; A'' = A' / s1, B'' = B' / s2 (one division per element)
    M         M[a][b] = ((0 + A''_0a B''_0b) + A''_1a B''_1b) + ...     (= A''^T B'', what scipy's orthogonal_procrustes factors)
    SVD       one-sided Jacobi (Hestenes), SWEEPS sweeps of the column pairs (0,1), (0,2), (1,2), whatever the data: G = M,
              V = I; for a pair (p, q): alpha = (G_0p G_0p + G_1p G_1p) + G_2p G_2p, beta likewise of q,
              gamma = (G_0p G_0q + G_1p G_1q) + G_2p G_2q; gamma == 0: nothing; else zeta = (beta - alpha) / (2 gamma),
              t = sgn / (|zeta| + sqrt(1 + zeta zeta)) with sgn = 1 for zeta >= 0 and -1 otherwise, c = 1 / sqrt(1 + t t),
              sn = c t, and for every row r of G and of V: (x_p, x_q) <- (c x_p - sn x_q, sn x_p + c x_q)
              sigma_i = sqrt((G_0i G_0i + G_1i G_1i) + G_2i G_2i), s = (sigma_0 + sigma_1) + sigma_2
    U         column i is LIVE when sigma_i > 0 and sigma_i > 2^-26 max(sigma); a live column is U_i = G_i / sigma_i, the others
              are completed (a rank-deficient M: all joints of a set equal, collinear or coplanar sets, J = 1):
                3 live  nothing to complete
                2 live  the third: U_i = U_(i+1) x U_(i+2), indices modulo 3
                1 live  x = U_i; m = the coordinate with the smallest |x_m| (the first of equals); w = e_m - x_m x,
                        U_(i+1) = w / sqrt((w_0 w_0 + w_1 w_1) + w_2 w_2), U_(i+2) = x x U_(i+1)
                0 live  U = I
              a x b = (a_1 b_2 - a_2 b_1, a_2 b_0 - a_0 b_2, a_0 b_1 - a_1 b_0)
    R         R[a][b] = (U_a0 V_b0 + U_a1 V_b1) + U_a2 V_b2: U V^T WITH reflections (scipy does not fix the determinant)
    aligned   aligned_ja = ((((B''_j0 R_a0 + B''_j1 R_a1) + B''_j2 R_a2) * s) * s1) + t1_a

State, all int64 (integer adds commute: the bytes do not depend on the order):
  hist [3,J,T+1]  a distance d adds one to bin #{t : thresholds[t] < d}; the last bin is "above every threshold"
  sum  [3,J]      += (int64)rint(d * 2^20), ties to even.  |v| < 2^20 bounds ab and rr by 2^23 and pa by 2^29 (|t1| < 2^20,
                  s <= 2, s1 < 2^24 for J <= 64), so a term is below 2^49 and the sum cannot overflow before 2^14 samples at
                  that bound -- or 2^33 samples (8.6e9) of errors below one metre (2^10 mm).  One quantum is 2^-20 mm, the
                  rounding error of a term at most 2^-21 mm.
  n    [2]        (fed, skipped)

compute(state, thresholds) mirrors EvalUtil.get_measures on the host.  The median is not offered: evaluate() computes it and
drops it (hpe_eval.py:213-217 bind it to `_`), and it cannot be had from a histogram and a sum.

SWEEPS = 10, from the convergence measured on the CPU over 20000 random 3 x 3 matrices U diag(sigma) V^T (well conditioned;
condition numbers up to 1e12; singular values equal to 1e-9 and to a few ulp; sigma^8 of a uniform sigma; scales 1e-3 .. 1): the
largest |gamma| / sqrt(alpha beta) of a column pair is 1.0 after 3 sweeps, 6.1e-10 after 4, 3.3e-16 after 5 and stays there
(2.7e-16 .. 3.4e-16 for 6 .. 12 sweeps); R changes by at most 6.7e-16 from one sweep to the next from the fourth on.  Five
sweeps converge every case, ten double that; tests/test_hpe_cpu.py::test_the_sweep_count_has_margin repeats the measurement on
a smaller set and asserts it.
"""
import math

import numpy as np

SWEEPS = 10
Q20 = 1048576.0
LIMIT = 1048576.0          # 2^20 mm: a coordinate at or beyond it makes the sample skipped
LIVE = 2.0 ** -26          # a column of G below this fraction of the largest is completed, not normalised
PAIRS = ((0, 1), (0, 2), (1, 2))
NAMES = ("absolute", "root-relative", "procrustes")


def new_state(joints, steps):
    return {"hist": np.zeros((3, joints, steps + 1), np.int64), "sum": np.zeros((3, joints), np.int64), "n": np.zeros((2,), np.int64)}


def merge(state, other):
    """the sum of two states (shards of one evaluation): an integer add"""
    return {k: state[k] + other[k] for k in ("hist", "sum", "n")}


def fed_mask(pred, gt, valid=None):
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    s = pred.shape[0]
    width = pred.shape[1] * 3
    both = np.concatenate([pred.reshape(s, width), gt.reshape(s, width)], axis=1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(both) < LIMIT, axis=1)                                                # (NaN and inf compare false)
    if valid is not None:
        ok = ok & (np.asarray(valid).reshape(s) != 0)
    return ok


def _dist(dx, dy, dz):
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def jacobi(m, sweeps=SWEEPS):
    """m: 3 x 3 nested lists of Python floats (IEEE doubles) -> (G, V) after `sweeps` sweeps"""
    g = [[float(m[r][c]) for c in range(3)] for r in range(3)]
    v = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            alpha = (g[0][p] * g[0][p] + g[1][p] * g[1][p]) + g[2][p] * g[2][p]
            beta = (g[0][q] * g[0][q] + g[1][q] * g[1][q]) + g[2][q] * g[2][q]
            gamma = (g[0][p] * g[0][q] + g[1][p] * g[1][q]) + g[2][p] * g[2][q]
            if gamma == 0.0:
                continue
            zeta = (beta - alpha) / (2.0 * gamma)
            sgn = 1.0 if zeta >= 0.0 else -1.0
            t = sgn / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            c = 1.0 / math.sqrt(1.0 + t * t)
            sn = c * t
            for x in (g, v):
                for r in range(3):
                    xp, xq = x[r][p], x[r][q]
                    x[r][p] = c * xp - sn * xq
                    x[r][q] = sn * xp + c * xq
    return g, v


def rotation(m, sweeps=SWEEPS):
    """m -> (R = U V^T with reflections, s = the sum of the singular values, sigma): the rule's SVD and completion"""
    g, v = jacobi(m, sweeps)
    sigma = [math.sqrt((g[0][i] * g[0][i] + g[1][i] * g[1][i]) + g[2][i] * g[2][i]) for i in range(3)]
    s = (sigma[0] + sigma[1]) + sigma[2]
    top = max(sigma)
    floor = LIVE * top
    live = [sigma[i] > 0.0 and sigma[i] > floor for i in range(3)]
    u = [[g[r][i] / sigma[i] for r in range(3)] if live[i] else [0.0, 0.0, 0.0] for i in range(3)]      # u[i] = COLUMN i
    count = sum(live)
    if count == 2:
        i = live.index(False)
        u[i] = cross(u[(i + 1) % 3], u[(i + 2) % 3])
    elif count == 1:
        i = live.index(True)
        x = u[i]
        mags = [abs(x[0]), abs(x[1]), abs(x[2])]
        k = 0
        if mags[1] < mags[k]:
            k = 1
        if mags[2] < mags[k]:
            k = 2
        w = [(1.0 if r == k else 0.0) - x[k] * x[r] for r in range(3)]
        length = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        y = [w[0] / length, w[1] / length, w[2] / length]
        u[(i + 1) % 3] = y
        u[(i + 2) % 3] = cross(x, y)
    elif count == 0:
        u = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    r = [[(u[0][a] * v[b][0] + u[1][a] * v[b][1]) + u[2][a] * v[b][2] for b in range(3)] for a in range(3)]
    return r, s, sigma


def procrustes_matrix(gt, pred):
    """one sample, fp64 [J,3] each -> (M, A'', B'', s1, t1) of the pa rule, Python floats"""
    a, b = [[float(x) for x in row] for row in gt], [[float(x) for x in row] for row in pred]
    j = len(a)
    t1, t2 = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for i in range(j):
        for c in range(3):
            t1[c] = t1[c] + a[i][c]
            t2[c] = t2[c] + b[i][c]
    t1, t2 = [x / float(j) for x in t1], [x / float(j) for x in t2]
    a = [[a[i][c] - t1[c] for c in range(3)] for i in range(j)]
    b = [[b[i][c] - t2[c] for c in range(3)] for i in range(j)]
    n1 = n2 = 0.0
    for i in range(j):
        for c in range(3):
            n1 = n1 + a[i][c] * a[i][c]
            n2 = n2 + b[i][c] * b[i][c]
    s1, s2 = math.sqrt(n1) + 1e-8, math.sqrt(n2) + 1e-8
    a = [[a[i][c] / s1 for c in range(3)] for i in range(j)]
    b = [[b[i][c] / s2 for c in range(3)] for i in range(j)]
    m = [[0.0] * 3 for _ in range(3)]
    for i in range(j):
        for p in range(3):
            for q in range(3):
                m[p][q] = m[p][q] + a[i][p] * b[i][q]
    return m, a, b, s1, t1


def align_w_scale(gt, pred, sweeps=SWEEPS):
    """one sample: gt, pred [J,3] -> aligned fp64 [J,3] (the rule's restatement of freihand/eval.py:72-95)"""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    m, _a, b, s1, t1 = procrustes_matrix(gt, pred)
    r, s, _sigma = rotation(m, sweeps)
    out = np.empty(gt.shape, np.float64)
    for i in range(gt.shape[0]):
        for a in range(3):
            out[i, a] = ((((b[i][0] * r[a][0] + b[i][1] * r[a][1]) + b[i][2] * r[a][2]) * s) * s1) + t1[a]
    return out


def distances(pred, gt, valid=None):
    """-> (fed bool [S], dist fp64 [S,3,J], aligned fp64 [S,J,3]); the rows of skipped samples are NaN"""
    pred32, gt32 = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    s, j = pred32.shape[0], pred32.shape[1]
    fed = fed_mask(pred32, gt32, valid)
    p, g = pred32.astype(np.float64), gt32.astype(np.float64)
    dist = np.full((s, 3, j), np.nan, np.float64)
    aligned = np.full((s, j, 3), np.nan, np.float64)
    for i in np.nonzero(fed)[0]:
        d = g[i] - p[i]
        dist[i, 0] = _dist(d[:, 0], d[:, 1], d[:, 2])
        d = (g[i] - g[i, 0]) - (p[i] - p[i, 0])
        dist[i, 1] = _dist(d[:, 0], d[:, 1], d[:, 2])
        aligned[i] = align_w_scale(g[i], p[i])
        d = g[i] - aligned[i]
        dist[i, 2] = _dist(d[:, 0], d[:, 1], d[:, 2])
    return fed, dist, aligned


def accumulate(pred, gt, thresholds, state=None, valid=None):
    """-> (state, dist, aligned): the state after feeding the batch (a new dict; `state` is not changed)"""
    thresholds = np.asarray(thresholds, np.float64).reshape(-1)
    pred32 = np.asarray(pred, np.float32)
    j, t = pred32.shape[1], thresholds.shape[0]
    old = new_state(j, t) if state is None else state
    out = {k: old[k].copy() for k in ("hist", "sum", "n")}
    fed, dist, aligned = distances(pred32, gt, valid)
    for i in np.nonzero(fed)[0]:
        d = dist[i]                                                                   # [3,J]
        bins = (thresholds[None, None, :] < d[:, :, None]).sum(axis=2)                # on the unquantised distance
        for a in range(3):
            out["hist"][a, np.arange(j), bins[a]] += 1
        out["sum"] += np.rint(d * Q20).astype(np.int64)
    out["n"][0] += int(fed.sum())
    out["n"][1] += int((~fed).sum())
    return out, dist, aligned


def trapz(y, x):
    """np.trapz(y, x) along the last axis, written out (the name left numpy 2's namespace for trapezoid)"""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return (np.diff(x) * (y[..., 1:] + y[..., :-1]) / 2.0).sum(axis=-1)


def compute(state, thresholds):
    """EvalUtil.get_measures for the three tables -> the evaluator's `results` dict (absolute / root-relative / procrustes ->
    mpjpe, auc) plus pck [3,T] (the mean over the joints), thresholds, fed and skipped.  fed == 0: NaN, no exception."""
    thresholds = np.asarray(thresholds, np.float64).reshape(-1)
    hist, total, n = (np.asarray(state[k], np.int64) for k in ("hist", "sum", "n"))
    fed, skipped = int(n[0]), int(n[1])
    with np.errstate(all="ignore"):
        pck = np.cumsum(hist, axis=2)[:, :, :-1].astype(np.float64) / np.float64(fed)          # [3,J,T]
        mean = (total.astype(np.float64) / Q20) / np.float64(fed)                              # [3,J]
        auc = trapz(pck, thresholds) / trapz(np.ones_like(thresholds), thresholds)             # [3,J]
        out = {name: {"mpjpe": float(np.mean(mean[a])), "auc": float(np.mean(auc[a]))} for a, name in enumerate(NAMES)}
        out["pck"] = np.mean(pck, axis=1)
    out["thresholds"] = thresholds
    out["fed"], out["skipped"] = fed, skipped
    return out
