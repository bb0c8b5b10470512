"""The detector's candidate selection (fcos_utils/fcos.py:591-628, det_utils.py:266-294, anchor_utils.py:82-132; csrc/fcos_post.hip
fcos_candidates_kernel, fcos_candidates_count_kernel + fcos_candidates_scatter_kernel) and the ext gather (fcos.py:299-320,
605-607, 631-647; fcos_ext_gather_kernel) as rules in float64, an fp32 emulation of each in the kernels' order, and those
emulations with one deliberate mistake each.  numpy only; nothing here reads the library.

Layout (what ops.fcos_candidates takes): per level l, cls_lr[l] [n, h, w, C + 2] (C class logits, then the two hand-side logits)
and reg_ctr[l] [n, h, w, 5] (four regressions, then the centre-ness logit).  The points of an image are numbered level by level,
row-major inside a level: the anchor order.  A result is a list with one dict per image: count (rows kept), total (points that
pass), and point / score / label / side / level / box of the kept rows, in anchor order, truncated to cap.
"""
import numpy as np

U = 2.0 ** -24
F = np.float32
D = np.float64
TINY = 2.0 ** -149
SCORE_TOL = 2e-7            # absolute; the project's figure for expf / sqrtf against torch (tests/test_fcos_gpu.py)
MUTANTS = ("last_tie", "no_sqrt", "gy_by_h", "half_unrounded", "level_off_by_one", "side_ge", "keep_last")
EXT_MUTANTS = ("no_clamp", "last_max", "keep_point_swapped")
FIELDS = ("point", "level", "label", "side", "box", "score")


# --------------------------------------------------------------------------------------------------------------------------
# candidates
# --------------------------------------------------------------------------------------------------------------------------
def starts_of(sizes):
    return np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).astype(np.int64)


def flatten(cls_lr, reg_ctr):
    """per-level NHWC tensors -> cls [n, P, C + 2], reg [n, P, 5] in anchor order, and the level sizes"""
    n = cls_lr[0].shape[0]
    sizes = [t.shape[1:3] for t in cls_lr]
    cls = np.concatenate([t.reshape(n, -1, t.shape[3]) for t in cls_lr], 1)
    reg = np.concatenate([t.reshape(n, -1, 5) for t in reg_ctr], 1)
    assert cls.dtype == F and reg.dtype == F
    return cls, reg, sizes


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def scores64(cls, reg, num_classes):
    """[n, P, C] float64: sqrt(sigmoid(cls_c) * sigmoid(ctr)) on the fp32 logits"""
    return np.sqrt(_sigmoid(cls[..., :num_classes].astype(D)) * _sigmoid(reg[..., 4:5].astype(D)))


def grid(sizes, strides, mutant=None):
    """per point of the anchor order: level, gx, gy, stride (int64 arrays of length P)"""
    lvl, gx, gy, st = [], [], [], []
    for l, ((h, w), s) in enumerate(zip(sizes, strides)):
        q = np.arange(h * w)
        y = q // (h if mutant == "gy_by_h" else w)
        lvl.append(np.full(h * w, l)); gy.append(y); gx.append(q - y * w); st.append(np.full(h * w, s))
    lvl, gx, gy, st = (np.concatenate(t).astype(np.int64) for t in (lvl, gx, gy, st))
    if mutant == "level_off_by_one":          # `i > start[l + 1]`: the first point of a level is given to the level before
        first = starts_of(sizes)[1:-1]
        lvl[first] -= 1
    return lvl, gx, gy, st


def boxes32(reg, sizes, strides, mutant=None):
    """[n, P, 4] fp32, the kernel's decode: base anchor [-s/2, -s/2, s/2, s/2].round() (half to even: 2.5 -> 2, 3.5 -> 4) shifted
    to (gx, gy) * stride, centre and size through the fp32 anchor corners, then centre -/+ reg * size with a separate multiply and
    add (no fma)."""
    _, gx, gy, st = grid(sizes, strides, mutant)
    stf = st.astype(F)
    half = (stf * F(0.5)).astype(F)
    if mutant != "half_unrounded":
        half = np.rint(half).astype(F)
    px, py = (gx * st).astype(F), (gy * st).astype(F)
    ax0, ay0, ax1, ay1 = px - half, py - half, px + half, py + half
    cx, cy = (F(0.5) * (ax0 + ax1)).astype(F), (F(0.5) * (ay0 + ay1)).astype(F)
    bw, bh = (ax1 - ax0).astype(F), (ay1 - ay0).astype(F)
    out = np.stack([cx - (reg[..., 0] * bw).astype(F), cy - (reg[..., 1] * bh).astype(F),
                    cx + (reg[..., 2] * bw).astype(F), cy + (reg[..., 3] * bh).astype(F)], -1)
    assert out.dtype == F
    return out


def _compact(score, label, side, lvl, box, passing, cap, keep_last=False):
    out = []
    for i in range(score.shape[0]):
        idx = np.nonzero(passing[i])[0]
        total = len(idx)
        idx = idx[-cap:] if keep_last else idx[:cap]
        out.append(dict(count=len(idx), total=total, point=idx.astype(np.int64), score=score[i, idx], label=label[i, idx],
                        side=side[i, idx], level=lvl[idx], box=box[i, idx]))
    return out


def rule64(cls_lr, reg_ctr, strides, num_classes, thresh, cap=None):
    """score = sqrt(sigmoid(cls_c) * sigmoid(ctr)) in float64, max over the classes with the FIRST index winning exact ties
    (torch.max); a point passes iff score > thresh (the fp32 threshold the kernel is handed); side = 1 iff lr[1] > lr[0] (sigmoid
    is monotonic; the first index wins a tie, torch.max again); boxes by boxes32 (compared bit for bit); anchor order, the first
    `cap` kept.  Membership, labels and sides are exact claims: the case generator keeps every decision away from float64's
    and fp32's disagreement (guards())."""
    cls, reg, sizes = flatten(cls_lr, reg_ctr)
    cap = cls.shape[1] if cap is None else cap
    sc = scores64(cls, reg, num_classes)
    label = sc.argmax(-1)                                     # first maximum
    best = np.take_along_axis(sc, label[..., None], -1)[..., 0]
    side = (cls[..., num_classes + 1] > cls[..., num_classes]).astype(np.int64)
    lvl = grid(sizes, strides)[0]
    return _compact(best, label, side, lvl, boxes32(reg, sizes, strides), best > float(F(thresh)), cap)


def emulate(cls_lr, reg_ctr, strides, num_classes, thresh, cap=None, mutant=None):
    """eval_point in numpy fp32 in the kernel's order: sctr = 1 / (1 + exp(-ctr)); per class sqrt(sigmoid * sctr) with `>` against
    the running best (from -1); pass iff best > thresh; side = sigmoid(lr1) > sigmoid(lr0); the decode of boxes32.  numpy's fp32
    exp is not the device's expf: scores agree with either to SCORE_TOL, not bit for bit."""
    assert mutant is None or mutant in MUTANTS
    cls, reg, sizes = flatten(cls_lr, reg_ctr)
    cap = cls.shape[1] if cap is None else cap
    one = F(1.0)
    with np.errstate(over="ignore"):
        sig = lambda x: (one / (one + np.exp(-x).astype(F))).astype(F)
        sctr = sig(reg[..., 4])
        best = np.full(cls.shape[:2], F(-1.0))
        label = np.zeros(cls.shape[:2], np.int64)
        for c in range(num_classes):
            p = (sig(cls[..., c]) * sctr).astype(F)
            sc = p if mutant == "no_sqrt" else np.sqrt(p).astype(F)
            win = sc >= best if mutant == "last_tie" else sc > best
            best, label = np.where(win, sc, best), np.where(win, c, label)
        s0, s1 = sig(cls[..., num_classes]), sig(cls[..., num_classes + 1])
    side = (s1 >= s0 if mutant == "side_ge" else s1 > s0).astype(np.int64)
    lvl = grid(sizes, strides, mutant)[0]
    assert best.dtype == F
    return _compact(best, label, side, lvl, boxes32(reg, sizes, strides, mutant), best > F(thresh), cap, keep_last=mutant == "keep_last")


def mutants():
    return {m: (lambda *a, _m=m, **k: emulate(*a, mutant=_m, **k)) for m in MUTANTS}


def guards(cls_lr, reg_ctr, num_classes, thresh):
    """[n, P] bool: the points whose decisions float64 and fp32 could take differently -- a float64 score within 1e-5 of the
    threshold; the logits of the top two classes neither equal bit for bit nor 1e-3 apart; the two side logits likewise.  The case
    generator resamples these until none is left; the tests assert that none is."""
    cls, reg, _ = flatten(cls_lr, reg_ctr)
    bad = np.abs(scores64(cls, reg, num_classes).max(-1) - float(F(thresh))) < 1e-5
    if num_classes > 1:
        top = np.sort(cls[..., :num_classes].astype(D), -1)[..., -2:]
        gap = top[..., 1] - top[..., 0]
        bad |= (gap != 0) & (gap < 1e-3)
    gap = np.abs(cls[..., num_classes + 1].astype(D) - cls[..., num_classes].astype(D))
    bad |= (gap != 0) & (gap < 1e-3)
    return bad


def check(out, want):
    """THE comparison (CPU and GPU tests), one property after the other per image: count; then point (membership and order),
    level, label, side and box bit for bit; then |score - rule| <= SCORE_TOL.  Returns the largest score deviation."""
    assert len(out) == len(want)
    worst = 0.0
    for i, (o, w) in enumerate(zip(out, want)):
        assert int(o["count"]) == w["count"], f"image {i}: count {int(o['count'])} != {w['count']} (of {w['total']} passing)"
        for f in FIELDS[:-1]:
            a, b = np.asarray(o[f]), np.asarray(w[f])
            assert a.shape == b.shape, (f, a.shape, b.shape)
            if f == "box":
                assert a.dtype == F
                same = a.view(np.int32) == b.view(np.int32)
            else:
                same = a.astype(np.int64) == b.astype(np.int64)
            assert same.all(), f"image {i}: {f} differs at row {np.argwhere(~same)[0].tolist()} of {w['count']}"
        s = np.asarray(o["score"])
        assert s.dtype == F and s.shape == w["score"].shape
        if s.size:
            dev = float(np.abs(s.astype(D) - w["score"].astype(D)).max())
            assert dev <= SCORE_TOL, f"image {i}: score deviates by {dev:.3e}"
            worst = max(worst, dev)
    return worst


# --------------------------------------------------------------------------------------------------------------------------
# ext gather
# --------------------------------------------------------------------------------------------------------------------------
EPS32 = float(F(1e-12))      # F.normalize's eps as the fp32 number both the reference and the kernel clamp with
TENTH = float(F(0.1))        # the fp32 constant 0.1f


def _ext_rows(ext, point, keep, count, swapped=False):
    """the gather: detection d of image i reads point[i, keep[i, d]] -> (image, row, e [8]) for d < count[i]"""
    n, cap = keep.shape
    flat = np.concatenate([t.reshape(n, -1, 8) for t in ext], 1)
    assert flat.shape[1] == cap and flat.dtype == F
    rows = [(i, d, flat[i, keep[i, point[i, d]] if swapped else point[i, keep[i, d]]]) for i in range(n) for d in range(int(count[i]))]
    return n, cap, rows


def ext_rule64(ext, point, keep, count):
    """(contacts [n, cap] int64, dxdymags [n, cap, 3] float64, bound [n, cap, 3]); rows at and beyond count[i] are zero.

    mag = e[0].  (dx, dy) * 0.1f / max(||(dx, dy)||, 1e-12f) in float64 with the fp32 constants.  contact = the first arg-max of
    the five contact logits (sigmoid is monotonic).

    Tiny magnitudes: the reference is 0.1 * F.normalize(d, p=2, dim=1) = d / max(||d||, eps) in fp32 (fcos.py:301-303).  Below
    |d| ~ 1e-19 the squares underflow in fp32 and the fp32 norm is 0 or garbage, but any norm below 1e-12 is replaced by the clamp,
    so the contract there is simply 0.1 * d / 1e-12 -- which float64 gives too; at (0, 0) it is 0, not NaN.

    bound, relative to |result|, u = 2^-24, first order: fl(dx dx), fl(dy dy) and their sum put 2u on the (positive) sum of
    squares, the square root halves that to u and rounds once (u), the division rounds once (u), the product with 0.1f once
    (u): 4u, and a fifth u for every second-order term.  bound = 5 u |result| + 2^-149.  An underflow of a square only matters
    where the norm is not clamped, i.e. >= 1e-12, and is then below 2^-149 / 1e-24 = 1.4e-21 of the sum: nothing against u."""
    n, cap, rows = _ext_rows(ext, point, keep, count)
    contacts = np.zeros((n, cap), np.int64)
    mags = np.zeros((n, cap, 3), D)
    for i, d, e in rows:
        e = e.astype(D)
        den = max(float(np.sqrt(e[1] * e[1] + e[2] * e[2])), EPS32)
        mags[i, d] = (e[0], e[1] * TENTH / den, e[2] * TENTH / den)
        contacts[i, d] = int(np.argmax(e[3:8]))
    bound = 5.0 * U * np.abs(mags) + TINY
    bound[..., 0] = TINY
    return contacts, mags, bound


def ext_emulate(ext, point, keep, count, mutant=None):
    """the kernel's chain in fp32: denom = fmaxf(sqrtf(dx * dx + dy * dy), 1e-12f); 0.1f * (d / denom); the running best of the
    five sigmoids with `>`"""
    assert mutant is None or mutant in EXT_MUTANTS
    n, cap, rows = _ext_rows(ext, point, keep, count, swapped=mutant == "keep_point_swapped")
    contacts = np.zeros((n, cap), np.int32)
    mags = np.zeros((n, cap, 3), F)
    one = F(1.0)
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        for i, d, e in rows:
            den = np.sqrt(F(F(e[1] * e[1]) + F(e[2] * e[2])))
            if mutant != "no_clamp":
                den = max(den, F(1e-12))
            mags[i, d] = (e[0], F(0.1) * F(e[1] / den), F(0.1) * F(e[2] / den))
            sg = (one / (one + np.exp(-e[3:8]).astype(F))).astype(F)
            best = 0
            for c in range(1, 5):
                if (sg[c] >= sg[best]) if mutant == "last_max" else (sg[c] > sg[best]):
                    best = c
            contacts[i, d] = best
    return contacts, mags


def ext_mutants():
    return {m: (lambda *a, _m=m: ext_emulate(*a, mutant=_m)) for m in EXT_MUTANTS}


def ext_check(contacts, mags, count, ref):
    """THE comparison for the ext gather: rows at and beyond count[i] zero; mag bit for bit (the gather itself); contacts equal;
    |dxdy - rule| <= bound (a NaN is outside any bound).  Returns max |err| / bound."""
    wc, wm, b = ref
    contacts, mags = np.asarray(contacts), np.asarray(mags)
    assert contacts.shape == wc.shape and mags.shape == wm.shape and mags.dtype == F, (contacts.shape, mags.shape, mags.dtype)
    for i, k in enumerate(count):
        assert not contacts[i, int(k):].any() and not mags[i, int(k):].view(np.int32).any(), f"image {i}: rows beyond count are not zero"
    assert np.array_equal(mags[..., 0].astype(D), wm[..., 0]), "mag differs"
    assert np.array_equal(contacts.astype(np.int64), wc), f"contact differs at {np.argwhere(contacts != wc)[0].tolist()}"
    ratio = np.abs(mags.astype(D) - wm) / b
    ratio[np.isnan(ratio)] = np.inf
    worst = float(ratio.max())
    assert worst <= 1.0, f"|err| / bound = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst
