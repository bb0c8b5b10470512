"""Shapes, seeded heads and handmade target sets for the FCOS criterion's tests (tests/fcos_loss_ref.py).  The first two cases
are the golden's two configurations (tests/golden/make_golden_fcos_loss.py imports them from here); each case's rule and bound
are computed once (reference()) and shared by the tests, read-only.

Head values: class, side, centre-ness and contact logits N(0, 2^2); regressions |N(0, 1)| * 1.5 (a ReLU's outputs); the ext
(mag, dx, dy) relu(N(0, 2^2)), so a quarter of the points have dx = dy = 0 and meet the normalisation's clamp."""
import functools
from dataclasses import dataclass

import numpy as np

import fcos_loss_ref as fr

F = np.float32
WORKLOAD = ((40, 34), (20, 17), (10, 9))        # a 320 x 288 canvas at strides 8 / 16 / 32: 1790 points, two 1024-point chunks
SMALL = ((5, 7), (3, 4), (2, 2))
OBJ = (-1.0, -1.0, 0.0, 0.0, 0.0)               # an object box's box_info: no contact state, no side, no offset


def _t(rows):
    """rows of (x0, y0, x1, y1, label, (contactstate, handside, mag, dx, dy)) -> (boxes [M, 4], labels [M], info [M, 5])"""
    if not rows:
        return np.zeros((0, 4), F), np.zeros((0,), np.int32), np.zeros((0, 5), F)
    return (np.array([r[:4] for r in rows], F), np.array([r[4] for r in rows], np.int32), np.array([r[5] for r in rows], F))


# The golden's first configuration.  Image 0, in canvas pixels (level 0 points lie on multiples of 8, range 0 < d < 64;
# level 1 on multiples of 16, 64 < d < 128):
#   rows 0, 1  nested, both match the level-0 points around (120, 120): the line-563 "areas" are -1000 and 96, the box areas 8000
#              and 768 -- the LARGER box has the larger key and wins; the true box area would pick the other
#   rows 2, 3  line-563 areas -5120 and -5118: both keys round to 100005120 in float32, the first index wins
#   row 4      its left edge x0 = 56 lies on the anchor centres (56, 208..224): x - x0 = 0 is not inside
#   row 5      the level-1 points (144|160, 240|256) are at distance exactly 64 = 4 * 16 (not above the lower bound) and the
#              level-0 point (144, 248) at exactly 64 = 8 * 8 (not below the upper bound); (152, 248) matches on level 0
G1_TARGETS = (
    _t([(80, 70, 160, 170, 1, (3.0, 1.0, 0.5, 0.06, -0.08)), (104, 108, 136, 132, 0, OBJ),
        (200, 40, 232, 72, 2, (1.0, 0.0, 0.25, -0.1, 0.0)), (200, 40.0625, 232, 72.0625, 0, OBJ),
        (56, 200, 72, 232, 1, (0.0, 1.0, 0.0, 0.0, 0.0)), (96, 200, 208, 296, 1, (4.0, 0.0, 0.75, 0.028, 0.096))]),
    _t([(40, 60, 250, 300, 1, (2.0, 1.0, 0.3, 0.1, 0.0))]),
    _t([(16, 16, 60, 70, 0, OBJ), (150, 100, 260, 180, 2, (1.0, 0.0, 0.6, -0.06, 0.08))]),
)
# The second: two overlapping boxes on level 0 (the second wins the shared points: line-563 areas 19 and -200), and an image
# without boxes
G2_TARGETS = (_t([(2, 3, 30, 22, 0, OBJ), (10, 5, 60, 45, 1, (0.0, 1.0, 0.0, 0.0, 0.0))]), _t([]))


@dataclass(frozen=True)
class Case:
    name: str
    sizes: tuple
    strides: tuple
    n: int
    num_classes: int
    ext: bool
    seed: int
    why: str
    targets: tuple = ()       # per image (boxes, labels, info); () = seeded (counts)
    counts: tuple = ()
    special: str = ""


CASES = (
    Case("golden-1", WORKLOAD, (8, 16, 32), 3, 3, True, 20261101, "the golden's first configuration", G1_TARGETS),
    Case("golden-2", SMALL, (8, 16, 32), 2, 2, False, 20261102, "the golden's second: ext off, an image without boxes", G2_TARGETS),
    Case("1pt", ((1, 1),), (8,), 1, 3, True, 20261103, "a one-level table: lower = 0 and upper = inf; one point, one box",
         (_t([(-3, -2, 5, 4, 1, (2.0, 0.0, 0.4, 0.08, 0.06))]),)),
    Case("edge", ((2, 3), (1, 2), (1, 1)), (8, 16, 32), 2, 3, True, 20261104,
         "foreground on every level of a 9-point table; image 1's box holds no point",
         (_t([(1, -3, 15, 7, 0, OBJ), (-100, -120, 140, 110, 1, (1.0, 1.0, 0.2, 0.0, 0.1))]),
          _t([(3, 3, 5, 5, 2, (0.0, 0.0, 0.1, 0.1, 0.0))]))),
    Case("chunks", WORKLOAD, (8, 16, 32), 3, 3, False, 20261105, "two chunks, a level boundary inside one; 64, 1 and 0 boxes",
         counts=(64, 1, 0)),
    Case("chunks-ext", WORKLOAD, (8, 16, 32), 3, 3, True, 20261106, "the same with ext; 64, 1 and 2 boxes", counts=(64, 1, 2)),
    Case("nofg", SMALL, (8, 16, 32), 2, 2, True, 20261107, "boxes that hold no point: the divisor is 1, GIoU and BCE sums exactly 0",
         (_t([(1, 1, 7, 7, 0, OBJ), (9, 17, 15, 23, 1, (1.0, 0.0, 0.5, 0.1, 0.0))]), _t([(33, 9, 39, 15, 1, (0.0, 1.0, 0.0, 0.0, 0.0))]))),
    Case("sat", SMALL, (8, 16, 32), 2, 2, True, 20261108, "logits of +-80 in every head", (G2_TARGETS[0], G2_TARGETS[0]),
         special="sat"),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)
GOLDEN = {"g1": "golden-1", "g2": "golden-2"}


def points(c):
    return sum(h * w for h, w in c.sizes)


def heads_flat(seed, n, p, num_classes, ext):
    """(cls [n, P, C + 2], reg [n, P, 5], ex [n, P, 8] or None) fp32 from the seed"""
    rng = np.random.default_rng(int(seed))
    cls = (rng.standard_normal((n, p, num_classes + 2)) * 2.0).astype(F)
    reg = rng.standard_normal((n, p, 5))
    reg[..., :4] = np.abs(reg[..., :4]) * 1.5
    reg[..., 4] *= 2.0
    ex = rng.standard_normal((n, p, 8)) * 2.0
    ex[..., :3] = np.maximum(ex[..., :3], 0.0)
    return cls, reg.astype(F), ex.astype(F) if ext else None


def _seeded_targets(rng, count):
    """`count` boxes on the 320 x 288 canvas, sides 10..150, a third of them object boxes"""
    cx, cy = rng.uniform(0, 288, count), rng.uniform(0, 320, count)
    w, h = rng.uniform(10, 150, count), rng.uniform(10, 150, count)
    rows = []
    for k in range(count):
        hand = k % 3 != 0
        info = (float(rng.integers(0, 5)), float(rng.integers(0, 2)), float(rng.uniform(0, 1)), float(rng.uniform(-0.1, 0.1)),
                float(rng.uniform(-0.1, 0.1))) if hand else OBJ
        rows.append((cx[k] - w[k] / 2, cy[k] - h[k] / 2, cx[k] + w[k] / 2, cy[k] + h[k] / 2, int(rng.integers(0, 3)), info))
    return _t(rows)


def pad_targets(targets, g=None, fill=0.0):
    """per-image (boxes, labels, info) -> the padded tables (gt_boxes [n, G, 4], gt_labels [n, G], gt_info [n, G, 5], gt_count [n])"""
    n = len(targets)
    g = max(1, max(len(t[1]) for t in targets)) if g is None else g
    boxes, labels, info = np.full((n, g, 4), fill, F), np.full((n, g), int(fill), np.int32), np.full((n, g, 5), fill, F)
    count = np.zeros((n,), np.int32)
    for i, (b, l, f) in enumerate(targets):
        k = len(l)
        boxes[i, :k], labels[i, :k], info[i, :k], count[i] = b, l, f, k
    return boxes, labels, info, count


@functools.lru_cache(maxsize=None)
def make(name):
    """(cls_lr, reg_ctr, ext or None per level, (gt_boxes, gt_labels, gt_info, gt_count)), read-only"""
    c = BY_NAME[name]
    p = points(c)
    cls, reg, ex = heads_flat(c.seed, c.n, p, c.num_classes, c.ext)
    if c.special == "sat":
        rng = np.random.default_rng(c.seed + 1)
        sign = lambda shape: np.where(rng.integers(0, 2, shape) == 1, F(80.0), F(-80.0))
        cls[...] = sign(cls.shape)
        reg[..., 4] = sign(reg.shape[:2])
        ex[..., 3:] = sign(ex[..., 3:].shape)
    targets = c.targets
    if not targets:
        rng = np.random.default_rng(c.seed + 2)
        targets = tuple(_seeded_targets(rng, k) for k in c.counts)
    starts = fr.cr.starts_of(c.sizes)
    levels = lambda t: [t[:, starts[l]:starts[l + 1]].reshape(c.n, h, w, t.shape[2]).copy() for l, (h, w) in enumerate(c.sizes)]
    out = (levels(cls), levels(reg), levels(ex) if ex is not None else None, pad_targets(targets))
    for t in out[0] + out[1] + (out[2] or []) + list(out[3]):
        t.setflags(write=False)
    return out


def args(name):
    """the positional arguments of fcos_loss_ref.rule / bound / emulate"""
    c = BY_NAME[name]
    cls_lr, reg_ctr, ext, gt = make(name)
    return (cls_lr, reg_ctr, ext, c.strides, c.num_classes) + tuple(gt)


@functools.lru_cache(maxsize=None)
def reference(name):
    a = args(name)
    ref = (fr.rule(*a), fr.bound(*a))
    for d in ref:
        for v in d.values():
            v.setflags(write=False)
    return ref


def image(name, i):
    """the arguments of image i of a case as a batch of one"""
    c = BY_NAME[name]
    cls_lr, reg_ctr, ext, gt = make(name)
    one = lambda ts: [t[i:i + 1] for t in ts]
    return (one(cls_lr), one(reg_ctr), one(ext) if ext is not None else None, c.strides, c.num_classes) + tuple(t[i:i + 1] for t in gt)
