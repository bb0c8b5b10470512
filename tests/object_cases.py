"""Seeded inputs of the held objects' tests (tests/test_objects_cpu.py, tests/test_objects_gpu.py): synthetic detections, contact
heads, slots, depth maps, silhouettes and joints made here, so the kernels and the rule (tests/object_ref.py) read identical bytes.
Labels as the detector of num_classes = 3 numbers them: 1 the object, 2 the hand."""
import collections
import functools

import numpy as np

import object_ref as orf

F = np.float32
OBJECT, HAND = 1, 2
# (N, K, H, W, cap): the smallest shape; a width that is no multiple of 64; 16 slots and about 300 object rows (more than one pass
# of the workgroup); strip_rows = 3; the depth plane of an RGB-D tensor (frame stride > H * W)
SHAPES = [(1, 1, 8, 8, 4), (2, 2, 33, 70, 40), (1, 16, 48, 130, 320), (3, 3, 2050, 8, 16), (2, 4, 120, 160, 64)]
LABEL_SHAPE = SHAPES[1]
BAND = 0.0625              # 2^-4: the band's edges below are exact
HOLES = (0.0, -0.5, np.nan, np.inf, -np.inf)      # the five kinds of invalid depth, as the cloud's cases
# per shape: (stride, min_points)
OPTIONS = {SHAPES[0]: (1, 3), SHAPES[1]: (2, 5), SHAPES[2]: (2, 50), SHAPES[3]: (2, 20), SHAPES[4]: (2, 50)}

Case = collections.namedtuple("Case", "n k h w cap stride min_points band boxes scores labels count contacts dxdymags det_index "
                                      "depth sil xyz_mm paras notes")
# boxes fp32 [N,cap,4]; scores fp32 [N,cap]; labels int32 [N,cap]; count int32 [N]; contacts int32 [N,cap]; dxdymags fp32 [N,cap,3];
# det_index int32 [N,K]; depth fp32 [N,H,W]; sil uint8 [N,H,W]; xyz_mm fp32 [N*K,21,3]; paras 4 floats; notes: {name: (i, k)} the
# slots built for one purpose


class _Frame:
    """the rows of one frame in rank order"""

    def __init__(self, rng, h, w):
        self.rng, self.h, self.w, self.rows, self.slots = rng, h, w, [], []

    def add(self, label, box, contact=0, vec=(0.0, 0.0, 0.0)):
        self.rows.append((label, tuple(float(v) for v in box), int(contact), tuple(float(v) for v in vec)))
        return len(self.rows) - 1

    def hand(self, box, contact, vec=(0.0, 0.0, 0.0)):
        self.slots.append(self.add(HAND, box, contact, vec))
        return len(self.slots) - 1

    def random_box(self, lo=0.15, hi=0.6):
        bw, bh = self.w * self.rng.uniform(lo, hi), self.h * self.rng.uniform(lo, hi)
        x1, y1 = self.rng.uniform(-0.3 * bw, self.w - 0.7 * bw), self.rng.uniform(-0.3 * bh, self.h - 0.7 * bh)
        return (x1, y1, x1 + bw, y1 + bh)

    def random_vec(self):
        a = self.rng.uniform(0, 2 * np.pi)
        return (self.rng.uniform(0, 0.004), np.cos(a), np.sin(a))

    def random_hand(self, contact=None):
        return self.hand(self.random_box(0.1, 0.3), int(self.rng.integers(1, 5)) if contact is None else contact, self.random_vec())

    def random_object(self):
        return self.add(OBJECT, self.random_box())

    def fill(self, rows, label=None):
        """random rows of either label (or of `label`) up to `rows`: hands beyond the slots are detections that took no slot"""
        while len(self.rows) < rows:
            lab = label if label is not None else (OBJECT if self.rng.random() < 0.7 else HAND)
            self.add(lab, self.random_box(), int(self.rng.integers(0, 5)), self.random_vec())


def _centred(cx, cy, bw, bh):
    return (cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2)


def _frames(shape, rng):
    """the frames of a shape and the notes: what each frame is for is said where it is built"""
    n, k, h, w, cap = shape
    frames, notes, counts = [_Frame(rng, h, w) for _ in range(n)], {}, [None] * n
    if shape == SHAPES[0]:
        f = frames[0]                      # the hand-computed case of test_objects_cpu.py: m * 10000 = 1.220703125 exactly
        f.hand((1, 1, 5, 5), 3, (2.0 ** -13, 1.0, 0.0))
        f.add(OBJECT, (3, 2, 7, 6))
        f.add(OBJECT, (0, 0, 4, 4))
        f.add(HAND, (4, 4, 8, 8), 1)
        notes["plain"] = (0, 0)
    elif shape == SHAPES[1]:
        f = frames[0]
        f.random_object()
        notes["plain"] = (0, f.random_hand(contact=3))
        # a box narrower than the stride, between two candidate columns, named by a vector of magnitude 0 from a hand centred on it
        notes["narrow"] = (0, f.hand(_centred(21.25, 12.0, 10, 8), 4))
        f.add(OBJECT, (20.6, 4.0, 21.9, 20.0))
        f.fill(30)
        counts[1] = 0                      # a frame without a detection; its rows hold rubbish that nobody may read
        frames[1].fill(cap)
        frames[1].slots = []
    elif shape == SHAPES[2]:
        f = frames[0]
        f.add(OBJECT, (30.0, 10.0, 50.0, 30.0))
        f.add(OBJECT, (float("nan"), 5.0, 60.0, 40.0))                   # a NaN box that is not the first object
        tie = f.add(OBJECT, _centred(64.0, 24.0, 40, 20))                # two objects at exactly equal distance (0) ...
        f.add(OBJECT, _centred(64.0, 24.0, 20, 40))
        notes["tie"] = (0, f.hand(_centred(64.0, 24.0, 16, 16), 3))     # ... from this hand: the earlier rank is expected
        notes["tie_row"] = tie
        notes["contact0"] = (0, f.hand(f.random_box(0.1, 0.3), 0, f.random_vec()))
        for _ in range(13):
            f.random_hand()
        f.fill(320 - 4, label=OBJECT)      # (about 300 object rows: the last of them in the second pass of a 256-thread workgroup)
        # equal distance (0) again, far down the table: the two rows behind this hand, in the workgroup's second pass
        f.hand(_centred(100.0, 40.0, 8, 8), 2)
        notes["far_tie_row"] = f.add(OBJECT, _centred(100.0, 40.0, 6, 10))
        f.add(OBJECT, _centred(100.0, 40.0, 12, 6))
        f.slots = f.slots[:14] + [f.slots[-1]]      # 15 filled slots and an empty one
        notes["far_tie"] = (0, 14)
    elif shape == SHAPES[3]:
        f = frames[0]                      # count above cap: clamped
        for _ in range(3):
            f.random_hand()
        f.add(OBJECT, (-3.0, 100.5, 5.5, 1900.25))                       # partly outside the frame
        f.add(OBJECT, (9.0, -50.0, 30.0, -2.0))                          # wholly outside
        f.add(OBJECT, (1.0, 1500.0, 7.0, 2100.0))
        f.hand(_centred(19.5, -26.0, 4, 4), 3)                           # a hand centred on the object that lies outside
        f.fill(cap, label=OBJECT)
        f.slots = [f.slots[0], f.slots[3], f.slots[1]]
        notes["outside"] = (0, 1)
        counts[0] = cap + 5
        g = frames[1]                      # hands, no objects
        for _ in range(3):
            g.random_hand()
        g.fill(9, label=HAND)
        frames[2].fill(12, label=OBJECT)   # objects, no hands
    else:
        f = frames[0]
        # two hands whose objects' boxes hold exactly min_points and min_points - 1 matches (the depth is stamped below)
        notes["enough"] = (0, f.hand(_centred(30.0, 30.0, 12, 12), 3))
        f.add(OBJECT, _centred(30.0, 30.0, 40, 40))
        notes["short"] = (0, f.hand(_centred(110.0, 80.0, 12, 12), 4))
        f.add(OBJECT, _centred(110.0, 80.0, 40, 40))
        notes["edges"] = (0, f.hand(_centred(110.0, 24.0, 10, 10), 1))  # the band's edges are stamped into this one's box
        f.add(OBJECT, _centred(110.0, 24.0, 30, 30))
        f.random_hand()
        f.fill(50)
        g = frames[1]
        g.add(OBJECT, (10.0, float("nan"), 90.0, 70.0))                  # a NaN box that IS the first object: never beaten
        g.random_object()
        notes["nan_first"] = (1, g.random_hand(contact=3))
        g.random_hand()
        g.random_hand(contact=0)
        g.fill(40)
    return frames, notes, counts


@functools.lru_cache(maxsize=None)
def case(n, k, h, w, cap) -> Case:
    """worked out once per shape, shared, never changed"""
    shape = (n, k, h, w, cap)
    stride, min_points = OPTIONS[shape]
    rng = np.random.default_rng(977 * h + 13 * w + cap)
    frames, notes, counts = _frames(shape, rng)
    boxes = rng.uniform(-50, 50, (n, cap, 4)).astype(F)                  # (rows at and beyond count: rubbish, as the detector leaves them)
    scores = rng.uniform(0, 1, (n, cap)).astype(F)
    labels = rng.integers(1, 3, (n, cap)).astype(np.int32)
    contacts = rng.integers(0, 5, (n, cap)).astype(np.int32)
    dxdymags = rng.uniform(0, 1, (n, cap, 3)).astype(F)
    count = np.zeros((n,), np.int32)
    det_index = np.full((n, k), -1, np.int32)
    for i, f in enumerate(frames):
        assert len(f.rows) <= cap and len(f.slots) <= k, (shape, i, len(f.rows), len(f.slots))
        for r, (lab, box, contact, vec) in enumerate(f.rows):
            boxes[i, r], labels[i, r], contacts[i, r], dxdymags[i, r] = box, lab, contact, vec
        scores[i, :len(f.rows)] = np.sort(rng.uniform(0.7, 1.0, len(f.rows)).astype(F))[::-1]
        count[i] = len(f.rows) if counts[i] is None else counts[i]
        det_index[i, :len(f.slots)] = f.slots
    xyz_mm = rng.uniform(-200, 200, (n * k, 21, 3)).astype(F)
    xyz_mm[:, 0, 2] = 500.0                                              # z_hand = 500 * 0.001f for every slot
    z_hand = F(500.0) * orf.MILLI
    depth = (z_hand + rng.uniform(-2 * BAND, 2 * BAND, (n, h, w)).astype(F)).astype(F)
    kinds = rng.integers(0, 20 * len(HOLES), (n, h, w))                  # a pixel in twenty is a hole, of the five kinds in turn
    for j, value in enumerate(HOLES):
        depth[kinds == j] = F(value)
    sil = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        for value in list(range(1, k + 1))[:3] + [0x80 | 1, 0x80, k + 1, 0x7F, 0x80 | (k + 1)]:
            bh, bw = max(1, int(h * rng.uniform(0.05, 0.2))), max(1, int(w * rng.uniform(0.05, 0.2)))
            r0, c0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
            sil[i, r0:r0 + bh, c0:c0 + bw] = value
    if shape == SHAPES[0]:
        depth[0] = z_hand                  # the hand-computed case: a flat wall, one hole of every kind, one pixel under a mesh
        sil[0] = 0
        for j, value in enumerate(HOLES):
            depth[0, 7, j] = F(value)
        depth[0, 3, 4], depth[0, 4, 5] = F(np.nan), F(0.0)
        sil[0, 2, 3], sil[0, 2, 4] = 0x81, 0x80
    if shape == SHAPES[4]:
        up, down = z_hand + F(BAND), z_hand - F(BAND)
        for name, matches in (("enough", min_points), ("short", min_points - 1)):
            x1, y1, x2, y2 = (int(v) for v in frames[0].rows[det_index[notes[name]] + 1][1])
            depth[0, y1:y2, x1:x2] = z_hand + F(4 * BAND)                # nothing in the box matches ...
            sil[0, y1:y2, x1:x2] = 0
            rows, cols = np.nonzero(np.ones((y2 - y1, x2 - x1), bool)[::stride, ::stride])
            pick = rng.permutation(len(rows))[:matches]                  # ... but exactly `matches` candidates
            depth[0, y1 + stride * rows[pick], x1 + stride * cols[pick]] = (z_hand + rng.uniform(-BAND / 2, BAND / 2, matches)).astype(F)
        x1, y1, x2, y2 = (int(v) for v in frames[0].rows[det_index[notes["edges"]] + 1][1])
        sil[0, y1:y2, x1:x2] = 0
        r, c = (y1 + stride) // stride * stride, (x1 + stride) // stride * stride
        stamps = ((up, True), (np.nextafter(up, F(np.inf)), False), (down, True), (np.nextafter(down, F(0)), False))
        for q, (value, inside) in enumerate(stamps):
            depth[0, r, c + q * stride] = value
            with np.errstate(all="ignore"):
                assert (np.abs(F(value) - z_hand) <= F(BAND)) == inside
        notes["edge_pixels"] = tuple((r, c + q * stride, inside) for q, (_, inside) in enumerate(stamps))
    paras = (0.9 * w + 0.343, 0.95 * w + 0.171, w / 2 - 0.37, h / 2 + 0.21)
    for a in (boxes, scores, labels, count, contacts, dxdymags, det_index, depth, sil, xyz_mm):
        a.setflags(write=False)
    return Case(n, k, h, w, cap, stride, min_points, BAND, boxes, scores, labels, count, contacts, dxdymags, det_index, depth, sil, xyz_mm,
                paras, notes)


def kwargs(c: Case) -> dict:
    return dict(object_label=OBJECT, band=c.band, stride=c.stride, min_points=c.min_points)


@functools.lru_cache(maxsize=None)
def expected(n, k, h, w, cap, with_silhouette=True):
    c = case(n, k, h, w, cap)
    return orf.hand_objects(c.boxes, c.scores, c.labels, c.count, c.contacts, c.dxdymags, c.det_index, c.depth, c.xyz_mm, c.paras,
                            silhouette=c.sil if with_silhouette else None, **kwargs(c))


def check_conditions():
    """what the cases must offer before a comparison means anything (the issue's list); a set of cases that misses one fails"""
    cases = {s: case(*s) for s in SHAPES}
    want = {s: expected(*s) for s in SHAPES}
    bare = {s: expected(*s, with_silhouette=False) for s in SHAPES}
    status = np.concatenate([want[s].object_count[..., 1].reshape(-1) for s in SHAPES])
    print("statuses over all cases:", {v: int((status == v).sum()) for v in (-1, 0, 1, 2)})
    assert all((status == v).sum() >= 2 for v in (-1, 0, 1, 2))
    c1, c2, c3, c4 = (cases[s] for s in SHAPES[1:])
    assert c1.count[1] == 0 and (want[SHAPES[1]].object_count[1, :, 1] == -1).all()                    # a frame with count 0
    assert c3.count[0] > c3.cap                                                                       # a count above cap
    assert (c3.labels[1, :c3.count[1]] == HAND).all() and (c3.det_index[1] >= 0).all()                # hands, no objects
    assert (want[SHAPES[3]].object_count[1, :, 1] == 1).all() and (want[SHAPES[3]].contact[1] > 0).any()
    assert (c3.labels[2, :c3.count[2]] == OBJECT).all() and (c3.det_index[2] < 0).all()               # objects, no hands
    assert any((cases[s].det_index < 0).any() and (cases[s].det_index >= 0).any() for s in SHAPES)    # an empty slot beside filled ones
    i, kk = c2.notes["contact0"]
    assert want[SHAPES[2]].contact[i, kk] == 0 and want[SHAPES[2]].object_count[i, kk, 1] == 1        # contact 0
    for name in ("tie", "far_tie"):                                                                   # equal distances: the earlier rank
        i, kk = c2.notes[name]
        row = c2.notes[name + "_row"]
        p = orf.point(c2.boxes[i, c2.det_index[i, kk]], c2.dxdymags[i, c2.det_index[i, kk]])
        d0, d1 = orf.distance2(c2.boxes[i, row], p), orf.distance2(c2.boxes[i, row + 1], p)
        assert d0 == d1 and c2.labels[i, row] == c2.labels[i, row + 1] == OBJECT
        assert want[SHAPES[2]].object_index[i, kk] == row, (name, want[SHAPES[2]].object_index[i, kk], row)
    assert c2.notes["far_tie_row"] >= 256                                                             # ... beyond one pass of the workgroup
    objects = np.nonzero(c2.labels[0, :c2.count[0]] == OBJECT)[0]
    assert len(objects) >= 290 and np.isnan(c2.boxes[0, objects[1]]).any() and not np.isnan(c2.boxes[0, objects[0]]).any()
    assert not (want[SHAPES[2]].object_index[0] == objects[1]).any()                                  # a NaN that is not first never wins
    first = np.nonzero(c4.labels[1, :c4.count[1]] == OBJECT)[0][0]
    assert np.isnan(c4.boxes[1, first]).any()                                                         # a NaN that is first always does
    held = want[SHAPES[4]].object_index[1][want[SHAPES[4]].object_count[1, :, 1] != 1]
    assert len(held) >= 2 and (held[held >= 0] == first).all() and (held >= 0).any()
    i, kk = c3.notes["outside"]                                                                       # boxes wholly and partly outside
    assert want[SHAPES[3]].object_index[i, kk] == 4 and tuple(want[SHAPES[3]].object_count[i, kk]) == (0, 2)
    assert any(b[0] < 0 < b[2] and w_.object_count[i, kk, 0] > 0 for s, w_ in want.items() for i in range(s[0]) for kk in range(s[1])
               for b in [w_.object_box[i, kk]])
    i, kk = c1.notes["narrow"]                                                                        # narrower than the stride
    b = want[SHAPES[1]].object_box[i, kk]
    assert b[2] - b[0] < c1.stride and tuple(want[SHAPES[1]].object_count[i, kk]) == (0, 2)
    for c in cases.values():                                                                          # the five kinds of hole
        assert all((np.isnan(c.depth).any() if np.isnan(v) else (c.depth == F(v)).any()) for v in HOLES)
    i, kk = c4.notes["edges"]                                                                         # D on both edges of the band
    b = want[SHAPES[4]].object_box[i, kk]
    for r, col, inside in c4.notes["edge_pixels"]:
        assert b[0] <= col + 0.5 < b[2] and b[1] <= r + 0.5 < b[3] and c4.sil[i, r, col] == 0
    (i, kk), (i2, kk2) = c4.notes["enough"], c4.notes["short"]                                        # min_points and one below
    assert tuple(want[SHAPES[4]].object_count[i, kk]) == (c4.min_points, 0)
    assert tuple(want[SHAPES[4]].object_count[i2, kk2]) == (c4.min_points - 1, 2)
    for s, c in cases.items():                                                                        # the silhouette's bytes
        who = c.sil & 0x7F
        assert ((c.sil & 0x80) != 0).any() and (who > c.k).any() and (c.sil == 0x80).any() or s == SHAPES[0]
    assert any((want[s].object_count[..., 0] < bare[s].object_count[..., 0]).any() for s in SHAPES)   # ... and they exclude pixels
    return want
