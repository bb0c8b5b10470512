"""Named cases for the crop stage and the joint conversion (tests/crop_ref.py).  Every table is built once (functools.cache) and
shared by the CPU and the GPU tests; each carries a comment saying which loop bound or branch of the kernels it reaches.
Non-finite box coordinates are kept out: the conversion of NaN or inf to int64 is undefined in C++, so nothing can be pinned."""
import functools

import numpy as np

import crop_ref as cr

F = np.float32
HAND = 2                       # the hand label of every table
SWEEP_H, SWEEP_W = 37, 53      # the box sweep's frame
LO, HI = -12, 69               # its integer corners
RESIZE_H, RESIZE_W = 200, 300
SMALL_H, SMALL_W = 40, 50
# (in_ch, cpad, reorder): depth; RGBD as the pipeline runs it; RGBD into a wider pixel (zero padding channels beyond the first
# four); three channels, which only the C entry takes (in_ch < 4 leaves o[3] zero)
CHANNELS = ((1, 4, False), (4, 4, True), (4, 8, True), (3, 4, False))

# the case on which each mutant of crop_ref must fail (tests/test_crop_cpu.py); None: no case can exist, with the reason
MUTANT_CASE = {
    "fma": ("box", (11.0, 3.0, 36.0, 9.0)),          # 11 - 0.4f * 25 = 0.99999985 exactly, 1.0 after the product's rounding
    "round": ("box", (3.0, 3.0, 7.0, 9.0)),          # t2 = 7 + 1.6 = 8.6: 8 truncated, 9 rounded
    "le_w": None,             # t == (float)w: trunc(t) == w, the value the other branch gives (w < 2^24 is exact in fp32)
    "mul_first": ("index", (26, 176, 88)),           # 88 * 26 / 176 = 13 exactly; 88 * fl(26 / 176) falls below 13
    "no_clamp": None,         # dst <= out - 1: dst * fl(in / out) <= in - in / out + in 2^-23 < in for every out < 2^22
    "shift_2in1": ("index", (3, 7, 2)),              # out = 7 = 2 * 3 + 1: floor(2 * 3 / 7) = 0, 2 >> 1 = 1
    "rank_skips_rejected": ("slots", "rejected-first"),
    "crop_w_for_v": ("convert", "J21-n13-rect"),
}


def position_depth(c, h, w, n=None):
    """depth that encodes position: 1 + the element's index in [n, c, h, w], exact in fp32 -> [c, h, w] (n None) or [n, c, h, w]:
    no two source pixels of any frame or channel hold the same value, so a neighbouring pixel, channel or frame is told from the
    right one with certainty, and a zero is never a pixel"""
    total = (n or 1) * c * h * w
    assert total + 1 < 2 ** 24
    d = (np.arange(total, dtype=np.int64) + 1).astype(F)
    return d.reshape((c, h, w) if n is None else (n, c, h, w))


# --------------------------------------------------------------------------------------------------------------------------
# the box sweep
# --------------------------------------------------------------------------------------------------------------------------
OUTSIDE = {    # wholly outside the frame on each side, far enough that the padding does not reach back in
    "above": (10.0, -30.0, 20.0, -10.0),      # padded y2 = -10 + 8 = -2: a negative stop
    "left": (-30.0, 5.0, -10.0, 20.0),        # padded x2 = -2: a negative stop
    "below": (10.0, 60.0, 20.0, 68.0),        # padded y1 = 56 > h: b3 clamps to h, the slice is empty with a positive stop
    "right": (70.0, 5.0, 80.0, 20.0),         # padded x1 = 66 > w
}
# an inverted box is the other way to a negative stop: x2 - 0.4 |bw| < 0 (and on the far side b0 lands beyond b2)
INVERTED = {"inverted-x": (40.0, 5.0, 2.0, 20.0), "inverted-y": (5.0, 30.0, 20.0, 1.0)}
ORIGIN_PIXEL = (0.2, 0.3, 0.9, 0.8)           # truncates to [0, 0, 0, 0]: pads to [0, 0, 0, 0] WITH a hand (a 1 x 1 crop)


@functools.cache
def sweep_boxes():
    """fp32 [B, 4].  Every integer pair (x1, x2) of LO..HI -- inverted, empty, at and beyond w --; (y1, y2) runs through the same
    pairs in another order (pair p of x meets pair 2731 p + 17 mod 82^2 of y; 2731 is coprime to 82^2), so both axes are
    exhaustive and a box's two axes hold different pairs.  Then the named extras."""
    r = np.arange(LO, HI + 1)
    m = len(r)
    p = np.arange(m * m)
    q = (p * 2731 + 17) % (m * m)
    grid = np.stack((r[p // m], r[q // m], r[p % m], r[q % m]), 1).astype(F)
    extra = list(OUTSIDE.values()) + list(INVERTED.values()) + [ORIGIN_PIXEL]
    for k in (0, 5, 16, 32, 36, 52):          # fractional corners: k + 0.999999 truncates to k (where fp32 holds it), -0.9 to 0
        extra += [(-0.9, -0.9, k + 0.999999, k + 0.999999), (k + 0.999999, 0.999999, 40.5, 30.5), (k - 0.9, -0.9, k + 8.999999, 9.5)]
    for bw in range(5, 60, 5):                # widths that are multiples of 5: 0.4f * bw sits next to the integer 0.4 * bw
        for x1 in (0, 1, 2, bw * 2 // 5, bw * 2 // 5 + 1, 30):
            extra.append((x1, x1 % 7, x1 + bw, x1 % 7 + bw))
    for d in (-1.0, -0.5, 0.0, 0.5, 1.0, 7.0):   # corners at and beyond w and h
        extra += [(20.0, 10.0, SWEEP_W + d, SWEEP_H + d), (SWEEP_W + d, SWEEP_H + d, SWEEP_W + d + 3, SWEEP_H + d + 3)]
    big = float(2 ** 24)                      # a corner beyond 2^24: float32(bw) and the padded corner round
    extra += [(5.0, 5.0, big + 2, 20.0), (5.0, 5.0, 20.0, 3.0e7), (-3.0e7, -big - 2, 20.0, 20.0), (3.0e7, 5.0, 3.0000004e7, 20.0),
              (1.0, 1.0, big + 4, big + 4)]
    return np.concatenate((grid, np.asarray(extra, F)))


# --------------------------------------------------------------------------------------------------------------------------
# the resize sweep
# --------------------------------------------------------------------------------------------------------------------------
@functools.cache
def _box_for_width(w):
    """{crop width: (x1, x2)} of detection corners whose padded box gives that width in a frame w wide: integer corners with
    x2 >= x1 >= 0, the first found; plus the key w + 1 for the box whose padded b2 reaches w (the inclusive width b2 + 1 - b0 is
    then w + 1 and the clamp cuts it to w: the full frame)"""
    x1, x2 = np.meshgrid(np.arange(w + 1), np.arange(w + 1), indexing="ij")
    keep = x2 >= x1
    x1, x2 = x1[keep], x2[keep]
    zeros = np.zeros_like(x1)
    box, ok = cr.pad_boxes(np.stack((x1, zeros, x2, zeros), 1).astype(F), w, 1)
    table = {}
    for a, b, o in zip(x1[ok], x2[ok], box[ok]):       # (not ok: x1 == w, a start beyond the last pixel)
        key = int(o[2] + 1 - o[0])
        table.setdefault(key, (float(a), float(b)))
    return table


@functools.cache
def resize_boxes(h, w):
    """fp32 [max(w, h) + 1, 4]: crop widths 1 .. w + 1 in order, each with one of the crop heights 1 .. h + 1 (height index
    7 i + 3 mod (h + 1): 7 is coprime to 201 and to 41, so every height occurs, and width and height differ in almost every crop)"""
    tw, th = _box_for_width(w), _box_for_width(h)
    assert all(k in tw for k in range(1, w + 2)) and all(k in th for k in range(1, h + 2))
    n = max(w, h) + 1
    rows = []
    for i in range(n):
        cw, ch = i % (w + 1) + 1, (7 * i + 3) % (h + 1) + 1
        rows.append((tw[cw][0], th[ch][0], tw[cw][1], th[ch][1]))
    return np.asarray(rows, F)


# frames smaller than the output, a single pixel, one row, one column: (h, w) -> boxes
TINY_FRAMES = {
    (1, 1): ((0.0, 0.0, 0.5, 0.5), (0.0, 0.0, 3.0, 3.0)),
    (1, 300): ((0.0, 0.0, 299.0, 0.0), (10.0, 0.0, 97.0, 0.0), (299.0, 0.0, 299.5, 0.5), (100.0, 0.0, 187.0, 5.0)),
    (300, 1): ((0.0, 0.0, 0.0, 299.0), (0.0, 10.0, 0.0, 97.0), (0.0, 299.0, 0.5, 299.5), (0.0, 100.0, 5.0, 187.0)),
    (5, 7): ((0.0, 0.0, 6.0, 4.0), (1.0, 1.0, 3.0, 2.0), (6.0, 4.0, 6.5, 4.5), (2.0, 0.0, 5.0, 4.0)),
}


# --------------------------------------------------------------------------------------------------------------------------
# the slot walk
# --------------------------------------------------------------------------------------------------------------------------
SLOT_CAP = 130
SLOT_KS = (1, 2, 15, 16)


def _row_box(r):
    """a box of its own for every row, inside the sweep's frame"""
    return (r % 40 + 0.25, r % 30 + 0.5, r % 40 + 5 + r % 7, r % 30 + 4 + r % 5)


@functools.cache
def slot_frames(k):
    """-> (names, boxes [n, cap, 4], labels [n, cap], scores [n, cap], sides [n, cap], counts [n]) for max_hands = k.  The walk
    takes the list 64 rows at a time and stops once k hands are found."""
    cap = SLOT_CAP
    frames = {}

    def frame(name, hands, count=cap, rejected=()):
        labels = np.array([r % 2 for r in range(cap)], np.int32)          # the other rows: labels 0 and 1
        labels[list(hands)] = HAND
        boxes = np.array([_row_box(r) for r in range(cap)], F)
        for r in rejected:
            boxes[r] = OUTSIDE["left"]
        frames[name] = (boxes, labels, count)

    frame("boundaries", (0, 63, 64, 127, 128))               # the last lane of a chunk, the first of the next, the third chunk
    frame("full-chunk", range(64))                           # 64 hands in the first chunk: ranks beyond k are dropped
    frame("scattered", range(3, 61, 3))                      # 20 hands in one chunk: more than max_hands
    frame("quota-at-63", list(range(64 - k, 64)) + [64, 65])  # the quota fills exactly at the chunk's end: rows 64, 65 unread
    frame("count-0", (0, 1, 2), count=0)                     # det_count = 0: the loop body never runs, every slot is zeroed
    frame("count-cap", (5, cap - 1), count=cap)              # det_count = cap: the last row is read
    frame("count-above", (5, cap - 1), count=cap + 57)       # det_count > cap: clamped, no read beyond the list
    frame("count-short", (1, 70, 100), count=71)             # rows at and beyond det_count are not hands
    frame("rejected-first", (2, 9, 11, 64), rejected=(2,))   # a rejected box in slot 0: the slot stays empty, the rank is used
    last = list(range(10, 10 + 2 * k, 2))                    # k hands: the k-th is rejected -> the last slot is empty
    frame("rejected-last", last + [100], rejected=(last[-1],))
    frame("none", ())                                        # no hand label at all
    names = tuple(frames)
    boxes = np.stack([frames[n][0] for n in names])
    labels = np.stack([frames[n][1] for n in names])
    counts = np.array([frames[n][2] for n in names], np.int32)
    scores = (F(0.99) - F(0.001) * np.arange(cap, dtype=F))[None].repeat(len(names), 0) - F(0.0001) * np.arange(len(names), dtype=F)[:, None]
    sides = ((np.arange(cap)[None] * 7 + np.arange(len(names))[:, None]) % 3 % 2).astype(np.int32)    # left hands mixed in
    return names, boxes, labels, scores.astype(F), sides, counts


# --------------------------------------------------------------------------------------------------------------------------
# the gather's second lap
# --------------------------------------------------------------------------------------------------------------------------
LAP_N, LAP_H, LAP_W, LAP_K, LAP_OUT = 5, 24, 32, 16, 176
GRID_THREADS = 8192 * 256          # grid_for's cap times the block: crops at and beyond this many pixels take a second lap


@functools.cache
def lap_boxes():
    """[5, 16, 4]: 80 crops of 176 x 176 = 2 478 080 pixels > 2 097 152 threads: the grid-stride loop's second lap starts inside
    crop 67.  Every slot is filled; the last slot's box is the frame's last pixel."""
    b = np.zeros((LAP_N, LAP_K, 4), F)
    for i in range(LAP_N):
        for k in range(LAP_K):
            x1, y1 = (3 * k + i) % 20, (2 * k + 3 * i) % 14
            b[i, k] = (x1, y1, x1 + 2 + (k + i) % 9, y1 + 1 + (k + 2 * i) % 8)
    b[-1, -1] = (LAP_W - 1, LAP_H - 1, LAP_W - 0.5, LAP_H - 0.5)
    return b


# --------------------------------------------------------------------------------------------------------------------------
# the joint conversion
# --------------------------------------------------------------------------------------------------------------------------
FRAME_H, FRAME_W = 480, 640
PARAS = (617.343, 617.343, 312.42, 241.42)
CONVERT_BOXES = np.array([
    (10, 20, 10, 40),          # width 0: u = x0 for every ku
    (10, 20, 11, 21),          # width 1
    (5, 7, 180, 182),          # 175
    (0, 0, 176, 176),          # 176: the scale is exactly 1
    (3, 2, 180, 179),          # 177
    (0, 0, 640, 480),          # the full frame, as the pad clamps it
    (600, 300, 640, 480),      # ros_demo's clamp as written: x0 = 600 is clamped to H = 480
    (-5, -7, 700, 650),        # ... and corners outside the frame to 0 and to W
    (100, 50, 300, 401),
], np.int64)
KP_SPECIAL = (0.0, 176.0, -3.5, 200.25, 96.0, 175.99999, 1e-3)       # 0, the crop's side, negative, beyond the crop
# (name, J, n, crop_w, crop_h): n * J on both sides of 256, the block of convert_joints_kernel; "rect": crop_w != crop_h
CONVERT_CASES = (
    ("J1-n257", 1, 257, 176, 176), ("J21-n12", 21, 12, 176, 176), ("J21-n13", 21, 13, 176, 176), ("J21-n13-rect", 21, 13, 176, 96),
    ("J64-n4", 64, 4, 176, 176), ("J64-n5-rect", 64, 5, 176, 96), ("J65-n3", 65, 3, 176, 176), ("J65-n4-rect", 65, 4, 176, 96),
)
CONVERT_BY_NAME = {c[0]: c for c in CONVERT_CASES}


@functools.cache
def convert_inputs(name):
    """-> dict(kp [n, J, 3] fp32, box int64 [n, 4], box_f32 [n, 4], sample_paras [n, 4], valid int32 [n]).  kp: the special
    values, then uniform values over [-20, 200]; depth in metres with exact zeros; NaN in single coordinates of row 1 (valid 1)
    and of the row with valid 2; valid cycles through 1, 1, 0, 1, 2, 1."""
    _, j, n, _, _ = CONVERT_BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    kp = rng.uniform(-20.0, 200.0, (n, j, 3)).astype(F)
    kp[..., 2] = rng.uniform(0.2, 1.5, (n, j)).astype(F)
    flat = kp.reshape(-1, 3)
    for i, v in enumerate(KP_SPECIAL):
        flat[i % len(flat), 0] = v
        flat[(i + 3) % len(flat), 1] = v
    flat[::5, 2] = 0.0                                  # a depth of 0
    valid = np.array([(1, 1, 0, 1, 2, 1)[i % 6] for i in range(n)], np.int32)
    if n > 1:
        kp[1, 0, 0] = np.nan
        kp[1, j // 2, 1] = np.nan
        kp[1, j - 1, 2] = np.nan
    if n > 4:
        kp[4, 0] = np.nan
    box = CONVERT_BOXES[np.arange(n) % len(CONVERT_BOXES)].copy()
    box_f32 = (box + rng.uniform(-0.5, 0.5, box.shape)).astype(F)       # the dataset's boxes have fractional corners
    sample_paras = (np.asarray(PARAS) * rng.uniform(0.9, 1.1, (n, 4))).astype(F)
    return dict(kp=kp, box=box, box_f32=box_f32, sample_paras=sample_paras, valid=valid)


# --------------------------------------------------------------------------------------------------------------------------
# the standardisation
# --------------------------------------------------------------------------------------------------------------------------
STD_JOINTS = (2, 21, 64, 65, 100)        # 65 and 100: the store loop's second lap (one wave, j += 64)
STD_ROWS = ("spread", "spread-b", "clustered", "same-u", "same-v", "invalid-0", "invalid-2", "nan-joint")


@functools.cache
def std_inputs(j):
    """-> (uvd [8, J, 3] fp32, valid int32 [8]): joints spread over a 640 x 480 frame; clustered within 1e-3 px around
    (600, 400) (the mean is 10^6 times the std: the statistics' cancellation; the gate refuses such a hand); collinear on one
    axis (std 0 there: 0 / 0); rows with valid 0 and 2; a NaN joint"""
    rng = np.random.default_rng(100 + j)
    uvd = np.empty((len(STD_ROWS), j, 3), F)
    uvd[..., 0] = rng.uniform(0, 640, uvd.shape[:2])
    uvd[..., 1] = rng.uniform(0, 480, uvd.shape[:2])
    uvd[..., 2] = rng.uniform(0.2, 1.5, uvd.shape[:2])
    uvd[2, :, 0] = F(600) + rng.integers(-16, 17, j).astype(F) * F(2.0 ** -14)     # fp32's grid at 600 is 2^-14 = 6.1e-5
    uvd[2, :, 1] = F(400) + rng.integers(-16, 17, j).astype(F) * F(2.0 ** -15)
    uvd[2, 0, :2], uvd[2, 1, :2] = (F(600) - F(2.0 ** -10), F(400) - F(2.0 ** -10)), (F(600) + F(2.0 ** -10), F(400) + F(2.0 ** -10))
    uvd[3, :, 0] = F(123.456)
    uvd[4, :, 1] = F(77.0)
    uvd[7, j // 2, 0] = np.nan
    valid = np.array([1, 1, 1, 1, 1, 0, 2, 1], np.int32)
    return uvd, valid
