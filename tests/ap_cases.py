"""Deterministic batches for the detector evaluation's tests: one image per KIND, every kind at every shape
large enough to hold it, packed into batches of the shape's size.  A shape is (images per batch, detection capacity, ground truths
per image and class).  `cases(shape)` -> the annotation cache dict, the image index, the batches (numpy, the detector's
fixed-capacity layout) and the kind of every image.

Conventions: a detection is built from the box its text-file line should hold (raw = that - 1); the rows beyond an image's count
hold a tempting record (score 0.99, a hand on the ground truth) that nobody may read; ground truth is padded to the shape's
number with far-away boxes, before the kind's own boxes in even images and behind them in odd ones, so the last lanes matter.
"""
import numpy as np

SHAPES = [(1, 1, 1), (3, 5, 2), (5, 64, 64), (2, 65, 3), (2, 130, 64)]
OVERFLOW_SHAPE, OVERFLOW_MAX_DETS = (2, 65, 3), 64          # the dedicated case: 65 hand records of one image, 64 places

B = [100, 100, 199, 219]          # the hand everybody detects
B2 = [400, 100, 499, 219]
OB = [180, 100, 219, 139]         # an object next to it
OB2 = [600, 300, 659, 379]
FAR = [2000, 2000, 2059, 2059]


def gt_hand(box, difficult=0, state=0, side=0, obj=None):
    return {"name": "hand", "bbox": list(box), "difficult": difficult, "handstate": state, "leftright": side, "objectbbox": obj}


def gt_obj(box, difficult=0):
    return {"name": "targetobject", "bbox": list(box), "difficult": difficult, "handstate": 0, "leftright": 0, "objectbbox": None}


def det(filed_box, score, label, state=0, side=0, v=(0.0, 0.0, 0.0)):
    return {"box": [np.float32(c) - np.float32(1.0) for c in filed_box], "score": np.float32(score), "label": label, "state": state,
            "side": side, "v": v}


def hand(filed_box, score, **kw):
    return det(filed_box, score, 2, **kw)


def obj(filed_box, score):
    return det(filed_box, score, 1)


def _shift(box, dx, dy=0):
    return [box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy]


def _image(hands=(), objs=(), dets=(), bare=False):
    return {"hands": list(hands), "objs": list(objs), "dets": list(dets), "bare": bare}


# every kind: (cap, g) -> list of images, or None when the shape cannot hold it
def no_detections(cap, g):
    return [_image([gt_hand(B)], [gt_obj(OB)])]


def no_ground_truth(cap, g):
    return [_image(dets=[hand(B, 0.9)] + ([obj(OB, 0.8)] if cap >= 2 else []), bare=True)]


def objects_no_hand(cap, g):
    return [_image([gt_hand(B)], [gt_obj(OB)], [obj(OB, 0.9)] + ([hand(B, 0.05)] if cap >= 2 else []))]


def difficult_hand(cap, g):
    return [_image([gt_hand(B, difficult=1)], dets=[hand(B, 0.9)])]


def taken_twice(cap, g):
    if cap < 2:
        return None
    return [_image([gt_hand(B)], dets=[hand(B, 0.9), hand(_shift(B, 2, 1), 0.8)] + ([hand(_shift(B, -1), 0.7)] if cap >= 3 else []))]


def overlap_half(cap, g):
    # a 10 x 10 box inside a 10 x 20 one (pixels inclusive): 100 / 200, not above 0.5
    return [_image([gt_hand([300, 300, 319, 309])], dets=[hand([305, 300, 314, 309], 0.9)])]


def equal_overlap(cap, g):
    if g < 2:
        return None
    dets = [hand([105, 100, 124, 109], 0.9, state=1)] + ([hand([105, 100, 124, 109], 0.8, state=1)] if cap >= 2 else [])
    return [_image([gt_hand([100, 100, 119, 109], state=1), gt_hand([110, 100, 129, 109], state=2)], dets=dets)]


def equal_distance(cap, g):
    if cap < 3:
        return None
    # the hand points at (199.5, 159.5); the first and the LAST object record sit 40 above and 40 below it
    first, last = OB, [180, 180, 219, 219]
    between = [obj(_shift(FAR, 70 * i), 0.85 - 0.005 * i) for i in range(min(cap - 3, 127))]
    dets = [hand(B, 0.95, state=1, v=(0.01, 0.5, 0.0)), obj(first, 0.9)] + between + [obj(last, 0.12)]
    return [_image([gt_hand(B, state=1, obj=[float(c) for c in first])], [gt_obj(first)], dets)]


def state0_with_objects(cap, g):
    if cap < 2:
        return None
    return [_image([gt_hand(B)], [gt_obj(OB)], [hand(B, 0.9, v=(0.01, 0.5, 0.0)), obj(OB, 0.85)])]


def both_absent(cap, g):
    return [_image([gt_hand(B, state=1)], dets=[hand(B, 0.9, state=1, v=(0.01, 0.5, 0.5))])]


def wrong_state(cap, g):
    return [_image([gt_hand(B, state=3, side=1)], dets=[hand(B, 0.9, state=1, side=1)])]


def wrong_side(cap, g):
    return [_image([gt_hand(B, state=1, side=1)], dets=[hand(B, 0.9, state=1, side=0)])]


def wrong_object(cap, g):
    if cap < 2:
        return None
    return [_image([gt_hand(B, state=1, obj=[400.5, 100.0, 460.0, 160.25])], [gt_obj(OB)],
                   [hand(B, 0.9, state=1, v=(0.01, 0.5, 0.0)), obj(OB, 0.8)])]


def object_iou_half(cap, g):
    if cap < 2:
        return None
    # plain IoU (no +1) of a 40 x 20 box inside a 40 x 40 one: 800 / 1600, not above 0.5
    return [_image([gt_hand(B, state=1, obj=[180.0, 100.0, 220.0, 120.0])], [gt_obj(OB)],
                   [hand(B, 0.9, state=1, v=(0.01, 0.5, 0.0)), obj([180, 100, 220, 140], 0.8)])]


def object_only_in_gt(cap, g):
    return [_image([gt_hand(B, obj=[1.0, 2.0, 30.0, 40.0])], dets=[hand(B, 0.9)])]


def object_only_in_det(cap, g):
    if cap < 2:
        return None
    return [_image([gt_hand(B, state=1)], [gt_obj(OB)], [hand(B, 0.9, state=1, v=(0.01, 0.5, 0.0)), obj(OB, 0.8)])]


def low_score(cap, g):
    if cap < 2:
        return [_image([gt_hand(B)], dets=[hand(B, np.float32(0.1))])]          # float32(0.1) is not above float32(0.1)
    return [_image([gt_hand(B), ] + ([gt_hand(B2)] if g >= 2 else []), [gt_obj(OB)],
                   [hand(B, 0.9), hand(B2, np.float32(0.1))] + ([obj(OB, 0.05)] if cap >= 3 else []))]


def other_labels(cap, g):
    return [_image([gt_hand(B)], [gt_obj(OB)], [det(B, 0.95, 3)] + ([hand(B, 0.9), det(OB, 0.8, 0)] if cap >= 3 else []))]


def halfway(cap, g):
    # %.3f: 0.8125 -> 0.812; %.1f after the float32 + 1: 9.25 -> 10.2, 9.75 -> 10.8, 18.25 -> 19.2 (all half to even).
    # The ground truth is 20 x 10 and the filed box lies inside it: its overlap is (x2 - x1 + 1) * h / 200 with x1 = 10.2, above
    # 0.5 from x2 = 19.3 on.  The second box ends at 28.75 + 1 -> 29.8 where half away from zero would not change it; its
    # left edge 18.75 + 1 -> 19.8 (half up would give the same) -- what counts for both is that the state's bytes are the rule's.
    d = hand([0, 0, 0, 0], 0.8125)
    d["box"] = [np.float32(9.25), np.float32(9.0), np.float32(18.25), np.float32(18.0)]
    dets = [d]
    if cap >= 2:
        e = hand([0, 0, 0, 0], 0.4375)
        e["box"] = [np.float32(9.75), np.float32(9.0), np.float32(28.75), np.float32(18.0)]
        e["v"] = (np.float32(0.0625), np.float32(0.1875), np.float32(0.3125))
        e["state"] = 1
        dets.append(e)
    return [_image([gt_hand([10, 10, 29, 19])], dets=dets)]


def equal_scores_across_images(cap, g):
    # 0.9004 and 0.9001: both 0.900 in the file, a TP in one image and an FP in the other
    return [_image([gt_hand(B)], dets=[hand(B, 0.9004)]), _image([gt_hand(B)], dets=[hand(FAR, 0.9001)])]


def full_capacity(cap, g):
    # as many hand records as the detector has rows; the first is the TP
    return [_image([gt_hand(B)], dets=[hand(_shift(B, 3 * i), 0.99 - 0.005 * i) for i in range(cap)])]


def association_far(cap, g):
    if cap < 2:
        return None
    # one hand and cap - 1 object records in a row; the hand points at the LAST of them (chunks of 64 crossed at 65 and 130)
    m = cap - 1
    boxes = [[1000 + 60 * i, 100, 1039 + 60 * i, 139] for i in range(m)]
    v = (0.1, (870 + 60 * (m - 1)) / 1000.0, -0.04)
    dets = [hand(B, 0.97, state=2, v=v)] + [obj(b, 0.9 - 0.005 * i) for i, b in enumerate(boxes)]
    return [_image([gt_hand(B, state=2, obj=[float(c) for c in boxes[-1]])], [gt_obj(boxes[0])], dets)]


def object_class_mix(cap, g):
    if cap < 4 or g < 2:
        return None
    dets = [hand(B, 0.95), obj(OB, 0.9), obj(_shift(OB, 1), 0.85), obj(OB2, 0.8)] + ([obj(FAR, 0.7)] if cap >= 5 else [])
    return [_image([gt_hand(B)], [gt_obj(OB), gt_obj(OB2, difficult=1)], dets)]


KINDS = [no_detections, no_ground_truth, objects_no_hand, difficult_hand, taken_twice, overlap_half, equal_overlap, equal_distance,
         state0_with_objects, both_absent, wrong_state, wrong_side, wrong_object, object_iou_half, object_only_in_gt,
         object_only_in_det, low_score, other_labels, halfway, equal_scores_across_images, full_capacity, association_far,
         object_class_mix]
TIE_KINDS = ("equal_overlap", "equal_distance", "equal_scores_across_images")


def rows_of(image, cap):
    """one image's detections in the detector's layout: score-descending rows, then the tempting rows nobody may read"""
    dets = sorted(image["dets"], key=lambda d: -float(d["score"]))
    assert len(dets) <= cap
    out = dict(boxes=np.zeros((cap, 4), np.float32), scores=np.zeros((cap,), np.float32), labels=np.zeros((cap,), np.int32),
               sides=np.zeros((cap,), np.int32), contacts=np.zeros((cap,), np.int32), dxdymags=np.zeros((cap, 3), np.float32))
    for k in range(cap):
        d = dets[k] if k < len(dets) else hand(B, 0.99, state=1, side=1, v=(0.5, 0.5, 0.5))
        out["boxes"][k], out["scores"][k], out["labels"][k] = d["box"], d["score"], d["label"]
        out["sides"][k], out["contacts"][k], out["dxdymags"][k] = d["side"], d["state"], d["v"]
    return out, len(dets)


def pack(images, ids, cap):
    """images -> one batch dict"""
    rows = [rows_of(im, cap) for im in images]
    batch = {k: np.stack([r[0][k] for r in rows]) for k in rows[0][0]}
    batch["count"] = np.array([r[1] for r in rows], np.int32)
    batch["image_ids"] = np.asarray(ids, np.int32)
    return batch


def annotations_of(image, number, g, uniform=False):
    """uniform: the padding hands carry an object box when the kind's own hands do (the reference stacks an image's object boxes
    into one numpy array, which wants them all present or all absent)"""
    if image["bare"]:
        return []
    pad_box = [7000.0, 7000.0, 7050.0, 7050.0] if uniform and any(h["objectbbox"] is not None for h in image["hands"]) else None
    pad_h = [gt_hand(_shift([5000, 5000, 5029, 5029], 50 * i), state=1, side=i % 2, obj=pad_box) for i in range(g - len(image["hands"]))]
    pad_o = [gt_obj(_shift([5000, 6000, 5029, 6029], 50 * i)) for i in range(g - len(image["objs"]))]
    assert len(image["hands"]) <= g and len(image["objs"]) <= g
    if number % 2 == 0:
        recs = pad_h + image["hands"] + pad_o + image["objs"]
    else:
        recs = image["hands"] + pad_h + image["objs"] + pad_o
    if number % 3 == 0:                                       # the class names compare in lower case
        recs = [dict(r, name=r["name"].capitalize()) for r in recs]
    return recs


_CASES = {}


def cases(shape, kinds=None, uniform=False):
    """-> dict(recs, image_index, batches, kinds (per image id), cap).  The batches' image ids are a fixed permutation of the
    images, so neighbours in a batch are no neighbours in the state; the table's last image is never fed."""
    key = (shape, None if kinds is None else tuple(k.__name__ for k in kinds), uniform)
    if key in _CASES:
        return _CASES[key]
    n, cap, g = shape
    images, names = [], []
    for kind in (KINDS if kinds is None else kinds):
        made = kind(cap, g)
        for im in made or []:
            images.append(im)
            names.append(kind.__name__)
    while len(images) % n:
        images.append(_image([gt_hand(B)], dets=[hand(B, 0.6)]))
        names.append("pad")
    total = len(images)
    order = np.random.RandomState(7 + total).permutation(total)          # image j of the list gets id order[j]
    recs, kind_of = {}, [None] * (total + 1)
    image_index = ["frame_%04d" % i for i in range(total + 1)]
    for j, im in enumerate(images):
        recs[image_index[order[j]]] = annotations_of(im, j, g, uniform)
        kind_of[order[j]] = names[j]
    recs[image_index[total]] = [gt_hand(B), gt_obj(OB), gt_obj(OB2, difficult=1)]
    kind_of[total] = "unfed"
    batches = [pack(images[lo:lo + n], order[lo:lo + n], cap) for lo in range(0, total, n)]
    _CASES[key] = dict(recs=recs, image_index=image_index, batches=batches, kinds=kind_of, cap=cap)
    return _CASES[key]


def kinds_that_fit(shape):
    _, cap, g = shape
    return [k.__name__ for k in KINDS if k(cap, g) is not None]


def concat(batches):
    return {k: np.concatenate([b[k] for b in batches]) for k in batches[0]}
