"""The detector evaluation's rule in numpy fp64, operation for operation: what trainval_net_fcos.py:107-173
selects per image, what pascal_voc.py:339-343 writes into the VOC text files and voc_eval.py reads back, the hand -> object
association of voc_eval.py:662-704, the matching of voc_eval.py:191-225,386-496 for the object class and the five hand tables,
and the epoch's end (voc_eval.py:56-87,227-237).  csrc/det_ap.hip is checked against `accumulate` byte for byte, and
hn_amd.metrics.compute_ap against `compute`.

A batch is a dict of numpy arrays, the detector's fixed-capacity output: boxes f32 [N,cap,4], scores f32 [N,cap], labels, sides,
contacts i32 [N,cap], dxdymags f32 [N,cap,3], count i32 [N], image_ids i32 [N].  A table is the annotation cache flattened
(`table_from_recs`).  A state is {'hand': i32 [I,M], 'obj': i32 [I,M], 'fed': i32 [I], 'overflow': i32 [1]}.

Quirks restated, not repaired: an image without hand records keeps no object records (the `if / if / else` of
trainval_net_fcos.py:161-169); val_objectbbox is true only for None/None or two boxes of plain IoU > 0.5; an overlap of exactly
the threshold is no match; a detection on a difficult box is neither TP nor FP.
"""
import numpy as np

TABLES = ("", "handstate", "handside", "objectbbox", "all")
NAMES = ("targetobject", "hand", "hand+handstate", "hand+handside", "hand+objectbbox", "hand+all")
SCORE_BITS, TP_SHIFT, FP_SHIFT, VALID = 10, 10, 15, 1 << 20
MAX_GT = 64


def file_1f(x):
    """float(format(x, '.1f')) of a float32 x, as the identity DESIGN.md 9n states it"""
    return np.rint(np.float64(np.float32(x)) * 10.0) / 10.0


def file_3f(x):
    return np.rint(np.float64(np.float32(x)) * 1000.0) / 1000.0


def table_from_recs(recs, image_index, hand_name="hand", object_name="targetobject"):
    """the cache dict (name -> list of {name, bbox, difficult, handstate, leftright, objectbbox}) in image_index order"""
    t = dict(hand_off=[0], hand_box=[], hand_meta=[], hand_obj=[], obj_off=[0], obj_box=[], obj_diff=[])
    for name in image_index:
        hands = [o for o in recs[name] if o["name"].lower() == hand_name]
        objs = [o for o in recs[name] if o["name"].lower() == object_name]
        assert len(hands) <= MAX_GT and len(objs) <= MAX_GT
        for o in hands:
            t["hand_box"].append([int(v) for v in o["bbox"]])
            ob = o["objectbbox"]
            t["hand_meta"].append([int(bool(o["difficult"])), int(o["handstate"]), int(o["leftright"]), int(ob is not None)])
            t["hand_obj"].append([0.0] * 4 if ob is None else [float(v) for v in ob])
        for o in objs:
            t["obj_box"].append([int(v) for v in o["bbox"]])
            t["obj_diff"].append(int(bool(o["difficult"])))
        t["hand_off"].append(len(t["hand_box"]))
        t["obj_off"].append(len(t["obj_box"]))
    out = dict(hand_off=np.array(t["hand_off"], np.int32), hand_box=np.array(t["hand_box"], np.int32).reshape(-1, 4),
               hand_meta=np.array(t["hand_meta"], np.int32).reshape(-1, 4), hand_obj=np.array(t["hand_obj"], np.float64).reshape(-1, 4),
               obj_off=np.array(t["obj_off"], np.int32), obj_box=np.array(t["obj_box"], np.int32).reshape(-1, 4),
               obj_diff=np.array(t["obj_diff"], np.int32).reshape(-1))
    out["num_images"] = len(image_index)
    out["npos_hand"] = int((out["hand_meta"][:, 0] == 0).sum())
    out["npos_obj"] = int((out["obj_diff"] == 0).sum())
    return out


def new_state(num_images, max_dets):
    return dict(hand=np.zeros((num_images, max_dets), np.int32), obj=np.zeros((num_images, max_dets), np.int32),
                fed=np.zeros((num_images,), np.int32), overflow=np.zeros((1,), np.int32))


def overlaps(bb, gt):
    """voc_eval.py:199-213: bb fp64 [4] (as parsed from the file), gt fp64 [G,4]; the +1 pixel convention"""
    ixmin = np.maximum(gt[:, 0], bb[0])
    iymin = np.maximum(gt[:, 1], bb[1])
    ixmax = np.minimum(gt[:, 2], bb[2])
    iymax = np.minimum(gt[:, 3], bb[3])
    iw = np.maximum(ixmax - ixmin + 1., 0.)
    ih = np.maximum(iymax - iymin + 1., 0.)
    inters = iw * ih
    uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (gt[:, 2] - gt[:, 0] + 1.) * (gt[:, 3] - gt[:, 1] + 1.) - inters)
    with np.errstate(all="ignore"):
        return inters / uni


def plain_iou(a, b):
    """voc_eval.py:593-615 without its asserts: no +1, 0.0 for disjoint boxes"""
    x_left, y_top = max(a[0], b[0]), max(a[1], b[1])
    x_right, y_bottom = min(a[2], b[2]), min(a[3], b[3])
    if x_right < x_left or y_bottom < y_top:
        return np.float64(0.0)
    inter = np.float64((x_right - x_left) * (y_bottom - y_top))
    area_a = np.float64((a[2] - a[0]) * (a[3] - a[1]))
    area_b = np.float64((b[2] - b[0]) * (b[3] - b[1]))
    with np.errstate(all="ignore"):
        return inter / (area_a + area_b - inter)


def same_object(gt_box, det_box, thr=0.5):
    """val_objectbbox (voc_eval.py:576-589): everything but None/None and a pair of IoU > 0.5 is false"""
    if gt_box is None and det_box is None:
        return True
    if gt_box is not None and det_box is not None:
        return bool(plain_iou(gt_box, det_box) > thr)
    return False


def image_records(batch, n, table, image, hand_label=2, object_label=1, score_min=0.1, ovthresh=0.5):
    """Steps 1-5 for row n of the batch against image `image` of the table -> (hand words, object words) in rank order, each
    word without its valid bit being decided by the caller: (milli, tp bits, fp bits) triples, or None for a score above 1."""
    count = int(min(max(int(batch["count"][n]), 0), batch["scores"].shape[1]))
    score = np.asarray(batch["scores"][n, :count], np.float32)
    label = batch["labels"][n, :count]
    picked = score > np.float32(score_min)
    hands = [k for k in range(count) if picked[k] and label[k] == hand_label]
    objs = [k for k in range(count) if picked[k] and label[k] == object_label]
    if not hands:                                       # the drop rule: no hand records, no object records either
        return [], []

    def parsed_box(k):
        return np.array([file_1f(np.float32(v) + np.float32(1.0)) for v in batch["boxes"][n, k]], np.float64)

    def packable(k):
        return bool(score[k] <= np.float32(1.0))

    def milli(k):
        return int(np.rint(np.float64(score[k]) * 1000.0))

    # the object class: plain voc_eval
    g0, g1 = int(table["obj_off"][image]), int(table["obj_off"][image + 1])
    gt, difficult = table["obj_box"][g0:g1].astype(np.float64), table["obj_diff"][g0:g1] != 0
    taken = [False] * (g1 - g0)
    obj_words, obj_boxes = [], []
    for k in objs:
        bb = parsed_box(k)
        obj_boxes.append(bb)
        tp = fp = 0
        ovmax = -np.inf
        if gt.size > 0:
            ov = overlaps(bb, gt)
            ovmax, jmax = np.max(ov), int(np.argmax(ov))
        if ovmax > ovthresh:
            if not difficult[jmax]:
                if not taken[jmax]:
                    tp, taken[jmax] = 1, True
                else:
                    fp = 1
        else:
            fp = 1
        obj_words.append((milli(k), tp, fp) if packable(k) else None)

    # the hand class: the association, then five tables with their own flags
    g0, g1 = int(table["hand_off"][image]), int(table["hand_off"][image + 1])
    gt, meta, gt_obj = table["hand_box"][g0:g1].astype(np.float64), table["hand_meta"][g0:g1], table["hand_obj"][g0:g1]
    taken = [[False] * (g1 - g0) for _ in TABLES]
    centres = np.array([[(o[0] + o[2]) / 2, (o[1] + o[3]) / 2] for o in obj_boxes], np.float64).reshape(-1, 2)
    hand_words = []
    for k in hands:
        bb = parsed_box(k)
        state, side = int(batch["contacts"][n, k]), int(batch["sides"][n, k])
        v = [file_3f(x) for x in batch["dxdymags"][n, k]]
        det_obj = None
        if not (state <= 0 or len(centres) == 0):
            cc = [(bb[0] + bb[2]) / 2, (bb[1] + bb[3]) / 2]
            point = np.array([cc[0] + v[0] * 10000 * v[1], cc[1] + v[0] * 10000 * v[2]])
            dist = np.sum((centres - point) ** 2, axis=1)
            det_obj = obj_boxes[int(np.argmin(dist))]
        tp, fp = [0] * 5, [0] * 5
        ovmax = -np.inf
        if gt.size > 0:
            ov = overlaps(bb, gt)
            ovmax, jmax = np.max(ov), int(np.argmax(ov))
        if ovmax > ovthresh:
            if not meta[jmax, 0]:
                ok_state, ok_side = meta[jmax, 1] == state, meta[jmax, 2] == side
                ok_obj = same_object(gt_obj[jmax] if meta[jmax, 3] else None, det_obj)
                holds = (True, ok_state, ok_side, ok_obj, ok_state and ok_side and ok_obj)
                for t in range(5):
                    if not taken[t][jmax] and holds[t]:
                        tp[t], taken[t][jmax] = 1, True
                    else:
                        fp[t] = 1
        else:
            fp = [1] * 5
        bits = lambda f: sum(b << t for t, b in enumerate(f))
        hand_words.append((milli(k), bits(tp), bits(fp)) if packable(k) else None)
    return hand_words, obj_words


def accumulate(batch, table, state=None, max_dets=100, **rule):
    """One batch into a state (a new zeroed one when None): the records of image id at [id, rank], written over what was there;
    fed[id] += 1; overflow += the records that do not fit (rank >= max_dets, or a score above 1) + the ids out of range."""
    if state is None:
        state = new_state(table["num_images"], max_dets)
    max_dets = state["hand"].shape[1]
    for n, image in enumerate(np.asarray(batch["image_ids"]).tolist()):
        if not 0 <= image < table["num_images"]:
            state["overflow"][0] += 1
            continue
        state["fed"][image] += 1
        for key, words in zip(("hand", "obj"), image_records(batch, n, table, image, **rule)):
            for rank, w in enumerate(words):
                if w is None or rank >= max_dets:
                    state["overflow"][0] += 1
                else:
                    state[key][image, rank] = VALID | w[0] | (w[1] << TP_SHIFT) | (w[2] << FP_SHIFT)
    return state


def voc_ap(rec, prec, use_07_metric=False):
    """voc_eval.py:56-87"""
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            if np.sum(rec >= t) == 0:
                p = 0
            else:
                p = np.max(prec[rec >= t])
            ap = ap + p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def curve(words, tp_bit, fp_bit, npos, use_07_metric=False):
    """Step 6 for one table: words i32 [I,M] in file order (image index, then rank)"""
    w = np.asarray(words, np.int32).reshape(-1)
    w = w[(w & VALID) != 0]
    confidence = (w & ((1 << SCORE_BITS) - 1)).astype(np.float64) / 1000.0
    tp = ((w >> tp_bit) & 1).astype(np.float64)
    fp = ((w >> fp_bit) & 1).astype(np.float64)
    if w.shape[0] > 0:
        sorted_ind = np.argsort(-confidence)
        tp, fp = tp[sorted_ind], fp[sorted_ind]
    fp = np.cumsum(fp)
    tp = np.cumsum(tp)
    with np.errstate(all="ignore"):
        rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        ap = voc_ap(rec, prec, use_07_metric)
    return {"ap": float(ap), "rec": rec, "prec": prec}


def compute(state, npos_hand, npos_obj, use_07_metric=False):
    if int(np.max(state["fed"], initial=0)) > 1:
        raise ValueError("an image was fed more than once")
    if int(state["overflow"][0]) > 0:
        raise ValueError("records overflowed")
    out = {NAMES[0]: curve(state["obj"], TP_SHIFT, FP_SHIFT, npos_obj, use_07_metric)}
    for t in range(5):
        out[NAMES[1 + t]] = curve(state["hand"], TP_SHIFT + t, FP_SHIFT + t, npos_hand, use_07_metric)
    out["mean_ap"] = float(np.mean([out[NAMES[0]]["ap"], out[NAMES[1]]["ap"]]))
    out["npos"] = {"targetobject": int(npos_obj), "hand": int(npos_hand)}
    out["fed"] = int(np.sum(state["fed"]))
    return out
