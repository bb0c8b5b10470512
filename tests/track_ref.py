"""The tracked hand slots' rule in plain Python integers and numpy, written from the rule's text and not
from the kernel: `step` takes a state and one batch of detection lists and returns every output of the tracked crop stage's slot
kernel and the new state; `crops` is the crop gather on the slots' boxes.  The tests compare the device against it byte for
byte."""
import numpy as np

C = 16              # candidates per frame
WORDS = 12          # int32 words of a state row


def empty_state(n, k):
    return np.zeros((n, 1 + k, WORDS), np.int32)


def pad_box(b, h, w):
    """The crop stage's padding of one float32 detection box (x1, y1, x2, y2): truncate to integers, 40 % of the integer width
    and height on every side in float32, clamp to the frame -> (ok, [x1, y1, x2, y2]); ok = 0 (and zeros) when the inclusive
    slice the crop would cut is empty."""
    f = np.float32
    b0, b1, b2, b3 = (int(f(v)) for v in b)
    pw, ph = f(0.4) * f(b2 - b0), f(0.4) * f(b3 - b1)
    t0, t1, t2, t3 = f(b0) - pw, f(b1) - ph, f(b2) + pw, f(b3) + ph
    b0 = int(t0) if t0 > 0 else 0
    b1 = int(t1) if t1 > 0 else 0
    b2 = int(t2) if t2 < f(w) else w
    b3 = int(t3) if t3 < f(h) else h
    ch, cw = min(b3 + 1, h) - b1, min(b2 + 1, w) - b0
    ok = int(ch > 0 and cw > 0 and b1 >= 0 and b0 >= 0)
    return ok, ([b0, b1, b2, b3] if ok else [0, 0, 0, 0])


def inter_union(a, b):
    """(I, U) of two integer boxes, as the rule states them."""
    i = max(0, min(a[2], b[2]) - max(a[0], b[0])) * max(0, min(a[3], b[3]) - max(a[1], b[1]))
    return i, (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - i


def _read_slots(rows):
    slots = []
    for r in rows[1:]:
        box = [int(v) for v in r[:8].copy().view(np.int64)]
        slots.append(dict(box=box, id=int(r[8]), age=int(r[9]), missed=int(r[10])))
    return slots


def _write_slots(rows, header, slots):
    rows[:] = 0
    rows[0, 0] = header
    for s, t in enumerate(slots):
        if t["id"]:
            rows[1 + s, :8] = np.array(t["box"], np.int64).view(np.int32)
            rows[1 + s, 8:11] = (t["id"], t["age"], t["missed"])


def step_frame(rows, boxes, scores, labels, sides, count, hand_label, k, h, w, thr_milli, hold, left_side):
    """One frame: rows = its [1 + k, 12] state (rewritten in place) -> per-slot outputs as lists."""
    assert h <= 32767 and w <= 32767
    header, slots = int(rows[0, 0]), _read_slots(rows)
    cnt = min(int(count), len(scores))
    # 1. candidates: the first 16 hand-label detections, whatever k; an empty padded slice takes no further part
    cands = []
    for j in range(cnt):
        if int(labels[j]) == hand_label and len(cands) < C:
            ok, box = pad_box(boxes[j], h, w)
            cands.append(dict(ok=ok, box=box, score=np.float32(scores[j]), index=j, side=-1 if sides is None else int(sides[j])))
    # 2. eligible pairs
    pairs = []
    for s, t in enumerate(slots):
        for c, d in enumerate(cands):
            if t["id"] and d["ok"]:
                i, u = inter_union(t["box"], d["box"])
                if i > 0 and 1000 * i >= thr_milli * u:
                    pairs.append((i, u, s, c))
    # 3. greedy: the largest IoU (cross-multiplied), ties to the lower slot, then the lower candidate
    took = {}
    while pairs:
        best = pairs[0]
        for p in pairs[1:]:
            l, r = p[0] * best[1], best[0] * p[1]
            if l > r or (l == r and (p[2], p[3]) < (best[2], best[3])):
                best = p
        took[best[2]] = best[3]
        pairs = [p for p in pairs if p[2] != best[2] and p[3] != best[3]]
    filled = {}
    for s, c in took.items():
        slots[s].update(box=list(cands[c]["box"]), age=slots[s]["age"] + 1, missed=0)
        filled[s] = c
    # 4. live slots without a match: held, or freed
    for s, t in enumerate(slots):
        if t["id"] and s not in took:
            t["missed"] += 1
            if t["missed"] > hold:
                slots[s] = dict(box=[0, 0, 0, 0], id=0, age=0, missed=0)
    # 5. candidates without a match, in score order, into the lowest free slot
    used = set(took.values())
    for c, d in enumerate(cands):
        if d["ok"] and c not in used:
            free = [s for s, t in enumerate(slots) if not t["id"]]
            if not free:
                break
            header += 1
            slots[free[0]] = dict(box=list(d["box"]), id=header, age=0, missed=0)
            filled[free[0]] = c
    # 6. outputs
    out = dict(crop_box=[], has_hand=[], score=[], det_index=[], side=[], mirror=[], track_id=[], track_age=[])
    for s, t in enumerate(slots):
        d = cands[filled[s]] if s in filled else None
        out["crop_box"].append(list(d["box"]) if d else [0, 0, 0, 0])
        out["has_hand"].append(1 if d else 0)
        out["score"].append(d["score"] if d else np.float32(0))
        out["det_index"].append(d["index"] if d else -1)
        out["side"].append(d["side"] if d else -1)
        out["mirror"].append(1 if d and sides is not None and d["side"] == left_side else 0)
        out["track_id"].append(t["id"])
        out["track_age"].append(t["age"])
    _write_slots(rows, header, slots)
    return out


def step(state, boxes, scores, labels, sides, count, hand_label=2, k=2, h=48, w=64, thr_milli=300, hold=5, left_side=0):
    """state int32 [N, 1 + k, 12]; boxes float32 [N, cap, 4], scores float32 [N, cap], labels [N, cap], sides [N, cap] or None,
    count [N] -> dict of crop_box int64 [N,k,4], has_hand / det_index / side / mirror / track_id / track_age int32 [N,k], score
    float32 [N,k] and `state`, the new state (the argument is not changed).  Unsided steps: side is -1 and mirror 0 everywhere
    (the device writes neither)."""
    state = np.array(state, np.int32, copy=True)
    n = state.shape[0]
    assert state.shape == (n, 1 + k, WORDS)
    per = [step_frame(state[i], boxes[i], scores[i], labels[i], None if sides is None else sides[i], count[i], hand_label, k,
                      h, w, thr_milli, hold, left_side) for i in range(n)]
    types = dict(crop_box=np.int64, score=np.float32)
    out = {name: np.array([p[name] for p in per], types.get(name, np.int32)) for name in per[0]}
    out["state"] = state
    return out


def crops(depth, crop_box, has_hand, mirror, out, cpad=4):
    """The crop gather: depth float32 [N,1,h,w], crop_box [N,k,4], has_hand / mirror [N,k] -> float32 [N*k,out,out,cpad]; nearest
    resize of the inclusive slice (source = min(floor(dst * (float32)in / out), in - 1), in float32), channel 0; a mirror slot's
    column ox reads the plain crop's column out - 1 - ox."""
    f = np.float32
    n, k = has_hand.shape
    h, w = depth.shape[-2:]
    res = np.zeros((n * k, out, out, cpad), np.float32)

    def source(size):
        if size == out:
            return np.arange(out)
        if out == 2 * size:
            return np.arange(out) >> 1
        return np.minimum(np.floor(np.arange(out, dtype=f) * (f(size) / f(out))).astype(np.int64), size - 1)
    for i in range(n):
        for s in range(k):
            if not has_hand[i, s]:
                continue
            x1, y1, x2, y2 = (int(v) for v in crop_box[i, s])
            sx, sy = source(min(x2 + 1, w) - x1), source(min(y2 + 1, h) - y1)
            if mirror[i, s]:
                sx = sx[::-1]
            res[i * k + s, :, :, 0] = depth[i, 0][np.ix_(y1 + sy, x1 + sx)]
    return res


def pack(dets, cap=8):
    """One frame's detection list [(box, score, label, side), ...] -> (boxes [cap,4], scores [cap], labels [cap], sides [cap],
    count); rows beyond the list hold a hand-label decoy the count must keep out."""
    boxes, scores = np.tile(np.array([1, 1, 40, 40], np.float32), (cap, 1)), np.full((cap,), 0.5, np.float32)
    labels, sides = np.full((cap,), 2, np.int32), np.zeros((cap,), np.int32)
    dets = dets[:cap]
    for j, (b, sc, lab, sd) in enumerate(dets):
        boxes[j], scores[j], labels[j], sides[j] = b, sc, lab, sd
    return boxes, scores, labels, sides, len(dets)


def random_stream(rng, steps, hands=3, cap=12, h=48, w=64):
    """A seeded walk of one camera stream: `hands` boxes that drift by a few pixels, drop out and come back at random, scores
    redrawn every step (so the score order keeps changing), non-hand detections in between -> a list of detection lists."""
    pos = [np.array([rng.integers(2, w - 22), rng.integers(2, h - 22)], np.float64) for _ in range(hands)]
    size = [rng.integers(6, 16, size=2) for _ in range(hands)]
    out = []
    for _ in range(steps):
        dets = []
        for p, s in zip(pos, size):
            p += rng.integers(-3, 4, size=2)
            p[0], p[1] = min(max(p[0], -4), w - 4), min(max(p[1], -4), h - 4)
            if rng.random() < 0.75:
                dets.append(([p[0] + 0.25, p[1] + 0.5, p[0] + s[0], p[1] + s[1]], 2, int(rng.integers(0, 2))))
        for _ in range(int(rng.integers(0, 4))):
            x, y = rng.integers(0, w - 10), rng.integers(0, h - 10)
            dets.append(([x, y, x + 9.5, y + 8.0], int(rng.integers(0, 2)), int(rng.integers(0, 2))))
        order = rng.permutation(len(dets))
        scores = np.sort(rng.uniform(0.05, 0.99, size=len(dets)).astype(np.float32))[::-1]
        out.append([(dets[j][0], scores[r], dets[j][1], dets[j][2]) for r, j in enumerate(order)][:cap])
    return out
