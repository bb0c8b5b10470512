"""The object each hand holds, in numpy float32 (csrc/hand_object.hip, hn_hand_objects_f32 and
hn_draw_object_labels_u8).  Every operation is one fp32 operation rounded on its own, in the order written here, so the device's
outputs can be compared bit for bit.  This file is the specification; nothing of the package is imported.

Notation: frame i, slot k, s = i * K + k, j = det_index[i, k], count = clamp(det.count[i], 0, cap).

  association   (the reference's gen_det_result, lib/datasets/voc_eval.py:687-699, on the detections AS THEY ARE: the
                evaluation's %.1f / %.3f file round trip and its +1 are left out on purpose)
                the frame's objects: the rows r < count with labels[i, r] == object_label, in rank order
                empty slot (j < 0, or j >= cap): contact -1, status -1, every other output zero, index -1
                contact = contacts[i, j]; contact <= 0 or no object in the frame: no object, status 1
                else  hc = ((x1 + x2) * 0.5, (y1 + y2) * 0.5) of the hand box boxes[i, j]
                      p  = (hc.x + (m * 10000) * vx, hc.y + (m * 10000) * vy), (m, vx, vy) = dxdymags[i, j]
                      oc = the object's centre, as hc;  dx = oc.x - p.x, dy = oc.y - p.y, d = dx * dx + dy * dy
                      best = the first object; then in rank order: if d < best_d: take.  (A tie keeps the earlier rank; a NaN
                      distance never wins, but a first object whose distance is NaN is never beaten.)
                object_point = p for every slot that is not empty (hc is not substituted), zeros for an empty one
  3-D           candidates: pixels (r, c) with r % stride == 0 and c % stride == 0 whose centre lies in the chosen box,
                x1 <= (float)c + 0.5 < x2 and y1 <= (float)r + 0.5 < y2 in fp32, whose depth D is valid (finite, > 0), whose
                silhouette byte -- if the step has one -- names no slot ((byte & 0x7F) == 0) and fabsf(D - z_hand) <= band,
                z_hand = xyz_mm[s, 0, 2] * 0.001f.  X, Y as the hand cloud's point (tests/cloud_ref.py).
                M matches; int64 sums of rint(X * 1e6), rint(Y * 1e6), rint(D * 1e6) (fp32 products); fp32 min / max of X, Y, D
                object_count = (M, status): 0 ok, 1 no object, 2 M < min_points, -1 empty slot
                object_xyz = (float)((double)sum / ((double)M * 1e6)), zeros unless the status is 0
                object_extent = (min x, y, z, max x, y, z), zeros when M == 0
  label image   for every slot with object_index >= 0, in slot order: the object's rectangle, then the line from the hand box's
                centre to the object box's centre (tests/draw_ref.py rectangle / line_points), both in (0, 0, 255); corners
                and centres ((a + b) * 0.5 in fp32) rounded to nearest-even and saturated at +-2^20, NaN -> 0
"""
import collections

import numpy as np

import draw_ref

F = np.float32
OBJECT_BAND = 0.15         # metres around the hand's root joint depth; a starting value, not tuned on any model
OBJECT_STRIDE = 2          # every second row and column; a starting value, not tuned on any model
OBJECT_MIN_POINTS = 50     # fewer matches: no centroid; a starting value, not tuned on any model
HALF, MICRO, MILLI, TENK = F(0.5), F(1e6), F(0.001), F(10000.0)
BLUE = (0, 0, 255)
FIELDS = ("contact", "object_index", "object_box", "object_score", "object_point", "object_xyz", "object_extent", "object_count")

HandObjects = collections.namedtuple("HandObjects", FIELDS)
# contact int32 [N,K]; object_index int32 [N,K]; object_box fp32 [N,K,4]; object_score fp32 [N,K]; object_point fp32 [N,K,2];
# object_xyz fp32 [N,K,3]; object_extent fp32 [N,K,6]; object_count int32 [N,K,2]


def centre(box):
    """((x1 + x2) * 0.5, (y1 + y2) * 0.5), fp32"""
    with np.errstate(all="ignore"):
        return (F(box[0]) + F(box[2])) * HALF, (F(box[1]) + F(box[3])) * HALF


def point(box, vec):
    """the point a hand's offset vector names: hand centre + (m * 10000) * (vx, vy), the product left to right"""
    cx, cy = centre(box)
    with np.errstate(all="ignore"):
        m = F(vec[0]) * TENK
        return cx + m * F(vec[1]), cy + m * F(vec[2])


def distance2(obox, p):
    ox, oy = centre(obox)
    with np.errstate(all="ignore"):
        dx, dy = ox - p[0], oy - p[1]
        return dx * dx + dy * dy


def scan(dists):
    """the sequential scan over the objects' distances in rank order: the position it keeps"""
    best, best_d = 0, dists[0]
    for q in range(1, len(dists)):
        if dists[q] < best_d:          # (False for a NaN on either side)
            best, best_d = q, dists[q]
    return best


def associate(boxes, scores, labels, count, contacts, dxdymags, det_index, object_label=1):
    """-> (contact [N,K], index [N,K], box [N,K,4], score [N,K], point [N,K,2], status [N,K])"""
    boxes, scores = np.asarray(boxes, F), np.asarray(scores, F)
    n, cap = scores.shape
    k = det_index.shape[1]
    contact = np.full((n, k), -1, np.int32)
    index = np.full((n, k), -1, np.int32)
    box, score, pt = np.zeros((n, k, 4), F), np.zeros((n, k), F), np.zeros((n, k, 2), F)
    status = np.full((n, k), -1, np.int32)
    for i in range(n):
        c = min(max(int(count[i]), 0), cap)
        objects = [r for r in range(c) if int(labels[i, r]) == object_label]
        for kk in range(k):
            j = int(det_index[i, kk])
            if j < 0 or j >= cap:
                continue
            contact[i, kk] = contacts[i, j]
            p = point(boxes[i, j], dxdymags[i, j])
            pt[i, kk] = p
            status[i, kk] = 1
            if contact[i, kk] <= 0 or not objects:
                continue
            r = objects[scan([distance2(boxes[i, r], p) for r in objects])]
            index[i, kk], box[i, kk], score[i, kk], status[i, kk] = r, boxes[i, r], scores[i, r], 0
    return contact, index, box, score, pt, status


def candidates(box, depth, sil, z_hand, band, stride):
    """ONE slot on ONE frame: depth fp32 [H,W], sil uint8 [H,W] or None -> (rows, cols) of the matches, row-major"""
    h, w = depth.shape
    x1, y1, x2, y2 = (F(v) for v in box)
    xc, yc = np.arange(w).astype(F) + HALF, np.arange(h).astype(F) + HALF
    with np.errstate(invalid="ignore"):
        inside = ((y1 <= yc) & (yc < y2))[:, None] & ((x1 <= xc) & (xc < x2))[None, :]
        valid = np.isfinite(depth) & (depth > 0)
        near = np.abs(depth - F(z_hand)) <= F(band)
    cand = np.zeros((h, w), bool)
    cand[::stride, ::stride] = True
    ok = cand & inside & valid & near
    if sil is not None:
        ok &= (sil & 0x7F) == 0
    return np.nonzero(ok)


def back_project(rows, cols, d, paras):
    fx, fy, cx, cy = (F(v) for v in paras)
    with np.errstate(all="ignore"):
        x = ((cols.astype(F) + HALF) - cx) * d / fx
        y = ((rows.astype(F) + HALF) - cy) * d / fy
    return x.astype(F), y.astype(F)


def reduce_points(x, y, d, status, min_points, order=None):
    """the matches' coordinates (fp32 arrays, in any order: `order` permutes them) -> (M, status, xyz [3], extent [6])"""
    m = len(d)
    if order is not None:
        x, y, d = x[order], y[order], d[order]
    if status == 0 and m < min_points:
        status = 2
    xyz, extent = np.zeros(3, F), np.zeros(6, F)
    if m:
        extent[:] = [x.min(), y.min(), d.min(), x.max(), y.max(), d.max()]
    if status == 0:
        for a, v in enumerate((x, y, d)):
            with np.errstate(all="ignore"):
                total = int(np.rint(v * MICRO).astype(np.int64).sum())
            xyz[a] = F(np.float64(total) / (np.float64(m) * np.float64(1e6)))
    return m, status, xyz, extent


def hand_objects(boxes, scores, labels, count, contacts, dxdymags, det_index, depth, xyz_mm, paras, *, object_label=1,
                 band=OBJECT_BAND, stride=OBJECT_STRIDE, min_points=OBJECT_MIN_POINTS, silhouette=None, order=None) -> HandObjects:
    """boxes fp32 [N,cap,4], scores fp32 [N,cap], labels int32 [N,cap], count int32 [N], contacts int32 [N,cap], dxdymags fp32
    [N,cap,3], det_index int32 [N,K], depth fp32 [N,H,W] (or [N,1,H,W]), xyz_mm fp32 [N*K,J,3] (or [N,K,J,3]), paras: 4 values
    or a row per frame [N,4], silhouette uint8 [N,H,W] or None; order(m): a permutation of m matches or None -> HandObjects"""
    det_index = np.asarray(det_index)
    n, k = det_index.shape
    depth = np.asarray(depth, F)
    depth = depth.reshape(n, *depth.shape[-2:])
    xyz_mm = np.asarray(xyz_mm, F).reshape(n * k, -1, 3)
    cams = np.asarray(paras, np.float64).astype(F)
    cams = np.tile(cams, (n, 1)) if cams.ndim == 1 else cams
    assert cams.shape == (n, 4) and stride >= 1 and min_points >= 1 and 1 <= k <= 16
    contact, index, box, score, pt, status = associate(boxes, scores, labels, count, contacts, dxdymags, det_index, object_label)
    xyz, extent, cnt = np.zeros((n, k, 3), F), np.zeros((n, k, 6), F), np.zeros((n, k, 2), np.int32)
    for i in range(n):
        for kk in range(k):
            st = int(status[i, kk])
            rows = cols = np.zeros(0, np.int64)
            if st == 0:
                with np.errstate(all="ignore"):
                    z_hand = xyz_mm[i * k + kk, 0, 2] * MILLI
                rows, cols = candidates(box[i, kk], depth[i], None if silhouette is None else np.asarray(silhouette)[i], z_hand, band,
                                        stride)
            d = depth[i, rows, cols]
            x, y = back_project(rows, cols, d, cams[i])
            m, st, xyz[i, kk], extent[i, kk] = reduce_points(x, y, d, st, min_points, None if order is None else order(len(d)))
            cnt[i, kk] = (m, st)
    return HandObjects(contact, index, box, score, pt, xyz, extent, cnt)


def pixel_of(v):
    """rint (ties to even), saturated at +-2^20; NaN -> 0"""
    v = F(v)
    if np.isnan(v):
        return 0
    return int(min(max(np.rint(v), F(-draw_ref.BOX_LIMIT)), F(draw_ref.BOX_LIMIT)))


def object_primitives(boxes, det_index, object_index):
    """[(frame, (x1, y1, x2, y2) of the rectangle, (x0, y0, x1, y1) of the line)] of the slots with an object, in slot order"""
    boxes = np.asarray(boxes, F)
    cap = boxes.shape[1]
    n, k = det_index.shape
    prims = []
    for i in range(n):
        for kk in range(k):
            o, j = int(object_index[i, kk]), int(det_index[i, kk])
            if o < 0 or o >= cap or j < 0 or j >= cap:
                continue
            rect = tuple(pixel_of(v) for v in boxes[i, o])
            line = tuple(pixel_of(v) for v in centre(boxes[i, j]) + centre(boxes[i, o]))
            prims.append((i, rect, line))
    return prims


def _paint(img, rect, line):
    h, w = img.shape[:2]
    draw_ref.rectangle(img, *rect, colour=BLUE)
    x0, y0, x1, y1 = line
    # (a saturated end point is a million pixels away: then only the pixels of the frame are asked, by the closed form)
    far = max(abs(x1 - x0), abs(y1 - y0)) > 4 * (h + w)
    for x, y in (_far_line(x0, y0, x1, y1, h, w) if far else draw_ref.line_points(x0, y0, x1, y1)):
        if 0 <= x < w and 0 <= y < h:
            img[y, x] = BLUE


def draw_object_labels(box_label, boxes, det_index, object_index):
    """box_label uint8 [N,H,W,3] -> (a copy with the rectangles and lines drawn, bool [N,H,W]: the pixels they cover)"""
    out = np.array(box_label, copy=True)
    mark = np.zeros_like(out)
    for i, rect, line in object_primitives(boxes, det_index, object_index):
        _paint(out[i], rect, line)
        _paint(mark[i], rect, line)
    return out, mark[..., 2] != 0


def _far_line(x0, y0, x1, y1, h, w):
    """line_points' pixels inside the frame for a very long line, from the closed form per pixel of the frame"""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    xmajor = dx >= dy
    major, minor = (dx, dy) if xmajor else (dy, dx)
    pts = []
    for y in range(h):
        for x in range(w):
            ex, ey = x - x0, y - y0
            i, t = (ex * sx, ey * sy) if xmajor else (ey * sy, ex * sx)
            if 0 <= i <= major and (2 * minor * i + major - 1) // (2 * major) == t:
                pts.append((x, y))
    return pts
