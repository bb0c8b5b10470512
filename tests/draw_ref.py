"""The rule of the live step's box_label / pose_label images restated in numpy, painter's style: the
frame is converted, the primitives are drawn one after the other in the reference's order and a later one overwrites an earlier
one.  (The kernels do the opposite -- every pixel looks for the last primitive that covers it -- so the two share no code path.)

ros_demo.py:310-326: cv2.rectangle on the RGB frame; cv2.resize of the colour crop to 176 x 176; VisualUtil('dexycb').plot.
"""
import numpy as np

CROP = 176
COORD_LIMIT = 8191          # joint pixels saturate here
BOX_LIMIT = 1 << 20         # box corners saturate here (frames are at most 16384 wide)
GREEN = (0, 255, 0)
# VisualUtil.color_pred, applied to the RGB image's channels in this order
COLOURS = ((102, 0, 0), (179, 0, 0), (255, 0, 0), (255, 77, 77), (255, 153, 153))
FINGER_JOINTS = ([1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16], [17, 18, 19, 20, 0])


def finger_bones(f):
    a = 4 * f + 1
    return [(0, a), (a, a + 1), (a + 1, a + 2), (a + 2, a + 3)]


def frame_to_rgb(frame):
    """One frame, fp32 [3,H,W] in 0..1 (rint(255 x), NaN -> 0) or uint8 [H,W,3] 'bgr8' -> uint8 [H,W,3] RGB."""
    frame = np.asarray(frame)
    if frame.dtype == np.uint8:
        return np.ascontiguousarray(frame[:, :, ::-1])
    q = np.rint(np.float32(255.0) * frame.astype(np.float32))
    q = np.where(np.isnan(q), np.float32(0), q)
    return np.ascontiguousarray(np.clip(q, 0, 255).astype(np.uint8).transpose(1, 2, 0))


def slot_box(box, flag, h, w, clamp):
    """box (x1,y1,x2,y2) -> (rectangle corners, crop origin, crop size, drawn)."""
    x1, y1, x2, y2 = (int(min(max(int(v), -BOX_LIMIT), BOX_LIMIT)) for v in box)
    if clamp:                   # ros_demo.py:280-281 as written: the first two to [0, H], the last two to [0, W]
        x1, y1 = min(max(x1, 0), h), min(max(y1, 0), h)
        x2, y2 = min(max(x2, 0), w), min(max(y2, 0), w)
    cx1, cx2 = min(max(x1, 0), w), min(max(x2, 0), w)
    cy1, cy2 = min(max(y1, 0), h), min(max(y2, 0), h)
    sw, sh = cx2 - cx1, cy2 - cy1
    drawn = (flag is None or int(flag) == 1) and sw > 0 and sh > 0
    return (x1, y1, x2, y2), (cx1, cy1), (sw, sh), drawn


def rectangle(img, x1, y1, x2, y2, colour=GREEN):
    """Thickness 1, inclusive corners; pixels outside the image are dropped."""
    h, w = img.shape[:2]

    def put(x, y):
        if 0 <= x < w and 0 <= y < h:
            img[y, x] = colour
    for y in range(max(y1, 0), min(y2, h - 1) + 1):
        put(x1, y)
        put(x2, y)
    for x in range(max(x1, 0), min(x2, w - 1) + 1):
        put(x, y1)
        put(x, y2)


def resize_taps(s):
    """cv2.resize INTER_LINEAR, 8-bit: per output index 0..175 the taps (i0, i1) and the weights (w0, w1), w0 + w1 = 2048."""
    scale = 1.0 / (176.0 / float(s))
    j = np.arange(CROP, dtype=np.float64)
    f = ((j + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(np.float32)
    low = i < 0
    i[low], f[low] = 0, 0
    high = i >= s - 1
    i[high], f[high] = s - 1, 0
    i1 = np.where(high, i, i + 1)
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return i, i1, w0, w1


def resize176(crop):
    """uint8 [sh,sw,3] -> uint8 [176,176,3]."""
    sh, sw = crop.shape[:2]
    ix0, ix1, a0, a1 = resize_taps(sw)
    iy0, iy1, b0, b1 = resize_taps(sh)
    src = crop.astype(np.int64)
    hrow = src[:, ix0] * a0[None, :, None] + src[:, ix1] * a1[None, :, None]        # [sh,176,3]
    h0, h1 = hrow[iy0], hrow[iy1]
    out = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def line_points(x0, y0, x1, y1):
    """8-connected Bresenham from (x0, y0), closed form."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    if dx >= dy:
        major, minor = dx, dy
    else:
        major, minor = dy, dx
    if major == 0:
        return [(x0, y0)]
    pts = []
    for i in range(major + 1):
        m = (2 * minor * i + major - 1) // (2 * major)
        pts.append((x0 + sx * i, y0 + sy * m) if dx >= dy else (x0 + sx * m, y0 + sy * i))
    return pts


def line_points_stepping(x0, y0, x1, y1):
    """The same line with an error accumulator (err = major - 2 minor; the minor axis steps when err < 0)."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    xmajor = dx >= dy
    major, minor = (dx, dy) if xmajor else (dy, dx)
    x, y, err = x0, y0, major - 2 * minor
    pts = [(x, y)]
    for _ in range(major):
        if err < 0:
            err += 2 * major
            if xmajor:
                y += sy
            else:
                x += sx
        err -= 2 * minor
        if xmajor:
            x += sx
        else:
            y += sy
        pts.append((x, y))
    return pts


def disc_points(x, y):
    return [(x + ex, y + ey) for ey in range(-2, 3) for ex in range(-2, 3) if ex * ex + ey * ey <= 4]


def joint_pixel(v, clamp):
    v = np.float32(v)
    if np.isnan(v):
        return 0
    if clamp:
        v = min(max(v, np.float32(0)), np.float32(CROP))
    return int(min(max(v, np.float32(-COORD_LIMIT)), np.float32(COORD_LIMIT)))       # int(): truncation toward zero


def skeleton_layers(keypoints, clamp):
    """[(kind, points, colour)] in draw order: per finger the discs, then the lines."""
    px = [(joint_pixel(k[0], clamp), joint_pixel(k[1], clamp)) for k in np.asarray(keypoints).reshape(21, 3)]
    layers = []
    for f in range(5):
        for j in FINGER_JOINTS[f]:
            layers.append(("disc", disc_points(*px[j]), COLOURS[f]))
        for a, b in finger_bones(f):
            layers.append(("line", line_points(*px[a], *px[b]), COLOURS[f]))
    return layers


def draw_skeleton(img, keypoints, clamp):
    for _, pts, colour in skeleton_layers(keypoints, clamp):
        for x, y in pts:
            if 0 <= x < CROP and 0 <= y < CROP:
                img[y, x] = colour
    return img


def draw_labels(keypoints, crop_box, drawn, k, frames, clamp=True, with_bare=False):
    """keypoints [S,21,3], crop_box [S,4], drawn [S] or None, frames = fp32 [N,3,H,W] or uint8 [N,H,W,3] (numpy)
    -> (box_label uint8 [N,H,W,3], pose_label uint8 [S,176,176,3]); with_bare: also the resized crops without the skeleton."""
    keypoints, crop_box = np.asarray(keypoints).reshape(-1, 21, 3), np.asarray(crop_box).reshape(-1, 4)
    s, n = keypoints.shape[0], len(frames)
    assert s == n * k
    rgb = [frame_to_rgb(f) for f in frames]
    h, w = rgb[0].shape[:2]
    box_label = np.stack(rgb).copy()
    pose = np.zeros((s, CROP, CROP, 3), np.uint8)
    bare = np.zeros_like(pose)
    for slot in range(s):
        i = slot // k
        (x1, y1, x2, y2), (cx, cy), (sw, sh), on = slot_box(crop_box[slot], None if drawn is None else drawn[slot], h, w, clamp)
        if not on:
            continue
        rectangle(box_label[i], x1, y1, x2, y2)
        bare[slot] = resize176(rgb[i][cy:cy + sh, cx:cx + sw])
        pose[slot] = draw_skeleton(bare[slot].copy(), keypoints[slot], clamp)
    return (box_label, pose, bare) if with_bare else (box_label, pose)
