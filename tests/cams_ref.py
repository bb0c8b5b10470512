"""A camera per frame, in numpy (helper of test_cams_cpu.py / test_cams_gpu.py; DESIGN.md "A camera per frame"): the overlay's
rule of tests/raster_ref.py -- and its occluded form, tests/occlude_ref.py -- is a rule for ONE frame and one camera.  With a
table of cameras [N,4], rows (fx, fy, cx, cy), frame i's k meshes are drawn with row i; nothing else changes.  So every function
here calls the one-frame helper once per frame with that frame's row and stacks the results.
"""
import numpy as np

import occlude_ref as oc
import raster_ref as rr

HW = (52, 70)            # neither side a multiple of the 8 x 8 tile, and the width no multiple of 4
# three cameras that move the same mesh by tens of pixels (the principal points alone lie 17 to 37 pixels apart) and scale it
# differently along both axes
CAMS = np.array([[150.0, 150.0, 35.0, 26.0],
                 [110.0, 190.0, 15.0, 30.0],
                 [200.0, 120.0, 52.0, 14.0]], np.float32)
RINGS, SEGS = 7, 9       # 65 vertices, 126 faces per ellipsoid: closed, hand-sized, a few pixels per face


def scene(k):
    """(meshes float32 [3,k,V,3], faces [F,3]): per frame a hand-sized ellipsoid half a metre away and -- k = 2 -- a larger one
    at 0.8 m behind it, overlapping on the screen but not in space.  The frames' meshes differ by a few millimetres, so that a
    kernel that read the wrong frame's vertices would show as well."""
    frames = []
    for i in range(len(CAMS)):
        dx = 0.004 * (i - 1)
        near, faces = rr.ellipsoid((0.01 + dx, -0.005, 0.5), (0.05, 0.08, 0.03), rings=RINGS, segs=SEGS)
        far, _ = rr.ellipsoid((0.04 - dx, 0.02, 0.8), (0.11, 0.09, 0.03), rings=RINGS, segs=SEGS)
        frames.append(np.stack([near, far][:k]))
    return np.stack(frames), faces


def frames_f32(bgr):
    """bgr8 [N,H,W,3] -> the same frames as fp32 [N,3,H,W] RGB in 0..1"""
    return np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))


def _lifted(lifted, i):
    return None if lifted is None else np.asarray(lifted)[i]


def render(meshes, faces, cams, frames, lifted=None):
    """meshes [N,K,V,3], cams [N,4], frames [N,...], lifted [N,K] or None -> (image uint8 [N,H,W,3], depth float64 [N,H,W],
    covered bool [N,H,W], ambiguous bool [N,H,W]): raster_ref.render of frame i with row i"""
    per = [rr.render(meshes[i], faces, cams[i], frames[i], _lifted(lifted, i)) for i in range(len(meshes))]
    return tuple(np.stack([p[j] for p in per]) for j in range(4))


def render_candidates(meshes, faces, cams, frames, lifted=None):
    """as render(), with raster_ref.render_candidates: (image, image of the second-nearest faces, covered, ambiguous)"""
    per = [rr.render_candidates(meshes[i], faces, cams[i], frames[i], _lifted(lifted, i)) for i in range(len(meshes))]
    return tuple(np.stack([p[j] for p in per]) for j in range(4))


def occluded(meshes, faces, cams, frames, depth, margin, lifted=None):
    """depth [N,H,W] metres -> one occlude_ref.Occluded per frame, frame i with row i"""
    return [oc.render(meshes[i], faces, cams[i], frames[i], depth[i], margin, _lifted(lifted, i)) for i in range(len(meshes))]


def hiding_depth(meshes, faces, cams, hw=HW):
    """A depth map [N,H,W] that hides part of the near mesh of every frame: a wall at the Z of the near ellipsoid's front pole
    (0.47 m; with a margin of 1 cm the pole's surroundings stay shown and the rim behind them is hidden) over the left half of
    what that mesh covers, far behind everything elsewhere; with a hole (0) and a NaN in the wall."""
    h, w = hw
    out = np.full((len(meshes), h, w), 5.0, np.float32)
    for i in range(len(meshes)):
        ras, _c = rr.rasterize(meshes[i][:1], faces, cams[i], h, w)
        cols = np.nonzero((ras.face >= 0).any(axis=0))[0]
        mid = (int(cols[0]) + int(cols[-1])) // 2
        out[i, :, :mid] = 0.47
        out[i, h // 2, max(0, mid - 3)] = 0.0
        out[i, h // 2 + 1, max(0, mid - 3)] = np.nan
    return out
