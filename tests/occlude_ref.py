"""The occluded overlay's rule in plain numpy float64 (helper of test_occlude_cpu.py / test_occlude_gpu.py; DESIGN.md "The
overlay behind the scene").  It continues tests/raster_ref.py, whose rasterize() gives the nearest and the second-nearest
face of every pixel:

  best       the nearest mesh Z of a covered pixel, slot = the slot (within the frame) of the face that won
  D          the camera's depth map at the pixel, metres; valid when finite and > 0 (holes -- 0, NaN --, inf and negative
             values hide nothing)
  hidden     D valid and best > D + margin (strict)
  image      the face's colour where covered and not hidden, the frame's own pixel everywhere else
  silhouette 0 where no mesh covers the pixel, slot + 1 where covered and shown, 0x80 | (slot + 1) where covered and hidden
  coverage   per slot: (pixels where the slot's mesh is the nearest mesh, the number of those that are shown)

A comparison with the fp32 kernel may leave out two kinds of pixels: the depth fights (raster_ref.ambiguous: the nearest two
faces closer than 1e-4 relative) and the threshold pixels, |best - (D + margin)| <= THRESHOLD_REL * best -- the project's
DEPTH_REL_BOUND of tests/test_render_gpu.py (4 x the measured fp32-against-float64 depth difference, 2.104e-7).
"""
import collections

import numpy as np

import raster_ref as rr

THRESHOLD_REL = 8.4e-7
HIDDEN = 0x80

Occluded = collections.namedtuple("Occluded", "image silhouette coverage fights threshold covered hidden slot slot2")
# image uint8 [H,W,3]; silhouette uint8 [H,W]; coverage int64 [K,2]; fights / threshold / covered / hidden bool [H,W];
# slot / slot2 int [H,W]: slot of the nearest / second-nearest face, -1 where there is none


def valid_depth(depth):
    d = np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def occlude(raster, colours, frame, depth, margin, slots, faces_per_slot):
    """raster, colours: raster_ref.rasterize() of the `slots` slots of ONE frame; frame: fp32 CHW or bgr8 HWC; depth [H,W]
    metres (fp32 values); margin: metres (the fp32 kernel argument's value)"""
    covered = raster.face >= 0
    d = np.asarray(depth, np.float32).astype(np.float64)
    limit = d + float(np.float32(margin))
    valid = valid_depth(d)
    with np.errstate(invalid="ignore"):
        hidden = covered & valid & (raster.z1 > limit)
        threshold = covered & valid & (np.abs(raster.z1 - limit) <= THRESHOLD_REL * raster.z1)
    slot = np.where(covered, raster.face // faces_per_slot, -1)
    slot2 = np.where(raster.face2 >= 0, raster.face2 // faces_per_slot, -1)
    image = rr.frame_u8(frame)
    shown = covered & ~hidden
    image[shown] = colours[raster.face[shown]]
    silhouette = np.where(covered, (slot + 1) | np.where(hidden, HIDDEN, 0), 0).astype(np.uint8)
    return Occluded(image, silhouette, count(silhouette, slots), rr.ambiguous(raster), threshold, covered, hidden, slot, slot2)


def count(silhouette, slots):
    """coverage [slots,2] counted off a silhouette [H,W]"""
    sil = np.asarray(silhouette)
    who = (sil & 0x7F).astype(np.int64)
    shown = (sil & HIDDEN) == 0
    return np.array([[int((who == s + 1).sum()), int(((who == s + 1) & shown).sum())] for s in range(slots)], np.int64).reshape(slots, 2)


def render(meshes, faces, paras, frame, depth, margin, lifted=None):
    """meshes [K,V,3] of one frame -> Occluded"""
    f8 = rr.frame_u8(frame)
    h, w = f8.shape[:2]
    ras, colours = rr.rasterize(meshes, faces, paras, h, w, lifted)
    return occlude(ras, colours, frame, depth, margin, len(meshes), len(faces))
