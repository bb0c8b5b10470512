"""Numpy statement of how a MIRRORED hand slot comes back un-mirrored (per-slot handedness of the K-hand live step:
hn_amd.live.LiveHandsEngine(handed=True)).  A slot with mirror == 1 is a left hand that went through the right-handed pose
network and lifter as its mirror image; three rules bring its results back into the frame's own coordinates.  Test
infrastructure only: every function is float32 numpy with one rounding per operation, as the kernels compute it.

  rule 3  crop keypoints     u = crop_w - u_m                      (the aggregation's epilogue)
  rule 4  the lifter's input column 0 of the standardised row of the PLAIN image joints negated (= the standardisation of
                             the mirrored joints: the mean negates, the std does not change); the gate sees the plain joints
  rule 5  the final mesh     ((-x) * 1000 + root_x) / 1000 on the x of the lifter's raw vertices; y, z as for any slot
"""
import numpy as np

CROP = np.float32(176.0)


def unmirror_keypoints(kp_m, mirror, crop=CROP):
    """kp_m [S,J,3] float32 as the network returns it for the (mirrored) crops, mirror [S] -> plain-crop (u,v,d)."""
    out = np.array(kp_m, dtype=np.float32, copy=True)
    m = np.asarray(mirror).astype(bool)
    out[m, :, 0] = np.float32(crop) - out[m, :, 0]
    return out


def mirror_joints(uv, c):
    """Image joints [J,2] mirrored in x about the line x = c / 2: u -> c - u (what the mirrored hand's joints are)."""
    out = np.array(uv, copy=True)
    out[:, 0] = c - out[:, 0]
    return out


def standardize64(uv):
    """(x - mean) / std per axis over the joints in float64 (population std): what the caller's chain reduces to."""
    x = np.asarray(uv, dtype=np.float64)
    return (x - x.mean(axis=0)) / x.std(axis=0)


def lifter_input_mirrored(p2d_plain, mirror, lifted=None):
    """p2d_plain [S,J,2] = the standardised rows of the plain joints (zeros where not lifted) -> the handed step's rows."""
    out = np.array(p2d_plain, dtype=np.float32, copy=True)
    m = np.asarray(mirror).astype(bool)
    if lifted is not None:
        m = m & np.asarray(lifted).astype(bool)
    out[m, :, 0] = -out[m, :, 0]
    return out


def final_mesh_mirrored(raw, perm, xyz0, mirror):
    """ros_demo.py:162,332-337 in numpy float32 for one slot, with rule 5: raw [V0,3] the lifter's vertices, perm
    graph_perm_reverse[:V] (None: no permutation and no camera offset), xyz0 [3] the first joint's camera position in mm."""
    raw = np.array(raw, dtype=np.float32, copy=True)
    if mirror:
        raw[:, 0] = -raw[:, 0]
    if perm is None:
        return raw
    want = raw[perm, :] * np.float32(1000.) + np.asarray(xyz0, np.float32)
    want /= np.float32(1000.)
    want[:, 1] *= -1
    want[:, 2] *= -1
    return want
