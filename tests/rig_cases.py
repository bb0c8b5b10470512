"""Inputs for the rig frame's tests (tests/test_rig_cpu.py, tests/test_rig_gpu.py): seeded synthetic rigs, and one scene of
exactly representable coordinates that sits on every edge of the association rule.  numpy only."""
import collections

import numpy as np

F = np.float32
J = 21
RigCase = collections.namedtuple("RigCase", "xyz_mm mesh has_hand lifted score side ext k radius")

EDGE_RADIUS = 0.25                    # r2 = 0.0625, exact
TINY = 2.0 ** -14                     # (TINY^2 + TINY^2) + 0.0625 is the next float above 0.0625


def rotation(axis, angle):
    """float64 rotation matrix about `axis` (Rodrigues)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def extrinsics(n, seed):
    """n camera -> rig transforms [n,3,4] float64: camera 0 near the identity, the others turned and moved by up to a metre"""
    rng = np.random.default_rng(seed)
    e = np.zeros((n, 3, 4))
    for i in range(n):
        e[i, :, :3] = rotation(rng.normal(size=3), rng.uniform(-1.2, 1.2) if i else 0.05)
        e[i, :, 3] = rng.uniform(-1.0, 1.0, size=3) if i else (0.01, -0.02, 0.03)
    return e


def hand_points(rng, count, centre):
    """`count` points of a hand-sized cloud (a box of 16 x 10 x 6 cm) around `centre`, float64 [count,3], metres"""
    return np.asarray(centre, np.float64) + rng.uniform(-0.5, 0.5, size=(count, 3)) * (0.16, 0.10, 0.06)


def to_camera(e, p_rig):
    """rig-frame points -> the camera's frame: R^T (p - t)"""
    return (p_rig - e[:, 3]) @ e[:, :3]


def _junk(rng, shape):
    """what an invalid row may hold: NaN, +-inf and huge values"""
    return rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -1e30], F), size=shape)


def _fill(rng, s, v):
    """every slot empty: junk rows, has_hand 0 (some 2: a crop with non-finite pixels), nothing lifted"""
    has = np.where(rng.random(s) < 0.3, 2, 0).astype(np.int32)
    return (_junk(rng, (s, J, 3)), _junk(rng, (s, v, 3)), has, np.zeros((s,), np.int32), np.zeros((s,), F),
            np.full((s,), -1, np.int32))


def _place(xyz, mesh, has, lifted, score, side, slot, joints_cam_m, verts_cam_m, w, sd, lift=True):
    """put a hand into `slot`: camera-frame joints / vertices in metres -> xyz_mm and the final mesh's (x, -y, -z)"""
    xyz[slot] = (np.asarray(joints_cam_m, np.float64) * 1000.0).astype(F)
    has[slot], score[slot], side[slot] = 1, w, sd
    if lift:
        mesh[slot] = (np.asarray(verts_cam_m, np.float64) * (1, -1, -1)).astype(F)
        lifted[slot] = 1


def random_case(n, k, v, seed, handed=False, noise_mm=3.0) -> RigCase:
    """A rig of n cameras and up to min(k, 4) physical hands 0.5 m apart: every camera sees every hand with probability 0.7,
    in a random slot, with noise of a few mm per view; further slots hold a hand that was not lifted (has_hand 1, lifted 0),
    a NaN row (has_hand 2) or nothing (junk).  handed: sides are handed over, and a second hand of the OTHER side stands at
    the place of hand 0."""
    rng = np.random.default_rng(seed)
    s, ext = n * k, extrinsics(n, seed + 1)
    xyz, mesh, has, lifted, score, side = _fill(rng, s, v)
    hands = [(np.array([0.5 * h, 0.1 * h, 0.6]), h % 2) for h in range(min(k, 4))]
    if handed and k >= 2:
        hands.append((hands[0][0] + 0.002, 1 - hands[0][1]))
    clouds = [(hand_points(rng, J, c), hand_points(rng, v, c)) for c, _ in hands]
    for i in range(n):
        free = list(rng.permutation(k))
        for (joints, verts), (_c, sd) in zip(clouds, hands):
            if not free or rng.random() > 0.7:
                continue
            slot = i * k + int(free.pop())
            noise = lambda p: p + rng.normal(scale=noise_mm / 1000.0, size=p.shape)  # noqa: E731
            _place(xyz, mesh, has, lifted, score, side, slot, to_camera(ext[i], noise(joints)), to_camera(ext[i], noise(verts)),
                   F(rng.uniform(0.3, 1.0)), sd)
        if free and rng.random() < 0.5:                                   # a hand the lifter's skip rule refused
            slot = i * k + int(free.pop())
            _place(xyz, mesh, has, lifted, score, side, slot, to_camera(ext[i], clouds[0][0]), None, F(0.4), hands[0][1], lift=False)
    return RigCase(xyz, mesh, has, lifted, score, side if handed else None, ext, k, 0.08)


def edge_case(n, k, v, seed=0) -> RigCase:
    """n >= 3 cameras with identity extrinsics, k >= 2, radius 0.25, sides given; every joint of a slot sits on ONE exactly
    representable point, so the slot's centre is that point and every distance below is exact:
        camera 0: slot 0 seeds A at (0, 0, 1), side 1; slot 1 seeds B at (0, 0, 3), side 0
        camera 1: slot 0 at (0.125, 0, 1) and slot 1 at (-0.125, 0, 1), side 1: a TIE in d2 from A -- slot 0 joins, slot 1 seeds C
        camera 2: slot 0 at (0, 0, 1.25), side 1: d2 == r2 from A, joins (A is a three-camera rig hand);
                  slot 1 at (2^-14, 2^-14, 3.25), side 0: d2 from B is the next float above r2, seeds D
        camera 3 (n >= 4): slot 0 at B's place with side 1: the side gate keeps it out of B, seeds E;
                  slot 1 at A's place, has_hand 1 but not lifted: takes no part
    The meshes are seeded clouds around the points; every other slot is empty and holds junk."""
    assert n >= 3 and k >= 2
    rng = np.random.default_rng(seed)
    s = n * k
    xyz, mesh, has, lifted, score, side = _fill(rng, s, v)
    ext = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (n, 1, 1))
    placed = [(0, 0, (0, 0, 1), 1, 0.75), (0, 1, (0, 0, 3), 0, 0.5), (1, 0, (0.125, 0, 1), 1, 0.625), (1, 1, (-0.125, 0, 1), 1, 0.875),
              (2, 0, (0, 0, 1.25), 1, 0.4375), (2, 1, (TINY, TINY, 3.25), 0, 0.5)]
    if n >= 4:
        placed += [(3, 0, (0, 0, 3), 1, 0.9375), (3, 1, (0, 0, 1), 1, 0.25)]
    for cam, slot, point, sd, w in placed:
        joints = np.tile(np.asarray(point, np.float64), (J, 1))
        _place(xyz, mesh, has, lifted, score, side, cam * k + slot, joints, hand_points(rng, v, point), F(w), sd,
               lift=(cam, slot) != (3, 1))
    return RigCase(xyz, mesh, has, lifted, score, side, ext, k, EDGE_RADIUS)


# the GPU test's shapes and, for each, a seed whose random_case (handed or not) holds what tests/test_rig_cpu.py asks of it
SHAPES = ((1, 1, 5), (3, 2, 5), (4, 16, 778), (16, 16, 7))
SEEDS = {(1, 1, 5): 1, (3, 2, 5): 21, (4, 16, 778): 6, (16, 16, 7): 1}

# what rig_ref must make of edge_case: (camera, slot) -> rig hand, and the members per rig hand
EDGE_GROUPS = {(0, 0): 0, (0, 1): 1, (1, 0): 0, (1, 1): 2, (2, 0): 0, (2, 1): 3, (3, 0): 4, (3, 1): -1}
EDGE_VIEWS = [3, 1, 1, 1, 1]
