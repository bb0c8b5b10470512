"""The rig frame without a GPU: the properties of the rule as tests/rig_ref.py states it, the layout and
the read() of a rig step, the host's checks, and the new entry of the C ABI."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest
import torch

import rig_cases as rc
import rig_ref as rr
from hn_amd.ops import RIG_FIELDS          # (the eight outputs, in the order the step delivers them)

F = np.float32


def _run(case, **kw):
    args = dict(radius=case.radius, side=case.side)
    args.update(kw)
    return rr.rig_fuse(case.xyz_mm, case.mesh, case.has_hand, case.lifted, case.score, rr.table(case.ext), case.k, **args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _identity(n):
    return np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (n, 1, 1))


# ------------------------------------------------------------------------------------------------- the rule's properties
def test_identity_extrinsics_keep_the_camera_frame():
    """identity extrinsics: rig_xyz == xyz_mm / 1000 and rig_mesh == mesh * (1, -1, -1), bit for bit, on the valid rows; zero
    rows elsewhere, whatever the invalid rows hold"""
    case = rc.random_case(3, 6, 11, seed=5)._replace(ext=_identity(3))
    out = _run(case)
    has, lifted = case.has_hand == 1, case.lifted == 1
    assert has.sum() >= 3 and lifted.sum() >= 3 and (~has).sum() >= 2 and not np.isfinite(case.xyz_mm[~has]).all()
    rig_xyz, rig_mesh = out.rig_xyz.reshape(18, 21, 3), out.rig_mesh.reshape(18, 11, 3)
    assert np.array_equal(_bits(rig_xyz[has]), _bits(case.xyz_mm[has] / F(1000)))
    assert np.array_equal(_bits(rig_mesh[lifted]), _bits(case.mesh[lifted] * np.array([1, -1, -1], F)))
    assert not _bits(rig_xyz[~has]).any() and not _bits(rig_mesh[~lifted]).any()
    for name in RIG_FIELDS:
        if name != "rig_count":
            assert np.isfinite(getattr(out, name)).all(), name


def test_the_table_rounds_once_and_drops_the_last_row():
    e = rc.extrinsics(3, seed=2)
    four = np.concatenate([e, np.tile([[[0.0, 0.0, 0.0, 1.0]]], (3, 1, 1))], axis=1)
    assert rr.table(e).dtype == F and rr.table(e).shape == (3, 12)
    assert np.array_equal(rr.table(e), rr.table(four)) and np.array_equal(rr.table(e).reshape(3, 3, 4), e.astype(F))


def _two_views(noise_mm=3.0, offset=(0.0, 0.0, 0.0), seed=3):
    """one hand P in the rig frame seen by two cameras with different R, t; camera 1's hand moved by `offset` (rig frame)"""
    rng = np.random.default_rng(seed)
    ext = rc.extrinsics(2, seed=seed)
    joints, verts = rc.hand_points(rng, 21, (0.1, -0.2, 0.7)), rc.hand_points(rng, 30, (0.1, -0.2, 0.7))
    s, v = 2, 30
    xyz, mesh = np.zeros((s, 21, 3), F), np.zeros((s, v, 3), F)
    has, lifted, score, side = np.zeros(s, np.int32), np.zeros(s, np.int32), np.zeros(s, F), np.zeros(s, np.int32)
    for i in range(2):
        shift = np.asarray(offset) * i
        jn, vn = (p + shift + rng.normal(scale=noise_mm / 1000.0, size=p.shape) for p in (joints, verts))
        rc._place(xyz, mesh, has, lifted, score, side, i, rc.to_camera(ext[i], jn), rc.to_camera(ext[i], vn), F(0.9 - 0.3 * i), 0)
    return rc.RigCase(xyz, mesh, has, lifted, score, None, ext, 1, rr.RIG_RADIUS), joints, verts


def test_two_cameras_fuse_one_hand():
    """two cameras with different R, t see one hand with a few mm of noise each: one rig hand with 2 views, and every fused
    point lies within the larger member deviation + 1e-6 m of the true point (a weighted mean is a convex combination; the
    1e-6 covers the fp32 rounding)"""
    case, joints, verts = _two_views()
    out = _run(case)
    assert out.rig_count == 1 and out.rig_hand.tolist() == [[0], [0]] and out.rig_views.tolist() == [2, 0]
    assert out.rig_seed.tolist() == [0, -1]
    for fused, members, truth in ((out.fused_xyz, out.rig_xyz, joints), (out.fused_mesh, out.rig_mesh, verts)):
        dev = np.linalg.norm(members[:, 0].astype(np.float64) - truth, axis=-1)            # [2, points]
        assert 1e-4 < dev.max() < 0.02                                                     # (the noise is there, and small)
        err = np.linalg.norm(fused[0].astype(np.float64) - truth, axis=-1)
        assert (err <= dev.max(axis=0) + 1e-6).all()
        assert not _bits(fused[1:]).any()
        assert not np.array_equal(fused[0], members[0, 0]) and not np.array_equal(fused[0], members[1, 0])


def test_a_one_view_rig_hand_is_its_member_and_far_hands_stay_apart():
    """two hands 0.5 m apart give two rig hands, each the copy of its member bit for bit"""
    case, _j, _v = _two_views(offset=(0.5, 0.0, 0.0))
    out = _run(case)
    assert out.rig_count == 2 and out.rig_hand.tolist() == [[0], [1]] and out.rig_views.tolist() == [1, 1]
    assert out.rig_seed.tolist() == [0, 1]
    for g in range(2):
        assert np.array_equal(_bits(out.fused_xyz[g]), _bits(out.rig_xyz[g, 0]))
        assert np.array_equal(_bits(out.fused_mesh[g]), _bits(out.rig_mesh[g, 0]))


def test_two_slots_of_one_camera_never_merge():
    """two lifted slots of the SAME camera 1 cm apart stay two rig hands; the second camera's hand joins the first (the seed)"""
    rng = np.random.default_rng(8)
    ext = rc.extrinsics(2, seed=8)
    joints, verts = rc.hand_points(rng, 21, (0, 0, 0.6)), rc.hand_points(rng, 9, (0, 0, 0.6))
    s = 4
    xyz, mesh = np.zeros((s, 21, 3), F), np.zeros((s, 9, 3), F)
    has, lifted, score, side = np.zeros(s, np.int32), np.zeros(s, np.int32), np.zeros(s, F), np.zeros(s, np.int32)
    for slot, cam, shift in ((0, 0, 0.0), (1, 0, 0.01), (2, 1, 0.004)):
        rc._place(xyz, mesh, has, lifted, score, side, slot, rc.to_camera(ext[cam], joints + (shift, 0, 0)),
                  rc.to_camera(ext[cam], verts + (shift, 0, 0)), F(0.5), 0)
    out = rr.rig_fuse(xyz, mesh, has, lifted, score, rr.table(ext), 2)
    assert out.rig_count == 2 and out.rig_hand.tolist() == [[0, 1], [0, -1]] and out.rig_views.tolist() == [2, 1, 0, 0]


def test_the_edges_of_the_association():
    """rig_cases.edge_case on exactly representable points: a tie in d2 keeps the lower k, d2 == r2 joins and the next float
    above does not, the side gate keeps a left and a right hand at one place apart (and without the gate they merge), a slot
    that is not lifted takes no part, a rig hand holds three cameras"""
    for n, k in ((3, 2), (4, 2), (4, 5)):
        case = rc.edge_case(n, k, 6)
        out = _run(case)
        want = np.full((n, k), -1)
        for (cam, slot), g in rc.EDGE_GROUPS.items():
            if cam < n:
                want[cam, slot] = g
        views = rc.EDGE_VIEWS[:want.max() + 1]
        assert out.rig_hand.tolist() == want.tolist() and out.rig_count == len(views)
        assert out.rig_views.tolist() == views + [0] * (n * k - len(views))
        assert out.rig_seed.tolist() == [0, 1, k + 1, 2 * k + 1, 3 * k][:len(views)] + [-1] * (n * k - len(views))
        centre = rr.centres(out.rig_xyz.reshape(n * k, 21, 3))
        d = centre[2 * k + 1] - centre[1]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        r2 = F(case.radius) * F(case.radius)
        assert d2 == np.nextafter(r2, F(1)) and centre[2 * k].tolist() == [0.0, 0.0, 1.25] and r2 == F(0.0625)
        # three members, summed in slot order: the fused point is ((w0 x0 + w1 x1) + w2 x2) / ((w0 + w1) + w2) in fp32
        m = [0, k, 2 * k]
        w, x = [F(case.score[i]) for i in m], [out.rig_mesh.reshape(n * k, 6, 3)[i] for i in m]
        assert np.array_equal(_bits(out.fused_mesh[0]), _bits(((w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]) / ((w[0] + w[1]) + w[2])))
        if n >= 4:                                                        # without the gate, E's slot joins B
            open_ = _run(case, side=None)
            assert open_.rig_hand[3, 0] == 1 and open_.rig_count == out.rig_count - 1


def test_a_nan_centre_seeds_alone():
    case, _j, _v = _two_views()
    case.xyz_mm[0, 4, 1] = np.nan
    out = _run(case)
    assert out.rig_count == 2 and out.rig_hand.tolist() == [[0], [1]] and out.rig_views.tolist() == [1, 1]
    case, _j, _v = _two_views()
    case.xyz_mm[1, 0, 0] = np.nan                     # (the later slot: it joins nothing and seeds its own rig hand)
    out = _run(case)
    assert out.rig_count == 2 and out.rig_hand.tolist() == [[0], [1]]


def test_nothing_lifted_gives_zero_outputs():
    case = rc.random_case(3, 2, 7, seed=1)
    case.lifted[:] = 0
    case.has_hand[case.has_hand == 1] = 0
    out = _run(case)
    assert out.rig_count == 0 and (out.rig_hand == -1).all() and (out.rig_seed == -1).all() and not out.rig_views.any()
    for name in ("rig_xyz", "rig_mesh", "fused_xyz", "fused_mesh"):
        assert not _bits(getattr(out, name)).any(), name


def test_the_random_rigs_fuse_across_cameras():
    """a condition on the GPU test's inputs (rig_cases.SHAPES with their seeds): the one-slot rig holds a lifted hand; every
    rig of three and more cameras holds a rig hand of at least three cameras, two rig hands or more and a slot without a hand;
    the 16-slot rigs also hold a hand that was not lifted, a NaN row (has_hand 2) and an empty slot; the rig hands of a handed
    rig are of one side each (what the gate changes is the edge scene's business)"""
    for n, k, v in rc.SHAPES:
        for handed in (False, True):
            case = rc.random_case(n, k, v, rc.SEEDS[n, k, v], handed=handed)
            out = _run(case)
            if n == 1:
                assert case.lifted.tolist() == [1] and out.rig_count == 1
                continue
            assert out.rig_views.max() >= 3 and out.rig_count >= 2 and (case.has_hand != 1).any()
            if k == 16:
                assert ((case.has_hand == 1) & (case.lifted == 0)).any() and (case.has_hand == 2).any() and (case.has_hand == 0).any()
            if handed:
                for g in range(out.rig_count):
                    assert len({int(s) for s in case.side[out.rig_hand.reshape(-1) == g]}) == 1


# --------------------------------------------------------------------------------------------------------------- layout
COMBOS = [(1, 1, 5, None, {}), (3, 2, 5, (5, 7), dict(overlay=True, labels=True, handed=True)),
          (2, 3, 778, (48, 64), dict(overlay=True, tracked=True, smoothed=True, occluded=True)),
          (7, 5, 13, (5, 7), dict(labels=True, tracked=True)), (16, 16, 778, None, dict(handed=True, tracked=True, smoothed=True))]


@pytest.mark.parametrize("n,k,v,hw,opts", COMBOS)
def test_rig_layout_appends_eight_aligned_parts_and_moves_nothing(n, k, v, hw, opts):
    from hn_amd.live import LiveLayout
    plain, rig = LiveLayout(n, k, v, hw, **opts), LiveLayout(n, k, v, hw, **opts, rig=True)
    assert not plain.rig and rig.rig and list(inspect.signature(LiveLayout).parameters)[-1] == "rig"
    names = [f for f in LiveLayout.__dataclass_fields__ if f.endswith("_at") and not f.startswith(("rig_", "fused_"))]
    assert len(names) == 12
    for f in names + ["record_rows", "record_bytes"]:
        assert getattr(plain, f) == getattr(rig, f), f
    s = n * k
    sizes = dict(rig_xyz=s * 21 * 12, rig_mesh=s * v * 12, rig_hand=s * 4, rig_count=4, rig_views=s * 4, rig_seed=s * 4,
                 fused_xyz=s * 21 * 12, fused_mesh=s * v * 12)
    end = plain.nbytes
    for name in RIG_FIELDS:
        at = getattr(rig, name + "_at")
        assert getattr(plain, name + "_at") is None
        assert at % 4 == 0 and end <= at < end + 4, name
        end = at + sizes[name]
    assert end == rig.nbytes
    buf = torch.zeros((rig.nbytes,), dtype=torch.uint8)
    pv, rv = plain.views(buf[:plain.nbytes]), rig.views(buf)
    assert rv._fields == pv._fields + RIG_FIELDS and type(rv).__name__.endswith("RigViews")
    for name in pv._fields:
        a, b = getattr(pv, name), getattr(rv, name)
        assert (a is None) == (b is None)
        if a is not None:
            assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype
    shapes = dict(rig_xyz=(s, 21, 3), rig_mesh=(s, v, 3), rig_hand=(s,), rig_count=(1,), rig_views=(s,), rig_seed=(s,),
                  fused_xyz=(s, 21, 3), fused_mesh=(s, v, 3))
    for name in RIG_FIELDS:
        t = getattr(rv, name)
        assert t.data_ptr() - buf.data_ptr() == getattr(rig, name + "_at") and tuple(t.shape) == shapes[name]
        assert t.dtype == (torch.float32 if name.endswith(("xyz", "mesh")) else torch.int32)


def test_rig_layout_refusals():
    from hn_amd.live import LiveLayout
    with pytest.raises(ValueError, match="K-hand"):
        LiveLayout(2, None, 778, rig=True)
    with pytest.raises(ValueError, match="256"):
        LiveLayout(257, 1, 778, rig=True)
    with pytest.raises(ValueError, match="256"):
        LiveLayout(17, 16, 778, rig=True)
    assert LiveLayout(16, 16, 778, rig=True).slots == 256 and LiveLayout(257, 1, 778).slots == 257


def test_read_appends_the_eight_fields_behind_every_other_field():
    from hn_amd.live import LiveHandsOutput, LiveLayout
    n, k, v, hw = 2, 3, 5, (5, 7)
    g = torch.Generator().manual_seed(4)
    for opts in (dict(), dict(overlay=True, handed=True, tracked=True, smoothed=True, occluded=True)):
        plain, rig = LiveLayout(n, k, v, hw, **opts), LiveLayout(n, k, v, hw, **opts, rig=True)
        host = torch.randint(0, 256, (rig.nbytes,), generator=g, dtype=torch.uint8)
        host[:plain.mesh_at] = 0
        r = LiveHandsOutput(None, None, None, None, None, host, n, k, layout=rig).read()
        p = LiveHandsOutput(None, None, None, None, None, host[:plain.nbytes], n, k, layout=plain).read()
        assert r._fields == p._fields + RIG_FIELDS and type(r).__name__ == type(p).__name__.replace("Read", "RigRead")
        for a, b in zip(r[:len(p)], p):
            assert torch.equal(a, b) if torch.is_tensor(a) else a == b
        v_ = rig.views(host)
        assert type(r.rig_count) is int and r.rig_count == int(v_.rig_count[0])
        assert tuple(r.rig_xyz.shape) == (n, k, 21, 3) and tuple(r.rig_mesh.shape) == (n, k, v, 3)
        assert tuple(r.rig_hand.shape) == (n, k) and r.rig_hand.dtype == torch.int32
        assert tuple(r.rig_views.shape) == tuple(r.rig_seed.shape) == (n * k,)
        assert tuple(r.fused_xyz.shape) == (n * k, 21, 3) and tuple(r.fused_mesh.shape) == (n * k, v, 3)
        for name in RIG_FIELDS:
            if name != "rig_count":
                got = getattr(r, name)
                assert torch.equal(got.reshape(-1).view(torch.uint8), getattr(v_, name).reshape(-1).view(torch.uint8)), name
                assert got.data_ptr() != getattr(v_, name).data_ptr()


# ---------------------------------------------------------------------------------------------------------- host checks
def test_rig_extrinsics_checks_and_rounds():
    from hn_amd import ops
    e = rc.extrinsics(3, seed=9)
    four = np.concatenate([e, np.tile([[[0.0, 0.0, 0.0, 1.0]]], (3, 1, 1))], axis=1)
    for form in (e, e.tolist(), torch.from_numpy(e), four, torch.from_numpy(four).float()):
        t = ops.rig_extrinsics(form, 3)
        assert t.dtype == np.float32 and t.shape == (3, 12) and t.flags.c_contiguous
    assert np.array_equal(ops.rig_extrinsics(e, 3), rr.table(e)) and np.array_equal(ops.rig_extrinsics(four), rr.table(e))
    assert np.array_equal(ops.rig_extrinsics(e.astype(np.float32)), rr.table(e))         # an fp32-rounded rotation passes
    bad_row = four.copy()
    bad_row[1, 3] = (0, 0, 0, 2)
    bad_row2 = four.copy()
    bad_row2[2, 3, 0] = 1e-9
    scaled, mirrored, sheared, nan, inf, huge = (e.copy() for _ in range(6))
    scaled[1, :, :3] *= 1.001
    mirrored[2, :, 0] *= -1
    sheared[0, 0, 1] += 1e-3
    nan[0, 1, 3], inf[1, 0, 0], huge[2, 2, 3] = np.nan, np.inf, 1e39
    for bad in (e[0], e[:, :2], e[:, :, :3], e[:0], np.zeros((3, 5, 4)), np.zeros((3, 4, 3)), "no", bad_row, bad_row2, scaled, mirrored,
                sheared, nan, inf, huge, np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match="extrinsics"):
            ops.rig_extrinsics(bad)
    for frames in (2, 4):
        with pytest.raises(ValueError, match=f"N = {frames}"):
            ops.rig_extrinsics(e, frames)


def test_rig_radius_and_slots():
    from hn_amd import ops
    assert ops.RIG_RADIUS == 0.08 == rr.RIG_RADIUS and ops.RIG_MAX_SLOTS == 256 == rr.MAX_SLOTS and ops.RIG_FIELDS == rr.RigFused._fields
    assert ops.check_rig_radius(0.08) == 0.08 and ops.check_rig_radius(1) == 1.0
    for bad in (0, -0.1, float("nan"), float("inf"), -float("inf"), 1e39, 1e-50, "wide", None):
        with pytest.raises(ValueError, match="rig_radius"):
            ops.check_rig_radius(bad)
    assert ops.check_rig_slots(16, 16) == 256 and ops.check_rig_slots(256, 1) == 256
    for n, k in ((257, 1), (1, 257), (17, 16), (0, 2)):
        with pytest.raises(ValueError, match="256 slots"):
            ops.check_rig_slots(n, k)
    d = {k: p.default for k, p in inspect.signature(ops.rig_fuse).parameters.items()}
    assert list(d) == ["xyz_mm", "mesh", "has_hand", "lifted", "score", "extrinsics_table", "k", "radius", "side", "out"]
    assert (d["radius"], d["side"], d["out"]) == (0.08, None, None)


class _Hand:
    device = "cpu"

    def set_convert(self, **kw):
        pass


class _Graph:
    v = 1280


class _Lifter:
    device = "cpu"
    graphs = [_Graph()]


def test_the_engine_refuses_what_the_rig_cannot_do():
    """before anything touches a device: the constructor's refusals, the table, set_extrinsics and the frame count"""
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    for fn in (HandNet.live_hands, LiveHandsEngine.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["extrinsics"].default is None and sig["rig_radius"].default == 0.08
    for fn in (HandNet.live, LiveHandEngine.__init__):
        assert "extrinsics" not in inspect.signature(fn).parameters
    assert "NOT tuned" in LiveHandsEngine.__init__.__doc__.split("rig_radius = 0.08")[1][:60]
    assert "NOT tuned" in HandNet.live_hands.__doc__.split("rig_radius = 0.08")[1][:60]
    paras, perm, ext = (600.0, 600.0, 320.0, 240.0), np.arange(778), rc.extrinsics(2, seed=1)
    make = lambda *a, **kw: LiveHandsEngine(_Hand(), _Lifter(), *a, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="perm_reverse"):
        make(paras, 2, extrinsics=ext)
    with pytest.raises(ValueError, match="paras"):
        make(None, 2, True, perm, extrinsics=ext)
    with pytest.raises(ValueError, match="left=True"):
        make(paras, 2, True, perm, left=True, extrinsics=ext)
    with pytest.raises(ValueError, match="256 slots"):
        make(paras, 16, True, perm, extrinsics=rc.extrinsics(17, seed=1))
    with pytest.raises(ValueError, match="rig_radius"):
        make(paras, 2, True, perm, extrinsics=ext, rig_radius=0.0)
    with pytest.raises(ValueError, match="extrinsics"):
        make(paras, 2, True, perm, extrinsics=ext * 1.01)
    eng = make(paras, 2, True, perm, handed=True, extrinsics=ext, rig_radius=0.1)
    assert eng.rig == 0.1 and eng.extrinsics.dtype == torch.float32 and tuple(eng.extrinsics.shape) == (2, 12)
    assert np.array_equal(eng.extrinsics.numpy(), rr.table(ext))
    assert eng._layout(2).rig and eng._layout(2, None).fused_mesh_at is not None and eng._key_options()[-2:] == ("rig", 0.1)
    eng._check_frames(2)
    with pytest.raises(ValueError, match="3 frames"):
        eng._check_frames(3)
    table = eng.extrinsics
    new = rc.extrinsics(2, seed=77)
    assert eng.set_extrinsics(new) is eng and eng.extrinsics is table and np.array_equal(table.numpy(), rr.table(new))
    for bad in (new[:1], rc.extrinsics(3, seed=1), new * 2.0):
        with pytest.raises(ValueError, match="extrinsics"):
            eng.set_extrinsics(bad)
    assert np.array_equal(table.numpy(), rr.table(new))
    plain = make(paras, 2, True, perm)
    assert plain.rig is None and plain.extrinsics is None and not plain._layout(2).rig and plain._key_options() == ()
    with pytest.raises(ValueError, match="built with extrinsics"):
        plain.set_extrinsics(new)


def test_extrinsics_count_against_a_camera_per_frame():
    from test_cams_cpu import _stub_engines
    from hn_amd.live import LiveHandsEngine
    cams = np.array([[617.343, 617.343, 312.42, 241.42], [580.1, 600.7, 290.3, 260.9]])
    hand, lifter = _stub_engines()
    with pytest.raises(ValueError, match="3 extrinsics"):
        LiveHandsEngine(hand, lifter, cams, 2, perm_reverse=np.arange(778), extrinsics=rc.extrinsics(3, seed=1))
    hand, lifter = _stub_engines()
    eng = LiveHandsEngine(hand, lifter, cams, 2, perm_reverse=np.arange(778), extrinsics=rc.extrinsics(2, seed=1))
    assert eng._layout(2).rig and tuple(eng.cams.shape) == (2, 4)


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_is_declared_exported_and_bound():
    from hn_amd import _lib, build
    build.build_library()
    name = "hn_rig_fuse_f32"
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert proto and name in _lib.SIGNATURES
    params = [p.strip() for p in proto.group(1).split(",")]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(params) == len(args) == 21
    for p, a in zip(params, args):
        if "*" in p:
            assert a is C.c_void_p, p
        elif p.startswith("float"):
            assert a is C.c_float, p
        else:
            assert p.startswith("int ") and a is C.c_int, p
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s\b" % name, out)
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION                  # a function added, no struct touched
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["rig_ops.hip"]


def test_the_entry_checks_its_sizes_before_any_launch():
    """no GPU here: every refusal comes back as HN_ERR_ARG with a message, before the device is touched"""
    from hn_amd import _lib
    lib = _lib.load()
    P = 4096        # stands for a device address

    def call(n=2, k=2, joints=21, v=778, radius=0.08, **null):
        ptrs = {name: P for name in ("xyz_mm", "mesh", "has_hand", "lifted", "score", "side", "ext") + RIG_FIELDS}
        ptrs.update(null)
        ins = [ptrs[x] for x in ("xyz_mm", "mesh", "has_hand", "lifted", "score", "side", "ext")]
        return lib.hn_rig_fuse_f32(*ins, n, k, joints, v, radius, *(ptrs[x] for x in RIG_FIELDS), None)
    for kw, word in ((dict(n=257, k=1), b"at most 256"), (dict(n=17, k=16), b"at most 256"), (dict(n=1 << 20, k=1 << 20), b"at most 256"),
                     (dict(n=-1), b"positive"), (dict(k=-2), b"positive"), (dict(n=0), b"positive"), (dict(joints=-21), b"positive"),
                     (dict(v=-778), b"positive"), (dict(v=0), b"positive"), (dict(radius=0.0), b"radius"),
                     (dict(radius=float("nan")), b"radius"), (dict(radius=float("inf")), b"radius"), (dict(xyz_mm=None), b"null pointer"),
                     (dict(ext=None), b"null pointer"), (dict(fused_mesh=None), b"null pointer"), (dict(rig_count=None), b"null pointer")):
        assert call(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_rig_fuse_f32: ") and word in err, (kw, err)
