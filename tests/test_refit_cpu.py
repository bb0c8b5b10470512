"""The iterated depth fit without a GPU: the numpy rule (tests/refit_ref.py) against the float64 raster and
against what it must recover, the invariants of the chain, what the GPU cases offer, and every host-side surface -- layout,
read(), keywords, refusals, scratch sizes, the C entries."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest
import torch

import fit_cases as fc
import fit_ref as fr
import raster_ref as rr
import refit_cases as rc
import refit_ref as rf

F = np.float32
DEPTH_REL_BOUND = 8.4e-7      # tests/test_render_gpu.py's fp32-against-float64 depth bound (occlude_ref.THRESHOLD_REL)
FIT_FIELDS = ("fit_mesh", "fit_xyz", "fit_rt", "fit_count", "fit_cost")


# ------------------------------------------------------------------------------------------------------------- the geometry
@pytest.mark.parametrize("name", list(rr.scenes()))
def test_geometry_against_the_float64_raster(name):
    """on raster_ref.scenes(): the coverage equals raster_ref.rasterize exactly, the fp32 depth lies within the existing bound
    outside depth fights, and the slot byte names the nearest face's slot there"""
    meshes, faces, lifted, paras, (h, w) = rr.scenes()[name]
    worst, covered_all = 0.0, 0
    for i in range(meshes.shape[0]):
        lif = None if lifted is None else lifted[i]
        depth, who = rf.geometry(meshes[i], faces, paras, h, w, lif)
        ras, _colours = rr.rasterize(meshes[i], faces, paras, h, w, lif)
        covered = ras.face >= 0
        assert depth.dtype == F and who.dtype == np.uint8 and depth.shape == who.shape == (h, w)
        assert np.array_equal(who != 0, covered) and np.array_equal(depth > 0, covered), (name, i)
        assert not depth[~covered].any()
        clear = covered & ~rr.ambiguous(ras)
        if clear.any():
            worst = max(worst, float(np.max(np.abs(depth[clear] - ras.z1[clear]) / ras.z1[clear])))
            assert np.array_equal(who[clear], ras.face[clear] // len(faces) + 1), (name, i)
        covered_all += int(covered.sum())
    print(f"{name}: {covered_all} covered pixels, depth off by {worst:.3e} relative (bound {DEPTH_REL_BOUND:.1e})")
    assert covered_all > 0 and worst <= DEPTH_REL_BOUND


def test_geometry_keeps_the_lower_slot_and_face_on_an_exact_tie():
    """two slots with the same mesh: slot 0 keeps every pixel; a duplicated face changes nothing"""
    mesh, faces = rr.ellipsoid((0.0, 0.0, 0.5), (0.05, 0.08, 0.03), rings=7, segs=9)
    paras, (h, w) = (123.0, 123.0, 32.0, 24.0), (48, 64)
    d1, w1 = rf.geometry(mesh[None], faces, paras, h, w)
    d2, w2 = rf.geometry(np.stack([mesh, mesh]), np.concatenate([faces, faces[:9]]), paras, h, w)
    assert d1.tobytes() == d2.tobytes() and w1.tobytes() == w2.tobytes() and set(np.unique(w2)) == {0, 1}
    d3, w3 = rf.geometry(np.stack([mesh, mesh]), faces, paras, h, w, lifted=[0, 1])
    assert d3.tobytes() == d1.tobytes() and set(np.unique(w3)) == {0, 2}


# ------------------------------------------------------------------------------------------------------------- the recovery
def recovery(seed, iters=4, thick=False):
    """test_fit_cpu.recovery's setup iterated: the moved ellipsoid is ray-cast again analytically before every step.  -> the RMS
    distance of the matched points to the measured surface before, and after each step (metres)"""
    rng = np.random.default_rng(seed)
    h, w, paras = 240, 320, (288.0, 288.0, 160.0, 120.0)
    z = rng.uniform(0.4, 0.7)
    centre = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.04, 0.04), z])
    axes = np.array([0.09, 0.045, 0.03 if thick else 0.015])
    pose = fc.rotation(rng, rng.uniform(0, 0.6))
    root = centre + np.array([0.0, 0.07, 0.0])
    turn = fc.rotation(rng, rng.uniform(0, 0.12))
    shift = rng.normal(size=3)
    shift *= rng.uniform(0, 0.02) / np.linalg.norm(shift)
    if thick:      # (turned about the root, 7 cm away)
        q1, moved = fc.quadric(axes, turn @ pose), turn @ (centre - root) + root + shift
    else:
        q1, moved = fc.quadric(axes, turn @ pose), centre + shift
    depth = fc.ray_cast(h, w, paras, moved, q1)
    depth = np.where(np.isnan(depth), 2.0, depth + rng.normal(0, 0.001, (h, w))).astype(F)
    rms = lambda pts: float(np.sqrt(np.mean(fc.surface_distance(pts, moved, q1) ** 2)))  # noqa: E731
    out = []
    cur_r, cur_c, cur_root = np.eye(3), centre.copy(), root.copy()       # the mesh ellipsoid's pose, centre and root now
    for t in range(iters):
        zs = fc.ray_cast(h, w, paras, cur_c, fc.quadric(axes, cur_r @ pose))
        hit = ~np.isnan(zs)
        best, sil = np.where(hit, zs, 0).astype(F), hit.astype(np.uint8)
        xyz = np.zeros((1, 21, 3), F)
        xyz[0] = (cur_root * 1000).astype(F)
        got = fr.mesh_fit(best[None], sil[None], depth[None], paras, np.zeros((1, 4, 3), F), xyz, 1)
        assert got.count[0, 1] == 0 and got.count[0, 0] >= fr.FIT_MIN_POINTS, (seed, t, got.count)
        rows, cols, _t = fr.terms(best, sil, depth, paras, xyz[0, 0], 0)
        p = np.stack(fr.point(rows, cols, best[rows, cols], paras), axis=-1).astype(np.float64)
        rt, c0 = got.rt[0].astype(np.float64), (xyz[0, 0] / F(1000)).astype(np.float64)
        rot, tr = rt[:9].reshape(3, 3), rt[9:]
        if t == 0:
            out.append(rms(p))
        out.append(rms((p - c0) @ rot.T + c0 + tr))
        cur_c, cur_root, cur_r = rot @ (cur_c - c0) + c0 + tr, rot @ (cur_root - c0) + c0 + tr, rot @ cur_r
    return out


@pytest.mark.parametrize("seed", range(8))
def test_three_steps_come_closer_than_one(seed):
    """the analytic recovery: RMS after three iterations <= RMS after one / 1.5 (measured 2.0 x to 4.7 x; seed 2 sits at the
    1 mm noise's floor after one step, hence the margin), and below the starting RMS after every iteration"""
    got = recovery(seed)
    print(f"seed {seed}: RMS distance to the measured surface (mm) before {1000 * got[0]:.2f}, after steps 1..4 "
          + " ".join(f"{1000 * v:.2f}" for v in got[1:]) + f" (three steps: {got[1] / got[3]:.1f} x closer than one)")
    assert got[3] <= got[1] / 1.5
    assert all(v < got[0] for v in got[1:])


@pytest.mark.parametrize("seed", (0, 4, 5))
def test_a_thick_body_about_a_far_pivot(seed):
    """DESIGN.md 9k's hard case -- 3 cm thick, turned about the root 7 cm away --: printed, and three steps no worse than one"""
    got = recovery(seed, thick=True)
    print(f"seed {seed}: thick body, RMS (mm) before {1000 * got[0]:.2f}, after steps 1..4 " + " ".join(f"{1000 * v:.2f}" for v in got[1:]))
    assert got[3] <= got[1] and all(v < got[0] for v in got[1:])


@pytest.mark.parametrize("seed", range(4))
def test_recovery_through_the_mesh_chain(seed):
    """refit_ref.mesh_fit_iters on a tessellated ellipsoid through the fp32 raster rule, stride 1, four iterations: the RMS
    distance of ALL vertices to the measured surface after four iterations is at most half of that after one (measured 3.9 x
    to 7 x), every iteration has status 0 and at least 200 matches"""
    c = rc.chain_case(seed)
    states = []
    out = rf.mesh_fit_iters(c.best, c.sil, c.depth, c.paras, c.mesh, c.xyz_mm, c.faces, 1, 4, stride=1, states=states)
    centre, q = c.truth[0]
    rms = lambda m: float(np.sqrt(np.mean(fc.surface_distance(m.astype(np.float64) * [1, -1, -1], centre, q) ** 2)))  # noqa: E731
    got = [rms(c.mesh[0])] + [rms(s.mesh[0]) for s in states]
    rho = [float(np.sqrt(cost / 2.0 ** 30 / max(1, m))) for m, _s, cost in out.trace[0].tolist()]
    print(f"seed {seed}: all-vertex RMS (mm) before {1000 * got[0]:.2f}, after steps 1..4 " + " ".join(f"{1000 * v:.2f}" for v in got[1:])
          + f"; matches {out.trace[0, :, 0].tolist()}; RMS residual along the normals (mm) " + " ".join(f"{1000 * v:.2f}" for v in rho))
    assert (out.trace[0, :, 1] == 0).all() and (out.trace[0, :, 0] >= 200).all()
    assert got[4] <= got[1] / 2.0
    assert out.mesh.tobytes() == states[-1].mesh.tobytes() and out.xyz.tobytes() == states[-1].xyz.tobytes()
    assert out.count.tobytes() == states[0].count.tobytes() and out.cost.tobytes() == states[0].cost.tobytes()


# ------------------------------------------------------------------------------------------------- the chain's invariants
def test_one_iteration_is_the_single_fit_byte_for_byte():
    shape = fc.SHAPES[2]
    c = fc.case(*shape)
    want, _census = fc.expected(*shape)
    faces = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    got = rf.mesh_fit_iters(c.best, c.sil, c.depth, c.paras, c.meshes[778], c.xyz_mm, faces, c.k, 1, **fc.kwargs(c))
    assert (want.count[:, 1] == 0).any() and (want.count[:, 1] != 0).any()
    for name in fr.MeshFit._fields:
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
    assert got.trace.dtype == np.int64 and got.trace.shape == (c.n * c.k, 1, 3)
    assert np.array_equal(got.trace[:, 0, :2], want.count) and np.array_equal(got.trace[:, 0, 2], want.cost)


@pytest.mark.parametrize("shape", rc.SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_the_composed_motion_reproduces_the_fitted_mesh(shape):
    """fit_rt applied in fp64 to the ORIGINAL mesh and joints reproduces fit_mesh / fit_xyz within 1e-5 m: at most 8 fp32
    roundings per iteration (2^-24 relative each) on coordinates below 2 m, 8 iterations -> 8 * 8 * 2 * 2^-24 = 7.6e-6"""
    c, want = rc.case(*shape), rc.expected(*shape)
    worst = 0.0
    for s in range(c.n * c.k):
        status = want.trace[s, :, 1]
        rt = want.rt[s].astype(np.float64)
        if (status != 0).all():
            assert want.rt[s].tobytes() == np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F).tobytes()
            assert want.mesh[s].tobytes() == c.mesh[s].tobytes() and want.xyz[s].tobytes() == c.xyz_mm[s].tobytes()
            continue
        rot = rt[:9].reshape(3, 3)
        assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-6
        c0 = (c.xyz_mm[s, 0] / F(1000)).astype(np.float64)
        cam = c.mesh[s].astype(np.float64) * [1, -1, -1]
        moved = ((cam - c0) @ rot.T + c0 + rt[9:]) * [1, -1, -1]
        joints = (c.xyz_mm[s].astype(np.float64) / 1000 - c0) @ rot.T + c0 + rt[9:]
        worst = max(worst, np.abs(moved - want.mesh[s]).max(), np.abs(joints - want.xyz[s].astype(np.float64) / 1000).max())
    print(f"{shape}: the composed motion misses the fitted mesh by at most {worst:.3e} m")
    assert worst <= 1e-5


def test_a_slot_that_is_never_fitted_keeps_its_bytes():
    """NaN, -0 and inf in a slot no iteration fits come out as they went in; the identity motion; the trace says why"""
    c = rc.case(*rc.SHAPES[1])
    mesh, xyz = c.mesh.copy(), c.xyz_mm.copy()
    s = c.n * c.k - 1                                                     # the unlifted slot
    mesh[s, :3] = (F(-0.0), F(np.nan), F(np.inf))
    xyz[s, 5] = (F(np.nan), F(-0.0), F(1.5))
    got = rf.mesh_fit_iters(c.best, c.sil, c.depth, c.paras, mesh, xyz, c.faces, c.k, 3, lifted=c.lifted, **rc.kwargs(c))
    assert got.mesh[s].tobytes() == mesh[s].tobytes() and got.xyz[s].tobytes() == xyz[s].tobytes()
    assert got.rt[s].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and (got.trace[s, :, 1] == 1).all()
    assert got.mesh[0].tobytes() != mesh[0].tobytes()


def test_a_failed_iteration_is_tried_again():
    """a cap that refuses the first, large step only: iteration 1 has status 3 and leaves the bytes, and the composition takes
    the later motions alone"""
    c = rc.chain_case(0)
    states = []
    kw = dict(stride=1, states=states)
    free = rf.mesh_fit_iters(c.best, c.sil, c.depth, c.paras, c.mesh, c.xyz_mm, c.faces, 1, 2, **kw)
    step1 = float(np.linalg.norm(states[0].rt[0, 9:]))
    states.clear()
    capped = rf.mesh_fit_iters(c.best, c.sil, c.depth, c.paras, c.mesh, c.xyz_mm, c.faces, 1, 2, max_shift=step1 / 2, **kw)
    assert free.trace[0, :, 1].tolist() == [0, 0] and capped.trace[0, :, 1].tolist() == [3, 3]
    assert capped.mesh.tobytes() == c.mesh.tobytes() and np.array_equal(capped.trace[0, 0], capped.trace[0, 1])
    # the composition skips what was refused: (status 3, anything) then one motion is that motion
    one = states[0].rt[0]
    assert rf.compose(c.xyz_mm[0, 0] / F(1000), [(3, one * 0, c.xyz_mm[0, 0] / F(1000)), (0, one, c.xyz_mm[0, 0] / F(1000))]).tobytes() \
        == one.tobytes()


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_gpu_cases_offer_what_they_must(shape):
    """the conditions test_refit_gpu.py checks before it compares, here on the reference alone: a slot with status 0 in every
    iteration in every case; an unlifted slot in every case of two slots or more; a lifted slot with a non-zero status in some
    iteration in every case of three slots or more (a step of one slot cannot hold all three)"""
    c, want = rc.case(*shape), rc.expected(*shape)
    rc.check_conditions(c, want)
    assert c.faces.shape[0] == (126 if c.h < 64 or c.k == 16 else 1550)
    assert (~fr.valid_depth(c.depth)).sum() >= c.depth.size // 40       # holes
    if c.k > 1:
        assert len(set(np.unique(c.sil)) - {0}) >= 2 or c.k == 2            # more than one slot drawn (K = 2: one is unlifted)


# -------------------------------------------------------------------------------------------------------------------- layout
COMBOS = [(1, 1, 5, (5, 7), {}), (3, 2, 5, (5, 7), dict(labels=True, handed=True)),
          (2, 3, 778, (48, 64), dict(tracked=True, smoothed=True)), (16, 16, 778, (33, 65), dict(handed=True, tracked=True))]


@pytest.mark.parametrize("rig", (False, True))
@pytest.mark.parametrize("cloud", (0, 7))
@pytest.mark.parametrize("n, k, v, hw, opts", COMBOS)
def test_layout_appends_the_trace_and_moves_nothing(n, k, v, hw, opts, cloud, rig):
    from hn_amd.live import LiveLayout
    for hands in (k, None):
        if hands is None and (opts or rig):
            continue
        if rig and n * k > 256:
            continue
        kw = dict(hw=hw, overlay=True, occluded=True, cloud=cloud, rig=rig, **(opts if hands else {}))
        one = LiveLayout(n, hands, v, fit=True, **kw)
        assert one.fit is True and one.fit_iters == 1 and one.fit_trace_at is None and "fit_trace" not in one.views(torch.zeros(one.nbytes, dtype=torch.uint8))._fields
        s = one.slots
        for iters in (2, 5, 8):
            lay = LiveLayout(n, hands, v, fit=iters, **kw)
            assert lay.fit == iters and lay.fit_iters == iters
            at = lay.fit_trace_at
            assert at % 8 == 0 and at == (one.nbytes + 7) // 8 * 8 and lay.nbytes == at + s * iters * 3 * 8
            for name in FIT_FIELDS + ("cloud", "cloud_count", "cloud_resid"):
                assert getattr(lay, name + "_at") == getattr(one, name + "_at"), name
            for name in LiveLayout.__dataclass_fields__:
                if name not in ("fit", "nbytes"):
                    assert getattr(lay, name) == getattr(one, name), name
            buf = torch.arange(lay.nbytes, dtype=torch.int64).to(torch.uint8)
            v1, vi = one.views(buf[:one.nbytes]), lay.views(buf)
            assert vi._fields == v1._fields + ("fit_trace",) and type(vi).__name__.endswith("TraceViews")
            assert vi.fit_trace.dtype == torch.int64 and tuple(vi.fit_trace.shape) == (s, iters, 3)
            assert vi.fit_trace.data_ptr() == buf.data_ptr() + at
            for name in v1._fields:
                a, b = getattr(v1, name), getattr(vi, name)
                assert (a is None and b is None) or (a.data_ptr() == b.data_ptr() and a.shape == b.shape), name
    assert not any(f.startswith("fit_") for f in LiveLayout.__dataclass_fields__)
    assert list(LiveLayout.__dataclass_fields__)[10:13] == ["fit", "cloud", "rig"]


def test_layout_refusals():
    from hn_amd.live import LiveLayout
    kw = dict(hw=(5, 7), overlay=True, occluded=True)
    for bad in (9, -1, 2.0, "3", 100):
        with pytest.raises(ValueError, match="fit"):
            LiveLayout(1, 2, 5, fit=bad, **kw)
    with pytest.raises(ValueError, match="occluded"):
        LiveLayout(1, 2, 5, hw=(5, 7), overlay=True, fit=3)
    assert LiveLayout(1, 2, 5, fit=False, **kw).fit_iters == 0 and LiveLayout(1, 2, 5, **kw).fit_trace_at is None


def test_read_appends_the_trace_behind_fit_cost():
    from hn_amd.live import LiveHandsOutput, LiveLayout, LiveOutput
    n, k, v, iters = 2, 3, 5, 4
    for cloud in (0, 6):
        lay = LiveLayout(n, k, v, hw=(5, 7), overlay=True, occluded=True, cloud=cloud, fit=iters)
        one = LiveLayout(n, k, v, hw=(5, 7), overlay=True, occluded=True, cloud=cloud, fit=True)
        host = torch.zeros(lay.nbytes, dtype=torch.uint8)
        trace = torch.arange(n * k * iters * 3, dtype=torch.int64).view(n * k, iters, 3) - 7
        lay.views(host).fit_trace.copy_(trace)
        out = LiveHandsOutput(hands=None, pose2d=None, lifted=None, mesh=None, pose3d=None, host=host, n=n, k=k, layout=lay)
        r = out.read()
        p = LiveHandsOutput(hands=None, pose2d=None, lifted=None, mesh=None, pose3d=None, host=host[:one.nbytes].clone(), n=n, k=k,
                            layout=one).read()
        assert r._fields == p._fields + ("fit_trace",) and r._fields[-2] == "fit_cost"
        assert type(r).__name__ == type(p).__name__[:-4] + "TraceRead" and type(p).__name__.endswith("FitRead")
        assert r.fit_trace.dtype == torch.int64 and tuple(r.fit_trace.shape) == (n, k, iters, 3)
        assert torch.equal(r.fit_trace, trace.view(n, k, iters, 3)) and r.fit_trace.data_ptr() != host.data_ptr()
        assert "fit_trace" in type(r).__doc__
    lay1 = LiveLayout(n, None, v, hw=(5, 7), overlay=True, occluded=True, fit=iters)
    host = torch.zeros(lay1.nbytes, dtype=torch.uint8)
    lay1.views(host).fit_trace.fill_(3)
    r1 = LiveOutput(hand=None, pose2d=None, mesh=None, pose3d=None, host=host, n=n, layout=lay1).read()
    assert r1._fields[-6:] == FIT_FIELDS + ("fit_trace",) and type(r1).__name__ == "LiveOverlayOccludedFitTraceRead"
    assert tuple(r1.fit_trace.shape) == (n, iters, 3) and bool((r1.fit_trace == 3).all())
    for cls in (LiveOutput, LiveHandsOutput):
        names = list(cls.__dataclass_fields__)
        assert names[names.index("fit_cost") + 1] == "fit_trace" and cls.__dataclass_fields__["fit_trace"].default is None


# --------------------------------------------------------------------------------------------------------------- the surfaces
def test_the_surfaces():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import ops
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    assert ops.FIT_MAX_ITERS == rf.MAX_ITERS == 8
    assert ops.MeshFitIters._fields == ("mesh", "xyz", "rt", "count", "cost", "trace") == rf.MeshFitIters._fields
    sig = inspect.signature(ops.mesh_fit_iters).parameters
    assert list(sig) == ["mesh_depth", "silhouette", "scene_depth", "paras", "mesh", "xyz_mm", "faces", "k", "iters", "lifted", "band",
                         "stride", "min_points", "damp", "max_shift", "max_angle", "out", "scratch", "work"]
    assert all(sig[name].kind is inspect.Parameter.KEYWORD_ONLY for name in list(sig)[8:]) and sig["iters"].default is inspect.Parameter.empty
    assert [sig[n].default for n in ("band", "stride", "min_points", "damp", "max_shift", "max_angle")] == [0.03, 2, 200, 1e-3, 0.05, 0.35]
    sig = inspect.signature(ops.mesh_geometry).parameters
    assert list(sig) == ["mesh", "faces", "paras", "hw", "lifted", "k", "out_depth", "out_who", "scratch"]
    assert all(sig[name].kind is inspect.Parameter.KEYWORD_ONLY for name in ("out_depth", "out_who", "scratch"))
    assert sig["lifted"].default is None and sig["k"].default == 1
    for fn in (HandNet.live, HandNet.live_hands, LiveHandEngine.__init__, LiveHandsEngine.__init__):
        params = inspect.signature(fn).parameters
        names = list(params)
        at = names.index("fit_iters")
        assert names[at:at + 3] == ["fit_iters", "fit_draw", "cloud"], fn.__qualname__       # directly in front of `cloud`
        assert params["fit_iters"].default == 1 and params["fit_draw"].default is False
        assert names[at - 1] in ("occlude_margin", "rig_radius")
    for doc in (LiveHandEngine.__doc__, LiveHandsEngine.__init__.__doc__, HandNet.live.__doc__, HandNet.live_hands.__doc__):
        assert "fit_iters" in doc and "fit_draw" in doc and "9l" in doc
    assert "DESIGN.md section 9l" in ops.mesh_fit_iters.__doc__ and "DESIGN.md section 9l" in ops.mesh_geometry.__doc__


def test_check_fit_iters():
    from hn_amd import ops
    assert [ops.check_fit_iters(i) for i in (1, 2, 8, np.int64(3))] == [1, 2, 8, 3]
    for bad in (0, 9, -1, 1.0, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="fit_iters"):
            ops.check_fit_iters(bad)


class _Hand:
    device = "cpu"

    def set_convert(self, **kw):
        pass


class _Graph:
    v = 1280


class _Lifter:
    device = "cpu"
    graphs = [_Graph()]


def test_the_engines_refuse_and_key():
    """before anything touches a device"""
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    paras, perm, faces = (600.0, 600.0, 320.0, 240.0), np.arange(778), np.array([[0, 1, 2]])
    hands = lambda *a, **kw: LiveHandsEngine(_Hand(), _Lifter(), paras, 2, True, *a, **kw)  # noqa: E731
    one = lambda *a, **kw: LiveHandEngine(_Hand(), _Lifter(), paras, True, *a, **kw)  # noqa: E731
    full = dict(faces=faces, occlude=True, fit=True)
    for make in (hands, one):
        for kw in (dict(fit_iters=2), dict(fit_draw=True), dict(fit_iters=3, fit_draw=True)):
            with pytest.raises(ValueError, match="need fit=True"):
                make(perm, **kw)
            with pytest.raises(ValueError, match="need fit=True"):
                make(perm, faces=faces, occlude=True, **kw)
        for bad in (0, 9, 2.0, True, "2", None):
            with pytest.raises(ValueError, match="fit_iters"):
                make(perm, fit_iters=bad, **full)
        for bad in (1, "yes", None):
            with pytest.raises(ValueError, match="fit_draw"):
                make(perm, fit_draw=bad, **full)
        plain = make(perm, **full)
        assert plain.fit_iters == 1 and plain.fit_draw is False and plain._layout(2, (5, 7)).fit is True
        assert plain._key_options() == make(perm, fit_iters=1, fit_draw=False, **full)._key_options()
        assert plain._key_options()[-7:] == ("fit", 0.03, 2, 200, 1e-3, 0.05, 0.35)
        keys = {plain._key_options()}
        for iters, draw in ((3, False), (1, True), (3, True), (4, True)):
            eng = make(perm, fit_iters=iters, fit_draw=draw, **full)
            assert eng._key_options()[-3:] == ("fit_iters", iters, draw) and eng._key_options()[:-3] == plain._key_options()
            lay = eng._layout(2, (5, 7))
            assert lay.fit == (True if iters == 1 else iters) and (lay.fit_trace_at is None) == (iters == 1)
            assert lay.nbytes >= plain._layout(2, (5, 7)).nbytes
            keys.add(eng._key_options())
        assert len(keys) == 5
        off = make(perm)
        assert off.fit is None and off.fit_iters == 1 and off.fit_draw is False and off._key_options() == ()


# --------------------------------------------------------------------------------------------------------------- the C entries
def test_the_entries_are_declared_exported_and_bound():
    from hn_amd import _lib, build
    build.build_library()
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    for name, result, count in (("hn_mesh_geometry_f32", "int", 17), ("hn_mesh_fit_iters_f32", "int", 36),
                                ("hn_mesh_fit_iters_scratch_bytes", "int64_t", 8)):
        proto = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (result, name), text)
        assert proto and name in _lib.SIGNATURES
        params = [p.strip() for p in proto.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is (C.c_int if result == "int" else C.c_int64) and len(params) == len(args) == count, (name, len(params), len(args))
        for p, a in zip(params, args):
            if "*" in p:
                assert a is C.c_void_p or a is _lib.c_f32p, p
            elif p.startswith("float"):
                assert a is C.c_float, p
            elif p.startswith("double"):
                assert a is C.c_double, p
            elif p.startswith("int64_t"):
                assert a is C.c_int64, p
            else:
                assert p.startswith("int ") and a is C.c_int, p
        assert re.search(r" T %s\b" % name, out)
    assert _lib.load().hn_abi_version() == 36 == _lib.ABI_VERSION          # functions added, no struct touched
    assert build.EXTRA_FLAGS["mesh_refit.hip"] == build.EXTRA_FLAGS["mesh_fit.hip"] and "-ffp-contract=off" in build.EXTRA_FLAGS["mesh_refit.hip"]
    rows = (build.CSRC / "build" / "mesh_refit.resources.txt").read_text().splitlines()
    assert len(rows) == 1 and "mesh_refit_compose" in rows[0]
    geo = [r for r in (build.CSRC / "build" / "mesh_raster.resources.txt").read_text().splitlines() if "mesh_geometry_tiles" in r]
    for r in rows + geo:
        assert " vgpr_spill 0 " in r and r.endswith("sgpr_spill 0") and " scratch 0 " in r, r
    assert len(geo) == 1
    raster = (build.CSRC / "mesh_raster.hip").read_text()
    walk = raster.split("void walk_tile(")[1].split("\n}\n")[0]      # (the walk the geometry kernel shares with the raster's)
    assert "on_hit(" in walk and "walk_tile(" in raster.split("mesh_geometry_tiles(")[1]
    src = (build.CSRC / "mesh_refit.hip").read_text() + walk + raster.split("mesh_geometry_tiles(")[1].split("}  // namespace")[0]
    assert "atomic" not in src.replace("No atomic", "")


def test_the_scratch_sizes():
    from hn_amd import _lib
    lib = _lib.load()
    up = lambda b: (b + 15) // 16 * 16  # noqa: E731

    def want(n, k, h, w, v, f, j, i):
        s = n * k
        return (up(s * v * 12) * min(i - 1, 2) + up((i - 1) * s * j * 12) + up(i * s * 48) + up(i * s * 8) + up(i * s * 8)
                + (up(n * h * w * 4) + up(n * h * w) + up(lib.hn_mesh_render_scratch_bytes(s, f)) if i > 1 else 0))
    for args in ((1, 1, 5, 7, 3, 1, 1, 1), (1, 1, 48, 64, 65, 126, 21, 2), (2, 2, 96, 128, 777, 1550, 21, 4), (1, 16, 203, 301, 778, 1538, 21, 8),
                 (32, 2, 480, 640, 778, 1538, 21, 3)):
        assert lib.hn_mesh_fit_iters_scratch_bytes(*args) == want(*args) > 0, args
    good = (2, 2, 48, 64, 778, 1538, 21, 3)
    for at, bad in ((0, 0), (0, 65536), (1, 0), (1, 17), (2, 0), (2, 16385), (3, 0), (3, 16385), (4, 0), (4, 2 ** 24 + 1), (5, 0), (6, 0),
                    (6, 4097), (7, 0), (7, 9), (7, -1)):
        args = list(good)
        args[at] = bad
        assert lib.hn_mesh_fit_iters_scratch_bytes(*args) == 0, args


def test_the_entries_check_their_arguments_before_any_launch():
    """no GPU here: every refusal comes back as HN_ERR_ARG with a message under the entry's own name, before the device is touched"""
    from hn_amd import _lib
    lib = _lib.load()
    P = 4096        # stands for a device address
    host4 = (C.c_float * 4)(600.0, 600.0, 320.0, 240.0)
    nan, inf = float("nan"), float("inf")
    faces_ok = (C.c_int32 * 6)(0, 1, 2, 2, 1, 0)
    faces_bad = (C.c_int32 * 6)(0, 1, 2, 2, 1, 778)

    def geometry(s=4, v=778, f=2, k=2, h=48, w=64, paras=host4, cams=None, scratch_bytes=None, faces_host=None, **ptrs):
        p = dict(mesh=P, faces=P, lifted=None, scratch=P, out_depth=P, out_who=P)
        p.update(ptrs)
        need = lib.hn_mesh_render_scratch_bytes(max(s, 1), max(f, 1)) if scratch_bytes is None else scratch_bytes
        return lib.hn_mesh_geometry_f32(p["mesh"], p["faces"], faces_host, p["lifted"], s, v, f, k, paras, cams, h, w, p["scratch"], need,
                                        p["out_depth"], p["out_who"], None)
    refusals = [(dict([(name, None)]), b"null pointer") for name in ("mesh", "faces", "scratch", "out_depth", "out_who")]
    refusals += [(dict(cams=P), b"exactly one of paras"), (dict(paras=None), b"exactly one of paras"), (dict(s=0), b"bad dims"),
                 (dict(v=0), b"bad dims"), (dict(f=0), b"bad dims"), (dict(k=0), b"multiple of k"), (dict(k=3), b"multiple of k"),
                 (dict(s=34, k=17), b"slot byte"), (dict(h=0), b"frame size"), (dict(w=16385), b"frame size"), (dict(h=-1), b"frame size"),
                 (dict(scratch_bytes=0), b"scratch of"), (dict(scratch_bytes=lib.hn_mesh_render_scratch_bytes(4, 2) - 1), b"scratch of"),
                 (dict(scratch=P + 8), b"16-byte aligned"), (dict(paras=None, cams=P + 2), b"cams must be aligned"),
                 (dict(out_depth=P + 2), b"out_depth must be aligned"), (dict(faces_host=faces_bad), b"uses vertex 778 of 778")]
    for kw, word in refusals:
        assert geometry(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_mesh_geometry_f32: ") and word in err, (kw, err)

    def iters(n=2, k=2, h=48, w=64, v=778, f=2, joints=21, iters=3, stride=2, band=0.03, min_points=200, damp=1e-3, shift2=0.0025,
              tan2=0.03, frame_stride=None, scratch_bytes=None, work_bytes=None, paras=host4, cams=None, faces_host=faces_ok, **ptrs):
        p = dict(best=P, sil=P, depth=P, mesh=P, xyz=P, faces=P, lifted=None, scratch=P, work=P, out_mesh=P, out_xyz=P, out_rt=P,
                 out_count=P, out_cost=P, out_trace=P)
        p.update(ptrs)
        need = lib.hn_mesh_fit_scratch_bytes(n, k, h) if scratch_bytes is None else scratch_bytes
        work = lib.hn_mesh_fit_iters_scratch_bytes(n, k, h, w, v, f, joints, iters) if work_bytes is None else work_bytes
        return lib.hn_mesh_fit_iters_f32(p["best"], p["sil"], p["depth"], h * w if frame_stride is None else frame_stride, paras, cams,
                                         p["mesh"], p["xyz"], p["faces"], faces_host, p["lifted"], n, k, h, w, v, f, joints, iters, stride,
                                         band, min_points, damp, shift2, tan2, p["scratch"], need, p["work"], work, p["out_mesh"],
                                         p["out_xyz"], p["out_rt"], p["out_count"], p["out_cost"], p["out_trace"], None)
    refusals = [(dict([(name, None)]), b"null pointer") for name in ("best", "sil", "depth", "mesh", "xyz", "faces", "scratch", "work", "out_mesh",
                                                                       "out_xyz", "out_rt", "out_count", "out_cost", "out_trace")]
    refusals += [(dict(cams=P), b"exactly one of paras"), (dict(paras=None), b"exactly one of paras"),
                 (dict(iters=0), b"iters = 0"), (dict(iters=9), b"iters = 9"), (dict(iters=-2), b"iters = -2"),
                 (dict(n=0), b"n = 0"), (dict(n=65536), b"n = 65536"), (dict(k=0), b"k = 0"), (dict(k=17), b"k = 17"),
                 (dict(h=0), b"frame size"), (dict(w=0), b"frame size"), (dict(h=16385), b"frame size"), (dict(w=16385), b"frame size"),
                 (dict(frame_stride=48 * 64 - 1), b"depth_frame_stride"), (dict(v=0), b"v = 0"), (dict(v=2 ** 24 + 1), b"vertices"),
                 (dict(f=0), b"f = 0"), (dict(f=-1), b"f = -1"), (dict(joints=0), b"joints = 0"), (dict(joints=4097), b"joints = 4097"),
                 (dict(stride=0), b"stride = 0"), (dict(band=0.0), b"band"), (dict(band=nan), b"band"), (dict(band=100.5), b"band"),
                 (dict(min_points=0), b"min_points = 0"), (dict(damp=-1e-3), b"damp"), (dict(damp=nan), b"damp"),
                 (dict(shift2=0.0), b"max_shift2"), (dict(shift2=inf), b"max_shift2"), (dict(tan2=0.0), b"tan2_half_angle"),
                 (dict(tan2=nan), b"tan2_half_angle"),
                 (dict(scratch_bytes=lib.hn_mesh_fit_scratch_bytes(2, 2, 48) - 1), b"scratch of"), (dict(scratch=P + 4), b"8-byte aligned"),
                 (dict(work_bytes=lib.hn_mesh_fit_iters_scratch_bytes(2, 2, 48, 64, 778, 2, 21, 3) - 1), b"work of"),
                 (dict(work_bytes=0), b"work of"), (dict(work=P + 8), b"16-byte aligned"), (dict(paras=None, cams=P + 2), b"cams must be"),
                 (dict(out_cost=P + 4), b"aligned"), (dict(out_trace=P + 4), b"aligned"), (dict(out_mesh=P + 2), b"aligned"),
                 (dict(out_xyz=P + 1), b"aligned"), (dict(out_rt=P + 3), b"aligned"), (dict(out_count=P + 2), b"aligned"),
                 (dict(faces_host=faces_bad), b"uses vertex 778 of 778")]
    for kw, word in refusals:
        assert iters(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_mesh_fit_iters_f32: ") and word in err, (kw, err)
