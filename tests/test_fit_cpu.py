"""The mesh fit without a GPU: the rule itself (tests/fit_ref.py) on cases whose answer is known, the layout of a fit step's
buffer, the surfaces (signatures, defaults, doc wording), the C entries' declarations and refusals, and the Python layer's
ValueErrors.  The kernel against the rule, bit for bit: tests/test_fit_gpu.py."""
import ctypes as C
import inspect
import math
import re
import subprocess

import numpy as np
import pytest
import torch

import fit_cases as fc
import fit_ref as fr

F = np.float32
FIT_FIELDS = ("fit_mesh", "fit_xyz", "fit_rt", "fit_count", "fit_cost")


# ----------------------------------------------------------------------------------------------------------------- the rule
def _patch(damp, h=24, w=32):
    """a fronto-parallel patch best = 0.5, D = 0.5 + 2^-6, symmetric about the principal point and about its root joint, so
    that every off-diagonal sum of the normal equations cancels exactly"""
    best, sil = np.zeros((1, h, w), F), np.zeros((1, h, w), np.uint8)
    best[0, 4:20, 6:26], sil[0, 4:20, 6:26] = 0.5, 1                      # rows 4..19 about cy = 12, columns 6..25 about cx = 16
    depth = np.where(sil != 0, F(0.5 + 2.0 ** -6), F(2.0)).astype(F)
    paras = (40.0, 40.0, 16.0, 12.0)
    xyz = np.zeros((1, 21, 3), F)
    xyz[0, :, 2] = 500.0
    xyz[0, 1:, :2] = np.random.default_rng(3).uniform(-80, 80, (20, 2)).astype(F)
    mesh = np.random.default_rng(4).uniform(-0.1, 0.1, (1, 9, 3)).astype(F) + np.array([0, 0, -0.5], F)
    return fr.mesh_fit(best, sil, depth, paras, mesh, xyz, 1, band=0.03, stride=1, min_points=50, damp=damp), mesh, xyz


def test_the_constant_depth_patch_moves_along_z_alone():
    for damp in (1e-3, 0.25, 1.0):
        out, mesh, xyz = _patch(damp)
        assert out.count.tolist() == [[14 * 18, 0]]                       # the patch's interior
        want = 2.0 ** -6 / (1.0 + damp)
        rt = out.rt[0].astype(np.float64)
        assert np.array_equal(rt[:9].reshape(3, 3), np.eye(3)) and rt[9] == 0 and rt[10] == 0
        assert rt[11] == float(F(rt[11])) and abs(rt[11] - want) <= 2.0 ** -24 * want        # (t is handed out as fp32)
        # ... and in fp64, before that rounding: the solve on the patch's sums
        _r, _c, t = fr.terms(*_patch_inputs(), 0, 0.03, 1)
        sums = [int(v) for v in t.sum(axis=0)]
        a = [[0.0] * 6 for _ in range(6)]
        for at, (j, k) in enumerate(fr.PAIRS):
            a[j][k] = a[k][j] = sums[at] / 2.0 ** 30
        assert all(a[j][k] == 0 for j in range(6) for k in range(6) if j != k) and a[0][0] == a[1][1] == a[5][5] == 0
        lam = damp * sums[28]
        for j in range(6):
            a[j][j] += lam * (1.0 if j < 3 else fr.FIT_ARM * fr.FIT_ARM)
        x = fr.cholesky_solve(a, [v / 2.0 ** 30 for v in sums[21:27]])
        assert x[0] == x[1] == x[3] == x[4] == x[5] == 0 and abs(x[2] - want) <= 1e-12 * want
        # the mesh and the joints moved by exactly that shift
        assert np.array_equal(out.mesh[0, :, :2], mesh[0, :, :2]) and np.array_equal(out.xyz[0, :, :2], xyz[0, :, :2])
        assert np.allclose(out.mesh[0, :, 2], mesh[0, :, 2] - want, rtol=0, atol=1e-6)       # (z is negated in the mesh)
        assert np.allclose(out.xyz[0, :, 2], xyz[0, :, 2] + 1000 * want, rtol=0, atol=1e-3)
        assert out.cost[0] == 14 * 18 * 2 ** 18                           # rho = 2^-6 exactly at every match


def _patch_inputs(h=24, w=32):
    best, sil = np.zeros((h, w), F), np.zeros((h, w), np.uint8)
    best[4:20, 6:26], sil[4:20, 6:26] = 0.5, 1
    depth = np.where(sil != 0, F(0.5 + 2.0 ** -6), F(2.0)).astype(F)
    return best, sil, depth, (40.0, 40.0, 16.0, 12.0), np.array([0, 0, 500], F)


def test_the_patch_without_damping_has_no_solution():
    """nx = 0 exactly at every match, so the first pivot is exactly 0: status 2, and the outputs are the inputs' bytes"""
    out, mesh, xyz = _patch(0.0)
    assert out.count.tolist() == [[14 * 18, 2]]
    assert out.rt[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert out.mesh.tobytes() == mesh.tobytes() and out.xyz.tobytes() == xyz.tobytes()


def test_the_cayley_rotation_is_orthonormal():
    rng = np.random.default_rng(11)
    for scale in (1e-9, 1e-3, 0.1, math.tan(0.35 / 2), 1.0, 30.0):
        for _ in range(50):
            a = (rng.normal(size=3) * scale).tolist()
            r = np.array(fr.cayley(a)).reshape(3, 3)
            assert np.abs(r @ r.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(r) - 1.0) <= 1e-15
            # the rotation by 2 atan(|a|) about a: it leaves a where it is
            assert np.abs(r @ np.array(a) - np.array(a)).max() <= 1e-15 * max(1.0, scale)
    status, rt = fr.solve([0] * 28 + [5], min_points=1, damp=1.0)
    assert status == 0 and rt.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def test_a_slot_that_is_not_fitted_keeps_its_bytes():
    """statuses 1, 2 and 3 of the GPU cases: R = I, t = 0 and byte copies -- NaN, -0.0 and inf included"""
    seen = set()
    for shape in fc.SHAPES:
        c = fc.case(*shape)
        for v in fc.VERTICES:
            want, _census = fc.expected(*shape, v=v)
            for s in np.nonzero(want.count[:, 1] != 0)[0]:
                seen.add(int(want.count[s, 1]))
                assert want.mesh[s].tobytes() == c.meshes[v][s].tobytes() and want.xyz[s].tobytes() == c.xyz_mm[s].tobytes()
                assert want.rt[s].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
            for s in np.nonzero(want.count[:, 1] == 0)[0]:
                assert want.mesh[s].tobytes() != c.meshes[v][s].tobytes() and want.xyz[s].tobytes() != c.xyz_mm[s].tobytes()
    assert seen == {1, 2, 3}
    c = fc.case(*fc.SHAPES[1])
    assert np.isnan(c.meshes[5][-1]).any() and np.isinf(c.meshes[5][-1]).any()     # the empty slot's odd values


def test_the_integer_sums_do_not_depend_on_the_order():
    c = fc.case(*fc.SHAPES[2])
    rng = np.random.default_rng(5)
    for i in range(c.n):
        for kk in range(c.k):
            _r, _c, t = fr.terms(c.best[i], c.sil[i], c.depth[i], c.paras, c.xyz_mm[i * c.k + kk, 0], kk, c.band, c.stride)
            if not len(t):
                continue
            first = [int(v) for v in t.sum(axis=0)]
            for _ in range(3):
                order = rng.permutation(len(t))
                acc = [0] * fr.TERMS
                for row in t[order]:                                      # one by one, Python integers
                    acc = [a + int(b) for a, b in zip(acc, row)]
                assert acc == first
            assert fr.solve(first, c.min_points, c.damp, *fr.caps(c.max_shift, c.max_angle))[0] == fc.expected(*fc.SHAPES[2])[0].count[i * c.k + kk, 1]


def recovery(seed):
    """a hand-sized ellipsoid at 0.4-0.7 m on a 240 x 320 frame, its copy moved by up to 0.12 rad and 2 cm with 1 mm depth
    noise, the defaults: (RMS distance of the matched mesh surface points to the measured surface before, after the fit)"""
    rng = np.random.default_rng(seed)
    h, w, paras = 240, 320, (288.0, 288.0, 160.0, 120.0)
    z = rng.uniform(0.4, 0.7)
    centre = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.04, 0.04), z])
    axes = np.array([0.09, 0.045, 0.015])                                # a hand: 18 x 9 x 3 cm
    pose = fc.rotation(rng, rng.uniform(0, 0.6))
    root = centre + np.array([0.0, 0.07, 0.0])
    turn = fc.rotation(rng, rng.uniform(0, 0.12))
    shift = rng.normal(size=3)
    shift *= rng.uniform(0, 0.02) / np.linalg.norm(shift)
    q0, q1, moved = fc.quadric(axes, pose), fc.quadric(axes, turn @ pose), centre + shift      # (turned about its own centre)
    zs, zd = fc.ray_cast(h, w, paras, centre, q0), fc.ray_cast(h, w, paras, moved, q1)
    hit = ~np.isnan(zs)
    best = np.where(hit, zs, 0).astype(F)
    sil = hit.astype(np.uint8)
    depth = np.where(np.isnan(zd), 2.0, zd + rng.normal(0, 0.001, (h, w))).astype(F)
    xyz = np.zeros((1, 21, 3), F)
    xyz[0] = (root * 1000).astype(F)
    mesh = np.zeros((1, 4, 3), F)
    out = fr.mesh_fit(best[None], sil[None], depth[None], paras, mesh, xyz, 1)
    assert out.count[0, 1] == 0 and out.count[0, 0] >= fr.FIT_MIN_POINTS, out.count
    rows, cols, _t = fr.terms(best, sil, depth, paras, xyz[0, 0], 0)
    p = np.stack(fr.point(rows, cols, best[rows, cols], paras), axis=-1).astype(np.float64)
    rt, c0 = out.rt[0].astype(np.float64), (xyz[0, 0] / F(1000)).astype(np.float64)
    after = (p - c0) @ rt[:9].reshape(3, 3).T + c0 + rt[9:]
    rms = lambda pts: float(np.sqrt(np.mean(fc.surface_distance(pts, moved, q1) ** 2)))  # noqa: E731
    return rms(p), rms(after), float(np.sqrt(out.cost[0] / 2.0 ** 30 / out.count[0, 0]))


@pytest.mark.parametrize("seed", range(8))
def test_one_step_brings_the_mesh_to_the_measured_surface(seed):
    before, after, rho = recovery(seed)
    print(f"seed {seed}: RMS distance to the measured surface {1000 * before:.2f} mm -> {1000 * after:.2f} mm "
          f"({before / after:.1f} x), RMS residual along the normals {1000 * rho:.2f} mm")
    assert before >= 3.0 * after


@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_gpu_cases_offer_what_they_must(shape):
    """the conditions test_fit_gpu.py checks before it compares, here without a GPU"""
    c = fc.case(*shape)
    want, census = fc.expected(*shape)
    fc.check_conditions(c, want, census)
    fc.check_statuses()
    who = c.sil & 0x7F
    if c.h >= 32:
        assert (c.sil & 0x80).any() and (who > c.k).any() and ((who >= 1) & (who <= c.k)).any()
        for value in fc.HOLES:
            assert (np.isnan(c.depth).any() if np.isnan(value) else (c.depth == F(value)).any()), value
    if c.k > 1 and c.h >= 48:      # slots drawn over each other: a pixel of one slot beside a pixel of another
        assert ((who[:, :, 1:] != who[:, :, :-1]) & (who[:, :, 1:] >= 1) & (who[:, :, :-1] >= 1) & (who[:, :, 1:] <= c.k)
                & (who[:, :, :-1] <= c.k)).any()


# ------------------------------------------------------------------------------------------------------------------- layout
COMBOS = [(1, 1, 5, (5, 7), {}), (3, 2, 5, (5, 7), dict(labels=True, handed=True)),
          (2, 3, 778, (48, 64), dict(tracked=True, smoothed=True)),
          (7, 5, 13, (5, 7), dict(labels=True, tracked=True)), (16, 16, 778, (33, 65), dict(handed=True, tracked=True, smoothed=True))]


@pytest.mark.parametrize("rig", [False, True])
@pytest.mark.parametrize("cloud", [0, 7])
@pytest.mark.parametrize("n,k,v,hw,opts", COMBOS)
def test_fit_layout_appends_five_aligned_parts_and_moves_nothing(n, k, v, hw, opts, cloud, rig):
    from hn_amd.live import LiveLayout
    opts = dict(opts, overlay=True, occluded=True, rig=rig, cloud=cloud)
    plain, fit = LiveLayout(n, k, v, hw, **opts), LiveLayout(n, k, v, hw, **opts, fit=True)
    params = list(inspect.signature(LiveLayout).parameters)
    assert plain.fit is False and fit.fit is True and params[-3:] == ["fit", "cloud", "rig"]
    for f in LiveLayout.__dataclass_fields__:
        if f not in ("fit", "nbytes"):
            assert getattr(plain, f) == getattr(fit, f), f
    assert not any(f.startswith("fit_") for f in LiveLayout.__dataclass_fields__)
    s = n * (k or 1)
    sizes = dict(fit_mesh=s * v * 12, fit_xyz=s * 21 * 12, fit_rt=s * 48, fit_count=s * 8, fit_cost=s * 8)
    aligns = dict(fit_mesh=4, fit_xyz=4, fit_rt=4, fit_count=4, fit_cost=8)
    end = plain.nbytes
    for name in FIT_FIELDS:
        at = getattr(fit, name + "_at")
        assert getattr(plain, name + "_at") is None
        assert at % aligns[name] == 0 and end <= at < end + aligns[name], name
        end = at + sizes[name]
    assert end == fit.nbytes
    assert (plain.cloud_at, plain.cloud_count_at, plain.cloud_resid_at) == (fit.cloud_at, fit.cloud_count_at, fit.cloud_resid_at)
    buf = torch.zeros((fit.nbytes + 8,), dtype=torch.uint8)
    buf = buf[(-buf.data_ptr()) % 8:][:fit.nbytes]
    pv, fv = plain.views(buf[:plain.nbytes]), fit.views(buf)
    assert fv._fields == pv._fields + FIT_FIELDS and type(fv).__name__.endswith("FitViews")
    assert ("Rig" in type(fv).__name__) == rig and ("Cloud" in type(fv).__name__) == bool(cloud)
    for name in pv._fields:
        a, b = getattr(pv, name), getattr(fv, name)
        assert (a is None) == (b is None)
        if a is not None:
            assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype
    shapes = dict(fit_mesh=(s, v, 3), fit_xyz=(s, 21, 3), fit_rt=(s, 12), fit_count=(s, 2), fit_cost=(s,))
    dtypes = dict(fit_mesh=torch.float32, fit_xyz=torch.float32, fit_rt=torch.float32, fit_count=torch.int32, fit_cost=torch.int64)
    for name in FIT_FIELDS:
        t = getattr(fv, name)
        assert t.data_ptr() - buf.data_ptr() == getattr(fit, name + "_at") and tuple(t.shape) == shapes[name] and t.dtype == dtypes[name]


def test_fit_layout_refusals():
    from hn_amd.live import LiveLayout
    with pytest.raises(ValueError, match="a fit step is an occluded step"):
        LiveLayout(2, 2, 778, (5, 7), overlay=True, fit=True)
    with pytest.raises(ValueError, match="a fit step is an occluded step"):
        LiveLayout(2, 2, 778, fit=True)
    assert LiveLayout(2, 2, 778, (5, 7), overlay=True, occluded=True).fit_cost_at is None
    for cloud in (0, 9):                                                  # the one-hand step
        one = LiveLayout(3, None, 778, (5, 7), overlay=True, occluded=True, fit=True, cloud=cloud)
        v = one.views(torch.zeros((one.nbytes,), dtype=torch.uint8))
        assert tuple(v.fit_mesh.shape) == (3, 778, 3) and tuple(v.fit_xyz.shape) == (3, 21, 3) and tuple(v.fit_rt.shape) == (3, 12)
        assert tuple(v.fit_count.shape) == (3, 2) and tuple(v.fit_cost.shape) == (3,)
        assert one.fit_cost_at % 8 == 0 and one.nbytes == one.fit_cost_at + 24
        assert one.fit_mesh_at >= LiveLayout(3, None, 778, (5, 7), overlay=True, occluded=True, cloud=cloud).nbytes


def test_read_appends_the_five_fields_behind_every_other_field():
    from hn_amd import live
    from hn_amd.live import LiveHandsOutput, LiveLayout, LiveOutput, _read_type
    n, k, v, hw = 2, 3, 5, (5, 7)
    g = torch.Generator().manual_seed(4)
    for opts in (dict(), dict(handed=True, tracked=True, smoothed=True), dict(rig=True), dict(cloud=6), dict(cloud=3, rig=True)):
        opts = dict(opts, overlay=True, occluded=True)
        plain, fit = LiveLayout(n, k, v, hw, **opts), LiveLayout(n, k, v, hw, **opts, fit=True)
        host = torch.randint(0, 256, (fit.nbytes,), generator=g, dtype=torch.uint8)
        host[:plain.mesh_at] = 0
        r = LiveHandsOutput(None, None, None, None, None, host, n, k, layout=fit).read()
        p = LiveHandsOutput(None, None, None, None, None, host[:plain.nbytes], n, k, layout=plain).read()
        assert r._fields == p._fields + FIT_FIELDS and type(r).__name__ == type(p).__name__[:-4] + "FitRead"
        assert type(r).__doc__.endswith("+ fit_mesh + fit_xyz + fit_rt + fit_count + fit_cost.")
        for a, b in zip(r[:len(p)], p):
            assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)) if torch.is_tensor(a) else a == b
        v_ = fit.views(host)
        assert [tuple(getattr(r, f).shape) for f in FIT_FIELDS] == [(n, k, v, 3), (n, k, 21, 3), (n, k, 12), (n, k, 2), (n, k)]
        assert [getattr(r, f).dtype for f in FIT_FIELDS] == [torch.float32] * 3 + [torch.int32, torch.int64]
        for name in FIT_FIELDS:
            got = getattr(r, name)
            assert torch.equal(got.reshape(-1).view(torch.uint8), getattr(v_, name).reshape(-1).view(torch.uint8)), name
            assert got.data_ptr() != getattr(v_, name).data_ptr()
    plain1, fit1 = LiveLayout(n, None, v, hw, True, occluded=True), LiveLayout(n, None, v, hw, True, occluded=True, fit=True)
    host = torch.randint(0, 256, (fit1.nbytes,), generator=g, dtype=torch.uint8)
    host[:plain1.mesh_at] = 0
    r1 = LiveOutput(None, None, None, None, host, n, layout=fit1).read()
    p1 = LiveOutput(None, None, None, None, host[:plain1.nbytes], n, layout=plain1).read()
    assert r1._fields == p1._fields + FIT_FIELDS and type(r1).__name__ == "LiveOverlayOccludedFitRead"
    assert r1.box_label is None and r1.pose_label is None
    assert [tuple(getattr(r1, f).shape) for f in FIT_FIELDS] == [(n, v, 3), (n, 21, 3), (n, 12), (n, 2), (n,)]
    assert list(inspect.signature(_read_type).parameters)[-1] == "cloud"        # (no parameter was added: a helper derives the type)
    assert live._fit_read_type(type(p1)) is type(r1) and live._fit_views(type(plain1.views(host[:plain1.nbytes]))) is type(fit1.views(host))


# ----------------------------------------------------------------------------------------------------------------- surfaces
NAMES = ["fit", "fit_band", "fit_stride", "fit_min_points", "fit_damp", "fit_max_shift", "fit_max_angle"]
DEFAULTS = (False, 0.03, 2, 200, 1e-3, 0.05, 0.35)


def test_the_surfaces():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import live, ops
    from hn_amd.live import LiveHandEngine, LiveHandsEngine, LiveHandsOutput, LiveOutput
    assert ((ops.FIT_BAND, ops.FIT_STRIDE, ops.FIT_MIN_POINTS, ops.FIT_DAMP, ops.FIT_MAX_SHIFT, ops.FIT_MAX_ANGLE) == DEFAULTS[1:]
            == (fr.FIT_BAND, fr.FIT_STRIDE, fr.FIT_MIN_POINTS, fr.FIT_DAMP, fr.FIT_MAX_SHIFT, fr.FIT_MAX_ANGLE))
    assert ops.MeshFit._fields == ("mesh", "xyz", "rt", "count", "cost") == fr.MeshFit._fields and live.FIT_FIELDS == FIT_FIELDS
    assert ops.fit_caps(0.05, 0.35) == fr.caps(0.05, 0.35) == (0.05 * 0.05, math.tan(0.175) ** 2)
    sig = inspect.signature(ops.mesh_fit).parameters
    assert list(sig) == ["mesh_depth", "silhouette", "scene_depth", "paras", "mesh", "xyz_mm", "k", "band", "stride", "min_points", "damp",
                         "max_shift", "max_angle", "out", "scratch"]
    for name, default in zip(list(sig)[7:], DEFAULTS[1:] + (None, None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    assert list(inspect.signature(ops.check_fit).parameters) == ["band", "stride", "min_points", "damp", "max_shift", "max_angle"]
    for fn in (HandNet.live, HandNet.live_hands, LiveHandEngine.__init__, LiveHandsEngine.__init__):
        params = inspect.signature(fn).parameters
        names = list(params)
        at = names.index("fit")
        assert names[at:at + 7] == NAMES and tuple(params[n].default for n in NAMES) == DEFAULTS, fn.__qualname__
        assert names[at - 1] in ("cloud_stride", "cloud_frame")             # directly behind the cloud's keywords
    for fn in (HandNet.live_hands, LiveHandsEngine.__init__):
        names = list(inspect.signature(fn).parameters)
        assert names[names.index("fit_max_angle") + 1] == "smooth" and names[-1] == "smooth_rate"
    for doc in (ops.mesh_fit.__doc__, ops.check_fit.__doc__, LiveHandEngine.__doc__, LiveHandsEngine.__init__.__doc__,
                HandNet.live.__doc__, HandNet.live_hands.__doc__):
        assert "starting values, NOT tuned on this model" in " ".join(doc.split("0.35 rad")[-1].split()), doc[:40]
    assert "DESIGN.md section 9k" in ops.mesh_fit.__doc__ and "x' = R (x - c0) + c0 + t" in ops.mesh_fit.__doc__
    for cls in (LiveOutput, LiveHandsOutput):
        names = list(cls.__dataclass_fields__)
        at = names.index("mesh_depth")
        assert tuple(names[at + 1:at + 6]) == FIT_FIELDS


def test_the_entries_are_declared_exported_and_bound():
    from hn_amd import _lib, build
    build.build_library()
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    for name, result, count in (("hn_mesh_fit_f32", "int", 28), ("hn_mesh_fit_scratch_bytes", "int64_t", 3)):
        proto = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (result, name), text)
        assert proto and name in _lib.SIGNATURES
        params = [p.strip() for p in proto.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is (C.c_int if result == "int" else C.c_int64) and len(params) == len(args) == count
        for p, a in zip(params, args):
            if "*" in p:
                assert a is C.c_void_p, p
            elif p.startswith("float"):
                assert a is C.c_float, p
            elif p.startswith("double"):
                assert a is C.c_double, p
            elif p.startswith("int64_t"):
                assert a is C.c_int64, p
            else:
                assert p.startswith("int ") and a is C.c_int, p
        assert re.search(r" T %s\b" % name, out)
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION                  # functions added, no struct touched
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["mesh_fit.hip"]
    rows = (build.CSRC / "build" / "mesh_fit.resources.txt").read_text().splitlines()
    assert len(rows) == 2 and all("mesh_fit_" in r and " vgpr_spill 0 " in r and r.endswith("sgpr_spill 0") and " scratch 0 " in r for r in rows)


def test_the_scratch_size():
    from hn_amd import _lib
    lib = _lib.load()
    row = fr.TERMS * 8
    assert lib.hn_mesh_fit_scratch_bytes(1, 1, 1) == 4 * row and lib.hn_mesh_fit_scratch_bytes(1, 2, 480) == 240 * 2 * row
    assert lib.hn_mesh_fit_scratch_bytes(3, 16, 203) == 3 * 104 * 16 * row and lib.hn_mesh_fit_scratch_bytes(2, 16, 16384) == 2 * 1024 * 16 * row
    for bad in ((0, 1, 5), (1, 0, 5), (1, 17, 5), (1, 1, 0), (1, 1, 16385), (-1, 1, 5)):
        assert lib.hn_mesh_fit_scratch_bytes(*bad) == 0, bad


def test_the_entry_checks_its_arguments_before_any_launch():
    """no GPU here: every refusal comes back as HN_ERR_ARG with a message under the entry's name, before the device is touched"""
    from hn_amd import _lib
    lib = _lib.load()
    P = 4096        # stands for a device address
    host4 = (C.c_float * 4)(600.0, 600.0, 320.0, 240.0)
    nan, inf = float("nan"), float("inf")

    def call(n=2, k=2, h=48, w=64, v=778, joints=21, stride=2, band=0.03, min_points=200, damp=1e-3, shift2=0.0025, tan2=0.03,
             frame_stride=None, scratch_bytes=None, paras=host4, cams=None, **ptrs):
        p = dict(best=P, sil=P, depth=P, mesh=P, xyz=P, scratch=P, out_mesh=P, out_xyz=P, out_rt=P, out_count=P, out_cost=P)
        p.update(ptrs)
        need = lib.hn_mesh_fit_scratch_bytes(n, k, h) if scratch_bytes is None else scratch_bytes
        return lib.hn_mesh_fit_f32(p["best"], p["sil"], p["depth"], h * w if frame_stride is None else frame_stride, paras, cams,
                                   p["mesh"], p["xyz"], n, k, h, w, v, joints, stride, band, min_points, damp, shift2, tan2, p["scratch"],
                                   need, p["out_mesh"], p["out_xyz"], p["out_rt"], p["out_count"], p["out_cost"], None)
    refusals = [(dict([(name, None)]), b"null pointer") for name in ("best", "sil", "depth", "mesh", "xyz", "scratch", "out_mesh", "out_xyz",
                                                                       "out_rt", "out_count", "out_cost")]
    refusals += [(dict(cams=P), b"exactly one of paras"), (dict(paras=None), b"exactly one of paras"),
                 (dict(n=0), b"n = 0"), (dict(n=65536), b"n = 65536"), (dict(k=0), b"k = 0"), (dict(k=17), b"k = 17"), (dict(k=-1), b"k = -1"),
                 (dict(h=0), b"frame size"), (dict(w=0), b"frame size"), (dict(h=16385), b"frame size"), (dict(w=16385), b"frame size"),
                 (dict(h=-4), b"frame size"),
                 (dict(frame_stride=48 * 64 - 1), b"depth_frame_stride"), (dict(frame_stride=0), b"depth_frame_stride"),
                 (dict(v=0), b"v = 0"), (dict(v=-3), b"v = -3"), (dict(v=2 ** 24 + 1), b"vertices"),
                 (dict(joints=0), b"joints = 0"), (dict(joints=4097), b"joints = 4097"),
                 (dict(stride=0), b"stride = 0"), (dict(stride=-2), b"stride = -2"),
                 (dict(band=0.0), b"band"), (dict(band=-0.03), b"band"), (dict(band=nan), b"band"), (dict(band=inf), b"band"),
                 (dict(band=100.5), b"band"),
                 (dict(min_points=0), b"min_points = 0"), (dict(min_points=-7), b"min_points = -7"),
                 (dict(damp=-1e-3), b"damp"), (dict(damp=nan), b"damp"), (dict(damp=inf), b"damp"),
                 (dict(shift2=0.0), b"max_shift2"), (dict(shift2=-1.0), b"max_shift2"), (dict(shift2=nan), b"max_shift2"),
                 (dict(shift2=inf), b"max_shift2"),
                 (dict(tan2=0.0), b"tan2_half_angle"), (dict(tan2=-1.0), b"tan2_half_angle"), (dict(tan2=nan), b"tan2_half_angle"),
                 (dict(tan2=inf), b"tan2_half_angle"),
                 (dict(scratch_bytes=lib.hn_mesh_fit_scratch_bytes(2, 2, 48) - 1), b"scratch of"), (dict(scratch_bytes=0), b"scratch of"),
                 (dict(scratch=P + 4), b"8-byte aligned"), (dict(out_cost=P + 4), b"aligned"), (dict(out_mesh=P + 2), b"aligned"),
                 (dict(out_xyz=P + 1), b"aligned"), (dict(out_rt=P + 3), b"aligned"), (dict(out_count=P + 2), b"aligned")]
    for kw, word in refusals:
        assert call(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_mesh_fit_f32: ") and word in err, (kw, err)


# ---------------------------------------------------------------------------------------------------------- the Python layer
def test_check_fit():
    from hn_amd import ops
    assert ops.check_fit() == (0.03, 2, 200, 1e-3, 0.05, 0.35) and ops.check_fit(100, 1, 1, 0, 1e-3, 3.0) == (100.0, 1, 1, 0.0, 1e-3, 3.0)
    assert ops.check_fit(np.float32(0.5), np.int64(3), np.int32(7), np.float64(0.5), np.float32(0.25), 1) == (0.5, 3, 7, 0.5, 0.25, 1.0)
    for bad in (0, -1, 2.0, True, "many", None, 2 ** 31):
        with pytest.raises(ValueError, match="fit_stride"):
            ops.check_fit(stride=bad)
        with pytest.raises(ValueError, match="fit_min_points"):
            ops.check_fit(min_points=bad)
    for bad in (0, -0.03, float("nan"), float("inf"), -float("inf"), 100.0001, 1e39, 1e-50, "wide", None, True):
        with pytest.raises(ValueError, match="fit_band"):
            ops.check_fit(band=bad)
    for bad in (-1e-9, float("nan"), float("inf"), "soft", None, True):
        with pytest.raises(ValueError, match="fit_damp"):
            ops.check_fit(damp=bad)
    for bad in (0, -0.05, float("nan"), float("inf"), 1e200, 1e-200, "far", None, True):
        with pytest.raises(ValueError, match="fit_max_shift"):
            ops.check_fit(max_shift=bad)
    for bad in (0, -0.35, math.pi, 4.0, float("nan"), float("inf"), 1e-200, "wide", None, True):
        with pytest.raises(ValueError, match="fit_max_angle"):
            ops.check_fit(max_angle=bad)


class _Hand:
    device = "cpu"

    def set_convert(self, **kw):
        pass


class _Graph:
    v = 1280


class _Lifter:
    device = "cpu"
    graphs = [_Graph()]


def test_the_engines_refuse_what_the_fit_cannot_do():
    """before anything touches a device"""
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    paras, perm, faces = (600.0, 600.0, 320.0, 240.0), np.arange(778), np.array([[0, 1, 2]])
    hands = lambda *a, **kw: LiveHandsEngine(_Hand(), _Lifter(), paras, 2, True, *a, **kw)  # noqa: E731
    one = lambda *a, **kw: LiveHandEngine(_Hand(), _Lifter(), paras, True, *a, **kw)  # noqa: E731
    for make in (hands, one):
        with pytest.raises(ValueError, match="fit=True needs occlude=True"):
            make(perm, fit=True)
        with pytest.raises(ValueError, match="fit=True needs occlude=True"):
            make(perm, faces=faces, fit=True)
        with pytest.raises(ValueError, match="occlude=True needs faces="):
            make(perm, occlude=True, fit=True)
        with pytest.raises(ValueError, match="perm_reverse"):
            make(None, faces=faces, occlude=True, fit=True)
        for kw, word in ((dict(fit_band=0), "fit_band"), (dict(fit_band=101), "fit_band"), (dict(fit_stride=0), "fit_stride"),
                         (dict(fit_stride=1.5), "fit_stride"), (dict(fit_min_points=0), "fit_min_points"), (dict(fit_damp=-1), "fit_damp"),
                         (dict(fit_max_shift=0), "fit_max_shift"), (dict(fit_max_angle=math.pi), "fit_max_angle")):
            with pytest.raises(ValueError, match=word):
                make(perm, faces=faces, occlude=True, fit=True, **kw)
        plain = make(perm)
        assert plain.fit is None and plain._key_options() == () and not plain._layout(2, (5, 7)).fit
        ignored = make(perm, fit_band=-1)                                  # (the parameters are read only with fit=True)
        assert ignored.fit is None
