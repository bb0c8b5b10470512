"""The iterated depth fit on the GPU: the raster's geometry pass (csrc/mesh_raster.hip through
ops.mesh_geometry and hn_mesh_geometry_f32), the iterated fit (csrc/mesh_refit.hip through ops.mesh_fit_iters and
hn_mesh_fit_iters_f32) and the live steps with fit_iters= / fit_draw= against the rule in numpy (tests/refit_ref.py), bit for
bit: no tolerance appears in this file."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import cams_ref
import cloud_ref
import raster_ref as rr
import refit_cases as rc
import refit_ref as rf
from test_occlude_gpu import H, LIVE_PARAS, W, _net, _run, _same, inputs, parts  # noqa: F401  (the synthetic pipeline's fixtures)

pytestmark = pytest.mark.gpu

F = np.float32
FIELDS = ("mesh", "xyz", "rt", "count", "cost", "trace")
PARTS = ("fit_mesh", "fit_xyz", "fit_rt", "fit_count", "fit_cost", "fit_trace")


def _bytes(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).tobytes()


def _device(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _raw(nbytes, fill=0xFF):
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def _differ(got, want, tag, fields=FIELDS):
    """every output against the rule's, as bytes; the figures are printed before they are asserted"""
    bad = []
    for name in fields:
        g, w = getattr(got, name), getattr(want, name)
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        g = g.reshape(w.shape)
        assert g.dtype == w.dtype, (tag, name, g.dtype, w.dtype)
        differ = int((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum())
        print(f"{tag}: {name} {g.shape}: {differ} bytes differ")
        if differ:
            bad.append((name, differ))
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------------- the geometry pass
def _geometry_both_ways(tag, meshes, faces, lifted, cams, h, w):
    """meshes [N,K,V,3], cams [N,4] (equal rows: the host's four values are used too) -> the device's (depth, who), checked
    against the rule, against the occluded raster, twice, into 0xFF-filled buffers, through the table and the C entry"""
    from hn_amd import _lib, ops
    n, k = meshes.shape[:2]
    flat = None if lifted is None else np.asarray(lifted, np.int32).reshape(-1)
    want_d, want_w = rf.geometry_frames(meshes.reshape(n * k, -1, 3), faces, cams, k, h, w, flat)
    mesh, fc_dev = _device(meshes, np.asarray(faces, np.int32))
    lif = None if flat is None else torch.from_numpy(flat).cuda()
    table = torch.from_numpy(np.asarray(cams, F)).cuda()
    one_camera = bool((np.asarray(cams) == np.asarray(cams)[0]).all())
    runs = []
    for paras in ([tuple(float(x) for x in cams[0])] if one_camera else []) + [table]:
        for _again in range(2):
            d, who = _raw(n * h * w * 4).view(torch.float32).view(n, h, w), _raw(n * h * w).view(n, h, w)
            got = ops.mesh_geometry(mesh, fc_dev, paras, (h, w), lifted=lif, k=k, out_depth=d, out_who=who)
            torch.cuda.synchronize()
            assert got[0].data_ptr() == d.data_ptr() and got[1].data_ptr() == who.data_ptr()
            runs.append((_bytes(d), _bytes(who)))
    covered = int((want_w != 0).sum())
    diff = lambda a, b: int((np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)).sum())  # noqa: E731
    print(f"{tag}: {covered} covered pixels, slots seen {sorted(set(np.unique(want_w).tolist()) - {0})}; depth "
          f"{diff(runs[0][0], want_d.tobytes())} bytes differ, who {diff(runs[0][1], want_w.tobytes())} bytes differ")
    for d, who in runs:
        assert d == want_d.tobytes() and who == want_w.tobytes(), tag
    # a host face list goes through the entry's own index check
    if int(np.min(faces)) >= 0 and int(np.max(faces)) < meshes.shape[2]:
        by_list = ops.mesh_geometry(mesh, np.asarray(faces), table, (h, w), lifted=lif, k=k)
    else:      # (a bad index on the device draws nothing; in a host list the entry refuses it)
        with pytest.raises(RuntimeError, match="uses vertex"):
            ops.mesh_geometry(mesh, np.asarray(faces), table, (h, w), lifted=lif, k=k)
        by_list = got
    # the occluded raster of the same meshes: its depth_out and silhouette & 0x7F are these bytes
    frame = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    scene = torch.full((n, h, w), 0.5, device="cuda")
    z = torch.full((n, h, w), -1.0, device="cuda")
    _img, sil, _cov = ops.mesh_render(mesh.view(n * k, -1, 3), fc_dev, table, frame, lifted=lif, k=k, depth_out=z, scene_depth=scene, margin=0.0)
    # the C entry on raw pointers
    lib = _lib.load()
    s, v, f = n * k, meshes.shape[2], len(faces)
    need = lib.hn_mesh_render_scratch_bytes(s, f)
    scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
    d, who = _raw(n * h * w * 4), _raw(n * h * w)
    st = lib.hn_mesh_geometry_f32(mesh.data_ptr(), fc_dev.data_ptr(), None, None if lif is None else lif.data_ptr(), s, v, f, k, None,
                                  table.data_ptr(), h, w, scratch.data_ptr(), need, d.data_ptr(), who.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.hn_last_error()
    assert (_bytes(d), _bytes(who)) == runs[0] == (_bytes(by_list[0]), _bytes(by_list[1])), tag
    assert _bytes(z) == runs[0][0] and _bytes(sil & 0x7F) == runs[0][1], (tag, "the occluded raster disagrees")
    return covered


@pytest.mark.parametrize("name", list(rr.scenes()))
def test_geometry_on_the_raster_scenes(name):
    """raster_ref.scenes() -- interpenetrating slots, borders crossed, unlifted slots and frames, degenerate and duplicated
    faces, rejected vertices, vertices on sample points -- at their own sizes: depth and slot byte equal refit_ref.geometry and
    the occluded raster's depth_out and silhouette & 0x7F, bit for bit"""
    meshes, faces, lifted, paras, (h, w) = rr.scenes()[name]
    cams = np.tile(np.asarray(paras, F), (meshes.shape[0], 1))
    assert _geometry_both_ways(name, meshes, faces, lifted, cams, h, w) > 0


def _soup(rng, centre, spread, count):
    """`count` seeded vertices about `centre` (camera frame) as out['mesh'] rows, a NaN one and one nearer than the near plane"""
    pts = np.asarray(centre) + rng.uniform(-1, 1, (count, 3)) * spread
    pts[-2] = (np.nan, 0.0, 0.5)
    pts[-1] = (0.0, 0.0, 0.01)
    return (pts * [1.0, -1.0, -1.0]).astype(F)


@functools.lru_cache(maxsize=None)
def _shape_scene(n, k, h, w):
    """N frames of K slots: a 126-face ellipsoid per slot on a grid over the frame (slots overlap their neighbours), plus per
    slot a soup of 40 seeded triangles over 24 more vertices (two of them rejected), four duplicated faces and two faces with a
    vertex index out of range; one slot per frame is not lifted where K > 1; a camera per frame"""
    rng = np.random.default_rng(100 * h + w + k)
    cols = int(np.ceil(np.sqrt(k)))
    rows = (k + cols - 1) // cols
    f = 0.9 * w / cols
    cams = np.array([[f * (1 + 0.05 * i), f * (1 - 0.03 * i), w / 2 - 0.37 + 2 * i, h / 2 + 0.21 - i] for i in range(n)], F)
    meshes, faces = [], None
    for i in range(n):
        frame = []
        for kk in range(k):
            r, c = divmod(kk, cols)
            u, v = (c + 0.5) * w / cols + rng.uniform(-3, 3), (r + 0.5) * h / rows + rng.uniform(-3, 3)
            z = 0.5 + 0.02 * rng.uniform(-1, 1)
            centre = ((u - w / 2) * z / f, (v - h / 2) * z / f, z)
            radii = np.array([0.62 * (w / cols) * z / f, 0.62 * (h / rows) * z / f, 0.03])
            ell, ef = rr.ellipsoid(centre, radii, rings=cams_ref.RINGS, segs=cams_ref.SEGS)
            frame.append(np.concatenate([ell, _soup(rng, centre, radii * [1.5, 1.5, 2.0], 24)]))
            if faces is None:
                nv = len(ell)
                soup = rng.integers(nv, nv + 24, (40, 3))
                faces = np.concatenate([ef, soup, ef[-2:], soup[:2], [[0, 1, nv + 24], [-1, 2, 3]]]).astype(np.int32)
        meshes.append(np.stack(frame))
    lifted = np.ones((n, k), np.int32)
    if k > 1:
        lifted[np.arange(n), rng.integers(0, k, n)] = 0
    return np.stack(meshes), faces, lifted, cams


@pytest.mark.parametrize("shape", [(1, 1, 5, 7), (2, 3, 33, 65), (3, 16, 203, 301), (1, 2, 480, 640)], ids=lambda s: "x".join(map(str, s)))
def test_geometry_at_the_shapes(shape):
    """a frame smaller than a tile, odd sizes with three slots, sixteen slots over three frames, the live frame: ellipsoids with
    a triangle soup, rejected vertices, duplicated faces, bad indices and an unlifted slot, a camera per frame"""
    n, k, h, w = shape
    meshes, faces, lifted, cams = _shape_scene(*shape)
    covered = _geometry_both_ways("x".join(map(str, shape)), meshes, faces, lifted if k > 1 else None, cams, h, w)
    assert covered >= h * w // 8


def test_geometry_is_the_occluded_raster_walk():
    """2 frames x 3 slots at 33 x 65 (no multiple of the 8 x 8 tile, an unlifted slot per frame), once with the host's four
    values and once with a camera per frame in a device table [2,4]: ops.mesh_geometry returns exactly the occluded
    ops.mesh_render's depth_out and silhouette & 0x7F -- both tile kernels make the one walk of csrc/mesh_raster.hip"""
    from hn_amd import ops
    n, k, h, w = 2, 3, 33, 65
    meshes, faces, lifted, cams = _shape_scene(n, k, h, w)
    mesh, fc_dev, lif, table = _device(meshes.reshape(n * k, -1, 3), faces, lifted.reshape(-1), cams)
    frame = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    scene = torch.full((n, h, w), 0.5, device="cuda")
    assert tuple(table.shape) == (2, 4) and not torch.equal(table[0], table[1])
    for tag, paras in (("four host values", tuple(float(x) for x in cams[0])), ("device table", table)):
        z = torch.full((n, h, w), -1.0, device="cuda")
        _img, sil, _cov = ops.mesh_render(mesh, fc_dev, paras, frame, lifted=lif, k=k, depth_out=z, scene_depth=scene, margin=0.0)
        depth, who = ops.mesh_geometry(mesh, fc_dev, paras, (h, w), lifted=lif, k=k)
        torch.cuda.synchronize()
        hidden = int((sil & 0x80).ne(0).sum())
        print(f"{tag}: {int(who.ne(0).sum())} covered pixels, {hidden} of them hidden, slots {sorted(set(who.unique().tolist()) - {0})}")
        assert int(who.ne(0).sum()) >= h * w // 8 and hidden > 0, tag      # (the hidden flag is there to be masked off)
        assert _bytes(depth) == _bytes(z) and _bytes(who) == _bytes(sil & 0x7F), tag


def test_geometry_refuses_bad_arguments():
    from hn_amd import ops
    mesh = torch.zeros((4, 5, 3), device="cuda")
    faces = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    good = dict(mesh=mesh, faces=faces, paras=(7.0, 7.0, 3.5, 2.5), hw=(5, 7), k=2)
    d, who = ops.mesh_geometry(**good)
    torch.cuda.synchronize()
    assert tuple(d.shape) == tuple(who.shape) == (2, 5, 7) and not d.any() and not who.any() and who.dtype == torch.uint8
    for kw in (dict(k=0), dict(k=17), dict(k=3), dict(mesh=torch.zeros((4, 5, 2), device="cuda")), dict(faces=np.zeros((2, 2), np.int32)),
               dict(faces=np.array([[0, 1, 5]])), dict(paras=torch.zeros((3, 4), device="cuda")), dict(lifted=torch.zeros(3, dtype=torch.int32, device="cuda")),
               dict(out_depth=torch.zeros((2, 5, 6), device="cuda")), dict(out_who=torch.zeros((2, 5, 7), device="cuda"))):
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            ops.mesh_geometry(**{**good, **kw})


# ---------------------------------------------------------------------------------------------------------- the iterated fit
def _filled(c, fill=0xFF):
    s, v = c.n * c.k, c.mesh.shape[1]
    return types.SimpleNamespace(fit_mesh=_raw(s * v * 12, fill).view(torch.float32).view(s, v, 3),
                                 fit_xyz=_raw(s * rc.JOINTS * 12, fill).view(torch.float32).view(s, rc.JOINTS, 3),
                                 fit_rt=_raw(s * 48, fill).view(torch.float32).view(s, 12),
                                 fit_count=_raw(s * 8, fill).view(torch.int32).view(s, 2), fit_cost=_raw(s * 8, fill).view(torch.int64),
                                 fit_trace=_raw(s * c.iters * 24, fill).view(torch.int64).view(s, c.iters, 3))


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fit_iters_against_the_rule(shape):
    """ops.mesh_fit_iters at the issue's four shapes on tessellated ellipsoids over ray-cast moved copies with noise and holes
    (a slot fitted in every iteration, a starved slot, an unlifted slot): the six outputs equal refit_ref.mesh_fit_iters bit for
    bit, written into buffers pre-filled with 0xFF; a second run gives the same bytes; so do a device camera table and the C
    entry on raw pointers; one iteration through the same entry is ops.mesh_fit"""
    from hn_amd import _lib, ops
    import fit_ref as fr
    c, want = rc.case(*shape), rc.expected(*shape)
    rc.check_conditions(c, want)
    best, sil, depth, mesh, xyz, faces, lifted = _device(c.best, c.sil, c.depth, c.mesh, c.xyz_mm, c.faces, c.lifted)
    kw = rc.kwargs(c)
    tag = "x".join(map(str, shape))
    out = _filled(c)
    got = ops.mesh_fit_iters(best, sil, depth, c.paras, mesh, xyz, faces, c.k, iters=c.iters, lifted=lifted, out=out, **kw)
    torch.cuda.synchronize()
    assert got.mesh.data_ptr() == out.fit_mesh.data_ptr() and got.trace.data_ptr() == out.fit_trace.data_ptr()
    _differ(got, want, tag)
    first = [_bytes(t) for t in got]
    again = ops.mesh_fit_iters(best, sil, depth, c.paras, mesh, xyz, faces, c.k, iters=c.iters, lifted=lifted, out=_filled(c, 0x00), **kw)
    table = torch.tensor([c.paras] * c.n, dtype=torch.float32, device="cuda")
    by_table = ops.mesh_fit_iters(best, sil, depth.unsqueeze(1), table, mesh, xyz, c.faces, c.k, iters=c.iters, lifted=lifted, **kw)
    torch.cuda.synchronize()
    assert [_bytes(t) for t in again] == first, "second run"
    assert [_bytes(t) for t in by_table] == first, "device table, host face list"
    # one iteration: the single fit's five outputs, and its (count, status, cost) as the trace
    one = ops.mesh_fit_iters(best, sil, depth, c.paras, mesh, xyz, faces, c.k, iters=1, lifted=lifted, **kw)
    single = ops.mesh_fit(best, sil, depth, c.paras, mesh, xyz, c.k, **kw)
    torch.cuda.synchronize()
    assert [_bytes(t) for t in one[:5]] == [_bytes(t) for t in single]
    assert torch.equal(one.trace[:, 0, :2], single.count.long()) and torch.equal(one.trace[:, 0, 2], single.cost)
    assert _bytes(one.count) == first[3] and _bytes(one.cost) == first[4]
    # the C entry on raw pointers
    lib = _lib.load()
    s, v, f = c.n * c.k, c.mesh.shape[1], c.faces.shape[0]
    need = lib.hn_mesh_fit_scratch_bytes(c.n, c.k, c.h)
    work_bytes = lib.hn_mesh_fit_iters_scratch_bytes(c.n, c.k, c.h, c.w, v, f, rc.JOINTS, c.iters)
    assert work_bytes == ops.mesh_fit_iters_scratch_bytes(c.n, c.k, c.h, c.w, v, f, rc.JOINTS, c.iters) > 0
    scratch, work = torch.empty((need,), dtype=torch.uint8, device="cuda"), _raw(work_bytes)
    raw = _filled(c)
    shift2, tan2 = fr.caps()
    st = lib.hn_mesh_fit_iters_f32(best.data_ptr(), sil.data_ptr(), depth.data_ptr(), c.h * c.w, None, table.data_ptr(), mesh.data_ptr(),
                                   xyz.data_ptr(), faces.data_ptr(), None, lifted.data_ptr(), c.n, c.k, c.h, c.w, v, f, rc.JOINTS, c.iters,
                                   c.stride, fr.FIT_BAND, c.min_points, fr.FIT_DAMP, shift2, tan2, scratch.data_ptr(), need,
                                   work.data_ptr(), work_bytes, *(getattr(raw, p).data_ptr() for p in PARTS),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.hn_last_error()
    assert [_bytes(getattr(raw, p)) for p in PARTS] == first


def test_fit_iters_refuses_bad_arguments():
    from hn_amd import ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    good = dict(mesh_depth=z(2, 5, 7), silhouette=z(2, 5, 7, dtype=torch.uint8), scene_depth=z(2, 1, 5, 7), paras=(7.0, 7.0, 3.5, 2.5),
                mesh=torch.ones((4, 3, 3), device="cuda"), xyz_mm=torch.ones((4, 21, 3), device="cuda"),
                faces=z(1, 3, dtype=torch.int32), k=2, iters=3)
    out = ops.mesh_fit_iters(**good)
    torch.cuda.synchronize()
    assert bool((out.mesh == 1).all()) and bool((out.xyz == 1).all()) and out.trace.tolist() == [[[0, 1, 0]] * 3] * 4
    assert out.rt.tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]] * 4 and out.count.tolist() == [[0, 1]] * 4 and not out.cost.any()
    assert out.trace.dtype == torch.int64 and tuple(out.trace.shape) == (4, 3, 3)
    for kw in (dict(iters=0), dict(iters=9), dict(iters=2.0), dict(iters=True), dict(k=0), dict(k=17), dict(faces=np.array([[0, 1, 3]])),
               dict(faces=z(0, 3, dtype=torch.int32)), dict(faces=z(2, 2, dtype=torch.int32)), dict(lifted=z(3, dtype=torch.int32)),
               dict(mesh=z(3, 3, 3)), dict(xyz_mm=z(5, 21, 3)), dict(scene_depth=z(1, 5, 7)), dict(paras=z(3, 4)), dict(stride=0),
               dict(band=0.0), dict(min_points=0), dict(damp=-1.0), dict(max_shift=0), dict(max_angle=4.0),
               dict(work=torch.zeros(16, dtype=torch.uint8, device="cuda"))):
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            ops.mesh_fit_iters(**{**good, **kw})
    with pytest.raises(TypeError):
        ops.mesh_fit_iters(**{k: v for k, v in good.items() if k != "iters"})


# ------------------------------------------------------------------------------------------------------------ whole steps
# (tests/test_fit_gpu.py's wide parameters: the synthetic pipeline's depth map is per-pixel noise in 0.3-1.5 m and its mesh a
# triangle soup -- a band and caps wide enough that a lifted slot is fitted; chosen for these frames, not for a camera)
FIT = dict(fit_band=1.0, fit_min_points=50, fit_max_shift=10.0, fit_max_angle=3.0)
RULE = dict(band=1.0, min_points=50, max_shift=10.0, max_angle=3.0)


def _slots(t, s):
    return t.numpy().reshape((s,) + tuple(t.shape[-2:]))


def _chain(tag, out, r, first, depth, paras, k, faces, iters, mesh=None, xyz=None):
    """refit_ref on the step's own device inputs -- `first` = (mesh depth, slot byte) its first iteration read, the depth map it
    ran on, the mesh it drew, the joints that go with it, its lifted flags -- against the six parts, bit for bit"""
    mesh = r.mesh if mesh is None else mesh
    xyz = (r.xyz_mm if hasattr(r, "xyz_mm") else r.more[1]) if xyz is None else xyz
    s = out.layout.slots
    lifted = (r.lifted if hasattr(r, "lifted") else r.has_hand).numpy().reshape(-1).astype(np.int32)
    want = rf.mesh_fit_iters(first[0], first[1], depth.cpu().numpy(), paras, _slots(mesh, s), _slots(xyz, s), np.asarray(faces), k, iters,
                             lifted=lifted, **RULE)
    print(f"{tag}: matches {want.trace[:, :, 0].tolist()}, status {want.trace[:, :, 1].tolist()}, cost {want.trace[:, :, 2].tolist()}")
    assert (want.trace[:, :, 1] == 0).all(axis=1).any(), (tag, "no slot was fitted in every iteration")
    got = types.SimpleNamespace(mesh=r.fit_mesh, xyz=r.fit_xyz, rt=r.fit_rt, count=r.fit_count, cost=r.fit_cost,
                                trace=r.fit_trace if iters > 1 else torch.from_numpy(want.trace))
    _differ(got, want, tag)
    for name in PARTS[:5 + (iters > 1)]:
        assert torch.equal(getattr(out, name).cpu().view(torch.uint8), getattr(r, name).view(torch.uint8)), (tag, name)
    return want


def _undrawn(out, r):
    """what a step without fit_draw fitted to: its raster's mesh depth and silhouette"""
    return out.mesh_depth.cpu().numpy(), r.silhouette.numpy()


def _check_drawn(tag, out, r, frames, depth, paras, k, faces, cloud_band=None):
    """a fit_draw step: overlay, silhouette, coverage and mesh depth equal ops.mesh_render of fit_mesh; the cloud equals
    cloud_ref on that raster"""
    from hn_amd import ops
    n, s = out.layout.frames, out.layout.slots
    lifted = (out.lifted.view(-1) if hasattr(out, "lifted") else out.hand.has_hand.view(-1)).contiguous()
    z = torch.full((n, H, W), -1.0, device="cuda")
    cams = paras if not isinstance(paras, np.ndarray) else torch.from_numpy(paras.astype(F)).cuda()
    img, sil, cov = ops.mesh_render(out.fit_mesh.reshape(s, -1, 3).contiguous(), torch.from_numpy(np.asarray(faces, np.int32)).cuda(), cams,
                                    frames, lifted=lifted, k=k, depth_out=z, scene_depth=depth, margin=ops.OCCLUDE_MARGIN)
    torch.cuda.synchronize()
    assert torch.equal(img.cpu(), r.overlay) and torch.equal(sil.cpu(), r.silhouette), tag
    assert torch.equal(cov.cpu().view(-1), r.coverage.view(-1)) and torch.equal(z, out.mesh_depth), tag
    assert int((sil != 0).sum()) >= 1000, (tag, "nothing drawn")
    if cloud_band is not None:
        want = cloud_ref.hand_cloud(z.cpu().numpy(), sil.cpu().numpy(), depth.cpu().numpy(), paras, k, cloud_ref.CLOUD_POINTS, cloud_band,
                                    cloud_ref.CLOUD_STRIDE, None)
        print(f"{tag}: the cloud of the fitted mesh: {want.count[:, 0].tolist()} points, resid (um) {want.resid.tolist()}")
        assert int(want.count[:, 0].sum()) >= 100
        for name, w in (("cloud", want.cloud), ("cloud_count", want.count), ("cloud_resid", want.resid)):
            assert _bytes(getattr(r, name)) == w.tobytes(), (tag, name)


def test_live_steps_end_to_end(parts, inputs, fcos_sd, a2j_sd, monkeypatch):  # noqa: F811
    """live_hands K = 2 and live on the synthetic pipeline.  fit_iters = 3: the six parts equal the reference chain on the step's
    own device inputs bit for bit, every other field and the host buffer's prefix are the fit=True step's.  fit_iters = 1:
    buffer bytes and launches are the fit=True step's.  fit_draw: the fit's parts are the same bytes, overlay, silhouette,
    coverage and mesh depth are ops.mesh_render of fit_mesh, the cloud is cloud_ref on that raster."""
    from hn_amd import ops
    _hand, lifter, perm, faces = parts
    rgb, depth = inputs
    net = _net(fcos_sd, a2j_sd)
    kw = dict(perm_reverse=perm, faces=faces, occlude=True, fit=True, **FIT)
    with torch.inference_mode():
        p_out, plain = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, **kw), rgb, depth)
        plain_host = p_out.host.clone()
        calls = []
        real = {name: getattr(ops, name) for name in ("mesh_fit", "mesh_fit_iters", "mesh_geometry", "mesh_render")}
        for name, fn in real.items():
            monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=fn, **k: calls.append(_n) or _f(*a, **k))
        o1, one = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, fit_iters=1, fit_draw=False, **kw), rgb, depth)
        assert calls == ["mesh_render", "mesh_fit"], calls
        del calls[:]
        out, r = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, fit_iters=3, **kw), rgb, depth)
        assert calls == ["mesh_render", "mesh_fit_iters"], calls
        del calls[:]
        d_out, drawn = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, fit_iters=3, fit_draw=True, cloud=True, cloud_band=1.0, **kw),
                            rgb, depth)
        assert calls == ["mesh_geometry", "mesh_fit_iters", "mesh_render"], calls
        del calls[:]
        d1_out, drawn1 = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, fit_draw=True, **kw), rgb, depth)
        assert calls == ["mesh_geometry", "mesh_fit", "mesh_render"], calls
        monkeypatch.undo()
    # one iteration, nothing redrawn: the fit=True step
    assert o1.layout == p_out.layout and torch.equal(o1.host, plain_host) and one._fields == plain._fields and o1.fit_trace is None
    # three iterations
    assert r._fields == plain._fields + ("fit_trace",) and type(r).__name__.endswith("FitTraceRead")
    assert tuple(r.fit_trace.shape) == (2, 2, 3, 3) and r.fit_trace.dtype == torch.int64 and tuple(out.fit_trace.shape) == (2, 2, 3, 3)
    _same(plain, r, [f for f in plain._fields if f not in ("fit_mesh", "fit_xyz", "fit_rt")], "three iterations: everything but the motion")
    at = out.layout.fit_mesh_at
    assert out.layout.nbytes > p_out.layout.nbytes and torch.equal(out.host[:at], plain_host[:at])
    assert torch.equal(out.mesh_depth, p_out.mesh_depth)
    want = _chain("live_hands K = 2, I = 3", out, r, _undrawn(out, r), depth, LIVE_PARAS, 2, faces, 3)
    assert torch.equal(r.fit_trace[:, :, 0, :2].reshape(-1, 2), plain.fit_count.reshape(-1, 2).long())
    assert not torch.equal(r.fit_mesh, plain.fit_mesh) and (want.trace[:, 1:, 1] == 0).any()
    # drawn from the fitted mesh: the same fit, another picture
    _same(r, drawn, PARTS, "fit_draw: the fit's parts")
    _same(plain, drawn1, PARTS[:5], "fit_draw, one iteration: the fit's parts")
    assert drawn1._fields == plain._fields and not torch.equal(drawn1.overlay, plain.overlay)
    for f in ("keypoints", "has_hand", "crop_box", "score", "xyz_mm", "lifted", "mesh", "words"):
        _same(r, drawn, (f,), "fit_draw: what is not drawn")
    _check_drawn("fit_draw I = 3", d_out, drawn, rgb, depth, LIVE_PARAS, 2, faces, cloud_band=1.0)
    _check_drawn("fit_draw I = 1", d1_out, drawn1, rgb, depth, LIVE_PARAS, 2, faces)
    assert not torch.equal(drawn.silhouette, r.silhouette)
    # the one-hand step
    with torch.inference_mode():
        lo, lr = _run(net.live(lifter, LIVE_PARAS, fit_iters=2, **kw), rgb, depth)
        ld, ldr = _run(net.live(lifter, LIVE_PARAS, fit_iters=2, fit_draw=True, **kw), rgb, depth)
    assert tuple(lr.fit_trace.shape) == (2, 2, 3) and lr._fields[-1] == "fit_trace"
    _chain("live, I = 2", lo, lr, _undrawn(lo, lr), depth, LIVE_PARAS, 1, faces, 2)
    _same(lr, ldr, PARTS, "live fit_draw: the fit's parts")
    _check_drawn("live fit_draw", ld, ldr, rgb, depth, LIVE_PARAS, 1, faces)


def test_graph_replay_and_raw_feed(parts):  # noqa: F811
    """One engine, one frame, fit_iters = 2 and fit_draw: the captured step equals the eager one byte for byte, twice; forward_raw
    with 16UC1 (millimetres) equals the fp32 feed of the same data; the capture owns its work buffers"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, occlude=True, fit=True, fit_iters=2, fit_draw=True, **FIT)
    ref = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, occlude=True, fit=True, fit_iters=2, **FIT)
    rng = np.random.default_rng(23)
    bgr = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    mm = rng.integers(300, 1500, size=(1, H, W)).astype(np.uint16)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    metres = torch.from_numpy(mm.astype(np.float32) / np.float32(1000.0)).unsqueeze(1).cuda()
    with torch.inference_mode():
        o_r, r = _run(ref, rgb, metres)
        _chain("eager, I = 2", o_r, r, _undrawn(o_r, r), metres, LIVE_PARAS, 2, faces, 2)
        o_e, e = _run(eng, rgb, metres)
        o_g, g = _run(eng, rgb, metres, graphed=True)
        first = o_g.host.clone()
        eng.graphed(rgb, metres)[0]()
        torch.cuda.synchronize()
        assert torch.equal(o_g.host, first)
        raw = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(mm))
        torch.cuda.synchronize()
        raw_read = raw.read()
    _same(r, e, PARTS, "fit_draw: the fit's parts")
    _same(e, g, e._fields, "graph replay")
    _same(e, raw_read, e._fields, "16UC1")
    _check_drawn("16UC1 fit_draw", raw, raw_read, rgb, metres, LIVE_PARAS, 2, faces)
    assert o_g.mesh_depth.data_ptr() != o_e.mesh_depth.data_ptr()
    assert eng._key_options()[-3:] == ("fit_iters", 2, True)
    work = [v for key, v in eng._mirrored.items() if key[0] == "cloud work"]
    # (graphed() and forward_raw share the one capture of these shapes: a step without `left` has no second key)
    assert len(work) == 1 and all(len(w) == 6 and all(t is not None for t in w[2:]) for w in work)
    assert work[0][0].data_ptr() == o_g.mesh_depth.data_ptr() == raw.mesh_depth.data_ptr()


def test_left_fits_to_the_mirrored_depth(parts, inputs):  # noqa: F811
    """left=True with fit_iters = 2 and fit_draw: the step equals the same step on frames and depth flipped along the width"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs[0][:1], inputs[1][:1]
    kw = dict(faces=faces, occlude=True, fit=True, fit_iters=2, **FIT)
    with torch.inference_mode():
        o_l, left = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, left=True, **kw), rgb, depth)
        flipped, frames = depth.flip(3).contiguous(), rgb.flip(3).contiguous()
        _o, want = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, **kw), frames, flipped)
        o_d, drawn = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, left=True, fit_draw=True, **kw), rgb, depth)
    _same(want, left, want._fields, "left")
    _chain("left, I = 2", o_l, left, _undrawn(o_l, left), flipped, LIVE_PARAS, 2, faces, 2)
    _same(left, drawn, PARTS, "left fit_draw: the fit's parts")
    _check_drawn("left fit_draw", o_d, drawn, frames, flipped, LIVE_PARAS, 2, faces)


def test_a_smoothed_step_iterates_on_the_signals_it_draws(parts, inputs):  # noqa: F811
    """track=True, smooth=True, fit_iters = 2: on the second step the chain runs on the smoothed mesh and joints (and not on the
    raw ones), and fit_draw leaves the smoothing state and the smoothed signals alone"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    kw = dict(track=True, smooth=True, faces=faces, occlude=True, fit=True, fit_iters=2, **FIT)
    nearer = (depth[:1] * 0.97).contiguous()
    got = []
    for draw in (False, True):
        eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, fit_draw=draw, **kw)
        eng.track_reset()
        with torch.inference_mode():
            _run(eng, rgb[:1], depth[:1])
            got.append(_run(eng, rgb[:1], nearer))
        eng.track_reset()
    (out, r), (o_d, drawn) = got
    assert bool(r.lifted.any()) and not torch.equal(r.smooth_mesh, r.mesh)
    want = _chain("smoothed, I = 2", out, r, _undrawn(out, r), nearer, LIVE_PARAS, 2, faces, 2, mesh=r.smooth_mesh, xyz=r.smooth_xyz)
    lifted = r.lifted.numpy().reshape(-1).astype(np.int32)
    raw = rf.mesh_fit_iters(*_undrawn(out, r), nearer.cpu().numpy(), LIVE_PARAS, _slots(r.mesh, 2), _slots(r.xyz_mm, 2), np.asarray(faces), 2, 2,
                            lifted=lifted, **RULE)
    assert raw.mesh.tobytes() != want.mesh.tobytes()
    _same(r, drawn, PARTS + ("smooth_xyz", "smooth_mesh", "mesh", "track_id"), "smoothed fit_draw")
    _check_drawn("smoothed fit_draw", o_d, drawn, rgb[:1], nearer, LIVE_PARAS, 2, faces)


def test_per_frame_cameras_and_set_cameras(parts, inputs):  # noqa: F811
    """paras [N,4], fit_iters = 2, fit_draw, captured: the chain equals the rule with a camera row per frame -- the first
    iteration's inputs drawn by the rule too --; after set_cameras the SAME graph's next replay follows the new rows"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    cams = np.array([LIVE_PARAS, (580.1, 600.7, 290.3, 260.9)])
    eng = LiveHandsEngine(hand, lifter, cams, 2, True, perm, faces=faces, occlude=True, fit=True, fit_iters=2, fit_draw=True, **FIT)

    def first(r, table):
        return rf.geometry_frames(_slots(r.mesh, 4), np.asarray(faces), table, 2, H, W, r.lifted.numpy().reshape(-1).astype(np.int32))
    with torch.inference_mode():
        out, r = _run(eng, rgb, depth, graphed=True)
        _chain("cameras", out, r, first(r, cams), depth, cams, 2, faces, 2)
        _check_drawn("cameras fit_draw", out, r, rgb, depth, cams, 2, faces)
        graphs = len(eng._graphs)
        new = cams[::-1].copy()
        eng.set_cameras(new)
        eng.graphed(rgb, depth)[0]()
        torch.cuda.synchronize()
        moved = out.read()
    assert len(eng._graphs) == graphs and not torch.equal(moved.fit_rt, r.fit_rt)
    _chain("after set_cameras", out, moved, first(moved, new), depth, new, 2, faces, 2)
    _check_drawn("after set_cameras", out, moved, rgb, depth, new, 2, faces)
