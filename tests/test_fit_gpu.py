"""The mesh fit on the GPU (csrc/mesh_fit.hip through ops.mesh_fit and hn_mesh_fit_f32, and the live steps with fit=True)
against the rule in numpy (tests/fit_ref.py), bit for bit: no tolerance appears in this file."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import fit_cases as fc
import fit_ref as fr
from test_occlude_gpu import H, LIVE_PARAS, W, _net, _run, _same, inputs, parts  # noqa: F401  (the synthetic pipeline's fixtures)

pytestmark = pytest.mark.gpu

FIELDS = ("mesh", "xyz", "rt", "count", "cost")
PARTS = ("fit_mesh", "fit_xyz", "fit_rt", "fit_count", "fit_cost")


def _bytes(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).tobytes()


def _differ(got, want, tag):
    """every output against the rule's, as bytes; the figures are printed before they are asserted"""
    bad = []
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        g = g.reshape(w.shape)
        assert g.dtype == w.dtype, (tag, name, g.dtype, w.dtype)
        differ = int((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum())
        print(f"{tag}: {name} {g.shape}: {differ} bytes differ")
        if differ:
            bad.append((name, differ))
    assert not bad, (tag, bad)


def _filled(c, v, fill=0xFF):
    """outputs pre-filled with `fill` bytes, as the `out=` object of ops.mesh_fit"""
    s = c.n * c.k
    raw = lambda nbytes: torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")  # noqa: E731
    return types.SimpleNamespace(fit_mesh=raw(s * v * 12).view(torch.float32).view(s, v, 3),
                                 fit_xyz=raw(s * fc.JOINTS * 12).view(torch.float32).view(s, fc.JOINTS, 3),
                                 fit_rt=raw(s * 48).view(torch.float32).view(s, 12),
                                 fit_count=raw(s * 8).view(torch.int32).view(s, 2), fit_cost=raw(s * 8).view(torch.int64))


def _device(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ---------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_against_the_rule(shape):
    """ops.mesh_fit at the issue's five shapes with V = 5 and V = 778 on ray-cast ellipsoids (slots drawn over each other, hidden
    flags, bytes that name no slot, holes of the five kinds, the band's exact edges, slots of all four statuses over the set):
    the five outputs equal fit_ref bit for bit, written into buffers pre-filled with 0xFF; a second run gives the same bytes;
    so do a device table of equal rows in place of the host's four values, an RGB-D-shaped depth tensor and the C entry on raw
    pointers."""
    from hn_amd import _lib, ops
    c = fc.case(*shape)
    want, census = fc.expected(*shape)
    fc.check_conditions(c, want, census)
    fc.check_statuses()
    best, sil, depth, xyz = _device(c.best, c.sil, c.depth, c.xyz_mm)
    kw = fc.kwargs(c)
    tag = "x".join(map(str, shape))
    for v in fc.VERTICES:
        mesh, = _device(c.meshes[v])
        out = _filled(c, v)
        got = ops.mesh_fit(best, sil, depth, c.paras, mesh, xyz, c.k, out=out, **kw)
        torch.cuda.synchronize()
        assert got.mesh.data_ptr() == out.fit_mesh.data_ptr() and got.cost.data_ptr() == out.fit_cost.data_ptr()
        _differ(got, fc.expected(*shape, v=v)[0], f"{tag} V={v}")
    first = [_bytes(t) for t in got]
    again = ops.mesh_fit(best, sil, depth, c.paras, mesh, xyz, c.k, out=_filled(c, v, 0x00), **kw)
    table = torch.tensor([c.paras] * c.n, dtype=torch.float32, device="cuda")
    by_table = ops.mesh_fit(best, sil, depth, table, mesh, xyz, c.k, **kw)
    rgbd = torch.full((c.n, 4, c.h, c.w), float("nan"), device="cuda")
    rgbd[:, 3] = depth
    by_rgbd = ops.mesh_fit(best, sil, rgbd, c.paras, mesh, xyz, c.k, **kw)
    by_4d = ops.mesh_fit(best, sil, depth.unsqueeze(1), c.paras, mesh, xyz, c.k, **kw)
    torch.cuda.synchronize()
    for other, name in ((again, "second run"), (by_table, "device table"), (by_rgbd, "RGB-D"), (by_4d, "[N,1,H,W]")):
        assert [_bytes(t) for t in other] == first, name
    # the C entry on raw pointers
    lib = _lib.load()
    need = lib.hn_mesh_fit_scratch_bytes(c.n, c.k, c.h)
    assert need == ops.mesh_fit_scratch_bytes(c.n, c.k, c.h) > 0
    scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
    raw = _filled(c, v)
    shift2, tan2 = fr.caps(c.max_shift, c.max_angle)
    st = lib.hn_mesh_fit_f32(best.data_ptr(), sil.data_ptr(), rgbd.data_ptr() + 3 * c.h * c.w * 4, 4 * c.h * c.w,
                             (C.c_float * 4)(*c.paras), None, mesh.data_ptr(), xyz.data_ptr(), c.n, c.k, c.h, c.w, v, fc.JOINTS,
                             c.stride, c.band, c.min_points, c.damp, shift2, tan2, scratch.data_ptr(), need,
                             *(getattr(raw, p).data_ptr() for p in PARTS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.hn_last_error()
    assert [_bytes(getattr(raw, p)) for p in PARTS] == first


def test_the_op_refuses_bad_arguments():
    from hn_amd import ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    good = dict(mesh_depth=z(2, 5, 7), silhouette=z(2, 5, 7, dtype=torch.uint8), scene_depth=z(2, 1, 5, 7), paras=(7.0, 7.0, 3.5, 2.5),
                mesh=torch.ones((4, 3, 3), device="cuda"), xyz_mm=torch.ones((4, 21, 3), device="cuda"), k=2)
    out = ops.mesh_fit(**good)
    torch.cuda.synchronize()
    assert tuple(out.mesh.shape) == (4, 3, 3) and bool((out.mesh == 1).all()) and bool((out.xyz == 1).all())
    assert out.count.tolist() == [[0, 1]] * 4 and not out.cost.any() and out.rt.tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]] * 4
    assert out.count.dtype == torch.int32 and out.cost.dtype == torch.int64
    for kw in (dict(k=0), dict(k=17), dict(scene_depth=z(2, 2, 5, 7)), dict(scene_depth=z(1, 5, 7)), dict(mesh_depth=z(2, 5, 6)),
               dict(paras=z(3, 4)), dict(paras=z(2, 4).double()), dict(mesh=z(3, 3, 3)), dict(mesh=z(4, 3, 2)), dict(xyz_mm=z(4, 21)),
               dict(xyz_mm=z(5, 21, 3)), dict(stride=0), dict(band=0.0), dict(band=float("nan")), dict(band=100.5), dict(min_points=0),
               dict(min_points=2.5), dict(damp=-1.0), dict(max_shift=0), dict(max_angle=4.0),
               dict(silhouette=z(2, 1, 5, 7, dtype=torch.uint8))):
        with pytest.raises((ValueError, TypeError)):
            ops.mesh_fit(**{**good, **kw})
    with pytest.raises(TypeError):
        ops.mesh_fit(**{**good, "silhouette": z(2, 5, 7)})
    with pytest.raises(TypeError):
        ops.mesh_fit(**{**good, "mesh": good["mesh"].double()})


# ------------------------------------------------------------------------------------------------------------ whole steps
# the synthetic pipeline's depth map is per-pixel noise in 0.3-1.5 m and its mesh a triangle soup: a band and caps wide enough
# that a lifted slot is fitted (status 0) -- chosen for these frames, not for a camera
FIT = dict(fit_band=1.0, fit_min_points=50, fit_max_shift=10.0, fit_max_angle=3.0)
RULE = dict(band=1.0, min_points=50, max_shift=10.0, max_angle=3.0)


def _rule(out, r, depth, paras, k, mesh, xyz):
    """fit_ref on what the step itself left: its mesh depth (device), its silhouette, the depth map it ran on, the mesh it drew
    and the joints that go with it (read())"""
    s = mesh.shape[0] * (mesh.shape[1] if k > 1 or mesh.dim() == 4 else 1)
    return fr.mesh_fit(out.mesh_depth.cpu().numpy(), r.silhouette.numpy(), depth.cpu().numpy(), paras, mesh.numpy().reshape(s, -1, 3),
                       xyz.numpy().reshape(s, -1, 3), k, **RULE)


def _check_read(tag, out, r, depth, paras, k, mesh=None, xyz=None):
    mesh = r.mesh if mesh is None else mesh
    xyz = (r.xyz_mm if hasattr(r, "xyz_mm") else r.more[1]) if xyz is None else xyz
    want = _rule(out, r, depth, paras, k, mesh, xyz)
    print(f"{tag}: matches per slot {want.count[:, 0].tolist()}, status {want.count[:, 1].tolist()}, cost {want.cost.tolist()}")
    assert (want.count[:, 1] == 0).any(), (tag, "no slot was fitted")
    _differ(types.SimpleNamespace(mesh=r.fit_mesh, xyz=r.fit_xyz, rt=r.fit_rt, count=r.fit_count, cost=r.fit_cost), want, tag)
    for name in PARTS:
        assert torch.equal(getattr(out, name).cpu().view(torch.uint8), getattr(r, name).view(torch.uint8)), (tag, name)
    return want


def test_live_steps_end_to_end(parts, inputs, fcos_sd, a2j_sd, monkeypatch):  # noqa: F811
    """live_hands K = 2 and live with fit=True on the synthetic pipeline: the five parts equal fit_ref(out.mesh_depth,
    read().silhouette, the step's depth, read().mesh, read().xyz_mm) bit for bit with at least one slot fitted; every other
    field equals the same engine's without fit, bit for bit, and the host buffer's prefix is unchanged; with the cloud on as
    well both options' parts are what each gives alone.  The step without fit calls neither ops.mesh_fit nor asks the raster
    for its depth, and owns no work buffers."""
    from hn_amd import ops
    _hand, lifter, perm, faces = parts
    rgb, depth = inputs
    net = _net(fcos_sd, a2j_sd)
    kw = dict(perm_reverse=perm, faces=faces, occlude=True)
    with torch.inference_mode():
        out, r = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, fit=True, **FIT, **kw), rgb, depth)
        host = out.host.clone()
        both_out, both = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, fit=True, cloud=True, cloud_band=1.0, **FIT, **kw), rgb, depth)
        _c, cloud = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, cloud=True, cloud_band=1.0, **kw), rgb, depth)
        calls = []
        real_render = ops.mesh_render
        monkeypatch.setattr(ops, "mesh_fit", lambda *a, **k: calls.append("mesh_fit"))
        monkeypatch.setattr(ops, "mesh_fit_scratch_bytes", lambda *a, **k: calls.append("scratch"))
        monkeypatch.setattr(ops, "mesh_render", lambda *a, **k: calls.append(("render", k.get("depth_out"))) or real_render(*a, **k))
        plain_eng = net.live_hands(lifter, LIVE_PARAS, max_hands=2, **kw)
        p_out, plain = _run(plain_eng, rgb, depth)
        monkeypatch.undo()
    assert calls == [("render", None)] and plain_eng._buffers[(2, (H, W))][3] is None and plain_eng.fit is None
    assert r._fields == plain._fields + PARTS and type(r).__name__.endswith("FitRead")
    assert [tuple(getattr(r, p).shape) for p in PARTS] == [(2, 2, 778, 3), (2, 2, 21, 3), (2, 2, 12), (2, 2, 2), (2, 2)]
    assert [getattr(r, p).dtype for p in PARTS] == [torch.float32] * 3 + [torch.int32, torch.int64]
    assert tuple(out.fit_mesh.shape) == (2, 2, 778, 3) and tuple(out.mesh_depth.shape) == (2, H, W) and p_out.fit_mesh is None
    assert out.cloud is None and p_out.mesh_depth is None
    _same(plain, r, plain._fields, "K = 2")
    assert host.numel() == out.layout.nbytes > p_out.host.numel() and torch.equal(host[:p_out.host.numel()], p_out.host)
    want = _check_read("live_hands K = 2", out, r, depth, LIVE_PARAS, 2)
    # a fitted slot's mesh is the drawn mesh moved by fit_rt about the root joint (fp64 here: a sanity check of the meaning,
    # the bits are checked above); a slot that is not fitted keeps its bytes
    for s in range(4):
        mesh, xyz = r.mesh.reshape(4, 778, 3)[s].numpy(), r.xyz_mm.reshape(4, 21, 3)[s].numpy()
        if want.count[s, 1] != 0:
            assert want.mesh[s].tobytes() == mesh.tobytes() and want.xyz[s].tobytes() == xyz.tobytes()
            continue
        rt, c0 = want.rt[s].astype(np.float64), xyz[0].astype(np.float64) / 1000.0
        cam = mesh.astype(np.float64) * [1, -1, -1]
        moved = ((cam - c0) @ rt[:9].reshape(3, 3).T + c0 + rt[9:]) * [1, -1, -1]
        assert np.abs(moved - want.mesh[s]).max() <= 1e-5 * max(1.0, np.abs(moved).max())
    # fit and cloud together: each option's parts are what it gives alone
    assert both._fields == plain._fields + ("cloud", "cloud_count", "cloud_resid") + PARTS
    _same(cloud, both, cloud._fields, "with the cloud: the cloud's parts")
    _same(r, both, PARTS, "with the cloud: the fit's parts")
    with torch.inference_mode():
        o1, one = _run(net.live(lifter, LIVE_PARAS, fit=True, **FIT, **kw), rgb, depth)
        _o, one_plain = _run(net.live(lifter, LIVE_PARAS, **kw), rgb, depth)
    assert one._fields == one_plain._fields + PARTS
    assert [tuple(getattr(one, p).shape) for p in PARTS] == [(2, 778, 3), (2, 21, 3), (2, 12), (2, 2), (2,)]
    _same(one_plain, one, one_plain._fields, "live")
    _check_read("live", o1, one, depth, LIVE_PARAS, 1)


def test_graph_replay_and_raw_feed(parts):  # noqa: F811
    """One engine, one frame: the captured step equals the eager one byte for byte; forward_raw with 16UC1 (millimetres)
    equals the fp32 feed of the same data, and its fit reads the static input the ingest kernel wrote."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, occlude=True, fit=True, **FIT)
    rng = np.random.default_rng(23)
    bgr = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    mm = rng.integers(300, 1500, size=(1, H, W)).astype(np.uint16)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    metres = torch.from_numpy(mm.astype(np.float32) / np.float32(1000.0)).unsqueeze(1).cuda()
    with torch.inference_mode():
        o_e, e = _run(eng, rgb, metres)
        _check_read("eager", o_e, e, metres, LIVE_PARAS, 2)
        o_g, g = _run(eng, rgb, metres, graphed=True)
        raw = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(mm))
        torch.cuda.synchronize()
    _same(e, g, e._fields, "graph replay")
    _same(e, raw.read(), e._fields, "16UC1")
    assert o_g.mesh_depth.data_ptr() != o_e.mesh_depth.data_ptr() != raw.mesh_depth.data_ptr()
    _check_read("16UC1", raw, raw.read(), metres, LIVE_PARAS, 2)
    assert eng._key_options()[2:] == ("fit", 1.0, 2, 50, 1e-3, 10.0, 3.0)


def test_left_fits_to_the_mirrored_depth(parts, inputs):  # noqa: F811
    """left=True: the fit equals the plain fit step's on frames and depth flipped along the width, and the rule applied to
    the mirrored depth map"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs[0][:1], inputs[1][:1]
    kw = dict(faces=faces, occlude=True, fit=True, **FIT)
    with torch.inference_mode():
        o_l, left = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, left=True, **kw), rgb, depth)
        flipped = depth.flip(3).contiguous()
        _o, want = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, **kw), rgb.flip(3).contiguous(), flipped)
    _same(want, left, want._fields, "left")
    _check_read("left", o_l, left, flipped, LIVE_PARAS, 2)


def test_a_smoothed_step_moves_the_signals_it_draws(parts, inputs):  # noqa: F811
    """track=True, smooth=True: on the second step the filter's output is no longer the raw mesh; the fit equals the rule on
    the smoothed mesh and joints (and not on the raw ones)"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, track=True, smooth=True, faces=faces, occlude=True, fit=True, **FIT)
    eng.track_reset()
    with torch.inference_mode():
        _run(eng, rgb[:1], depth[:1])
        nearer = (depth[:1] * 0.97).contiguous()
        out, r = _run(eng, rgb[:1], nearer)
    assert r._fields[-9:] == ("smooth_xyz", "smooth_mesh", "silhouette", "coverage") + PARTS
    assert bool(r.lifted.any()) and not torch.equal(r.smooth_mesh, r.mesh)
    want = _check_read("smoothed", out, r, nearer, LIVE_PARAS, 2, mesh=r.smooth_mesh, xyz=r.smooth_xyz)
    raw = _rule(out, r, nearer, LIVE_PARAS, 2, r.mesh, r.xyz_mm)
    assert raw.mesh.tobytes() != want.mesh.tobytes()
    eng.track_reset()


def test_per_frame_cameras_and_set_cameras(parts, inputs):  # noqa: F811
    """paras [N,4]: the captured step's fit equals the rule with a camera row per frame; after set_cameras the SAME graph's
    next replay gives the rule's fit with the new rows"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    cams = np.array([LIVE_PARAS, (580.1, 600.7, 290.3, 260.9)])
    eng = LiveHandsEngine(hand, lifter, cams, 2, True, perm, faces=faces, occlude=True, fit=True, **FIT)
    with torch.inference_mode():
        out, r = _run(eng, rgb, depth, graphed=True)
        _check_read("cameras", out, r, depth, cams, 2)
        graphs = len(eng._graphs)
        new = cams[::-1].copy()
        eng.set_cameras(new)
        run = eng.graphed(rgb, depth)[0]
        run()
        torch.cuda.synchronize()
        moved = out.read()
    assert len(eng._graphs) == graphs and not torch.equal(moved.fit_rt, r.fit_rt)
    _check_read("after set_cameras", out, moved, depth, new, 2)
