"""The hand cloud on the GPU (csrc/hand_cloud.hip through ops.hand_cloud and hn_hand_cloud_f32, and the live steps with
cloud=True) against the rule in numpy float32 (tests/cloud_ref.py), bit for bit: no tolerance appears in this file."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import cloud_cases as cc
import cloud_ref as cr
import rig_cases as rc
import rig_ref as rr
from test_occlude_gpu import H, LIVE_PARAS, W, _net, _run, _same, inputs, parts  # noqa: F401  (the synthetic pipeline's fixtures)

pytestmark = pytest.mark.gpu

RIG_SEED = 5
FIELDS = ("cloud", "count", "resid")


def _bytes(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).tobytes()


def _differ(got, want, tag):
    """every output against the rule's, as bytes; the figures are printed before they are asserted"""
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        g = g.reshape(w.shape)
        assert g.dtype == w.dtype, (tag, name, g.dtype, w.dtype)
        differ = int((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum())
        print(f"{tag}: {name} {g.shape}: {differ} bytes differ")
        assert differ == 0, (tag, name, differ)


def _filled(c, fill=0xFF):
    """outputs pre-filled with `fill` bytes, as the `out=` object of ops.hand_cloud"""
    s = c.n * c.k
    raw = lambda nbytes: torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")  # noqa: E731
    return types.SimpleNamespace(cloud=raw(s * c.points * 12).view(torch.float32).view(s, c.points, 3),
                                 cloud_count=raw(s * 8).view(torch.int32).view(s, 2), cloud_resid=raw(s * 8).view(torch.int64))


def _device(c):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return d(c.best), d(c.sil), d(c.depth)


# ---------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_against_the_rule(shape):
    """ops.hand_cloud at the issue's five shapes on seeded silhouettes (blobs, hidden flags, bytes that name no slot, an empty
    slot), best in 0.3-1.2, D = best + noise over +-2 band with holes of the five kinds and the band's exact edges: the three
    outputs equal cloud_ref bit for bit, written into buffers pre-filled with 0xFF; a second run gives the same bytes; so do a
    device table of equal rows in place of the host's four values and an RGB-D-shaped depth tensor; the rig frame with a
    seeded [N,12] table equals the rule's; and the C entry on raw pointers gives the same bytes once more."""
    from hn_amd import _lib, ops
    c, want = cc.case(*shape), cc.expected(*shape)
    cc.check_conditions(c, want)
    for (i, r, col, inside) in c.edges:                              # the band's edges fall where the rule puts them
        assert (cr.matches(c.best[i], c.sil[i], c.depth[i], c.k, c.band, c.stride)[r, col] >= 0) == inside
    best, sil, depth = _device(c)
    kw = dict(points=c.points, band=c.band, stride=c.stride)
    out = _filled(c)
    got = ops.hand_cloud(best, sil, depth, c.paras, c.k, out=out, **kw)
    torch.cuda.synchronize()
    assert got.cloud.data_ptr() == out.cloud.data_ptr() and got.resid.data_ptr() == out.cloud_resid.data_ptr()
    tag = "x".join(map(str, shape))
    _differ(got, want, tag)
    first = [_bytes(t) for t in got]
    again = ops.hand_cloud(best, sil, depth, c.paras, c.k, out=_filled(c, 0x00), **kw)
    table = torch.tensor([c.paras] * c.n, dtype=torch.float32, device="cuda")
    by_table = ops.hand_cloud(best, sil, depth, table, c.k, **kw)
    rgbd = torch.full((c.n, 4, c.h, c.w), float("nan"), device="cuda")
    rgbd[:, 3] = depth
    by_rgbd = ops.hand_cloud(best, sil, rgbd, c.paras, c.k, **kw)
    by_4d = ops.hand_cloud(best, sil, depth.unsqueeze(1), c.paras, c.k, **kw)
    torch.cuda.synchronize()
    for other, name in ((again, "second run"), (by_table, "device table"), (by_rgbd, "RGB-D"), (by_4d, "[N,1,H,W]")):
        assert [_bytes(t) for t in other] == first, name
    # the rig frame
    ext = torch.from_numpy(ops.rig_extrinsics(rc.extrinsics(c.n, seed=RIG_SEED), c.n)).cuda()
    rig = ops.hand_cloud(best, sil, depth, c.paras, c.k, extrinsics_table=ext, out=_filled(c), **kw)
    torch.cuda.synchronize()
    _differ(rig, cc.expected(*shape, rig_seed=RIG_SEED), tag + " rig")
    assert _bytes(rig.count) == first[1] and _bytes(rig.resid) == first[2] and _bytes(rig.cloud) != first[0]
    # the C entry on raw pointers
    lib = _lib.load()
    need = lib.hn_hand_cloud_scratch_bytes(c.n, c.k, c.h)
    assert need == ops.hand_cloud_scratch_bytes(c.n, c.k, c.h) > 0
    scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
    raw = _filled(c)
    st = lib.hn_hand_cloud_f32(best.data_ptr(), sil.data_ptr(), rgbd.data_ptr() + 3 * c.h * c.w * 4, 4 * c.h * c.w,
                               (C.c_float * 4)(*c.paras), None, None, c.n, c.k, c.h, c.w, c.points, c.stride, c.band,
                               scratch.data_ptr(), need, raw.cloud.data_ptr(), raw.cloud_count.data_ptr(), raw.cloud_resid.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.hn_last_error()
    assert [_bytes(raw.cloud), _bytes(raw.cloud_count), _bytes(raw.cloud_resid)] == first


def test_the_op_refuses_bad_arguments():
    from hn_amd import ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    good = dict(mesh_depth=z(2, 5, 7), silhouette=z(2, 5, 7, dtype=torch.uint8), scene_depth=z(2, 1, 5, 7), paras=(7.0, 7.0, 3.5, 2.5), k=2)
    out = ops.hand_cloud(**good, points=3)
    torch.cuda.synchronize()
    assert tuple(out.cloud.shape) == (4, 3, 3) and not out.cloud.any() and not out.count.any() and not out.resid.any()
    assert out.count.dtype == torch.int32 and out.resid.dtype == torch.int64
    for kw in (dict(k=0), dict(k=17), dict(scene_depth=z(2, 2, 5, 7)), dict(scene_depth=z(1, 5, 7)), dict(mesh_depth=z(2, 5, 6)),
               dict(paras=z(3, 4)), dict(paras=z(2, 4).double()), dict(extrinsics_table=z(3, 12)), dict(points=0), dict(stride=0),
               dict(band=0.0), dict(band=float("nan")), dict(band=100.5), dict(points=2.5), dict(silhouette=z(2, 1, 5, 7, dtype=torch.uint8))):
        with pytest.raises((ValueError, TypeError)):
            ops.hand_cloud(**{**good, **kw})
    with pytest.raises(TypeError):
        ops.hand_cloud(**{**good, "silhouette": z(2, 5, 7)})


# ------------------------------------------------------------------------------------------------------------ whole steps
BAND = 1.0                 # wide, so that a step has at least FLOOR points in all
FLOOR = 100


def _rule(out, r, depth, paras, k, band=BAND, table=None, points=cr.CLOUD_POINTS, stride=cr.CLOUD_STRIDE):
    """cloud_ref on what the step itself left: its mesh depth (device), its silhouette (read()) and the depth map it ran on"""
    return cr.hand_cloud(out.mesh_depth.cpu().numpy(), r.silhouette.numpy(), depth.cpu().numpy(), paras, k, points, band, stride, table)


def _check_read(tag, out, r, depth, paras, k, **kw):
    want = _rule(out, r, depth, paras, k, **kw)
    total = int(want.count[:, 0].sum())
    print(f"{tag}: {total} points, per slot {want.count[:, 0].tolist()}, resid (um) {want.resid.tolist()}")
    assert total >= FLOOR, (tag, total)
    _differ(types.SimpleNamespace(cloud=r.cloud, count=r.cloud_count, resid=r.cloud_resid), want, tag)
    for name, dev in (("cloud", out.cloud), ("cloud_count", out.cloud_count), ("cloud_resid", out.cloud_resid)):
        assert torch.equal(dev.cpu(), getattr(r, name)), (tag, name)
    return want


def test_live_steps_end_to_end(parts, inputs, fcos_sd, a2j_sd):  # noqa: F811
    """live_hands K = 2 and live with cloud=True on the synthetic pipeline: read().cloud / .cloud_count / .cloud_resid equal
    cloud_ref(out.mesh_depth, read().silhouette, the step's depth, paras) bit for bit; every other field equals the same
    engine's without cloud, bit for bit, and the host buffer's prefix is unchanged."""
    _hand, lifter, perm, faces = parts
    rgb, depth = inputs
    net = _net(fcos_sd, a2j_sd)
    kw = dict(perm_reverse=perm, faces=faces, occlude=True)
    with torch.inference_mode():
        out, r = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, cloud=True, cloud_band=BAND, **kw), rgb, depth)
        host = out.host.clone()
        p_out, plain = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, **kw), rgb, depth)
    assert r._fields == plain._fields + ("cloud", "cloud_count", "cloud_resid") and type(r).__name__.endswith("CloudRead")
    assert tuple(r.cloud.shape) == (2, 2, 4096, 3) and tuple(r.cloud_count.shape) == (2, 2, 2) and tuple(r.cloud_resid.shape) == (2, 2)
    assert r.cloud.dtype == torch.float32 and r.cloud_count.dtype == torch.int32 and r.cloud_resid.dtype == torch.int64
    assert tuple(out.cloud.shape) == (2, 2, 4096, 3) and tuple(out.mesh_depth.shape) == (2, H, W) and p_out.cloud is None
    _same(plain, r, plain._fields, "K = 2")
    assert host.numel() == out.layout.nbytes > p_out.host.numel() and torch.equal(host[:p_out.host.numel()], p_out.host)
    want = _check_read("live_hands K = 2", out, r, depth, LIVE_PARAS, 2)
    # the points are where the camera saw them: every written point reprojects to its pixel's centre within the rounding of
    # three fp32 operations, and lies under its slot's silhouette
    fx, fy, cx, cy = LIVE_PARAS
    sil = r.silhouette.numpy()
    for s in range(4):
        pts = want.cloud[s, :want.count[s, 1]].astype(np.float64)
        u, v = pts[:, 0] * fx / pts[:, 2] + cx - 0.5, pts[:, 1] * fy / pts[:, 2] + cy - 0.5
        assert np.abs(u - np.rint(u)).max(initial=0) < 1e-3 and np.abs(v - np.rint(v)).max(initial=0) < 1e-3
        assert ((sil[s // 2, np.rint(v).astype(int), np.rint(u).astype(int)] & 0x7F) == s % 2 + 1).all()
    with torch.inference_mode():
        o1, one = _run(net.live(lifter, LIVE_PARAS, cloud=True, cloud_band=BAND, **kw), rgb, depth)
        _o, one_plain = _run(net.live(lifter, LIVE_PARAS, **kw), rgb, depth)
    assert one._fields == one_plain._fields + ("cloud", "cloud_count", "cloud_resid")
    assert tuple(one.cloud.shape) == (2, 4096, 3) and tuple(one.cloud_count.shape) == (2, 2) and tuple(one.cloud_resid.shape) == (2,)
    _same(one_plain, one, one_plain._fields, "live")
    _check_read("live", o1, one, depth, LIVE_PARAS, 1)


def test_graph_replay_and_raw_feed(parts):  # noqa: F811
    """One engine, one frame: the captured step equals the eager one; forward_raw with 16UC1 (millimetres) equals the fp32
    feed of the same data, and its cloud is cut out of the static input the ingest kernel wrote."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, occlude=True, cloud=True, cloud_band=BAND)
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
    assert ("cloud", 4096, BAND, 2, "camera") == eng._key_options()[2:7]


def test_left_cuts_the_mirrored_depth(parts, inputs):  # noqa: F811
    """left=True: the cloud equals the plain cloud step's on frames and depth flipped along the width, and the rule applied
    to the mirrored depth map"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs[0][:1], inputs[1][:1]
    kw = dict(faces=faces, occlude=True, cloud=True, cloud_band=BAND)
    with torch.inference_mode():
        o_l, left = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, left=True, **kw), rgb, depth)
        flipped = depth.flip(3).contiguous()
        _o, want = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, **kw), rgb.flip(3).contiguous(), flipped)
    _same(want, left, want._fields, "left")
    _check_read("left", o_l, left, flipped, LIVE_PARAS, 2)


def test_a_smoothed_step_cuts_against_the_mesh_it_draws(parts, inputs):  # noqa: F811
    """track=True, smooth=True: on the second step the filter's output is no longer the raw mesh; the mesh depth the cloud is
    cut against is the smoothed mesh's (the plain cloud step's differs), and the cloud equals the rule on it"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    kw = dict(faces=faces, occlude=True, cloud=True, cloud_band=BAND)
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, track=True, smooth=True, **kw)
    eng.track_reset()
    with torch.inference_mode():
        _run(eng, rgb[:1], depth[:1])
        nearer = (depth[:1] * 0.97).contiguous()
        out, r = _run(eng, rgb[:1], nearer)
        smooth_depth = out.mesh_depth.clone()
        assert r._fields[-7:] == ("smooth_xyz", "smooth_mesh", "silhouette", "coverage", "cloud", "cloud_count", "cloud_resid")
        assert bool(r.lifted.any()) and not torch.equal(r.smooth_mesh, r.mesh)
        _check_read("smoothed", out, r, nearer, LIVE_PARAS, 2)
        # what the smoothed mesh draws: the overlay's own depth output for smooth_mesh, from a plain render call
        from hn_amd import ops
        redo = torch.zeros_like(smooth_depth)
        ops.mesh_render(r.smooth_mesh.cuda(), eng.faces, LIVE_PARAS, rgb[:1].contiguous(), lifted=r.lifted.int().cuda().view(-1), k=2,
                        depth_out=redo)
        raw = torch.zeros_like(smooth_depth)
        ops.mesh_render(r.mesh.cuda(), eng.faces, LIVE_PARAS, rgb[:1].contiguous(), lifted=r.lifted.int().cuda().view(-1), k=2, depth_out=raw)
        torch.cuda.synchronize()
    assert torch.equal(redo, smooth_depth) and not torch.equal(raw, smooth_depth)
    eng.track_reset()


def test_per_frame_cameras_and_set_cameras(parts, inputs):  # noqa: F811
    """paras [N,4]: the captured step's cloud equals the rule with a camera row per frame; after set_cameras the SAME graph's
    next replay gives the rule's cloud with the new rows"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    cams = np.array([LIVE_PARAS, (580.1, 600.7, 290.3, 260.9)])
    eng = LiveHandsEngine(hand, lifter, cams, 2, True, perm, faces=faces, occlude=True, cloud=True, cloud_band=BAND)
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
    assert len(eng._graphs) == graphs and not torch.equal(moved.cloud, r.cloud)
    _check_read("after set_cameras", out, moved, depth, new, 2)


def test_rig_frame_and_set_extrinsics(parts, inputs):  # noqa: F811
    """cloud_frame="rig" on two cameras: the cloud equals the rule with the extrinsics table; count and resid equal the camera
    frame's; after set_extrinsics the same graph's next replay follows the new table; identity extrinsics give the camera
    frame's cloud bit for bit"""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    ext, new = rc.extrinsics(2, seed=3), rc.extrinsics(2, seed=12)
    kw = dict(faces=faces, occlude=True, cloud=True, cloud_band=BAND)
    with torch.inference_mode():
        _o, cam = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, extrinsics=ext, **kw), rgb, depth)
        eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, extrinsics=ext, cloud_frame="rig", **kw)
        out, r = _run(eng, rgb, depth, graphed=True)
        _check_read("rig", out, r, depth, LIVE_PARAS, 2, table=rr.table(ext))
        assert torch.equal(r.cloud_count, cam.cloud_count) and torch.equal(r.cloud_resid, cam.cloud_resid)
        assert not torch.equal(r.cloud, cam.cloud)
        _same(cam, r, [f for f in cam._fields if f != "cloud"], "rig against camera")
        graphs = len(eng._graphs)
        eng.set_extrinsics(new)
        eng.graphed(rgb, depth)[0]()
        torch.cuda.synchronize()
        moved = out.read()
        assert len(eng._graphs) == graphs and not torch.equal(moved.cloud, r.cloud)
        _check_read("after set_extrinsics", out, moved, depth, LIVE_PARAS, 2, table=rr.table(new))
        identity = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (2, 1, 1))
        _o, same = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, extrinsics=identity, cloud_frame="rig", **kw), rgb, depth)
    assert torch.equal(same.cloud, cam.cloud)
