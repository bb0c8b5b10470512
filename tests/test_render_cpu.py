"""The overlay without a GPU: the numpy statement of the rule (tests/raster_ref.py) on cases that can be checked by hand, the
pinhole reduction of pyrender's IntrinsicsCamera, the extended buffer layouts, and the new entry points' declarations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import raster_ref as rr

UNIT = (1.0, 1.0, 0.0, 0.0)          # fx = fy = 1, cx = cy = 0: at Z = 1 a vertex (x, -y, -1) lands on pixel position (x, y)


def _flat(points):
    """pixel positions [(x, y)] -> out['mesh'] vertices at Z = 1 for the UNIT camera"""
    return np.array([[x, -y, -1.0] for x, y in points], np.float32)


@pytest.mark.parametrize("flip", [False, True])
def test_top_left_rule_on_a_shared_edge(flip):
    """A 4 x 4 pixel square (0.5, 0.5)-(4.5, 4.5) cut along its diagonal: every edge passes exactly through sample points.
    The top and left edges' samples belong to the square, the right and bottom ones do not; the diagonal's samples belong to
    the lower right triangle alone (for it the diagonal is a left edge).  Each of the 16 pixels is covered exactly once, for
    both windings."""
    v = _flat([(0.5, 0.5), (4.5, 0.5), (0.5, 4.5), (4.5, 4.5)])
    upper, lower = np.array([[0, 1, 2]]), np.array([[1, 3, 2]])
    if flip:
        upper, lower = upper[:, ::-1], lower[:, ::-1]
    ru, _ = rr.rasterize(v[None], upper, UNIT, 8, 8)
    rl, _ = rr.rasterize(v[None], lower, UNIT, 8, 8)
    want_u = np.zeros((8, 8), bool)
    want_l = np.zeros((8, 8), bool)
    for r in range(4):
        for c in range(4):
            (want_u if c + r <= 3 else want_l)[r, c] = True
    assert np.array_equal(ru.count == 1, want_u) and int(ru.count.sum()) == 10
    assert np.array_equal(rl.count == 1, want_l) and int(rl.count.sum()) == 6
    both, _ = rr.rasterize(v[None], np.concatenate([upper, lower]), UNIT, 8, 8)
    assert np.array_equal(both.count, (want_u | want_l).astype(np.int64))
    assert np.all(both.z1[want_u | want_l] == 1.0) and np.all(np.isinf(both.z2))


def test_degenerate_rejected_and_outside_faces_draw_nothing():
    v = _flat([(0.5, 0.5), (4.5, 0.5), (2.5, 0.5), (0.5, 4.5)])
    ras, _ = rr.rasterize(v[None], np.array([[0, 1, 2], [0, 0, 3]]), UNIT, 8, 8)            # collinear; repeated vertex
    assert int(ras.count.sum()) == 0
    for bad in ([np.nan, 0, -1], [0, np.inf, -1], [0, 0, -0.04], [0, 0, -101.0], [0, 0, 1.0], [70000.0, 0, -1]):
        vv = v.copy()
        vv[0] = bad
        ras, _ = rr.rasterize(vv[None], np.array([[0, 1, 3]]), UNIT, 8, 8)
        assert int(ras.count.sum()) == 0, bad
    ras, _ = rr.rasterize(v[None], np.array([[0, 1, 3]]), UNIT, 8, 8, lifted=[0])
    assert int(ras.count.sum()) == 0
    ras, _ = rr.rasterize(v[None], np.array([[0, 1, 4]]), UNIT, 8, 8)                       # index beyond the mesh
    assert int(ras.count.sum()) == 0
    far = _flat([(-40.5, -30.5), (-10.5, -30.5), (-40.5, -3.5)])                             # wholly left of / above the frame
    ras, _ = rr.rasterize(far[None], np.array([[0, 1, 2]]), UNIT, 8, 8)
    assert int(ras.count.sum()) == 0


def test_closed_ellipsoids_cover_every_pixel_an_even_number_of_times():
    """The issue's two-ellipsoid scene: no crack and no double hit along any shared edge (every covered pixel is covered 2 or
    4 times), 777 vertices / 1550 faces each, and depth fights stay rare (the cap of test_render_gpu.py: 1 %)."""
    paras = (615.0, 615.0, 320.0, 240.0)
    v1, f = rr.ellipsoid((0.02, -0.01, 0.55), (0.05, 0.08, 0.03))
    v2, _ = rr.ellipsoid((0.06, 0.02, 0.56), (0.06, 0.04, 0.04))
    assert v1.shape == (777, 3) and f.shape == (1550, 3)
    ras, _ = rr.rasterize(np.stack([v1, v2]), f, paras, 480, 640)
    covered = ras.count > 0
    assert covered.sum() > 15000
    assert set(np.unique(ras.count[covered]).tolist()) <= {2, 4}
    amb = rr.ambiguous(ras)
    print(f"covered {int(covered.sum())}, ambiguous {int(amb.sum())} ({amb.sum() / covered.sum():.2%})")
    assert amb.sum() <= 0.01 * covered.sum()
    # the nearer surface wins: in front of the first ellipsoid's centre the depth is its front pole's
    row, col = int(round(240 - 0.5 + 615 * -0.01 / 0.52)), int(round(320 - 0.5 + 615 * 0.02 / 0.52))
    assert abs(ras.z1[row, col] - 0.52) < 2e-3


def test_shading_formula():
    a, b, c = np.array([0, 0, -0.5]), np.array([0.01, 0, -0.5]), np.array([0, 0.01, -0.5])
    assert rr.face_colour(a, b, c).tolist() == [255, 255, 230]            # facing the camera: 0.3 + 2.4 / pi > 1 -> clamped
    assert rr.face_colour(a, c, b).tolist() == [255, 255, 230]            # either winding
    edge_on = rr.face_colour(a, b, np.array([0, 0, -0.51]))               # normal across the view axis: ambient only
    assert edge_on.tolist() == [int(np.floor(255 * 0.3 + 0.5)), int(np.floor(255 * 0.3 + 0.5)), int(np.floor(255 * 0.27 + 0.5))]
    tilted = rr.face_colour(a, b, np.array([0, 0.01, -0.51]))             # 45 degrees: l = cos 45
    shade = 0.3 + 2.4 * np.sqrt(0.5) / np.pi
    assert tilted.tolist() == [int(np.floor(255 * shade + 0.5))] * 2 + [int(np.floor(255 * shade * 0.9 + 0.5))]


def test_pyrender_intrinsics_camera_reduces_to_the_pinhole():
    """pyrender's IntrinsicsCamera.get_projection_matrix (width W, height H, znear 0.05, zfar 100), written out from its
    definition, applied to the OpenGL-camera point (x, y, z) = (X, -Y, -Z) and mapped to window coordinates with row 0 at the
    top: u = fx X / Z + cx, v = fy Y / Z + cy."""
    rng = np.random.default_rng(0)
    fx, fy, cx, cy, W, H, zn, zf = 617.343, 615.1, 312.42, 241.42, 640, 480, 0.05, 100.0
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2.0 * fx / W, 2.0 * fy / H
    P[0, 2], P[1, 2] = 1.0 - 2.0 * cx / W, 2.0 * cy / H - 1.0
    P[2, 2], P[2, 3] = (zf + zn) / (zn - zf), 2.0 * zf * zn / (zn - zf)
    P[3, 2] = -1.0
    X, Y = rng.uniform(-0.5, 0.5, 1000), rng.uniform(-0.5, 0.5, 1000)
    Z = rng.uniform(0.2, 3.0, 1000)
    clip = P @ np.stack([X, -Y, -Z, np.ones_like(Z)])
    ndc = clip[:3] / clip[3]
    win_x = (ndc[0] + 1.0) * 0.5 * W
    win_y_from_top = H - (ndc[1] + 1.0) * 0.5 * H          # OpenGL's window origin is the bottom left corner
    assert np.abs(win_x - (fx * X / Z + cx)).max() < 1e-9
    assert np.abs(win_y_from_top - (fy * Y / Z + cy)).max() < 1e-9
    assert np.all(np.abs(ndc[2]) < 1.0)


@pytest.mark.parametrize("n,k,v", [(1, 1, 778), (1, 2, 778), (32, 2, 778)])
def test_overlay_layout_keeps_every_offset(n, k, v):
    from hn_amd.live import LiveHandsOutput, LiveHandsRead, LiveLayout, LiveOutput
    from hn_amd.pipeline import record_bytes
    h, w, s = 48, 64, n * k
    plain, ext = LiveLayout(n, k, v), LiveLayout(n, k, v, (h, w), overlay=True)
    front = lambda a: (a.record_rows, a.record_bytes, a.side_at, a.lifted_at, a.mesh_at)
    assert front(ext) == front(plain) and plain.overlay_at is None and ext.overlay_at == plain.nbytes
    assert ext.nbytes == plain.nbytes + n * h * w * 3
    one_plain, one_ext = LiveLayout(n, None, v), LiveLayout(n, None, v, (h, w), overlay=True)
    mo, oo, total = one_ext.mesh_at, one_ext.overlay_at, one_ext.nbytes
    assert mo == (n + 1) * record_bytes(3) and oo == mo + n * v * 12 and total == oo + n * h * w * 3
    assert front(one_plain) == front(one_ext) and one_plain.nbytes == oo and one_plain.overlay_at is None
    # a step without faces: read().overlay is None and the read has the fields it always had
    host = torch.zeros((plain.nbytes,), dtype=torch.uint8)
    out = LiveHandsOutput(None, None, None, torch.empty((n, k, v, 3)), None, host, n, k, layout=plain)
    r = out.read()
    assert out.overlay is None and r.overlay is None and isinstance(r, LiveHandsRead) and "overlay" not in r._fields
    assert len(r) == 10
    one = LiveOutput(None, None, torch.empty((n, v, 3)), None, torch.zeros((mo + n * v * 12,), dtype=torch.uint8), n,
                     layout=one_plain)
    r1 = one.read()
    assert one.overlay is None and r1.overlay is None and len(r1) == 6
    # a step with faces: the overlay is read from behind the mesh, everything else from where it was
    g = torch.Generator().manual_seed(n * k)
    host = torch.randint(0, 256, (ext.nbytes,), generator=g, dtype=torch.uint8)
    host[:plain.mesh_at] = 0
    shown = LiveHandsOutput(None, None, None, torch.empty((n, k, v, 3)), None, host, n, k, None,
                            torch.empty((n, h, w, 3), dtype=torch.uint8), layout=ext).read()
    assert torch.equal(shown.overlay, host[plain.nbytes:].view(n, h, w, 3)) and shown.overlay.dtype == torch.uint8
    assert torch.equal(shown.mesh.view(torch.uint8).view(-1), host[plain.mesh_at:plain.nbytes])
    assert tuple(shown.mesh.shape) == (n, k, v, 3)
    host1 = torch.randint(0, 256, (total,), generator=g, dtype=torch.uint8)
    host1[:mo] = 0
    r1 = LiveOutput(None, None, torch.empty((n, v, 3)), None, host1, n, None, torch.empty((n, h, w, 3), dtype=torch.uint8),
                    layout=one_ext).read()
    assert len(r1) == 7 and torch.equal(r1.overlay, host1[oo:].view(n, h, w, 3)) and tuple(r1.mesh.shape) == (n, v, 3)


def test_faces_need_perm_reverse_and_valid_indices():
    """The engines refuse faces= without perm_reverse= before they touch anything, and the host-side face check names the
    offending index."""
    import inspect
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import ops
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    for fn in (HandNet.live, HandNet.live_hands, LiveHandEngine.__init__, LiveHandsEngine.__init__):
        assert inspect.signature(fn).parameters["faces"].default is None
    with pytest.raises(ValueError, match="778 vertices"):
        ops.mesh_faces(np.array([[0, 1, 778]]), 778, "cpu")
    with pytest.raises(ValueError, match="vertices"):
        ops.mesh_faces(np.array([[0, 1, -1]]), 778, "cpu")
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        ops.mesh_faces(np.zeros((0, 3), np.int64), 778, "cpu")
    f = ops.mesh_faces(np.array([[0, 1, 777]], np.int64), 778, "cpu")
    assert f.dtype == torch.int32 and f.tolist() == [[0, 1, 777]]

    class _Hand:
        device = "cpu"

        def set_convert(self, **kw):
            pass

    class _Graph:
        v = 1280

    class _Lifter:
        device = "cpu"
        graphs = [_Graph()]
    with pytest.raises(ValueError, match="perm_reverse"):
        LiveHandsEngine(_Hand(), _Lifter(), (600.0, 600.0, 320.0, 240.0), 2, True, None, faces=np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="perm_reverse"):
        LiveHandEngine(_Hand(), _Lifter(), (600.0, 600.0, 320.0, 240.0), True, None, faces=np.array([[0, 1, 2]]))


def test_render_entry_points_are_declared_bound_and_exported():
    import subprocess
    from hn_amd import _lib, build
    text = (build.REPO_ROOT / "include" / "handnet_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    for name in ("hn_mesh_render_u8", "hn_mesh_render_scratch_bytes"):
        proto = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert proto, name
        params = [p.strip() for p in proto.group(2).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, a in zip(params, args):       # pointers are pointers, int64 is int64, the rest are C ints
            if "*" in p:
                assert a in (C.c_void_p, _lib.c_f32p), (name, p)
            elif p.startswith("int64_t"):
                assert a is C.c_int64, (name, p)
            else:
                assert p.startswith("int ") and a is C.c_int, (name, p)
        assert res is (C.c_int64 if proto.group(1) == "int64_t" else C.c_int)
        assert re.search(r" T %s\b" % name, out), name
    assert re.search(r"#define HN_FRAME_F32_CHW (\d)", text).group(1) == str(_lib.FRAME_F32_CHW)
    assert re.search(r"#define HN_FRAME_U8_BGR_HWC (\d)", text).group(1) == str(_lib.FRAME_U8_BGR_HWC)
    assert _lib.load().hn_abi_version() == 36          # additive functions keep the version (the header's rule)


def test_render_argument_errors_do_not_need_a_gpu():
    """Every argument check of hn_mesh_render_u8 comes before its first launch: bad calls return HN_ERR_ARG and set
    hn_last_error without a device (the pointers below are never dereferenced, except the HOST intrinsics and face list)."""
    from hn_amd import _lib
    lib = _lib.load()
    need = lib.hn_mesh_render_scratch_bytes(2, 1538)
    assert need >= 2 * 1538 * 48 and lib.hn_mesh_render_scratch_bytes(0, 5) == 0 and lib.hn_mesh_render_scratch_bytes(2, 0) == 0
    paras = (C.c_float * 4)(600, 600, 320, 240)
    faces_host = (C.c_int32 * 6)(0, 1, 2, 2, 3, 4)
    P = 4096        # stands for a device address

    def call(mesh=P, faces=P, fh=None, s=2, v=4, f=2, k=2, frame=P, fmt=0, h=480, w=640, scratch=P, sb=need, out=P, depth=None):
        return lib.hn_mesh_render_u8(mesh, faces, fh, None, s, v, f, k, paras, frame, fmt, h, w, scratch, sb, out, depth, None)
    for kw, word in ((dict(v=0), b"positive"), (dict(f=0), b"positive"), (dict(s=0), b"positive"), (dict(out=None), b"out_image"),
                     (dict(mesh=None), b"null"), (dict(scratch=None), b"null"), (dict(k=3), b"multiple"), (dict(fmt=2), b"format"),
                     (dict(sb=16), b"scratch"), (dict(scratch=P + 4), b"aligned"), (dict(w=0), b"frame size"),
                     (dict(fh=C.cast(faces_host, C.c_void_p)), b"face 1 uses vertex 4 of 4")):
        assert call(**kw) == 1, kw
        assert word in lib.hn_last_error(), (kw, lib.hn_last_error())
