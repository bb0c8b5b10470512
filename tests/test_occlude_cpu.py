"""The occluded overlay without a GPU: the numpy statement of the rule (tests/occlude_ref.py) on cases that can be checked by
hand, the extended buffer layout, and the new entry point's declaration, binding and argument checks."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import occlude_ref as oc
import raster_ref as rr

UNIT = (1.0, 1.0, 0.0, 0.0)          # fx = fy = 1, cx = cy = 0: at Z = z a vertex (x z, -y z, -z) lands on pixel position (x, y)
H, W = 16, 24


def _square(x0, y0, x1, y1, z=1.0):
    """A flat square over pixel positions (x0, y0)-(x1, y1) at depth z for the UNIT camera: (vertices [4,3], faces [2,3])"""
    v = np.array([[x * z, -y * z, -z] for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))], np.float32)
    return v, np.array([[0, 1, 2], [2, 1, 3]], np.int32)


def _frame(seed=0):
    return rr.frame_bgr8(1, H, W, seed)[0]


def _run(meshes, faces, depth, margin=0.0, lifted=None, frame=None):
    frame = _frame() if frame is None else frame
    return oc.render(np.asarray(meshes, np.float32), faces, UNIT, frame, depth, margin, lifted), rr.frame_u8(frame)


def test_a_square_in_front_of_behind_and_across_a_depth_plane():
    """A 12 x 8 pixel square at Z = 1: in front of a plane at 2 m everything is shown, behind a plane at 0.5 m everything is
    hidden and the image is the frame, and across the tilted plane D = 1 + 0.01 (col - 8) the columns left of 8 are hidden
    (D < 1), column 8 is not (D = 1: the comparison is strict) and the margin moves the cut by margin / 0.01 columns."""
    v, f = _square(2.5, 3.5, 14.5, 11.5)
    inside = np.zeros((H, W), bool)
    inside[3:11, 2:14] = True
    front, f8 = _run(v[None], f, np.full((H, W), 2.0, np.float32))
    assert np.array_equal(front.covered, inside) and not front.hidden.any()
    assert np.array_equal(front.silhouette, inside.astype(np.uint8)) and front.coverage.tolist() == [[96, 96]]
    assert np.array_equal(front.image[inside], np.tile(rr.face_colour(v[0], v[1], v[2]), (96, 1)))
    assert np.array_equal(front.image[~inside], f8[~inside])
    behind, f8 = _run(v[None], f, np.full((H, W), 0.5, np.float32))
    assert np.array_equal(behind.hidden, inside) and np.array_equal(behind.image, f8)
    assert np.array_equal(behind.silhouette, np.where(inside, 0x81, 0)) and behind.coverage.tolist() == [[96, 0]]
    plane = np.float32(1.0) + np.float32(0.01) * (np.arange(W, dtype=np.float32)[None, :] - 8).repeat(H, 0)
    across, f8 = _run(v[None], f, plane)
    want = inside & (np.arange(W)[None, :] < 8)
    assert np.array_equal(across.hidden, want) and across.coverage.tolist() == [[96, 96 - 8 * 6]]
    assert np.array_equal(across.image[want], f8[want]) and not np.array_equal(across.image[inside & ~want], f8[inside & ~want])
    assert across.threshold[3:11, 8].all() and int(across.threshold.sum()) == 8       # D + margin == best on column 8 only
    moved, _ = _run(v[None], f, plane, margin=0.025)           # hidden where 1 > D + 0.025: col - 8 < -2.5
    assert np.array_equal(moved.hidden, inside & (np.arange(W)[None, :] < 6))


def test_invalid_depth_never_hides():
    """D = 0 (a 16UC1 hole), NaN (a 32FC1 hole), +inf, -inf and a negative value hide nothing, whatever the margin."""
    v, f = _square(2.5, 3.5, 14.5, 11.5)
    for bad in (0.0, np.nan, np.inf, -np.inf, -0.5):
        for margin in (0.0, 0.03, -1e3):
            got, f8 = _run(v[None], f, np.full((H, W), bad, np.float32), margin)
            assert not got.hidden.any() and not got.threshold.any(), (bad, margin)
            assert got.coverage.tolist() == [[96, 96]] and int((got.silhouette == 1).sum()) == 96
    # ... and only those: a map hiding everything, with one hole of each kind
    d = np.full((H, W), 0.5, np.float32)
    d[5, 4], d[5, 5], d[5, 6], d[5, 7] = 0.0, np.nan, np.inf, -1.0
    got, _ = _run(v[None], f, d)
    assert got.coverage.tolist() == [[96, 4]] and (got.silhouette[5, 4:8] == 1).all() and got.silhouette[5, 8] == 0x81


def test_huge_margins():
    """margin = +1e3 hides nothing; margin = -1e3 hides every covered pixel whose D is valid."""
    v, f = _square(2.5, 3.5, 14.5, 11.5)
    d = np.random.default_rng(3).uniform(0.3, 1.5, (H, W)).astype(np.float32)
    d[6, 6], d[7, 7] = 0.0, np.nan
    plain, _, _, _ = rr.render(v[None], f, UNIT, _frame())
    none, _ = _run(v[None], f, d, 1e3)
    assert not none.hidden.any() and np.array_equal(none.image, plain) and not (none.silhouette & oc.HIDDEN).any()
    every, f8 = _run(v[None], f, d, -1e3)
    assert np.array_equal(every.hidden, every.covered & oc.valid_depth(d)) and int(every.hidden.sum()) == 94
    assert np.array_equal(every.image[every.hidden], f8[every.hidden]) and every.coverage.tolist() == [[96, 2]]


def test_the_nearer_slot_wins_and_its_id_is_in_the_silhouette():
    """Two slots: a square at Z = 1 (slot 0) and an overlapping one at Z = 0.8 (slot 1).  Slot 1 wins the overlap, the
    silhouette carries 2 there, a plane at 0.9 m hides slot 0's pixels alone, and a slot that is not lifted counts (0, 0)."""
    a, f = _square(2.5, 3.5, 14.5, 11.5, 1.0)
    b, _ = _square(10.5, 1.5, 20.5, 9.5, 0.8)
    in_a, in_b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    in_a[3:11, 2:14], in_b[1:9, 10:20] = True, True
    got, f8 = _run(np.stack([a, b]), f, np.full((H, W), 0.9, np.float32))
    assert np.array_equal(got.slot == 1, in_b) and np.array_equal(got.slot == 0, in_a & ~in_b)
    assert np.array_equal(got.silhouette, np.where(in_b, 2, np.where(in_a, 0x81, 0)))
    assert got.coverage.tolist() == [[96 - 24, 0], [80, 80]]
    assert np.array_equal(got.slot2[in_a & in_b], np.zeros(24, np.int64)) and (got.slot2[~(in_a & in_b)] == -1).all()
    assert np.array_equal(got.image[in_a & ~in_b], f8[in_a & ~in_b])
    only_a, _ = _run(np.stack([a, b]), f, np.full((H, W), 0.9, np.float32), lifted=[1, 0])
    assert only_a.coverage.tolist() == [[96, 0], [0, 0]] and np.array_equal(only_a.silhouette, np.where(in_a, 0x81, 0))


def test_coverage_is_what_one_counts_off_the_silhouette():
    """On the interpenetrating ellipsoids under a noise depth map: coverage equals the counts of the silhouette's values,
    slot by slot, and both kinds of pixel occur."""
    e1, f = rr.ellipsoid((0.02, -0.01, 0.55), (0.05, 0.08, 0.03), rings=9, segs=11)
    e2, _ = rr.ellipsoid((0.06, 0.02, 0.56), (0.06, 0.04, 0.04), rings=9, segs=11)
    d = np.random.default_rng(11).uniform(0.45, 0.65, (120, 160)).astype(np.float32)
    frame = rr.frame_bgr8(1, 120, 160, 4)[0]
    got = oc.render(np.stack([e1, e2]), f, (154.0, 154.0, 80.0, 60.0), frame, d, 0.01)
    sil = got.silhouette
    for s in range(2):
        assert got.coverage[s, 0] == int(((sil & 0x7F) == s + 1).sum()) > 200
        assert got.coverage[s, 1] == int((sil == s + 1).sum())
        assert 50 < got.coverage[s, 1] < got.coverage[s, 0] - 50
    assert int(got.coverage[:, 0].sum()) == int(got.covered.sum()) == int((sil != 0).sum())
    assert np.array_equal(oc.count(sil, 2), got.coverage)


FRAMES, HANDS, SIZES = (1, 2, 3, 32), (None, 1, 2, 3, 16), ((5, 7), (48, 64), (480, 640))


def test_occluded_layout_appends_two_aligned_parts_and_moves_nothing():
    """LiveLayout(..., occluded=True) over the golden table's frames x hands x sizes grid (5 x 7 frames included, whose images
    end off a dword), with and without labels, sides, tracker and filter: silhouette uint8 [frames,h,w] and then coverage int32
    [slots,2] are the last parts, each on a dword; every offset in front of them, the record rows and bytes equal the layout
    without the option, whose views keep their class and fields."""
    from hn_amd.live import LiveLayout, LiveSmoothedViews, LiveTrackedViews, LiveViews
    front = ("record_rows", "record_bytes", "side_at", "track_id_at", "track_age_at", "lifted_at", "mesh_at", "overlay_at",
             "box_label_at", "pose_label_at", "smooth_xyz_at", "smooth_mesh_at")
    padded = 0
    for n in FRAMES:
        for k in HANDS:
            for hw in SIZES:
                for labels in (False, True):
                    for handed, tracked, smoothed in ((False, False, False),) + (
                            () if k is None else ((True, False, False), (False, True, False), (True, True, True))):
                        plain = LiveLayout(n, k, 778, hw, True, labels, handed, tracked, smoothed)
                        ext = LiveLayout(n, k, 778, hw, True, labels, handed, tracked, smoothed, occluded=True)
                        assert [getattr(ext, c) for c in front] == [getattr(plain, c) for c in front]
                        assert plain.silhouette_at is None and plain.coverage_at is None and not plain.occluded
                        s = n * (k or 1)
                        assert ext.silhouette_at % 4 == 0 and ext.coverage_at % 4 == 0
                        assert plain.nbytes <= ext.silhouette_at < plain.nbytes + 4
                        assert ext.silhouette_at + n * hw[0] * hw[1] <= ext.coverage_at < ext.silhouette_at + n * hw[0] * hw[1] + 4
                        assert ext.nbytes == ext.coverage_at + s * 8
                        padded += (ext.silhouette_at != plain.nbytes) + (ext.coverage_at != ext.silhouette_at + n * hw[0] * hw[1])
                        if n > 3 or hw[0] > 48:
                            continue
                        buf = torch.zeros((ext.nbytes,), dtype=torch.uint8)
                        v, pv = ext.views(buf), plain.views(buf[:plain.nbytes])
                        kind = LiveSmoothedViews if smoothed else LiveTrackedViews if tracked else LiveViews
                        assert type(pv) is kind and v._fields == kind._fields + ("silhouette", "coverage")
                        assert v.silhouette.dtype == torch.uint8 and tuple(v.silhouette.shape) == (n,) + hw
                        assert v.coverage.dtype == torch.int32 and tuple(v.coverage.shape) == (s, 2)
                        assert v.silhouette.data_ptr() - buf.data_ptr() == ext.silhouette_at
                        assert v.coverage.data_ptr() - buf.data_ptr() == ext.coverage_at
                        for name in kind._fields:
                            a, b = getattr(v, name), getattr(pv, name)
                            assert (a is None) == (b is None)
                            if a is not None:
                                assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype
    assert padded > 0
    with pytest.raises(ValueError, match="overlay"):
        LiveLayout(1, 2, 778, (48, 64), False, True, occluded=True)
    with pytest.raises(ValueError, match="overlay"):
        LiveLayout(1, None, 778, occluded=True)


def test_read_appends_silhouette_and_coverage_behind_every_other_field():
    from hn_amd.live import LiveHandsOutput, LiveHandsOverlayRead, LiveLayout, LiveOutput, LiveOverlayRead
    n, k, v, hw = 2, 2, 5, (5, 7)
    g = torch.Generator().manual_seed(1)
    for tracked, smoothed in ((False, False), (True, True)):
        plain = LiveLayout(n, k, v, hw, True, False, False, tracked, smoothed)
        ext = LiveLayout(n, k, v, hw, True, False, False, tracked, smoothed, occluded=True)
        host = torch.randint(0, 256, (ext.nbytes,), generator=g, dtype=torch.uint8)
        host[:plain.mesh_at] = 0
        r = LiveHandsOutput(None, None, None, None, None, host, n, k, layout=ext).read()
        p = LiveHandsOutput(None, None, None, None, None, host[:plain.nbytes], n, k, layout=plain).read()
        assert r._fields == p._fields + ("silhouette", "coverage") and type(r).__name__.endswith("OccludedRead")
        if not tracked:
            assert type(p) is LiveHandsOverlayRead
        assert tuple(r.silhouette.shape) == (n,) + hw and r.silhouette.dtype == torch.uint8
        assert tuple(r.coverage.shape) == (n, k, 2) and r.coverage.dtype == torch.int32
        assert torch.equal(r.silhouette.view(-1), host[ext.silhouette_at:ext.silhouette_at + n * 35])
        assert torch.equal(r.coverage.view(torch.uint8).view(-1), host[ext.coverage_at:])
        for a, b in zip(r[:len(p)], p):
            assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    plain1, ext1 = LiveLayout(n, None, v, hw, True), LiveLayout(n, None, v, hw, True, occluded=True)
    host = torch.randint(0, 256, (ext1.nbytes,), generator=g, dtype=torch.uint8)
    host[:plain1.mesh_at] = 0
    r1 = LiveOutput(None, None, None, None, host, n, layout=ext1).read()
    p1 = LiveOutput(None, None, None, None, host[:plain1.nbytes], n, layout=plain1).read()
    assert type(p1) is LiveOverlayRead and r1._fields == p1._fields + ("silhouette", "coverage") and len(r1) == 9
    assert tuple(r1.coverage.shape) == (n, 2) and tuple(r1.silhouette.shape) == (n,) + hw


def test_entry_point_is_declared_bound_and_exported():
    import subprocess
    from hn_amd import _lib, build
    name = "hn_mesh_render_occluded_u8"
    text = (build.REPO_ROOT / "include" / "handnet_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert proto and name in _lib.SIGNATURES
    params = [p.strip() for p in proto.group(1).split(",")]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(params) == len(args) == 23
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (C.c_void_p, _lib.c_f32p), p
        elif p.startswith("int64_t"):
            assert a is C.c_int64, p
        elif p.startswith("float"):
            assert a is C.c_float, p
        else:
            assert p.startswith("int ") and a is C.c_int, p
    # the arguments of hn_mesh_render_u8, in its order, plus the five new ones
    old = re.search(r"\bint\s+hn_mesh_render_u8\s*\(([^)]*)\)\s*;", text).group(1)
    names = lambda ps: [re.split(r"[\s*]+", p.strip())[-1] for p in ps]
    new_names = names(params)
    assert [p for p in new_names if p in names(old.split(","))] == names(old.split(","))
    assert [p for p in new_names if p not in names(old.split(","))] == ["scene_depth", "depth_frame_stride", "margin",
                                                                        "out_silhouette", "out_coverage"]
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s\b" % name, out)
    lib = _lib.load()
    assert getattr(lib, name) is not None and lib.hn_abi_version() == 36 == _lib.ABI_VERSION   # an additive function


def test_argument_errors_do_not_need_a_gpu():
    """Every argument check of hn_mesh_render_occluded_u8 comes before its first launch: the renderer's own refusals under the
    new name, and a null scene_depth / out_silhouette, a short frame stride, k > 16 and a margin that is not finite."""
    from hn_amd import _lib
    lib = _lib.load()
    need = lib.hn_mesh_render_scratch_bytes(2, 1538)
    paras = (C.c_float * 4)(600, 600, 320, 240)
    faces_host = (C.c_int32 * 6)(0, 1, 2, 2, 3, 4)
    P = 4096        # stands for a device address

    def call(mesh=P, faces=P, fh=None, s=2, v=4, f=2, k=2, frame=P, fmt=0, h=480, w=640, depth=P, stride=480 * 640, margin=0.03,
             scratch=P, sb=need, out=P, zout=None, sil=P, cov=None):
        return lib.hn_mesh_render_occluded_u8(mesh, faces, fh, None, s, v, f, k, paras, frame, fmt, h, w, depth, stride, margin,
                                              scratch, sb, out, zout, sil, cov, None)
    for kw, word in ((dict(v=0), b"positive"), (dict(f=0), b"positive"), (dict(s=0), b"positive"), (dict(out=None), b"out_image"),
                     (dict(mesh=None), b"null"), (dict(scratch=None), b"null"), (dict(k=3), b"multiple"), (dict(fmt=2), b"format"),
                     (dict(sb=16), b"scratch"), (dict(scratch=P + 4), b"aligned"), (dict(w=0), b"frame size"),
                     (dict(fh=C.cast(faces_host, C.c_void_p)), b"face 1 uses vertex 4 of 4"),
                     (dict(depth=None), b"scene_depth is NULL"), (dict(sil=None), b"out_silhouette is NULL"),
                     (dict(stride=480 * 640 - 1), b"depth_frame_stride"), (dict(s=34, k=17, sb=1 << 30), b"1..16"),
                     (dict(margin=float("nan")), b"finite"), (dict(margin=float("inf")), b"finite")):
        assert call(**kw) == 1, kw
        assert word in lib.hn_last_error() and lib.hn_last_error().startswith(b"hn_mesh_render_occluded_u8: "), (kw, lib.hn_last_error())
    # the plain renderer's messages keep their own name
    assert lib.hn_mesh_render_u8(P, P, None, None, 2, 0, 2, 2, paras, P, 0, 480, 640, P, need, P, None, None) == 1
    assert lib.hn_last_error().startswith(b"hn_mesh_render_u8: bad dims")


def test_python_layer_refuses_what_it_cannot_do():
    """occlude needs faces= (and perm_reverse=); the margin is finite in fp32; the options default to off at every level."""
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import ops
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    for fn in (HandNet.live, HandNet.live_hands, LiveHandEngine.__init__, LiveHandsEngine.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["occlude"].default is False and sig["occlude_margin"].default == 0.03
    sig = inspect.signature(ops.mesh_render).parameters
    for name, default in (("scene_depth", None), ("margin", 0.03), ("silhouette_out", None), ("coverage_out", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(ValueError, match="occlude_margin"):
            ops.check_occlude_margin(bad)
    assert ops.check_occlude_margin(-1e3) == -1e3 and ops.check_occlude_margin(0) == 0.0

    class _Hand:
        device = "cpu"

        def set_convert(self, **kw):
            pass

    class _Graph:
        v = 1280

    class _Lifter:
        device = "cpu"
        graphs = [_Graph()]
    paras, perm = (600.0, 600.0, 320.0, 240.0), np.arange(778)
    with pytest.raises(ValueError, match="occlude=True needs faces="):
        LiveHandsEngine(_Hand(), _Lifter(), paras, 2, True, perm, occlude=True)
    with pytest.raises(ValueError, match="occlude=True needs faces="):
        LiveHandEngine(_Hand(), _Lifter(), paras, True, perm, occlude=True)
    with pytest.raises(ValueError, match="occlude=True needs faces="):
        LiveHandEngine(_Hand(), _Lifter(), paras, True, None, occlude=True)
    with pytest.raises(ValueError, match="perm_reverse"):
        LiveHandsEngine(_Hand(), _Lifter(), paras, 2, True, None, faces=np.array([[0, 1, 2]]), occlude=True)
    plain = LiveHandsEngine(_Hand(), _Lifter(), paras, 2, True, perm)
    assert plain.occlude is None and plain._key_options() == ()
