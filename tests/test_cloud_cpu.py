"""The hand cloud without a GPU: the properties of the rule (tests/cloud_ref.py), the layout of a cloud step's copy buffer, the
public surfaces, and every refusal of the C entry and of the Python layer (all of them come before any launch)."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest
import torch

import cloud_cases as cc
import cloud_ref as cr
import rig_cases as rc
import rig_ref as rr

F = np.float32
PARAS = (61.5, 60.25, 31.75, 23.5)
CLOUD_FIELDS = ("cloud", "cloud_count", "cloud_resid")


def _square(h=48, w=64, z=0.75, slot=0, box=(10, 30, 12, 40)):
    """a fronto-parallel square under slot `slot`'s byte: best = D = z inside, nothing outside"""
    sil, best = np.zeros((1, h, w), np.uint8), np.zeros((1, h, w), F)
    r0, r1, c0, c1 = box
    sil[0, r0:r1, c0:c1] = slot + 1
    best[0, r0:r1, c0:c1] = z
    return best, sil, best.copy()


# ----------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_a_square_reprojects_to_its_pixel_centres(stride):
    best, sil, depth = _square()
    out = cr.hand_cloud(best, sil, depth, PARAS, 1, 4096, 0.03, stride)
    on = np.zeros(sil.shape[1:], bool)
    on[::stride, ::stride] = True
    rows, cols = np.nonzero(on & (sil[0] == 1))
    assert out.count.tolist() == [[len(rows), len(rows)]] and len(rows) > 50 and out.resid.tolist() == [0]
    pts = out.cloud[0, :len(rows)].astype(np.float64)
    fx, fy, cx, cy = PARAS
    u, v = pts[:, 0] * fx / pts[:, 2] + cx, pts[:, 1] * fy / pts[:, 2] + cy
    assert np.abs(u - (cols + 0.5)).max() < 1e-4 and np.abs(v - (rows + 0.5)).max() < 1e-4      # the pixel centre, row-major
    assert (pts[:, 2] == 0.75).all() and not out.cloud[0, len(rows):].any()
    assert out.cloud.dtype == F and out.count.dtype == np.int32 and out.resid.dtype == np.int64


@pytest.mark.parametrize("h,w,stride", [(5, 7, 1), (33, 65, 2), (33, 65, 3), (7, 5, 3), (1, 1, 5)])
def test_strides_on_odd_sizes(h, w, stride):
    sil, best = np.ones((1, h, w), np.uint8), np.full((1, h, w), 0.5, F)
    out = cr.hand_cloud(best, sil, best, PARAS, 1, 10000, 0.03, stride)
    want = [(r, c) for r in range(0, h, stride) for c in range(0, w, stride)]
    assert out.count.tolist() == [[len(want), len(want)]]
    for at, (r, c) in enumerate(want):
        assert np.array_equal(out.cloud[0, at], cr.point(r, c, 0.5, PARAS))
    x = ((F(want[-1][1]) + F(0.5)) - F(PARAS[2])) * F(0.5) / F(PARAS[0])                  # subtract, multiply, divide
    assert out.cloud[0, len(want) - 1, 0] == x


def test_identity_rig_is_the_camera_frame_and_a_general_rig_is_rig_refs_transform():
    c = cc.case(*cc.SHAPES[2])
    cam = cc.expected(*cc.SHAPES[2])
    identity = rr.table(np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (c.n, 1, 1)))
    same = cr.hand_cloud(c.best, c.sil, c.depth, c.paras, c.k, c.points, c.band, c.stride, identity)
    for a, b in zip(same, cam):
        assert a.tobytes() == b.tobytes()
    table = rr.table(rc.extrinsics(c.n, seed=4))
    rig = cr.hand_cloud(c.best, c.sil, c.depth, c.paras, c.k, c.points, c.band, c.stride, table)
    assert np.array_equal(rig.count, cam.count) and np.array_equal(rig.resid, cam.resid)
    for s in range(c.n * c.k):
        written = cam.count[s, 1]
        assert rig.cloud[s, :written].tobytes() == rr.transform(table[s // c.k], cam.cloud[s, :written]).tobytes()
        assert not rig.cloud[s, written:].any()
    assert not np.array_equal(rig.cloud, cam.cloud)


def test_the_band_edges_on_exact_values():
    """e == +-band is in, the next float beyond is out"""
    band = 0.25
    sil = np.ones((1, 1, 6), np.uint8)
    above, below = np.nextafter(F(0.25), F(1)), np.nextafter(F(0.75), F(0))
    #                 e = +band       next e above     e = -band   D one float lower: e = -(band + 2^-24)   far
    best = np.array([[[0.5, 0.0, 0.0, 1.0, 1.0, 0.5]]], F)
    depth = np.array([[[0.75, 0.25, above, 0.75, below, 0.5 + 0.2500001]]], F)
    e = cr.residual(depth, best)[0, 0]
    assert e[0] == F(0.25) and e[1] == F(0.25) and e[2] == above and e[3] == F(-0.25) and e[4] == -(F(0.25) + F(2.0 ** -24))
    slot = cr.matches(best[0], sil[0], depth[0], 1, band, 1)
    assert slot[0].tolist() == [0, 0, -1, 0, -1, -1]
    out = cr.hand_cloud(best, sil, depth, PARAS, 1, 8, band, 1)
    assert out.count.tolist() == [[3, 3]] and out.resid.tolist() == [250000 + 250000 - 250000]


def test_invalid_depth_reaches_no_output():
    best, sil, depth = _square()
    clean = cr.hand_cloud(best, sil, depth, PARAS, 1, 4096, 0.03, 1)
    holes = depth.copy()
    spots = [(10, 12), (11, 13), (12, 14), (13, 15), (14, 16)]
    for (r, c), value in zip(spots, cc.HOLES):
        holes[0, r, c] = value
    assert len(cc.HOLES) == 5
    out = cr.hand_cloud(best, sil, holes, PARAS, 1, 4096, 0.03, 1)
    assert out.count.tolist() == [[clean.count[0, 0] - 5] * 2] and np.isfinite(out.cloud).all() and out.resid.tolist() == [0]
    kept = {(r, c) for r in range(10, 30) for c in range(12, 40)} - set(spots)
    assert {tuple(p) for p in out.cloud[0, :out.count[0, 1]].tolist()} == {tuple(cr.point(r, c, 0.75, PARAS).tolist()) for r, c in kept}


def test_hidden_flag_matches_and_a_foreign_slot_byte_does_not():
    best, sil, depth = _square()
    plain = cr.hand_cloud(best, sil, depth, PARAS, 2, 4096, 0.03, 2)
    hidden = sil.copy()
    hidden[0, 10:20] |= 0x80
    flagged = cr.hand_cloud(best, hidden, depth, PARAS, 2, 4096, 0.03, 2)
    for a, b in zip(flagged, plain):
        assert a.tobytes() == b.tobytes()
    for byte in (3, 0x7F, 0x80 | 3, 17):
        foreign = np.where(sil != 0, byte, 0).astype(np.uint8)
        out = cr.hand_cloud(best, foreign, depth, PARAS, 2, 4096, 0.03, 2)
        assert not out.count.any() and not out.cloud.any() and not out.resid.any()
    second = np.where(sil != 0, 0x80 | 2, 0).astype(np.uint8)
    out = cr.hand_cloud(best, second, depth, PARAS, 2, 4096, 0.03, 2)
    assert out.count[0].tolist() == [0, 0] and out.count[1].tolist() == plain.count[0].tolist()
    assert out.cloud[1].tobytes() == plain.cloud[0].tobytes()


def test_the_cap_keeps_the_first_in_row_major_order():
    best, sil, depth = _square()
    full = cr.hand_cloud(best, sil, depth, PARAS, 1, 4096, 0.03, 1)
    total = int(full.count[0, 0])
    capped = cr.hand_cloud(best, sil, depth, PARAS, 1, 37, 0.03, 1)
    assert total > 37 and capped.count.tolist() == [[total, 37]] and capped.resid.tolist() == full.resid.tolist()
    assert capped.cloud[0].tobytes() == full.cloud[0, :37].tobytes()
    first = [(r, c) for r in range(10, 30) for c in range(12, 40)][:37]
    assert capped.cloud[0].tobytes() == np.stack([cr.point(r, c, 0.75, PARAS) for r, c in first]).tobytes()


def test_the_residual_is_a_plain_integer_sum_over_all_matches():
    c, want = cc.case(*cc.SHAPES[2]), cc.expected(*cc.SHAPES[2])
    for i in range(c.n):
        slot = cr.matches(c.best[i], c.sil[i], c.depth[i], c.k, c.band, c.stride)
        for kk in range(c.k):
            total = 0
            for r, col in zip(*np.nonzero(slot == kk)):
                e = F(c.depth[i, r, col]) - F(c.best[i, r, col])
                total += int(np.int32(np.rint(e * F(1e6))))
            assert total == int(want.resid[i * c.k + kk])
    assert (want.count[:, 0] > c.points).any() and want.resid.any()          # truncated slots: the sum runs over ALL matches


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_gpu_cases_offer_what_they_must(shape):
    """the conditions test_cloud_gpu.py checks before it compares, here without a GPU"""
    c = cc.case(*shape)
    cc.check_conditions(c, cc.expected(*shape))
    who = c.sil & 0x7F
    assert (c.sil & 0x80).any() and (who > c.k).any() and ((who >= 1) & (who <= c.k)).any()
    for value in cc.HOLES:
        assert (np.isnan(c.depth).any() if np.isnan(value) else (c.depth == F(value)).any()), value
    assert len(c.edges) == 4 or shape == cc.SHAPES[0]
    slot = cr.matches(c.best[0], c.sil[0], c.depth[0], c.k, c.band, c.stride)
    for (_i, r, col, inside) in c.edges:
        assert (slot[r, col] >= 0) == inside


# ------------------------------------------------------------------------------------------------------------------- layout
COMBOS = [(1, 1, 5, (5, 7), {}), (3, 2, 5, (5, 7), dict(labels=True, handed=True)),
          (2, 3, 778, (48, 64), dict(tracked=True, smoothed=True)),
          (7, 5, 13, (5, 7), dict(labels=True, tracked=True)), (16, 16, 778, (33, 65), dict(handed=True, tracked=True, smoothed=True))]


@pytest.mark.parametrize("rig", [False, True])
@pytest.mark.parametrize("points", [1, 7, 4096])
@pytest.mark.parametrize("n,k,v,hw,opts", COMBOS)
def test_cloud_layout_appends_three_aligned_parts_and_moves_nothing(n, k, v, hw, opts, points, rig):
    from hn_amd.live import LiveLayout
    opts = dict(opts, overlay=True, occluded=True, rig=rig)
    plain, cloud = LiveLayout(n, k, v, hw, **opts), LiveLayout(n, k, v, hw, **opts, cloud=points)
    params = list(inspect.signature(LiveLayout).parameters)
    assert plain.cloud == 0 and cloud.cloud == points and params[-2:] == ["cloud", "rig"]
    for f in LiveLayout.__dataclass_fields__:
        if f not in ("cloud", "nbytes"):
            assert getattr(plain, f) == getattr(cloud, f), f
    assert not any(f.startswith("cloud_") for f in LiveLayout.__dataclass_fields__)
    s = n * k
    sizes, aligns = dict(cloud=s * points * 12, cloud_count=s * 8, cloud_resid=s * 8), dict(cloud=4, cloud_count=4, cloud_resid=8)
    end = plain.nbytes
    for name in CLOUD_FIELDS:
        at = getattr(cloud, name + "_at")
        assert getattr(plain, name + "_at") is None
        assert at % aligns[name] == 0 and end <= at < end + aligns[name], name
        end = at + sizes[name]
    assert end == cloud.nbytes
    buf = torch.zeros((cloud.nbytes + 8,), dtype=torch.uint8)
    buf = buf[(-buf.data_ptr()) % 8:][:cloud.nbytes]
    pv, cv = plain.views(buf[:plain.nbytes]), cloud.views(buf)
    assert cv._fields == pv._fields + CLOUD_FIELDS and type(cv).__name__.endswith("CloudViews")
    assert ("Rig" in type(cv).__name__) == rig
    for name in pv._fields:
        a, b = getattr(pv, name), getattr(cv, name)
        assert (a is None) == (b is None)
        if a is not None:
            assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype
    shapes = dict(cloud=(s, points, 3), cloud_count=(s, 2), cloud_resid=(s,))
    dtypes = dict(cloud=torch.float32, cloud_count=torch.int32, cloud_resid=torch.int64)
    for name in CLOUD_FIELDS:
        t = getattr(cv, name)
        assert t.data_ptr() - buf.data_ptr() == getattr(cloud, name + "_at") and tuple(t.shape) == shapes[name] and t.dtype == dtypes[name]


def test_cloud_layout_refusals_and_the_one_hand_step():
    from hn_amd.live import LiveLayout
    with pytest.raises(ValueError, match="occluded"):
        LiveLayout(2, 2, 778, (5, 7), overlay=True, cloud=16)
    with pytest.raises(ValueError, match="occluded"):
        LiveLayout(2, 2, 778, cloud=16)
    for bad in (-1, 2.5, True, "many"):
        with pytest.raises(ValueError, match="cloud"):
            LiveLayout(2, 2, 778, (5, 7), overlay=True, occluded=True, cloud=bad)
    one = LiveLayout(3, None, 778, (5, 7), overlay=True, occluded=True, cloud=9)
    v = one.views(torch.zeros((one.nbytes,), dtype=torch.uint8))
    assert tuple(v.cloud.shape) == (3, 9, 3) and tuple(v.cloud_count.shape) == (3, 2) and tuple(v.cloud_resid.shape) == (3,)
    assert one.cloud_resid_at % 8 == 0 and one.nbytes == one.cloud_resid_at + 24


def test_read_appends_the_three_fields_behind_every_other_field():
    from hn_amd.live import LiveHandsOutput, LiveLayout, LiveOutput, _read_type, _HANDS_FIELDS
    n, k, v, hw, points = 2, 3, 5, (5, 7), 6
    g = torch.Generator().manual_seed(4)
    for opts in (dict(), dict(handed=True, tracked=True, smoothed=True), dict(rig=True)):
        opts = dict(opts, overlay=True, occluded=True)
        plain, cloud = LiveLayout(n, k, v, hw, **opts), LiveLayout(n, k, v, hw, **opts, cloud=points)
        host = torch.randint(0, 256, (cloud.nbytes,), generator=g, dtype=torch.uint8)
        host[:plain.mesh_at] = 0
        r = LiveHandsOutput(None, None, None, None, None, host, n, k, layout=cloud).read()
        p = LiveHandsOutput(None, None, None, None, None, host[:plain.nbytes], n, k, layout=plain).read()
        assert r._fields == p._fields + CLOUD_FIELDS and type(r).__name__ == type(p).__name__.replace("Read", "CloudRead")
        for a, b in zip(r[:len(p)], p):
            assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)) if torch.is_tensor(a) else a == b
        v_ = cloud.views(host)
        assert tuple(r.cloud.shape) == (n, k, points, 3) and tuple(r.cloud_count.shape) == (n, k, 2) and tuple(r.cloud_resid.shape) == (n, k)
        assert r.cloud.dtype == torch.float32 and r.cloud_count.dtype == torch.int32 and r.cloud_resid.dtype == torch.int64
        for name in CLOUD_FIELDS:
            got = getattr(r, name)
            assert torch.equal(got.reshape(-1).view(torch.uint8), getattr(v_, name).reshape(-1).view(torch.uint8)), name
            assert got.data_ptr() != getattr(v_, name).data_ptr()
    plain1, cloud1 = LiveLayout(n, None, v, hw, True, occluded=True), LiveLayout(n, None, v, hw, True, occluded=True, cloud=points)
    host = torch.randint(0, 256, (cloud1.nbytes,), generator=g, dtype=torch.uint8)
    host[:plain1.mesh_at] = 0
    r1 = LiveOutput(None, None, None, None, host, n, layout=cloud1).read()
    p1 = LiveOutput(None, None, None, None, host[:plain1.nbytes], n, layout=plain1).read()
    assert r1._fields == p1._fields + CLOUD_FIELDS and type(r1).__name__ == "LiveOverlayOccludedCloudRead"
    assert tuple(r1.cloud.shape) == (n, points, 3) and tuple(r1.cloud_count.shape) == (n, 2) and tuple(r1.cloud_resid.shape) == (n,)
    sig = inspect.signature(_read_type).parameters
    assert list(sig)[-1] == "cloud" and sig["cloud"].default is False
    assert _read_type("LiveHands", _HANDS_FIELDS, True, False, False, False, False, True, True, True)._fields[-3:] == CLOUD_FIELDS


# ----------------------------------------------------------------------------------------------------------------- surfaces
def test_the_surfaces():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import live, ops
    from hn_amd.live import LiveHandEngine, LiveHandsEngine, LiveHandsOutput, LiveOutput
    assert (ops.CLOUD_POINTS, ops.CLOUD_BAND, ops.CLOUD_STRIDE) == (4096, 0.03, 2) == (cr.CLOUD_POINTS, cr.CLOUD_BAND, cr.CLOUD_STRIDE)
    assert ops.HandCloud._fields == ("cloud", "count", "resid") == cr.HandCloud._fields and live.CLOUD_FIELDS == CLOUD_FIELDS
    sig = inspect.signature(ops.hand_cloud).parameters
    assert list(sig) == ["mesh_depth", "silhouette", "scene_depth", "paras", "k", "points", "band", "stride", "extrinsics_table", "out",
                         "scratch"]
    for name, default in (("points", 4096), ("band", 0.03), ("stride", 2), ("extrinsics_table", None), ("out", None), ("scratch", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    assert list(inspect.signature(ops.check_cloud).parameters) == ["points", "band", "stride"]
    for fn in (HandNet.live, HandNet.live_hands, LiveHandEngine.__init__, LiveHandsEngine.__init__):
        d = {k: p.default for k, p in inspect.signature(fn).parameters.items()}
        assert (d["cloud"], d["cloud_points"], d["cloud_band"], d["cloud_stride"]) == (False, 4096, 0.03, 2), fn.__qualname__
    for fn in (HandNet.live_hands, LiveHandsEngine.__init__):
        assert inspect.signature(fn).parameters["cloud_frame"].default == "camera"
    for fn in (HandNet.live, LiveHandEngine.__init__):
        assert "cloud_frame" not in inspect.signature(fn).parameters
    for doc in (ops.hand_cloud.__doc__, ops.check_cloud.__doc__, LiveHandEngine.__doc__, LiveHandsEngine.__init__.__doc__,
                HandNet.live.__doc__, HandNet.live_hands.__doc__):
        assert "NOT tuned" in " ".join(doc.split("cloud_points = 4096" if "cloud_points = 4096" in doc else "4096")[1][:160].split()), doc[:40]
    assert "pixel centre at +0.5" in ops.hand_cloud.__doc__ and "x right, y down, z forward" in ops.hand_cloud.__doc__
    for cls in (LiveOutput, LiveHandsOutput):
        names = list(cls.__dataclass_fields__)
        at = names.index("cloud")
        assert names[at:at + 4] == ["cloud", "cloud_count", "cloud_resid", "mesh_depth"]


def test_the_entries_are_declared_exported_and_bound():
    from hn_amd import _lib, build
    build.build_library()
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    for name, result, count in (("hn_hand_cloud_f32", "int", 20), ("hn_hand_cloud_scratch_bytes", "int64_t", 3)):
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
            elif p.startswith("int64_t"):
                assert a is C.c_int64, p
            else:
                assert p.startswith("int ") and a is C.c_int, p
        assert re.search(r" T %s\b" % name, out)
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION                  # functions added, no struct touched
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["hand_cloud.hip"]
    rows = (build.CSRC / "build" / "hand_cloud.resources.txt").read_text().splitlines()
    assert len(rows) == 2 and all("hand_cloud_" in r and " vgpr_spill 0 " in r and r.endswith("sgpr_spill 0") and " scratch 0 " in r for r in rows)


def test_the_scratch_size():
    from hn_amd import _lib
    lib = _lib.load()
    assert lib.hn_hand_cloud_scratch_bytes(1, 1, 1) == 4 * 12 and lib.hn_hand_cloud_scratch_bytes(1, 2, 480) == 240 * 2 * 12
    assert lib.hn_hand_cloud_scratch_bytes(3, 16, 203) == 3 * 104 * 16 * 12 and lib.hn_hand_cloud_scratch_bytes(2, 16, 16384) == 2 * 1024 * 16 * 12
    for bad in ((0, 1, 5), (1, 0, 5), (1, 17, 5), (1, 1, 0), (1, 1, 16385), (-1, 1, 5)):
        assert lib.hn_hand_cloud_scratch_bytes(*bad) == 0, bad
    sizes = [lib.hn_hand_cloud_scratch_bytes(1, 1, h) for h in range(1, 16385, 61)]
    assert min(sizes) == 48 and max(sizes) <= 1024 * 12 and all(s % 48 == 0 for s in sizes)


def test_the_entry_checks_its_arguments_before_any_launch():
    """no GPU here: every refusal comes back as HN_ERR_ARG with a message under the entry's name, before the device is touched"""
    from hn_amd import _lib
    lib = _lib.load()
    P = 4096        # stands for a device address
    host4 = (C.c_float * 4)(600.0, 600.0, 320.0, 240.0)

    def call(n=2, k=2, h=48, w=64, points=16, stride=2, band=0.03, frame_stride=None, scratch_bytes=None, paras=host4, cams=None, **ptrs):
        p = dict(best=P, sil=P, depth=P, ext=None, scratch=P, cloud=P, count=P, resid=P)
        p.update(ptrs)
        need = lib.hn_hand_cloud_scratch_bytes(n, k, h) if scratch_bytes is None else scratch_bytes
        return lib.hn_hand_cloud_f32(p["best"], p["sil"], p["depth"], h * w if frame_stride is None else frame_stride, paras, cams,
                                     p["ext"], n, k, h, w, points, stride, band, p["scratch"], need, p["cloud"], p["count"], p["resid"], None)
    refusals = [(dict(best=None), b"null pointer"), (dict(sil=None), b"null pointer"), (dict(depth=None), b"null pointer"),
                (dict(scratch=None), b"null pointer"), (dict(cloud=None), b"null pointer"), (dict(count=None), b"null pointer"),
                (dict(resid=None), b"null pointer"),
                (dict(cams=P), b"exactly one of paras"), (dict(paras=None), b"exactly one of paras"),
                (dict(k=0), b"k = 0"), (dict(k=17), b"k = 17"), (dict(k=-1), b"k = -1"),
                (dict(h=0), b"frame size"), (dict(w=0), b"frame size"), (dict(h=16385), b"frame size"), (dict(w=16385), b"frame size"),
                (dict(h=-4), b"frame size"),
                (dict(frame_stride=48 * 64 - 1), b"depth_frame_stride"), (dict(frame_stride=0), b"depth_frame_stride"),
                (dict(points=0), b"points"), (dict(points=-5), b"points"), (dict(stride=0), b"stride = 0"), (dict(stride=-2), b"stride = -2"),
                (dict(band=0.0), b"band"), (dict(band=-0.03), b"band"), (dict(band=float("nan")), b"band"),
                (dict(band=float("inf")), b"band"), (dict(band=100.5), b"band"),
                (dict(scratch_bytes=lib.hn_hand_cloud_scratch_bytes(2, 2, 48) - 1), b"scratch of"), (dict(scratch_bytes=0), b"scratch of"),
                (dict(n=0), b"n = 0"), (dict(scratch=P + 4), b"8-byte aligned"), (dict(resid=P + 4), b"aligned")]
    for kw, word in refusals:
        assert call(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_hand_cloud_f32: ") and word in err, (kw, err)


# ---------------------------------------------------------------------------------------------------------- the Python layer
def test_check_cloud():
    from hn_amd import ops
    assert ops.check_cloud() == (4096, 0.03, 2) and ops.check_cloud(1, 100, 1) == (1, 100.0, 1)
    assert ops.check_cloud(np.int64(7), np.float32(0.5), np.int32(3)) == (7, 0.5, 3)
    for bad in (0, -1, 2.0, True, "many", None, 2 ** 31):
        with pytest.raises(ValueError, match="cloud_points"):
            ops.check_cloud(points=bad)
        with pytest.raises(ValueError, match="cloud_stride"):
            ops.check_cloud(stride=bad)
    for bad in (0, -0.03, float("nan"), float("inf"), -float("inf"), 100.0001, 1e39, 1e-50, "wide", None):
        with pytest.raises(ValueError, match="cloud_band"):
            ops.check_cloud(band=bad)


class _Hand:
    device = "cpu"

    def set_convert(self, **kw):
        pass


class _Graph:
    v = 1280


class _Lifter:
    device = "cpu"
    graphs = [_Graph()]


def test_the_engines_refuse_what_the_cloud_cannot_do():
    """before anything touches a device"""
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    paras, perm, faces = (600.0, 600.0, 320.0, 240.0), np.arange(778), np.array([[0, 1, 2]])
    ext = rc.extrinsics(2, seed=1)
    hands = lambda *a, **kw: LiveHandsEngine(_Hand(), _Lifter(), paras, 2, True, *a, **kw)  # noqa: E731
    for make in (hands, lambda *a, **kw: LiveHandEngine(_Hand(), _Lifter(), paras, True, *a, **kw)):
        with pytest.raises(ValueError, match="cloud=True needs occlude=True"):
            make(perm, cloud=True)
        with pytest.raises(ValueError, match="cloud=True needs occlude=True"):
            make(perm, faces=faces, cloud=True)
        with pytest.raises(ValueError, match="occlude=True needs faces="):
            make(perm, occlude=True, cloud=True)
        with pytest.raises(ValueError, match="perm_reverse"):
            make(None, faces=faces, occlude=True, cloud=True)
    for kw, word in ((dict(cloud_points=0), "cloud_points"), (dict(cloud_points=1.5), "cloud_points"), (dict(cloud_band=0), "cloud_band"),
                     (dict(cloud_band=float("nan")), "cloud_band"), (dict(cloud_band=101), "cloud_band"), (dict(cloud_stride=0), "cloud_stride"),
                     (dict(cloud_frame="rig"), "needs extrinsics="), (dict(cloud_frame="world"), "cloud_frame"),
                     (dict(cloud_frame=None), "cloud_frame")):
        with pytest.raises(ValueError, match=word):
            hands(perm, faces=faces, occlude=True, cloud=True, **kw)
    with pytest.raises(ValueError, match="cloud_frame"):
        hands(perm, cloud_frame="Rig", extrinsics=ext)
    with pytest.raises(TypeError):
        LiveHandEngine(_Hand(), _Lifter(), paras, True, perm, cloud_frame="rig")
    plain = hands(perm)
    assert plain.cloud is None and plain.cloud_frame == "camera" and plain._key_options() == () and plain._layout(2, (5, 7)).cloud == 0
    rig = hands(perm, extrinsics=ext, cloud_frame="rig")
    assert rig.cloud is None and rig.cloud_frame == "rig" and rig._key_options() == ("rig", 0.08)
