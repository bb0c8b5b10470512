"""A camera per frame without a GPU: the per-frame helper against the batched rule, the test scenes' depth fights, the new
entries of the C ABI, the public surface, and the engines' bookkeeping (layout, tables, errors) on stub engines."""
import inspect
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import cams_ref as cr
import raster_ref as rr

AMBIGUOUS_CAP = 0.01
NEW_ENTRIES = ("hn_mesh_render_cams_u8", "hn_mesh_render_cams_occluded_u8")


def test_equal_rows_are_the_batched_rule():
    """N equal rows: the per-frame helper gives raster_ref.render of every frame with that one camera, byte for byte -- and
    with the rows of CAMS it does not."""
    meshes, faces = cr.scene(2)
    bgr = rr.frame_bgr8(3, *cr.HW, seed=11)
    lifted = np.array([[1, 1], [1, 0], [1, 1]], np.int32)
    for frames in (bgr, cr.frames_f32(bgr)):
        same = np.repeat(cr.CAMS[1:2], 3, axis=0)
        got = cr.render(meshes, faces, same, frames, lifted)
        got2 = cr.render_candidates(meshes, faces, same, frames, lifted)
        for i in range(3):
            want = rr.render(meshes[i], faces, tuple(cr.CAMS[1]), frames[i], lifted[i])
            for g, w in zip(got, want):
                assert np.array_equal(g[i], w)
            assert np.array_equal(got2[0][i], want[0])
        other = cr.render(meshes, faces, cr.CAMS, frames, lifted)
        assert np.array_equal(other[0][1], got[0][1]) and not np.array_equal(other[0][0], got[0][0])


@pytest.mark.parametrize("k", (1, 2))
def test_the_scenes_have_few_depth_fights(k):
    """A condition on the GPU tests' inputs: in every frame at most 1 % of the covered pixels are depth fights
    (raster_ref.ambiguous), every frame draws, and the three cameras put the same mesh tens of pixels apart."""
    meshes, faces = cr.scene(k)
    bgr = rr.frame_bgr8(3, *cr.HW, seed=k)
    _img, _dep, covered, amb = cr.render(meshes, faces, cr.CAMS, bgr)
    centres = []
    for i in range(3):
        assert covered[i].sum() >= 500, (i, int(covered[i].sum()))
        assert amb[i].sum() <= AMBIGUOUS_CAP * covered[i].sum(), (i, int(amb[i].sum()), int(covered[i].sum()))
        one = rr.render(meshes[0][:1], faces, cr.CAMS[i], bgr[0])[2]          # frame 0's near mesh through camera i
        centres.append(np.array(np.nonzero(one)).mean(axis=1))
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert np.abs(centres[a] - centres[b]).max() >= 10, (a, b, centres[a], centres[b])
    for o in cr.occluded(meshes, faces, cr.CAMS, bgr, cr.hiding_depth(meshes, faces, cr.CAMS), 0.01):
        assert (o.fights | o.threshold).sum() <= AMBIGUOUS_CAP * o.covered.sum()
        assert o.hidden.sum() >= 100 and (o.covered & ~o.hidden).sum() >= 100


def test_the_library_exports_the_new_entries():
    """declared in include/handnet_hip.h, exported by the built library, bound in hn_amd/_lib.py -- with `cams` a pointer where
    the one-camera entries take the host's four floats, and nothing else different."""
    from hn_amd import _lib, build
    build.build_library()
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hn_[a-z0-9_]+)", out))
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in exported and name in _lib.SIGNATURES, name
        old = _lib.SIGNATURES[name.replace("_cams", "")]
        new = _lib.SIGNATURES[name]
        assert new[0] is old[0] and len(new[1]) == len(old[1])
        differ = [i for i, (a, b) in enumerate(zip(new[1], old[1])) if a is not b]
        assert differ == [8] and new[1][8] is _lib.VP, (name, differ)
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, text, flags=re.S).group(1)
        assert "const float* cams" in decl and "paras" not in decl
    lib = _lib.load()
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 36         # functions added, no struct touched
    # argument errors need no GPU: no table, and the old entries' message for no paras
    assert lib.hn_mesh_render_cams_u8(*([None] * 4), 1, 1, 1, 1, None, None, 0, 8, 8, None, 0, None, None, None) == 1
    assert b"hn_mesh_render_cams_u8: null pointer" in lib.hn_last_error()
    assert lib.hn_mesh_render_u8(*([None] * 4), 1, 1, 1, 1, None, None, 0, 8, 8, None, 0, None, None, None) == 1
    assert b"hn_mesh_render_u8: null pointer" in lib.hn_last_error()


def test_the_public_surface_takes_the_new_arguments():
    from a2j.a2j import A2JModel
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd.live import CropMeshEngine, CropMeshOutput, CropMeshRead, LiveHandEngine, LiveHandsEngine
    from hn_amd.pipeline import HandNetEngine
    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert names(A2JModel.mesh) == ["self", "lifter", "clamp", "perm_reverse", "faces"]
    assert inspect.signature(A2JModel.mesh).parameters["faces"].default is None
    assert names(CropMeshEngine.__init__) == ["self", "a2j", "lifter", "clamp", "perm_reverse", "faces"]
    for fn in (CropMeshEngine.forward_device, CropMeshEngine.graphed):
        assert names(fn)[:5] == ["self", "crops", "box_f32", "paras", "frames"]
        assert inspect.signature(fn).parameters["frames"].default is None
    for fn, doc in ((HandNet.live, HandNet.live.__doc__), (HandNet.live_hands, HandNet.live_hands.__doc__),
                    (LiveHandEngine.__init__, LiveHandEngine.__doc__), (LiveHandsEngine.__init__, LiveHandsEngine.__init__.__doc__),
                    (HandNetEngine.set_convert, HandNetEngine.set_convert.__doc__), (HandNet.set_convert, HandNet.set_convert.__doc__)):
        assert "paras" in names(fn) and "[N,4]" in doc, fn
    for cls in (LiveHandEngine, LiveHandsEngine, HandNetEngine):
        assert names(cls.set_cameras) == ["self", "paras"]
    # read()'s result: the five items it always had, as a tuple, and .overlay
    r = CropMeshRead(1, 2, 3, 4, [0, 0, 0, 0])
    a, b, c, d, words = r
    assert len(r) == 5 and r == (1, 2, 3, 4, [0, 0, 0, 0]) and r.overlay is None and r.mesh == 4 and words == [0] * 4
    assert CropMeshRead(1, 2, 3, 4, [], overlay="image").overlay == "image"
    assert [f.name for f in CropMeshOutput.__dataclass_fields__.values()][-2:] == ["overlay", "host_overlay"]


def _stub_engines():
    """A HandNetEngine and a lifter without networks, on the CPU: what the live engines' constructors and set_cameras touch"""
    from hn_amd.pipeline import HandNetEngine
    hand = HandNetEngine.__new__(HandNetEngine)
    hand.device, hand._graphs, hand._host_records, hand._convert = torch.device("cpu"), {}, {}, None
    lifter = types.SimpleNamespace(device=torch.device("cpu"), graphs=[types.SimpleNamespace(v=1152)])
    return hand, lifter


def test_camera_paras_rounds_like_the_one_camera():
    from hn_amd import ops
    one = ops.camera_paras([617.343, 617.343, 312.42, 241.42])
    assert one == (617.343, 617.343, 312.42, 241.42) and ops.camera_paras(None) is None
    assert ops.camera_paras(np.float32([1, 2, 3, 4])) == (1.0, 2.0, 3.0, 4.0)
    rows = [[617.343, 617.343, 312.42, 241.42], [580.1, 600.7, 290.3, 260.9]]
    for form in (rows, np.array(rows), torch.tensor(rows, dtype=torch.float64), torch.tensor(rows)):
        t = ops.camera_paras(form)
        assert t.dtype == np.float32 and t.shape == (2, 4) and t.flags.c_contiguous
        assert np.array_equal(t, np.array(rows, np.float64).astype(np.float32))      # what ctypes' c_float makes of the tuple
    for bad in ([[1, 2, 3]], [[[1, 2, 3, 4]]], np.zeros((0, 4))):
        with pytest.raises(ValueError):
            ops.camera_paras(bad)


def test_layout_and_tables_of_a_multi_camera_engine():
    """The buffer layout of a multi-camera step is the single-camera step's with the same options, whatever the options; the
    engine keeps a table with a row per frame (raster) and one with a row per slot (conversion), set_cameras rewrites both in
    place; a single-camera engine has neither and raises; a step over another number of frames raises."""
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    perm = np.arange(778)
    faces = np.array([[0, 1, 2], [2, 3, 4]])
    cams = np.array([[617.343, 617.343, 312.42, 241.42], [580.1, 600.7, 290.3, 260.9]])
    one = tuple(cams[0])
    options = [dict(), dict(perm_reverse=perm, faces=faces), dict(perm_reverse=perm, faces=faces, labels=True, occlude=True),
               dict(labels=True, left=True), dict(perm_reverse=perm, faces=faces, handed=True, track=True, smooth=True)]
    for opt in options:
        for hw in ((48, 64),) if opt.get("occlude") else (None, (48, 64)):      # (an occluded step always draws)
            hand, lifter = _stub_engines()
            multi = LiveHandsEngine(hand, lifter, cams, 2, **opt)._layout(2, hw)
            single = LiveHandsEngine(hand, lifter, one, 2, **opt)._layout(2, hw)
            assert multi == single and multi.nbytes == single.nbytes
        if not (opt.get("handed") or opt.get("track")):
            hand, lifter = _stub_engines()
            assert LiveHandEngine(hand, lifter, cams, **opt)._layout(2, (48, 64)) == LiveHandEngine(hand, lifter, one, **opt)._layout(2, (48, 64))
    hand, lifter = _stub_engines()
    eng = LiveHandsEngine(hand, lifter, cams, 2, perm_reverse=perm, faces=faces)
    assert eng.paras is None and tuple(eng.cams.shape) == (2, 4) and eng.cams.dtype == torch.float32
    assert np.array_equal(eng.cams.numpy(), cams.astype(np.float32))
    spec = hand._convert_spec(None, (48, 64), 2, 2)
    assert spec["paras"] is None and np.array_equal(spec["sample_paras"].numpy(), np.repeat(cams.astype(np.float32), 2, axis=0))
    raster_table, slot_table = eng.cams, spec["sample_paras"]
    eng.set_cameras(cams[::-1] + 1.0)
    assert eng.cams is raster_table and hand._convert_spec(None, (48, 64), 2, 2)["sample_paras"] is slot_table
    assert np.array_equal(raster_table.numpy(), (cams[::-1] + 1.0).astype(np.float32))
    assert np.array_equal(slot_table.numpy(), np.repeat((cams[::-1] + 1.0).astype(np.float32), 2, axis=0))
    assert hand._fields() == 3
    for bad in (one, cams[:1], np.zeros((3, 4))):
        with pytest.raises(ValueError, match="one row per frame"):
            eng.set_cameras(bad)
    with pytest.raises(ValueError, match="3 frames"):
        eng._check_frames(3)
    with pytest.raises(ValueError, match="3 frames"):
        hand._convert_spec(None, (48, 64), 3, 2)
    eng._check_frames(2)
    # one camera: as ever -- a tuple, no table, no set_cameras
    hand, lifter = _stub_engines()
    single = LiveHandsEngine(hand, lifter, one, 2, perm_reverse=perm, faces=faces)
    assert single.paras == one and single.cams is None and hand._convert["cams"] is None and hand._convert["paras"] == one
    assert "sample_paras" not in hand._convert_spec(None, (48, 64), 5, 2)
    single._check_frames(5)
    with pytest.raises(ValueError, match="camera per frame"):
        single.set_cameras(cams)
    with pytest.raises(ValueError, match="camera per frame"):
        hand.set_cameras(cams)

