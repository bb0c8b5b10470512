"""The overlay on the GPU (csrc/mesh_raster.hip, ops.mesh_render, the live engines' faces=) against the numpy statement of
the rule (tests/raster_ref.py): coverage bit for bit, depth and colour on the pixels that are not depth fights."""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_ref as rr

pytestmark = pytest.mark.gpu

PARAS = rr.PARAS
LIVE_PARAS = (617.343, 617.343, 312.42, 241.42)
# fp32 barycentric depth against the helper's float64: 4 x the largest relative difference measured on the scenes below on an
# MI355X (2.104e-7, profiles/bench_render.json "depth_max_rel"; DESIGN.md "The overlay"); must itself stay below 1e-4
DEPTH_REL_BOUND = 4 * 2.104e-7
assert DEPTH_REL_BOUND < 1e-4
AMBIGUOUS_CAP = 0.01


_frame_u8 = rr.frame_bgr8
SCENES = rr.scenes()


def _gpu_render(meshes, faces, lifted, paras, frame, depth=True, scratch=None):
    from hn_amd import ops
    n, k = meshes.shape[:2]
    m = torch.from_numpy(np.ascontiguousarray(meshes)).cuda()
    fr = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    h, w = (frame.shape[1:3] if frame.dtype == np.uint8 else frame.shape[2:])
    d = torch.full((n, h, w), -1.0, device="cuda") if depth else None
    lf = None if lifted is None else torch.from_numpy(lifted.reshape(-1).astype(np.int32)).cuda()
    img = ops.mesh_render(m, faces, paras, fr, lifted=lf, k=k, depth_out=d, scratch=scratch)
    torch.cuda.synchronize()
    return img.cpu().numpy(), (d.cpu().numpy() if depth else None)


def _compare(name, got_img, got_depth, meshes, faces, lifted, paras, frame_one, stats):
    """One frame against the helper: coverage exact, untouched pixels equal the frame, depth / colour off the depth fights."""
    want_img, want_depth, covered, amb = rr.render(meshes, faces, paras, frame_one, lifted)
    if got_depth is not None:
        assert np.array_equal(got_depth > 0, covered), f"{name}: coverage differs on {int(((got_depth > 0) != covered).sum())} pixels"
    assert np.array_equal(got_img[~covered], rr.frame_u8(frame_one)[~covered]), f"{name}: an uncovered pixel is not the frame's"
    share = amb.sum() / max(1, covered.sum())
    clear = covered & ~amb
    rel = 0.0
    if got_depth is not None and clear.any():
        rel = float((np.abs(got_depth[clear].astype(np.float64) - want_depth[clear]) / want_depth[clear]).max())
    lev = int(np.abs(got_img[clear].astype(np.int64) - want_img[clear].astype(np.int64)).max()) if clear.any() else 0
    print(f"{name}: covered {int(covered.sum())}, ambiguous {int(amb.sum())} ({share:.2%}), depth max rel {rel:.3e}, "
          f"colour max diff {lev} level(s)")
    stats.append((name, int(covered.sum()), int(amb.sum()), rel, lev))
    assert share <= AMBIGUOUS_CAP, f"{name}: {share:.2%} of the covered pixels are depth fights"
    assert rel <= DEPTH_REL_BOUND, f"{name}: depth off by {rel:.3e} relative (bound {DEPTH_REL_BOUND:.3e})"
    assert lev <= 1, f"{name}: colour off by {lev} levels"
    return covered


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_matches_the_rule(name):
    """Coverage (`depth > 0`) equals the helper's bit for bit and every uncovered pixel is the frame's, for both frame formats;
    depth within DEPTH_REL_BOUND and colour within one level on covered pixels that are not depth fights; depth fights are at
    most 1 % of the covered pixels."""
    meshes, faces, lifted, paras, (h, w) = SCENES[name]
    n = meshes.shape[0]
    bgr = _frame_u8(n, h, w, seed=len(name))
    f32 = np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    img_u8, dep_u8 = _gpu_render(meshes, faces, lifted, paras, bgr)
    img_f32, dep_f32 = _gpu_render(meshes, faces, lifted, paras, f32)
    assert np.array_equal(img_u8, img_f32) and np.array_equal(dep_u8, dep_f32)     # the frame's format changes nothing
    stats, total = [], 0
    for i in range(n):
        lf = None if lifted is None else lifted[i]
        total += int(_compare(f"{name} [frame {i}, bgr8]", img_u8[i], dep_u8[i], meshes[i], faces, lf, paras, bgr[i], stats).sum())
        _compare(f"{name} [frame {i}, fp32]", img_f32[i], dep_f32[i], meshes[i], faces, lf, paras, f32[i], stats)
    assert total > 0, "the scene draws nothing"
    again, dep_again = _gpu_render(meshes, faces, lifted, paras, bgr)
    assert np.array_equal(again, img_u8) and np.array_equal(dep_again, dep_u8)     # two runs: bit-identical
    no_depth, _ = _gpu_render(meshes, faces, lifted, paras, bgr, depth=False)
    assert np.array_equal(no_depth, img_u8)


def test_occlusion_is_independent_of_the_slot_order():
    """Two slots of one frame, the nearer mesh in slot 1: the nearer wins where they overlap, and swapping the slots gives
    the identical image and depth."""
    far, f = rr.ellipsoid((0.0, 0.0, 0.70), (0.10, 0.10, 0.03))
    near, _ = rr.ellipsoid((0.03, 0.01, 0.50), (0.04, 0.05, 0.03))
    bgr = _frame_u8(1, 480, 640, seed=5)
    img_a, dep_a = _gpu_render(np.stack([far, near])[None], f, None, PARAS, bgr)
    img_b, dep_b = _gpu_render(np.stack([near, far])[None], f, None, PARAS, bgr)
    assert np.array_equal(img_a, img_b) and np.array_equal(dep_a, dep_b)
    img_n, dep_n = _gpu_render(near[None, None], f, None, PARAS, bgr)
    img_f, dep_f = _gpu_render(far[None, None], f, None, PARAS, bgr)
    on_near = dep_n[0] > 0
    assert on_near.sum() > 1000 and (on_near & (dep_f[0] > 0)).sum() > 1000
    assert np.array_equal(dep_a[0][on_near], dep_n[0][on_near]) and np.array_equal(img_a[0][on_near], img_n[0][on_near])
    only_far = (dep_f[0] > 0) & ~on_near
    assert np.array_equal(dep_a[0][only_far], dep_f[0][only_far]) and np.array_equal(img_a[0][only_far], img_f[0][only_far])


def test_a_frame_without_a_lifted_hand_is_the_frame():
    """Three frames in one call, the middle one with lifted == 0 in every slot (its vertices are there all the same), into a
    scratch that a fully drawn call of the same shape has just filled, so that stale face records and slot boxes are present:
    the middle frame's overlay is its input frame and its depth is 0 everywhere, for both frame formats; its neighbours are
    drawn.  (The scene itself is also compared against the rule by test_scene_matches_the_rule.)"""
    from hn_amd import ops
    meshes, faces, lifted, paras, (h, w) = SCENES["a whole frame with lifted = 0"]
    n, k = meshes.shape[:2]
    assert not lifted[1].any() and lifted[0].all() and lifted[2].any()
    bgr = _frame_u8(n, h, w, seed=77)
    f32 = np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    scratch = torch.empty((ops.mesh_render_scratch_bytes(n * k, faces.shape[0]),), dtype=torch.uint8, device="cuda")
    for frame in (bgr, f32):
        full_img, full_dep = _gpu_render(meshes, faces, np.ones_like(lifted), paras, frame, scratch=scratch)
        assert all(int((full_dep[i] > 0).sum()) > 15000 for i in range(n))            # stale records for every slot
        img, dep = _gpu_render(meshes, faces, lifted, paras, frame, scratch=scratch)
        assert np.array_equal(img[1], rr.frame_u8(frame[1])), frame.dtype
        assert not dep[1].any(), frame.dtype
        assert np.array_equal(img[0], full_img[0]) and np.array_equal(dep[0], full_dep[0])
        # (frame 2 draws its second slot alone: semi-axes 6 x 4 cm at 0.56 m are 66 x 44 px, an ellipse of ~9100 pixels)
        assert 8500 < int((dep[2] > 0).sum()) < 9700 and not np.array_equal(img[2], full_img[2])


# ---------------------------------------------------------------------------------------------------- the live engines
H, W = 480, 640
# The seeded lifter's vertices spread over metres (std ~4 units read as metres), so that nearly every face is behind the camera
# or out of range.  The fixture scales its LAST graph convolution (weight and bias; no normalisation follows it) by 0.01: the
# same network with a hand-sized output (std ~4 cm around the wrist), which projects into the frame.  A lifted frame must then
# draw at least this many pixels (a 4 cm blob at the farthest synthetic depth, 1.5 m, is ~16 px of std across; measured
# meshes cover thousands), else the comparisons below would compare frames with frames:
DRAWN_FLOOR = 1000
LIFTER_OUTPUT_SCALE = 0.01


def _synthetic_faces(seed=7, nv=778):
    """A face list over the synthetic 778-vertex mesh, as tests/golden/make_golden_p2m.py builds one (seeded Delaunay)."""
    from scipy.spatial import Delaunay
    pts = np.random.default_rng(seed).random((nv, 2))
    return Delaunay(pts).simplices.astype(np.int64)


@pytest.fixture(scope="module")
def parts(golden_dir, fcos_sd, a2j_sd):
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    g = np.load(golden_dir / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    p2m_sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    last = max(int(key.split(".")[2]) for key in p2m_sd if key.startswith("pose2mesh.cl."))
    for key in (f"pose2mesh.cl.{last}.weight", f"pose2mesh.cl.{last}.bias"):
        p2m_sd[key] = p2m_sd[key] * LIFTER_OUTPUT_SCALE
    hand = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    lifter = Pose2MeshEngine(p2m_sd, graphs, device="cuda")
    return hand, lifter, g["perm_reverse"][:778], _synthetic_faces()


def _run(eng, rgb, depth, graphed=False):
    if graphed:
        run, s_img, s_dep, out = eng.graphed(rgb, depth)
        s_img.copy_(rgb)
        s_dep.copy_(depth)
        run()
    else:
        out = eng.forward_device(rgb, depth)
    torch.cuda.synchronize()
    return out, out.read()


def _check_overlay(tag, overlay, mesh, lifted, frames, faces, paras=LIVE_PARAS):
    """read().overlay against the helper applied to read().mesh, read().lifted and the input frames.  The step hands over no
    depth map, so coverage is read off the image: every uncovered pixel is the frame's, exactly; every covered pixel carries
    the nearest face's colour within one level -- or, where the pixel is a depth fight, the nearest's or the second-nearest's --
    and a covered pixel may equal the frame's only where the frame's own pixel lies within a level of such a colour (noise
    frames: a handful of pixels at most).  A frame with a lifted slot draws at least DRAWN_FLOOR pixels; a frame without one
    comes back as it went in.  Returns the pixels drawn per frame."""
    drawn = []
    for i in range(overlay.shape[0]):
        want, want2, covered, amb = rr.render_candidates(mesh[i], faces, paras, frames[i], lifted[i])
        f8 = rr.frame_u8(frames[i])
        got = overlay[i].astype(np.int64)
        assert np.array_equal(overlay[i][~covered], f8[~covered]), f"{tag}: frame {i}: an uncovered pixel is not the frame's"
        d1 = np.abs(got - want.astype(np.int64)).max(axis=2)
        d2 = np.abs(got - want2.astype(np.int64)).max(axis=2)
        clear = covered & ~amb
        worst = int(d1[clear].max()) if clear.any() else 0
        fights = int(np.minimum(d1, d2)[covered & amb].max()) if (covered & amb).any() else 0
        unchanged = covered & (overlay[i] == f8).all(axis=2)
        print(f"{tag}: frame {i}: lifted {lifted[i].tolist()}, covered {int(covered.sum())}, depth fights {int(amb.sum())} "
              f"({amb.sum() / max(1, covered.sum()):.2%}), colour max diff {worst} (fights {fights}), covered pixels equal to "
              f"the frame's {int(unchanged.sum())}")
        assert worst <= 1 and fights <= 1, f"{tag}: frame {i}"
        assert int(unchanged.sum()) <= 8, f"{tag}: frame {i}: {int(unchanged.sum())} covered pixels were left as the frame's"
        if lifted[i].any():
            assert int(covered.sum()) >= DRAWN_FLOOR, f"{tag}: frame {i}: only {int(covered.sum())} pixels drawn"
        else:
            assert np.array_equal(overlay[i], f8) and not covered.any()
        drawn.append(int(covered.sum()))
    return drawn


def _net(fcos_sd, a2j_sd):
    import types
    from handnet_pipeline.handnet_pipeline import HandNet
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    net.detector.load_state_dict(fcos_sd, strict=False)
    net.a2j.load_state_dict(a2j_sd, strict=False)
    return net.cuda().eval()


def test_live_hands_overlay_end_to_end(parts, fcos_sd, a2j_sd):
    """HandNet.live_hands(..., faces=F) on the synthetic pipeline (hand-sized lifter output): read().overlay is the helper's
    image of read().mesh / read().lifted over the input frame and every lifted frame draws at least DRAWN_FLOOR pixels; every
    other field equals the same engine built without faces bit for bit; K = 1 live_hands and live give the same, drawn,
    overlay; ops.mesh_render on the step's own tensors reproduces the step's overlay."""
    from hn_amd import ops, synth
    _hand, lifter, perm, faces = parts
    net = _net(fcos_sd, a2j_sd)
    n, k = 2, 2
    rgb, depth = synth.make_rgb(n, seed=1000).cuda(), synth.make_depth(n, seed=2000).cuda()
    with torch.inference_mode():
        out, r = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=k, perm_reverse=perm, faces=faces), rgb, depth)
        _o, plain = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=k, perm_reverse=perm), rgb, depth)
    assert plain.overlay is None and _o.overlay is None
    assert tuple(r.overlay.shape) == (n, H, W, 3) and r.overlay.dtype == torch.uint8
    assert torch.equal(out.overlay.cpu(), r.overlay)
    for f in plain._fields:
        if f == "words":
            assert plain.words == r.words
        else:
            assert torch.equal(getattr(plain, f), getattr(r, f)), f
    assert bool(r.lifted[:, 0].all())
    drawn = _check_overlay("live_hands", r.overlay.numpy(), r.mesh.numpy(), r.lifted.numpy(), rgb.cpu().numpy(), faces)
    assert min(drawn) >= DRAWN_FLOOR
    # the two hands of a frame are two different meshes, and the frames differ: nothing here is one image compared with itself
    assert not torch.equal(r.overlay[0], r.overlay[1])
    again = ops.mesh_render(out.mesh, ops.mesh_faces(faces, 778, "cuda"), LIVE_PARAS, rgb, lifted=out.lifted.reshape(-1), k=k)
    assert torch.equal(again.cpu(), r.overlay)
    with torch.inference_mode():
        _o1, one = _run(net.live(lifter, LIVE_PARAS, perm_reverse=perm, faces=faces), rgb, depth)
        _o2, k1 = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=1, perm_reverse=perm, faces=faces), rgb, depth)
        _o3, one_plain = _run(net.live(lifter, LIVE_PARAS, perm_reverse=perm), rgb, depth)
    assert len(one) == 7 and len(one_plain) == 6 and one_plain.overlay is None
    for a, b in zip(one[:6], one_plain):
        if torch.is_tensor(a):
            assert torch.equal(a, b)
    drawn1 = _check_overlay("live", one.overlay.numpy(), one.mesh.numpy()[:, None], (one.has_hand.numpy() != 0)[:, None],
                            rgb.cpu().numpy(), faces)
    assert min(drawn1) >= DRAWN_FLOOR
    assert torch.equal(one.overlay, k1.overlay)
    # one hand drawn is not two hands drawn: the K = 2 image differs from the K = 1 image where the second hand lies
    assert not torch.equal(one.overlay, r.overlay)


def test_a_frame_without_a_hand_comes_back_untouched(parts, monkeypatch):
    """The live_hands step on three frames of which the middle one loses its hands after the crop stage (flags, boxes and crops
    zeroed, as tests/test_hands_gpu.py empties slots): that frame's slots are not lifted and its overlay is the input frame,
    while its neighbours are drawn (>= DRAWN_FLOOR pixels each)."""
    import parity_cases as pc
    from hn_amd import pipeline
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    n, k = 3, 2
    keep = torch.ones((n, k), dtype=torch.int32, device="cuda")
    keep[1] = 0
    real = pipeline.ops.crop_resize_hands

    def crop(*a, **kw):
        box, has, score, index, crops = real(*a, **kw)
        has.mul_(keep)
        box.mul_(keep[..., None].to(box.dtype))
        crops.mul_(keep.view(-1, 1, 1, 1).to(crops.dtype))
        return box, has, score, index, crops
    monkeypatch.setattr(pipeline.ops, "crop_resize_hands", crop)
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, k, True, perm, faces=faces)
    rgb, depth = pc.noise_frames(n, seed=3100).cuda(), pc.depth_noise(n, seed=4100).cuda()
    for graphed in (False, True):
        _o, r = _run(eng, rgb, depth, graphed=graphed)
        assert not bool(r.lifted[1].any()) and bool(r.lifted[0].any()) and bool(r.lifted[2].any())
        drawn = _check_overlay(f"no hand (graphed {graphed})", r.overlay.numpy(), r.mesh.numpy(), r.lifted.numpy(),
                               rgb.cpu().numpy(), faces)
        assert drawn[1] == 0 and drawn[0] >= DRAWN_FLOOR and drawn[2] >= DRAWN_FLOOR
        assert np.array_equal(r.overlay[1].numpy(), rr.frame_u8(rgb[1].cpu().numpy()))


def test_graph_replay_and_raw_frames(parts):
    """Eager against the captured step over several different frames through ONE graph: overlays bit-identical; forward_raw
    (bgr8 + 16UC1) equals the fp32 feed of the same frames; two runs are bit-identical; every frame draws at least DRAWN_FLOOR
    pixels and the frames' overlays differ from one another."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces)
    rng = np.random.default_rng(23)
    graph, seen = None, []
    for i in range(3):
        bgr = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
        mm = rng.integers(300, 1500, size=(1, H, W)).astype(np.uint16)
        rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
        dep = torch.from_numpy(mm.astype(np.float32) / 1000.0).unsqueeze(1).cuda()
        _o, e = _run(eng, rgb, dep)
        _o, g = _run(eng, rgb, dep, graphed=True)
        graph = graph or eng._graphs[(tuple(rgb.shape), tuple(dep.shape))][0]
        assert eng._graphs[(tuple(rgb.shape), tuple(dep.shape))][0] is graph and len(eng._graphs) == 1
        _o, g2 = _run(eng, rgb, dep, graphed=True)
        raw = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(mm))
        torch.cuda.synchronize()
        r = raw.read()
        for f in e._fields:
            if f == "words":
                assert e.words == g.words == r.words
            else:
                assert torch.equal(getattr(e, f), getattr(g, f)), (i, f)
                assert torch.equal(getattr(g, f), getattr(g2, f)), (i, f)
                assert torch.equal(getattr(g, f), getattr(r, f)), (i, f)
        drawn = _check_overlay(f"replay {i}", g.overlay.numpy(), g.mesh.numpy(), g.lifted.numpy(), rgb.cpu().numpy(), faces)
        assert drawn[0] >= DRAWN_FLOOR
        seen.append(g.overlay.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_faces_need_perm_reverse_on_the_gpu_engines(parts):
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    hand, lifter, perm, faces = parts
    with pytest.raises(ValueError, match="perm_reverse"):
        LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, None, faces=faces)
    with pytest.raises(ValueError, match="perm_reverse"):
        LiveHandEngine(hand, lifter, LIVE_PARAS, True, None, faces=faces)
    bad = faces.copy()
    bad[3, 1] = 778
    with pytest.raises(ValueError, match="778"):
        LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=bad)


def test_c_abi_on_raw_pointers():
    """hn_mesh_render_u8 through ctypes on raw device pointers equals ops.mesh_render; bad arguments return the error code,
    set hn_last_error and launch nothing (the outputs keep their fill)."""
    from hn_amd import _lib, ops
    lib = _lib.load()
    e1, f = rr.ellipsoid((0.02, -0.01, 0.55), (0.05, 0.08, 0.03))
    e2, _ = rr.ellipsoid((0.06, 0.02, 0.56), (0.06, 0.04, 0.04))
    mesh = torch.from_numpy(np.stack([e1, e2])).cuda()
    faces = torch.from_numpy(f).cuda()
    bgr = torch.from_numpy(_frame_u8(1, 480, 640, seed=9)).cuda()
    lifted = torch.ones((2,), dtype=torch.int32, device="cuda")
    want_depth = torch.zeros((1, 480, 640), device="cuda")
    want = ops.mesh_render(mesh, faces, PARAS, bgr, lifted=lifted, k=2, depth_out=want_depth)
    need = lib.hn_mesh_render_scratch_bytes(2, f.shape[0])
    scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 480, 640, 3), 7, dtype=torch.uint8, device="cuda")
    depth = torch.full((1, 480, 640), -3.0, device="cuda")
    paras = (C.c_float * 4)(*PARAS)
    host_faces = np.ascontiguousarray(f)
    stream = torch.cuda.current_stream().cuda_stream

    def call(v=777, nf=f.shape[0], fh=None, out_p=out.data_ptr(), s=2, k=2):
        return lib.hn_mesh_render_u8(mesh.data_ptr(), faces.data_ptr(), fh, lifted.data_ptr(), s, v, nf, k, paras, bgr.data_ptr(),
                                     _lib.FRAME_U8_BGR_HWC, 480, 640, scratch.data_ptr(), need, out_p, depth.data_ptr(), stream)
    for kw, word in ((dict(v=0), b"positive"), (dict(nf=0), b"positive"), (dict(out_p=None), b"out_image"),
                     (dict(v=700, fh=host_faces.ctypes.data), b"of 700"), (dict(k=3), b"multiple")):
        assert call(**kw) == 1, kw
        assert word in lib.hn_last_error(), (kw, lib.hn_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((depth == -3.0).all())           # nothing was launched
    assert call(fh=host_faces.ctypes.data) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(depth, want_depth)
    assert bool((depth > 0).sum() > 15000)
