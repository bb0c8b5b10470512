"""A camera per frame on the GPU (csrc/mesh_raster.hip's table form, ops.mesh_render with a table, the live engines with paras
[N,4], set_cameras, CropMeshEngine's overlay) against the per-frame rule in numpy (tests/cams_ref.py) and against the
one-camera path, which the existing tests pin to the reference."""
import functools

import numpy as np
import pytest
import torch

import cams_ref as cr
import occlude_ref as oc
import raster_ref as rr
from test_render_gpu import DEPTH_REL_BOUND          # the fp32-against-float64 depth bound of the one-camera test

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.01
H, W = 480, 640
LIVE_CAMS = np.array([[617.343, 617.343, 312.42, 241.42], [580.0, 600.0, 290.0, 260.0]], np.float32)
NEW_CAMS = np.array([[600.5, 630.25, 330.0, 225.5], [640.0, 590.0, 301.75, 250.0]], np.float32)
LIFTER_OUTPUT_SCALE = 0.01       # the hand-sized lifter of tests/test_render_gpu.py (its last graph convolution x 0.01)
DRAWN_FLOOR = 1000


# ---------------------------------------------------------------------------------------------------------------- op level
@functools.lru_cache(maxsize=None)
def _scene(k):
    meshes, faces = cr.scene(k)
    bgr = rr.frame_bgr8(len(meshes), *cr.HW, seed=40 + k)
    return meshes, faces, bgr, cr.frames_f32(bgr)


@functools.lru_cache(maxsize=None)
def _want(k, fmt):
    """the helper's images of the scene, worked out once and shared (nothing changes them)"""
    meshes, faces, bgr, f32 = _scene(k)
    frames = bgr if fmt == "bgr8" else f32
    image, depth, covered, amb = cr.render(meshes, faces, cr.CAMS, frames)
    _i, image2, _c, _a = cr.render_candidates(meshes, faces, cr.CAMS, frames)
    return image, image2, depth, covered, amb


def _gpu(meshes, faces, paras, frames, lifted=None, scene_depth=None, margin=0.01):
    """ops.mesh_render -> numpy (overlay, mesh Z[, silhouette, coverage]); paras: a 4-tuple, or [N,4] -> a device table"""
    from hn_amd import ops
    n, k = meshes.shape[:2]
    m = torch.from_numpy(np.ascontiguousarray(meshes)).cuda()
    fr = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    h, w = frames.shape[1:3] if frames.dtype == np.uint8 else frames.shape[2:]
    z = torch.full((n, h, w), -1.0, device="cuda")
    lf = None if lifted is None else torch.from_numpy(np.asarray(lifted, np.int32).reshape(-1)).cuda()
    if np.ndim(paras) == 2:
        paras = torch.from_numpy(np.ascontiguousarray(paras, np.float32)).cuda()
    more = {} if scene_depth is None else dict(scene_depth=torch.from_numpy(np.ascontiguousarray(scene_depth)).cuda(), margin=margin)
    res = ops.mesh_render(m, faces, paras, fr, lifted=lf, k=k, depth_out=z, **more)
    torch.cuda.synchronize()
    res = res if isinstance(res, tuple) else (res,)
    return (res[0].cpu().numpy(), z.cpu().numpy()) + tuple(t.cpu().numpy() for t in res[1:])


@pytest.mark.parametrize("fmt", ("bgr8", "fp32"))
@pytest.mark.parametrize("k", (1, 2))
def test_op_against_the_rule(k, fmt):
    """ops.mesh_render with a [3,4] table: coverage equals the helper's exactly; off the depth fights the overlay equals
    cams_ref byte for byte and the mesh Z lies within the one-camera test's bound; on a depth fight the colour is one of the two
    candidates'; depth fights are at most 1 % of the covered pixels of every frame; two runs are bit-identical."""
    meshes, faces, bgr, f32 = _scene(k)
    frames = bgr if fmt == "bgr8" else f32
    want, want2, want_z, covered, amb = _want(k, fmt)
    img, z = _gpu(meshes, faces, cr.CAMS, frames)
    for i in range(len(meshes)):
        share = amb[i].sum() / max(1, covered[i].sum())
        clear = covered[i] & ~amb[i]
        rel = float((np.abs(z[i][clear].astype(np.float64) - want_z[i][clear]) / want_z[i][clear]).max())
        wrong = int((img[i][~amb[i]] != want[i][~amb[i]]).any(axis=-1).sum())
        print(f"k {k} {fmt} frame {i}: covered {int(covered[i].sum())}, depth fights {int(amb[i].sum())} ({share:.2%}), depth max "
              f"rel {rel:.3e}, pixels off the helper's image {wrong}")
        assert covered[i].sum() >= 500
        assert share <= AMBIGUOUS_CAP, f"frame {i}: {share:.2%} of the covered pixels are depth fights"
        assert np.array_equal(z[i] > 0, covered[i]), f"frame {i}: coverage differs"
        assert wrong == 0, f"frame {i}: {wrong} pixels off the depth fights differ from the helper's image"
        assert rel <= DEPTH_REL_BOUND, f"frame {i}: depth off by {rel:.3e} relative"
        fight = amb[i]
        one_of = (img[i][fight] == want[i][fight]).all(axis=-1) | (img[i][fight] == want2[i][fight]).all(axis=-1)
        assert one_of.all(), f"frame {i}: a depth fight shows neither candidate"
    again, z_again = _gpu(meshes, faces, cr.CAMS, frames)
    assert np.array_equal(again, img) and np.array_equal(z_again, z)


def test_equal_cameras_are_the_scalar_path():
    """A table of three copies of one camera against the 4-tuple call on the same inputs: overlay and mesh Z bit-identical, no
    pixel left out; with scene_depth, silhouette and coverage too."""
    meshes, faces, bgr, f32 = _scene(2)
    lifted = np.array([[1, 1], [0, 1], [1, 1]], np.int32)
    depth = cr.hiding_depth(meshes, faces, np.repeat(cr.CAMS[:1], 3, axis=0))
    for row in cr.CAMS[:2]:
        table, one = np.repeat(row[None], 3, axis=0), tuple(float(v) for v in row)
        for frames in (bgr, f32):
            a, b = _gpu(meshes, faces, table, frames, lifted), _gpu(meshes, faces, one, frames, lifted)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert (a[1] > 0).sum() > 1500
            a, b = _gpu(meshes, faces, table, frames, lifted, depth), _gpu(meshes, faces, one, frames, lifted, depth)
            assert len(a) == len(b) == 4
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            assert (a[2] & oc.HIDDEN).any() and ((a[2] != 0) & ((a[2] & oc.HIDDEN) == 0)).any()


def test_row_indexing():
    """N = 3, k = 2, one slot not lifted: frame i equals the 4-tuple call on frame i alone with row i, byte for byte (image, Z,
    and -- occluded -- silhouette and coverage); the slot with lifted == 0 draws nothing; frame 1 drawn with row 0 is another
    image."""
    meshes, faces, bgr, _f32 = _scene(2)
    lifted = np.array([[1, 1], [1, 0], [1, 1]], np.int32)
    depth = cr.hiding_depth(meshes, faces, cr.CAMS)
    whole = _gpu(meshes, faces, cr.CAMS, bgr, lifted)
    whole_occ = _gpu(meshes, faces, cr.CAMS, bgr, lifted, depth)
    for i in range(3):
        one = tuple(float(v) for v in cr.CAMS[i])
        alone = _gpu(meshes[i:i + 1], faces, one, bgr[i:i + 1], lifted[i:i + 1])
        assert np.array_equal(whole[0][i], alone[0][0]) and np.array_equal(whole[1][i], alone[1][0]), i
        alone = _gpu(meshes[i:i + 1], faces, one, bgr[i:i + 1], lifted[i:i + 1], depth[i:i + 1])
        assert np.array_equal(whole_occ[0][i], alone[0][0]) and np.array_equal(whole_occ[1][i], alone[1][0]), i
        assert np.array_equal(whole_occ[2][i], alone[2][0]) and np.array_equal(whole_occ[3][2 * i:2 * i + 2], alone[3]), i
    # frame 1's second slot is not drawn: the frame equals the call with the near mesh alone
    near = _gpu(meshes[1:2, :1], faces, tuple(float(v) for v in cr.CAMS[1]), bgr[1:2])
    assert np.array_equal(whole[0][1], near[0][0]) and np.array_equal(whole[1][1], near[1][0])
    assert whole_occ[3][3].tolist() == [0, 0] and not ((whole_occ[2][1] & 0x7F) == 2).any()
    both = _gpu(meshes[1:2], faces, tuple(float(v) for v in cr.CAMS[1]), bgr[1:2])
    assert not np.array_equal(both[0][0], whole[0][1])                      # (the far mesh would have shown)
    wrong_row = _gpu(meshes[1:2], faces, tuple(float(v) for v in cr.CAMS[0]), bgr[1:2], lifted[1:2])
    assert not np.array_equal(wrong_row[0][0], whole[0][1])                 # (the cameras do differ)


def test_occluded_form_against_the_rule():
    """The k = 2 scene behind a depth map that hides part of the near mesh of every frame: overlay, silhouette and coverage
    against occlude_ref per frame with that frame's row, off the depth fights and threshold pixels (at most 1 % of the covered
    pixels); on those the silhouette's slot is the nearest or the second-nearest face's; coverage equals the counts of the
    GPU's own silhouette exactly."""
    meshes, faces, bgr, _f32 = _scene(2)
    depth, margin = cr.hiding_depth(meshes, faces, cr.CAMS), 0.01
    img, _z, sil, cov = _gpu(meshes, faces, cr.CAMS, bgr, None, depth, margin)
    for i, want in enumerate(cr.occluded(meshes, faces, cr.CAMS, bgr, depth, margin)):
        out = want.fights | want.threshold
        clear = ~out
        n_cov, n_out = int(want.covered.sum()), int((want.covered & out).sum())
        mine = oc.count(sil[i], 2)
        print(f"frame {i}: covered {n_cov}, hidden {int(want.hidden.sum())}, left out {n_out} ({n_out / max(1, n_cov):.3%}), "
              f"coverage {cov[2 * i:2 * i + 2].tolist()} (helper {want.coverage.tolist()})")
        assert want.hidden.sum() >= 100 and (want.covered & ~want.hidden).sum() >= 100
        assert n_out <= AMBIGUOUS_CAP * n_cov
        assert np.array_equal(sil[i][clear], want.silhouette[clear])
        assert np.array_equal(img[i][clear], want.image[clear])
        who = (sil[i][out].astype(np.int64) & 0x7F) - 1
        assert np.array_equal(sil[i][out] != 0, want.covered[out])
        assert (((who == want.slot[out]) | ((who == want.slot2[out]) & (want.slot2[out] >= 0))) | ~want.covered[out]).all()
        assert np.array_equal(cov[2 * i:2 * i + 2], mine)
        assert int(np.abs(cov[2 * i:2 * i + 2].astype(np.int64) - want.coverage).max()) <= n_out


def test_the_op_refuses_a_bad_table():
    from hn_amd import ops
    meshes, faces, bgr, _f32 = _scene(1)
    m, fr = torch.from_numpy(meshes).cuda(), torch.from_numpy(bgr).cuda()
    good = torch.from_numpy(cr.CAMS).cuda()
    for bad in (good[:2].contiguous(), good.double(), good.cpu(), good.t().contiguous(), good[:, None, :].contiguous(),
                good.repeat(1, 2)[:, :4]):
        with pytest.raises(ValueError):
            ops.mesh_render(m, faces, bad, fr, k=1)
    assert ops.mesh_render(m, faces, good, fr, k=1).shape == (3, *cr.HW, 3)
    # a 4-sequence routes as ever, a 1-D tensor of four values included
    a = ops.mesh_render(m, faces, tuple(float(v) for v in cr.CAMS[0]), fr, k=1)
    assert torch.equal(a, ops.mesh_render(m, faces, torch.from_numpy(cr.CAMS[0]), fr, k=1))


# ------------------------------------------------------------------------------------------------------------ whole steps
@pytest.fixture(scope="module")
def lifter(golden_dir):
    from hn_amd import synth
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    from test_render_gpu import _synthetic_faces
    g = np.load(golden_dir / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    p2m_sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    last = max(int(key.split(".")[2]) for key in p2m_sd if key.startswith("pose2mesh.cl."))
    for key in (f"pose2mesh.cl.{last}.weight", f"pose2mesh.cl.{last}.bias"):
        p2m_sd[key] = p2m_sd[key] * LIFTER_OUTPUT_SCALE
    return Pose2MeshEngine(p2m_sd, graphs, device="cuda"), g["perm_reverse"][:778], _synthetic_faces()


@pytest.fixture(scope="module")
def net(fcos_sd, a2j_sd):
    from test_render_gpu import _net
    return _net(fcos_sd, a2j_sd)


@functools.lru_cache(maxsize=None)
def _inputs(n, steps=1):
    from hn_amd import synth
    return [(synth.make_rgb(n, seed=1000 + 10 * t).cuda(), synth.make_depth(n, seed=2000 + 10 * t).cuda()) for t in range(steps)]


def _run_steps(eng, inputs):
    """the engine's eager step on every input in turn -> the reads (the trackers and filters start empty)"""
    if getattr(eng, "track", None) is not None:
        eng.track_reset()
    reads = []
    with torch.inference_mode():
        for rgb, depth in inputs:
            out = eng.forward_device(rgb, depth)
            torch.cuda.synchronize()
            reads.append(out.read())
    return reads


def _same_frame(tag, a, b, i):
    """frame i of two reads of the same step type, byte for byte: every field (records, mesh, images, tracker, filters)"""
    assert type(a)._fields == type(b)._fields
    for f in type(a)._fields:
        x, y = getattr(a, f), getattr(b, f)
        if f == "words":
            assert x == y, (tag, f)
        elif isinstance(x, (list, tuple)):             # (the one-hand step's [image_uvd, xyz_mm])
            assert len(x) == len(y) and all(torch.equal(p[i], q[i]) for p, q in zip(x, y)), (tag, f, i)
        else:
            assert torch.equal(x[i], y[i]), (tag, f, i)


def _whole_step(make, n, steps=1):
    """The multi-camera step against the one-camera step with the same options, frame by frame: engine(cams[i]) runs on the
    SAME batch of n frames (equal batches, equal convolution plans), and its frame i must be the multi-camera step's frame i.
    The engines share one HandNet engine, whose conversion the engine built last owns: build, run, read, then build the next."""
    inputs = _inputs(n, steps)
    multi = _run_steps(make(LIVE_CAMS[:n]), inputs)
    for i in range(n):
        single = _run_steps(make(tuple(float(v) for v in LIVE_CAMS[i])), inputs)
        for t in range(steps):
            _same_frame(f"step {t}", multi[t], single[t], i)
    return multi


def test_whole_step_frame_by_frame(net, lifter):
    """live_hands (K = 2, faces, perm_reverse, labels) and live with [N,4] cameras, N = 2: frame i equals frame i of the same
    step built with the 4-tuple cams[i] -- records, mesh, overlay, box_label, pose_label -- and the two frames' cameras do
    change the result (xyz, mesh and overlay of frame 1 differ from the step built with camera 0 alone)."""
    lift, perm, faces = lifter
    opts = dict(perm_reverse=perm, faces=faces, labels=True)
    multi = _whole_step(lambda p: net.live_hands(lift, p, max_hands=2, **opts), 2)[0]
    assert multi.overlay is not None and multi.box_label is not None and bool(multi.lifted[:, 0].all())
    for i in range(2):
        frame = torch.from_numpy(rr.frame_u8(_inputs(2)[0][0][i].cpu().numpy()))
        assert int((multi.overlay[i] != frame).any(dim=-1).sum()) >= DRAWN_FLOOR                     # (the mesh is drawn)
    cam0 = _run_steps(net.live_hands(lift, tuple(float(v) for v in LIVE_CAMS[0]), max_hands=2, **opts), _inputs(2))[0]
    assert torch.equal(cam0.keypoints, multi.keypoints) and torch.equal(cam0.image_uvd, multi.image_uvd)
    assert not torch.equal(cam0.xyz_mm[1], multi.xyz_mm[1]) and not torch.equal(cam0.mesh[1], multi.mesh[1])
    assert not torch.equal(cam0.overlay[1], multi.overlay[1])
    one = _whole_step(lambda p: net.live(lift, p, **opts), 2)[0]
    assert one.overlay is not None and one.pose_label is not None


def test_whole_step_occluded(net, lifter):
    lift, perm, faces = lifter
    multi = _whole_step(lambda p: net.live_hands(lift, p, max_hands=2, perm_reverse=perm, faces=faces, occlude=True), 2)[0]
    assert multi.silhouette is not None and int(multi.coverage[..., 0].sum()) >= DRAWN_FLOOR


def test_whole_step_tracked_and_smoothed(net, lifter):
    lift, perm, faces = lifter
    multi = _whole_step(lambda p: net.live_hands(lift, p, max_hands=2, perm_reverse=perm, faces=faces, track=True, smooth=True),
                        2, steps=3)
    assert bool((multi[2].track_id[:, 0] > 0).all()) and multi[2].smooth_mesh is not None


def _equal_reads(a, b):
    for i in range(a.keypoints.shape[0]):
        _same_frame("read", a, b, i)


def test_capture_and_set_cameras(net, lifter):
    """The captured multi-camera step equals the eager one byte for byte; after set_cameras the SAME graph (none added) gives
    what a fresh engine built with the new rows gives eagerly; a 4-tuple engine has no set_cameras; N + 1 frames raise."""
    lift, perm, faces = lifter
    (rgb, depth), = _inputs(2)
    make = lambda p: net.live_hands(lift, p, max_hands=2, perm_reverse=perm, faces=faces, labels=True, occlude=True)  # noqa: E731
    eng = make(LIVE_CAMS)
    eager = _run_steps(eng, [(rgb, depth)])[0]
    with torch.inference_mode():
        run, s_img, s_dep, out = eng.graphed(rgb, depth)
        s_img.copy_(rgb)
        s_dep.copy_(depth)
        run()
        torch.cuda.synchronize()
        captured = out.read()
        _equal_reads(eager, captured)
        graphs, graph = len(eng._graphs), next(iter(eng._graphs.values()))[0]
        tables = (eng.cams.data_ptr(), eng._cameras.rows(2).data_ptr())
        eng.set_cameras(NEW_CAMS)
        run()
        torch.cuda.synchronize()
        moved = out.read()
        assert len(eng._graphs) == graphs and next(iter(eng._graphs.values()))[0] is graph
        assert (eng.cams.data_ptr(), eng._cameras.rows(2).data_ptr()) == tables
        assert torch.equal(eng.cams.cpu(), torch.from_numpy(NEW_CAMS))
        moved_eager = eng.forward_device(rgb, depth)
        torch.cuda.synchronize()
        _equal_reads(moved, moved_eager.read())
        with pytest.raises(ValueError, match="3 frames"):
            eng.forward_device(torch.cat([rgb, rgb[:1]]), torch.cat([depth, depth[:1]]))
        with pytest.raises(ValueError, match="3 frames"):
            eng.graphed(torch.cat([rgb, rgb[:1]]), torch.cat([depth, depth[:1]]))
        assert len(eng._graphs) == graphs
    assert not torch.equal(moved.xyz_mm, captured.xyz_mm) and not torch.equal(moved.overlay, captured.overlay)
    assert torch.equal(moved.keypoints, captured.keypoints)
    fresh = _run_steps(make(NEW_CAMS), [(rgb, depth)])[0]
    _equal_reads(moved, fresh)
    single = make(tuple(float(v) for v in LIVE_CAMS[0]))
    with pytest.raises(ValueError, match="camera per frame"):
        single.set_cameras(NEW_CAMS)
    with pytest.raises(ValueError, match="camera per frame"):
        net.live(lift, tuple(float(v) for v in LIVE_CAMS[0]), perm_reverse=perm).set_cameras(NEW_CAMS)


# ---------------------------------------------------------------------------------------------------------- crop-mesh step
def _crop_batch(k, seed):
    """dataset-like samples: depth crops, float32 boxes, per-sample intrinsics that clearly differ, full images (bgr8)"""
    from hn_amd import synth
    g = torch.Generator().manual_seed(seed)
    crops = synth.make_crops(k, 176, seed=seed)
    x1, y1 = 150 + torch.rand((k,), generator=g) * 150, 100 + torch.rand((k,), generator=g) * 100
    box = torch.stack([x1, y1, x1 + 120 + torch.rand((k,), generator=g) * 80, y1 + 120 + torch.rand((k,), generator=g) * 80], dim=1)
    paras = torch.from_numpy(LIVE_CAMS[:k].copy()) + torch.rand((k, 4), generator=g) * 20
    frames = torch.from_numpy(rr.frame_bgr8(k, H, W, seed=seed))
    return crops.cuda(), box.float().cuda(), paras.float().cuda(), frames.cuda()


def test_crop_mesh_step_draws_every_sample_with_its_own_camera(a2j_sd, lifter):
    """A2JModel.mesh(lifter, perm_reverse=, faces=) on K = 2 crops with two cameras and two full images, eager and captured:
    .overlay[i] is ops.mesh_render (4-tuple path) of the step's own mesh[i] over frames[i] with paras[i], byte for byte; the
    five items of read() equal those of the engine built without faces bit for bit, whose `host` has today's size; a second
    captured step takes new frames and intrinsics from the static inputs without a new capture."""
    from a2j.a2j import A2JModel
    from hn_amd import ops
    lift, perm, faces = lifter
    a2j = A2JModel(21, 176, 176)
    a2j.load_state_dict(a2j_sd, strict=False)
    a2j = a2j.cuda().eval()
    eng, plain = a2j.mesh(lift, perm_reverse=perm, faces=faces), a2j.mesh(lift, perm_reverse=perm)
    dev_faces = ops.mesh_faces(faces, 778, "cuda")
    k = 2

    def check(tag, out, r, frames, paras):
        assert tuple(r.overlay.shape) == (k, H, W, 3) and r.overlay.dtype == torch.uint8 and torch.equal(out.overlay.cpu(), r.overlay)
        for i in range(k):
            one = tuple(float(v) for v in paras[i].cpu())
            want = ops.mesh_render(out.mesh[i:i + 1].contiguous(), dev_faces, one, frames[i:i + 1].contiguous(), k=1)
            assert torch.equal(want[0].cpu(), r.overlay[i]), (tag, i)
            drawn = int((r.overlay[i] != torch.from_numpy(rr.frame_u8(frames[i].cpu().numpy()))).any(dim=-1).sum())
            print(f"{tag}: sample {i}: {drawn} pixels drawn")
            assert drawn >= 100, (tag, i, drawn)
        other = ops.mesh_render(out.mesh[1:2].contiguous(), dev_faces, tuple(float(v) for v in paras[0].cpu()),
                                frames[1:2].contiguous(), k=1)
        assert not torch.equal(other[0].cpu(), r.overlay[1]), tag                 # (sample 1 was drawn with ITS camera)

    def same_five(a, b):
        assert len(a) == len(b) == 5
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x, y)
        assert a[4] == b[4]

    crops, box, paras, frames = _crop_batch(k, seed=51)
    for fr in (frames, torch.from_numpy(cr.frames_f32(frames.cpu().numpy())).cuda()):
        out = eng.forward_device(crops, box, paras, fr)
        torch.cuda.synchronize()
        r = out.read()
        check(f"eager {fr.dtype}", out, r, fr, paras)
    p_out = plain.forward_device(crops, box, paras)
    torch.cuda.synchronize()
    p = p_out.read()
    kp, img, xyz, mesh, words = p                                             # (unpacks into five items, as ever)
    assert p.overlay is None and p_out.overlay is None and p_out.host_overlay is None
    same_five(r, p)
    assert p_out.host.dtype == torch.float32 and p_out.host.numel() == 3 * k * 21 * 3 + k * 778 * 3 + 4 == out.host.numel()
    assert torch.equal(p_out.host, out.host)
    no_frames = eng.forward_device(crops, box, paras)                         # (an engine with faces, a step without frames)
    torch.cuda.synchronize()
    assert no_frames.overlay is None and no_frames.read().overlay is None
    with pytest.raises(ValueError, match="faces"):
        plain.forward_device(crops, box, paras, frames)
    # captured, then a second batch through the same graph
    run, s_crops, s_box, s_paras, s_frames, g_out = eng.graphed(crops, box, paras, frames)
    p_run, p_crops, p_box, p_paras, pg_out = plain.graphed(crops, box, paras)
    seen = []
    for seed in (51, 52):
        crops, box, paras, frames = _crop_batch(k, seed=seed)
        for dst, src in ((s_crops, crops), (s_box, box), (s_paras, paras), (s_frames, frames), (p_crops, crops), (p_box, box),
                         (p_paras, paras)):
            dst.copy_(src)
        run()
        p_run()
        torch.cuda.synchronize()
        g = g_out.read()
        check(f"captured, batch {seed}", g_out, g, frames, paras)
        same_five(g, pg_out.read())
        seen.append(g.overlay)
        assert len(eng._graphs) == 1
    assert not torch.equal(seen[0], seen[1])
