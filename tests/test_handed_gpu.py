"""Left hands in the live chain on the GPU: the whole-frame mirror (left=True: the reference's ImageListener(left=True)) and
per-slot handedness (handed=True: left-hand slots go mirrored through A2J and the lifter and come back un-mirrored).  Every
expectation is built from ops that existed before, from torch / numpy, or from tests/handed_ref.py -- never from the new
arguments themselves."""
import numpy as np
import pytest
import torch

import handed_ref as hr
import parity_cases as pc
from test_labels_gpu import _check_against_rule, _kernel_launches, _same
from test_render_gpu import DRAWN_FLOOR, LIFTER_OUTPUT_SCALE, _check_overlay, _synthetic_faces

pytestmark = pytest.mark.gpu

H, W = 480, 640
PARAS = (617.343, 617.343, 312.42, 241.42)
# noise frames on which the detector's first two hand detections differ in side in frames 1 and 2 (sides 0,1 / 0,1) and agree in
# frames 0 and 3 (0,0), by the CPU oracle (oracle/fcos_ref.py); the tests assert what they need of it on the step's own output
SEED = 3000


@pytest.fixture(scope="module")
def parts(golden_dir, fcos_sd, a2j_sd):
    """(HandNetEngine, Pose2MeshEngine with a hand-sized output as tests/test_render_gpu.py's, perm_reverse[:778], faces)"""
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


def _frames(n=4, first=0):
    rgb, depth = pc.noise_frames(4, seed=SEED), pc.depth_noise(4, seed=SEED + 1000)
    return rgb[first:first + n].contiguous().cuda(), depth[first:first + n].contiguous().cuda()


def _host(eng, rgb, depth, graphed=False):
    """The step's whole host buffer (a copy) and its output object."""
    if graphed:
        run, s_img, s_dep, out = eng.graphed(rgb, depth)
        s_img.copy_(rgb)
        s_dep.copy_(depth)
        run()
    else:
        out = eng.forward_device(rgb, depth)
    torch.cuda.synchronize()
    return out.host.clone(), out


def _engine(parts, hands, **kw):
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
    hand, lifter, perm, faces = parts
    if hands is None:
        return LiveHandEngine(hand, lifter, PARAS, True, perm, **kw)
    return LiveHandsEngine(hand, lifter, PARAS, hands, True, perm, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. left=True is the same engine on flipped input
# ---------------------------------------------------------------------------------------------------------------------
def _camera(seed, h, w):
    rng = np.random.default_rng(seed)
    bgr = rng.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8)
    mm = rng.integers(300, 1500, size=(1, h, w)).astype(np.uint16)
    return bgr, mm


@pytest.mark.parametrize("w", [640, 642, 7])
@pytest.mark.parametrize("kind", ["16UC1", "32FC1", "none"])
def test_ingest_flip_is_ingest_of_the_flipped_arrays(kind, w):
    from hn_amd import ops
    bgr, mm = _camera(5, 12, w)
    raw = {"16UC1": mm, "32FC1": mm.astype(np.float32) / np.float32(1000.0), "none": None}[kind]
    flipped = (torch.from_numpy(np.ascontiguousarray(np.flip(bgr, 2))),
               None if raw is None else torch.from_numpy(np.ascontiguousarray(np.flip(raw, 2))))
    for place in ("device", "pinned"):
        put = (lambda t: None if t is None else t.cuda()) if place == "device" else (lambda t: None if t is None else t.pin_memory())
        # (the kernel reads pinned memory when it runs, not when it is launched: the inputs live until the sync below)
        src = put(torch.from_numpy(bgr)), put(None if raw is None else torch.from_numpy(raw))
        src_f = put(flipped[0]), put(flipped[1])
        got = ops.ingest_raw(*src, flip_w=True, want_rgbd=raw is not None)
        want = ops.ingest_raw(*src_f, want_rgbd=raw is not None)
        plain = ops.ingest_raw(*src, flip_w=False, want_rgbd=raw is not None)
        torch.cuda.synchronize()
        for g, x, p in zip(got, want, plain):
            assert (g is None) == (x is None)
            if g is not None:
                assert torch.equal(g, x), (kind, w, place)
                assert torch.equal(p.flip(-1), x)


@pytest.mark.parametrize("shape,other", [((2, 3, 48, 640), (2, 1, 48, 640)), ((1, 3, 9, 642), (1, 4, 9, 642)), ((3, 5, 7), None),
                                         ((1, 3, 480, 640), (1, 1, 480, 640))])
def test_flip_w_op(shape, other):
    from hn_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.rand(shape, generator=g).cuda()
    if other is None:
        out = ops.flip_w(x)
        torch.cuda.synchronize()
        assert torch.equal(out, x.flip(-1))
        return
    y = torch.rand(other, generator=g).cuda()
    ox, oy = ops.flip_w(x, y)
    torch.cuda.synchronize()
    assert torch.equal(ox, x.flip(-1)) and torch.equal(oy, y.flip(-1))
    with pytest.raises(ValueError):
        ops.flip_w(x, out=x)


@pytest.mark.parametrize("w", [640, 642])
@pytest.mark.parametrize("hands", [None, 2])
def test_left_is_the_engine_on_flipped_input(parts, hands, w):
    """Every host buffer of a left=True step -- records, lifted, mesh, overlay, box_label, pose_label -- equals the buffer of the
    same engine without `left` on frames flipped along the width: eager, captured, and from raw camera buffers (uint16 and
    float32 depth; pinned host and device memory)."""
    faces = parts[3]
    plain, lefty = _engine(parts, hands, faces=faces, labels=True), _engine(parts, hands, faces=faces, labels=True, left=True)
    assert plain.left is False and lefty.left is True
    bgr, mm = _camera(70 + w, H, w)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    dep = torch.from_numpy(mm.astype(np.float32) / 1000.0).unsqueeze(1).cuda()
    rgb_f, dep_f = rgb.flip(-1).contiguous(), dep.flip(-1).contiguous()
    for graphed in (False, True):
        want, o_want = _host(plain, rgb_f, dep_f, graphed)
        got, o_got = _host(lefty, rgb, dep, graphed)
        assert got.numel() == want.numel() and torch.equal(got, want), ("graphed" if graphed else "eager", hands, w)
        # (the inputs the caller handed in are not touched)
        assert torch.equal(rgb.flip(-1), rgb_f)
    assert bool(want.any()) and int((o_want.read().has_hand != 0).sum()) > 0, "the fixture detects no hand"
    # a mirrored frame is another frame: the step's results differ from the unflipped ones
    unflipped, _o = _host(plain, rgb, dep)
    assert not torch.equal(unflipped, want)
    bgr_f, mm_f = np.ascontiguousarray(np.flip(bgr, 2)), np.ascontiguousarray(np.flip(mm, 2))
    for kind in ("16UC1", "32FC1"):
        conv = (lambda a: torch.from_numpy(a)) if kind == "16UC1" else (lambda a: torch.from_numpy(a.astype(np.float32) / np.float32(1000.0)))
        for place in ("pinned", "device", "pageable"):
            put = {"pinned": lambda t: t.pin_memory(), "device": lambda t: t.cuda(), "pageable": lambda t: t}[place]
            held = put(torch.from_numpy(bgr_f)), put(conv(mm_f)), put(torch.from_numpy(bgr)), put(conv(mm))
            o = plain.forward_raw(held[0], held[1])
            torch.cuda.synchronize()
            want_raw = o.host.clone()
            o = lefty.forward_raw(held[2], held[3])
            torch.cuda.synchronize()
            assert torch.equal(o.host, want_raw), (kind, place, hands, w)
            assert torch.equal(want_raw, want)        # ... and the raw feed is the fp32 feed of the same frames
    # the capture forward_raw replays holds no mirror launch: it is not the one graphed() made
    assert len(lefty._graphs) == 2 and len(plain._graphs) == 1


def test_left_with_handed_raises(parts):
    with pytest.raises(ValueError):
        _engine(parts, 2, left=True, handed=True)


# ---------------------------------------------------------------------------------------------------------------------
# 2. handed=False is today's step; handed=True adds no launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [False, True])
def test_handed_false_is_todays_step_and_handed_adds_no_launch(parts, labels):
    from hn_amd import live
    rgb, dep = _frames(1, first=1)
    default, explicit, handed = _engine(parts, 2, labels=labels), _engine(parts, 2, labels=labels, handed=False), \
        _engine(parts, 2, labels=labels, handed=True)
    hw = (H, W) if labels else None
    assert default._layout(1, hw).nbytes == explicit._layout(1, hw).nbytes == handed._layout(1, hw).nbytes - 4 * 2
    assert default._layout(1).nbytes == live.LiveLayout(1, 2, 778).nbytes == 21880
    for graphed in (False, True):
        a, oa = _host(default, rgb, dep, graphed)
        b, ob = _host(explicit, rgb, dep, graphed)
        assert torch.equal(a, b) and oa.side is None and ob.side is None and "side" not in ob.read()._fields
    counts = [_kernel_launches(lambda e=e: e.forward_device(rgb, dep)) for e in (default, explicit, handed)]
    print(f"K=2 labels={labels}: kernel launches of an eager step: default {counts[0]}, handed=False {counts[1]}, handed=True {counts[2]}")
    assert counts[0] == counts[1] == counts[2]
    if counts[0] is not None:
        assert counts[2] == (146 if labels else 144)


# ---------------------------------------------------------------------------------------------------------------------
# 3. side
# ---------------------------------------------------------------------------------------------------------------------
def _expected_side(out):
    det, idx = out.hands.detections, out.hands.det_index.reshape(out.n, out.k).long()
    gathered = torch.gather(det.sides, 1, idx.clamp(min=0))
    return torch.where(idx >= 0, gathered, torch.full_like(gathered, -1)).to(torch.int32)


def test_side_is_the_detectors_side_of_the_slot(parts):
    from hn_amd import ops
    rgb, dep = _frames(4)
    eng = _engine(parts, 2, handed=True)
    _h, out = _host(eng, rgb, dep, graphed=True)
    r = out.read()
    assert r._fields[-1] == "side" and r.side.dtype == torch.int32 and tuple(r.side.shape) == (4, 2)
    want = _expected_side(out).cpu()
    assert torch.equal(r.side, want) and torch.equal(out.side.cpu(), want)
    filled = r.has_hand != 0
    print("sides per frame:", r.side.tolist(), "filled:", filled.tolist())
    assert bool((r.side[~filled] == -1).all())
    assert bool((r.side[filled] == 0).any()) and bool((r.side[filled] == 1).any()), "both sides must occur"
    both = filled.all(dim=1) & (r.side[:, 0] != r.side[:, 1])
    assert bool(both.any()), "no frame holds one hand of each side"
    assert torch.equal(out.mirror.cpu(), (filled & (r.side == 0)).to(torch.int32))
    # left_side picks the other hands
    _h, other = _host(_engine(parts, 2, handed=True, left_side=1), rgb, dep)
    assert torch.equal(other.read().side, r.side)
    assert torch.equal(other.mirror.cpu(), (filled & (r.side == 1)).to(torch.int32))
    # the drop-in's forward_hands hands the sides over as a sixth result, from the engine's own record
    hand = parts[0]
    o = hand.forward_hands(rgb, dep, 2, to_host=True, handed=True)
    torch.cuda.synchronize()
    from hn_amd.pipeline import read_hands_tail
    _s, _i, side = read_hands_tail(o.host_record, 8, handed=True)
    assert torch.equal(side.view(4, 2), r.side)
    # empty slots at op level: a frame with one hand detection among others and a frame with none, K = 3
    det = ops.alloc_detections(2, 8, "cuda")
    det.boxes[0, :3] = torch.tensor([[10.0, 10.0, 60.0, 60.0], [200.0, 150.0, 248.0, 198.0], [300.0, 100.0, 380.0, 190.0]])
    det.labels[0, :3] = torch.tensor([1, 2, 2], dtype=torch.int32)
    det.sides[0, :3] = torch.tensor([0, 1, 0], dtype=torch.int32)
    det.scores[0, :3] = torch.tensor([0.95, 0.9, 0.8])
    det.count[0] = 3
    _b, has, _sc, idx, crops, side, mirror = ops.crop_resize_hands(det, 2, dep[:2].contiguous(), 3, handed=True, left_side=0)
    torch.cuda.synchronize()
    assert idx.tolist() == [[1, 2, -1], [-1, -1, -1]] and has.tolist() == [[1, 1, 0], [0, 0, 0]]
    assert side.tolist() == [[1, 0, -1], [-1, -1, -1]] and mirror.tolist() == [[0, 1, 0], [0, 0, 0]]
    assert not bool(crops[2:].any()) and bool(crops[0].any()) and bool(crops[1].any())


# ---------------------------------------------------------------------------------------------------------------------
# 4. mirrored slots by composition of the ops that existed before
# ---------------------------------------------------------------------------------------------------------------------
def _compose(parts, det, depth, mirror, k):
    """The handed chain from existing ops only: plain crops -> flip the mirrored ones -> the A2J engine -> 176 - u in torch
    -> the caller's clamps + convert_joints -> the gated lifter input, column 0 negated -> the lifter -> x negated ->
    mesh_finish.  mirror: bool [S] on the device."""
    from hn_amd import ops
    hand, lifter, perm, _faces = parts
    box, has, _score, _idx, crops = ops.crop_resize_hands(det, 2, depth, k)
    s = crops.shape[0]
    m = mirror.view(s)
    crops_m = torch.where(m.view(s, 1, 1, 1), crops.flip(2), crops).contiguous()
    valid = has.view(s).clone()
    kp_m = hand.a2j.forward_nhwc(crops_m, valid=valid)
    kp = kp_m.clone()
    kp[:, :, 0] = torch.where(m.view(s, 1), torch.tensor(176.0, device="cuda") - kp_m[:, :, 0], kp_m[:, :, 0])
    kc = torch.clamp(kp, 0.0, 176.0)
    bc = box.view(s, 4).clone()
    bc[:, :2] = torch.clamp(bc[:, :2], 0, depth.shape[2])
    bc[:, 2:] = torch.clamp(bc[:, 2:], 0, depth.shape[3])
    img = ops.convert_joints(kc, bc, valid=valid)
    xyz = ops.convert_joints(kc, bc, valid=valid, paras=PARAS)
    p2d, lifted = ops.lifter_input_gated(img, valid=valid)
    flip = m & (lifted != 0)
    p2d = p2d.clone()
    p2d[:, :, 0] = torch.where(flip.view(s, 1), -p2d[:, :, 0], p2d[:, :, 0])
    raw, _pose3d = lifter.forward(p2d.contiguous())
    raw = raw.clone()
    raw[:, :, 0] = torch.where(m.view(s, 1), -raw[:, :, 0], raw[:, :, 0])
    mesh = ops.mesh_finish(raw.contiguous(), torch.as_tensor(perm).to(torch.int64).cuda(), xyz, valid=lifted)
    torch.cuda.synchronize()
    return dict(crops=crops_m, keypoints=kp, image_uvd=img, xyz_mm=xyz, lifted=lifted, mesh=mesh, has=valid, box=box, p2d=p2d)


def test_captured_handed_step_is_the_composition(parts):
    """The captured handed step (N = 4, K = 2: the batch of the composition, the same slot order): crops, records, lifted and
    mesh bit for bit."""
    rgb, dep = _frames(4)
    eng = _engine(parts, 2, handed=True)
    _h, out = _host(eng, rgb, dep, graphed=True)
    r = out.read()
    mirror = out.mirror.reshape(-1) != 0
    assert bool(mirror.any()) and not bool(mirror.all()), "the fixture needs mirrored and plain slots"
    want = _compose(parts, out.hands.detections, dep, mirror, 2)
    assert torch.equal(out.hands.crops_nhwc, want["crops"])
    # (a mirrored crop is not its plain crop: the comparison above is not vacuous)
    plain_eng = _engine(parts, 2)
    _h2, plain = _host(plain_eng, rgb, dep, graphed=True)
    assert not torch.equal(plain.hands.crops_nhwc[mirror], out.hands.crops_nhwc[mirror])
    assert torch.equal(plain.hands.crops_nhwc[~mirror], out.hands.crops_nhwc[~mirror])
    s = 8
    assert torch.equal(out.hands.has_hand.view(s), want["has"])
    assert torch.equal(r.keypoints.view(s, 21, 3), want["keypoints"].cpu())
    assert torch.equal(r.image_uvd.view(s, 21, 3), want["image_uvd"].cpu())
    assert torch.equal(r.xyz_mm.view(s, 21, 3), want["xyz_mm"].cpu())
    assert torch.equal(r.lifted.view(s), want["lifted"].cpu() != 0) and bool(r.lifted.view(s)[mirror.cpu()].any())
    assert torch.equal(out.pose2d, want["p2d"])
    assert torch.equal(r.mesh.view(s, 778, 3), want["mesh"].cpu())
    # slots that are not mirrored are the plain step's, bit for bit
    pr = plain.read()
    keep = ~mirror.cpu()
    for f in ("keypoints", "image_uvd", "xyz_mm", "mesh", "lifted", "crop_box", "score", "det_index"):
        a, b = getattr(r, f), getattr(pr, f)
        assert torch.equal(a.reshape((s,) + a.shape[2:])[keep], b.reshape((s,) + b.shape[2:])[keep]), f
    # the eager step: the same batch (no slot is empty here, so A2J is not compacted): bit for bit too
    _h3, eager = _host(eng, rgb, dep)
    _same(eager.read(), r, "eager vs captured")


@pytest.mark.parametrize("mask", ["zeros", "ones", "mixed"])
def test_ops_with_an_explicit_mirror_mask(parts, mask):
    """The same comparison at op level with a mask of the test's choosing (the detections' sides are overwritten): all
    plain, all mirrored, mixed."""
    from hn_amd import ops
    hand, lifter, perm, _faces = parts
    rgb, dep = _frames(4)
    k, s = 2, 8
    det, _cand = hand.fcos.detect(rgb)
    m = {"zeros": torch.zeros(s, dtype=torch.bool), "ones": torch.ones(s, dtype=torch.bool),
         "mixed": torch.tensor([1, 0, 0, 1, 1, 1, 0, 0], dtype=torch.bool)}[mask].cuda()
    _b, has0, _s0, idx0, _c = ops.crop_resize_hands(det, 2, dep, k)
    assert bool((has0 != 0).all())
    sides = torch.full_like(det.sides, 7)
    sides.scatter_(1, idx0.long(), torch.where(m.view(4, 2), 3, 5).to(torch.int32))
    det3 = ops.Detections(det.boxes, det.scores, det.labels, sides, det.level, det.keep, det.count)
    box, has, score, idx, crops, side, mirror = ops.crop_resize_hands(det3, 2, dep, k, handed=True, left_side=3)
    assert torch.equal(mirror.view(s) != 0, m) and torch.equal(side.view(s), torch.where(m, 3, 5).to(torch.int32))
    want = _compose(parts, det, dep, m, k)
    assert torch.equal(crops, want["crops"]) and torch.equal(idx, idx0)
    valid = has.view(s).clone()
    conv = dict(crop_box=box.view(s, 4), paras=PARAS, crop=176, clamp_keypoints=True, clamp_box=(H, W), mirror=mirror.view(s))
    kp, img, xyz = hand.a2j.forward_nhwc(crops, valid=valid, convert=conv)
    assert torch.equal(kp, want["keypoints"]) and torch.equal(img, want["image_uvd"]) and torch.equal(xyz, want["xyz_mm"])
    p2d, lifted = ops.lifter_input_gated(img, valid=valid, mirror=mirror.view(s))
    assert torch.equal(lifted, want["lifted"]) and torch.equal(p2d, want["p2d"]) and bool(lifted.any())
    raw, _p3 = lifter.forward(p2d)
    perm_t = torch.as_tensor(perm).to(torch.int64).cuda()
    mesh = ops.mesh_finish(raw, perm_t, xyz, valid=lifted, mirror=mirror.view(s))
    assert torch.equal(mesh, want["mesh"])
    # without the final mesh's permutation: the raw vertices, x negated where mirrored, zero rows where not lifted
    bare = ops.mesh_finish(raw, None, None, valid=lifted, mirror=mirror.view(s))
    sign = torch.where(m.view(s, 1, 1), torch.tensor([-1.0, 1.0, 1.0], device="cuda"), torch.ones(3, device="cuda"))
    assert torch.equal(bare, raw * sign * lifted.view(s, 1, 1))
    # ... and handed_ref's numpy statement of rule 5 on one mirrored, lifted slot
    pick = int(torch.nonzero(lifted != 0).flatten()[0])
    ref = hr.final_mesh_mirrored(raw[pick].cpu().numpy(), np.asarray(perm), xyz[pick, 0].cpu().numpy(), bool(m[pick]))
    assert np.array_equal(mesh[pick].cpu().numpy(), ref)
    if mask == "zeros":     # the mirror entries with an all-zero mask are the plain entries
        kp0, img0, xyz0 = hand.a2j.forward_nhwc(crops, valid=has.view(s).clone(), convert={c: v for c, v in conv.items() if c != "mirror"})
        assert torch.equal(kp0, kp) and torch.equal(img0, img) and torch.equal(xyz0, xyz)
        assert torch.equal(ops.mesh_finish(raw, perm_t, xyz, valid=lifted), mesh)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a mirrored slot is a mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_a_mirrored_slot_is_the_mirror_image_of_the_plain_slot_on_the_mirrored_frame(parts):
    """Frame 0 and its mirror image as frame 1, one forced detection each whose PADDED boxes are mirror images (88 px wide and
    high, so the nearest-neighbour resize is the exact 2x and commutes with the flip): slot 0 runs mirrored on the original,
    slot 1 plain on the mirror image.  Same crop -> crop keypoints (176 - u, v, d) and a mesh reflected in x about the root
    joint, at the suite's batch-consistency bounds (1e-4 on keypoints, 2e-3 on mesh vertices)."""
    from hn_amd import ops
    hand, lifter, perm, _faces = parts
    d0 = pc.depth_noise(1, seed=SEED + 7)
    depth = torch.cat([d0, d0.flip(-1)]).contiguous().cuda()
    det = ops.alloc_detections(2, 8, "cuda")
    det.boxes[0, 0] = torch.tensor([200.0, 150.0, 248.0, 198.0])
    det.boxes[1, 0] = torch.tensor([392.0, 150.0, 440.0, 198.0])
    det.labels[:, 0] = 2
    det.scores[:, 0] = 0.9
    det.sides[0, 0], det.sides[1, 0] = 0, 1
    det.count[:] = 1
    box, has, _sc, _ix, crops, side, mirror = ops.crop_resize_hands(det, 2, depth, 1, handed=True, left_side=0)
    assert mirror.view(-1).tolist() == [1, 0] and has.view(-1).tolist() == [1, 1]
    b = box.view(2, 4).cpu()
    assert b[0].tolist() == [180, 130, 267, 217]
    # mirror-image boxes: columns b0 .. b2 of the original are columns W-1-b2 .. W-1-b0 of the mirror image
    assert b[1, 0] == W - 1 - b[0, 2] and b[1, 2] == W - 1 - b[0, 0] and b[1, 1] == b[0, 1] and b[1, 3] == b[0, 3]
    assert torch.equal(crops[0], crops[1]) and bool(crops[0].any())
    valid = has.view(2).clone()
    conv = dict(crop_box=box.view(2, 4), paras=PARAS, crop=176, clamp_keypoints=True, clamp_box=(H, W), mirror=mirror.view(2))
    kp, img, xyz = hand.a2j.forward_nhwc(crops, valid=valid, convert=conv)
    want = kp[1].clone()
    want[:, 0] = 176.0 - want[:, 0]
    err_kp = (kp[0] - want).abs().max().item()
    p2d, lifted = ops.lifter_input_gated(img, valid=valid, mirror=mirror.view(2))
    assert lifted.tolist() == [1, 1], "the forced hands must pass the lifter's gate"
    raw, _p3 = lifter.forward(p2d)
    mesh = ops.mesh_finish(raw, torch.as_tensor(perm).to(torch.int64).cuda(), xyz, valid=lifted, mirror=mirror.view(2))
    torch.cuda.synchronize()
    # out['mesh'] = (x, -y, -z) of (vertex + root): relative to the root joint, slot 0 is slot 1 with x reflected
    root = xyz[:, 0] / 1000.0 * torch.tensor([1.0, -1.0, -1.0], device="cuda")
    rel = mesh - root[:, None, :]
    err_mesh = (rel[0] - rel[1] * torch.tensor([-1.0, 1.0, 1.0], device="cuda")).abs().max().item()
    # the image joints are mirror images too: u0 = W - 1 - u1
    err_img = (img[0, :, 0] - (W - 1 - img[1, :, 0])).abs().max().item()
    print(f"mirrored slot vs plain slot on the mirrored frame: keypoints {err_kp:.3e}, image u {err_img:.3e}, mesh {err_mesh:.3e}; "
          f"mesh extent in x {float(rel[1, :, 0].abs().max()):.3f} m")
    assert err_kp < 1e-4 and err_mesh < 2e-3 and err_img < 1e-4 * 88 / 176 + 1e-4
    assert float(rel[1, :, 0].abs().max()) > 10 * 2e-3, "the mesh is too small for the bound to tell a reflection from none"


# ---------------------------------------------------------------------------------------------------------------------
# 6. the images of a handed step
# ---------------------------------------------------------------------------------------------------------------------
def test_images_of_a_handed_step_follow_the_rules(parts):
    """Overlay and labels of a handed step equal tests/raster_ref.py / tests/draw_ref.py fed the step's own mesh, keypoints and
    boxes -- with the pixel rules of tests/test_render_gpu.py and tests/test_labels_gpu.py."""
    faces = parts[3]
    rgb, dep = _frames(2, first=1)
    eng = _engine(parts, 2, faces=faces, labels=True, handed=True)
    _h, out = _host(eng, rgb, dep, graphed=True)
    r = out.read()
    assert r._fields[-4:] == ("overlay", "box_label", "pose_label", "side")
    mirrored = (out.mirror.cpu() != 0) & r.lifted
    assert bool(mirrored.any()) and bool((r.lifted & ~mirrored).any()), "the fixture needs a lifted mirrored and a lifted plain slot"
    drawn = _check_overlay("handed", r.overlay.numpy(), r.mesh.numpy(), r.lifted.numpy(), rgb.cpu().numpy(), faces, PARAS)
    assert min(drawn) >= DRAWN_FLOOR
    _check_against_rule("handed", r, r.lifted.numpy(), 2, rgb)
    # the images differ from the plain step's where a mirrored hand is drawn
    _h2, plain = _host(_engine(parts, 2, faces=faces, labels=True), rgb, dep, graphed=True)
    pr = plain.read()
    assert not torch.equal(pr.pose_label[mirrored], r.pose_label[mirrored])
    plain_slots = out.mirror.cpu() == 0
    assert torch.equal(pr.pose_label[plain_slots], r.pose_label[plain_slots])


# ---------------------------------------------------------------------------------------------------------------------
# 7. degenerate and empty slots
# ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_slots_do_not_poison_the_handed_step(parts, a2j_sd, fcos_sd):
    """tests/test_live_hands_gpu.py::test_degenerate_slots_do_not_poison_the_step with handed=True: A2J's output convolutions
    zeroed put every joint of a slot on one point, so the gate refuses every slot; the captured handed step raises nothing,
    lifts nothing and hands over all-zero, finite rows; an empty frame's slots are zeros with side -1."""
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandsEngine
    from hn_amd.pipeline import HandNetEngine, check_range_contract
    _hand, lifter, perm, _faces = parts
    sd = {k: v.clone() for k, v in a2j_sd.items()}
    for head in ("regressionModel", "classificationModel", "DepthRegressionModel"):
        sd[f"{head}.output.weight"].zero_()
        sd[f"{head}.output.bias"].zero_()
    hand = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(sd, device="cuda"), 3)
    eng = LiveHandsEngine(hand, lifter, PARAS, 2, True, perm, handed=True)
    rgb, dep = _frames(2, first=1)
    _h, out = _host(eng, rgb, dep, graphed=True)
    r = out.read()
    assert int((r.has_hand == 1).sum()) == 4
    assert bool((out.mirror.cpu() != 0).any())
    check_range_contract(r.keypoints, r.words, has_hand=r.has_hand)
    assert not any(r.words[:3])
    assert not bool(r.lifted.any()) and not r.mesh.any() and not bool(out.pose2d.any())
    assert bool(torch.isfinite(out.raw_mesh).all()) and bool(torch.isfinite(out.pose3d).all()) and bool(torch.isfinite(r.keypoints).all())
    ref = hand.forward_hands(rgb, dep, max_hands=2, handed=True)
    torch.cuda.synchronize()
    assert torch.equal(r.keypoints, ref.keypoints.cpu()) and torch.equal(r.crop_box, ref.crop_box.cpu())
    assert torch.equal(r.side, ref.side.cpu())
    # empty slots: a detector whose hand class never passes the score threshold fills no slot
    quiet = HandNetEngine(FCOSEngine(pc.shift_detector_bias(fcos_sd, hand_shift=-40.0), 3, device="cuda"), hand.a2j, 3)
    _h, out = _host(LiveHandsEngine(quiet, lifter, PARAS, 2, True, perm, handed=True), rgb, dep, graphed=True)
    e = out.read()
    assert not bool(e.has_hand.any()) and bool((e.side == -1).all()) and bool((e.det_index == -1).all())
    assert not bool(out.mirror.any()) and not bool(e.lifted.any())
    for f in ("keypoints", "crop_box", "score", "image_uvd", "xyz_mm", "mesh"):
        assert not bool(getattr(e, f).any()), f
    assert not any(e.words[:3]) and bool(torch.isfinite(out.raw_mesh).all()) and bool(torch.isfinite(out.pose3d).all())


# ---------------------------------------------------------------------------------------------------------------------
# the capture owns what its launches write; the drop-in; the compacted eager step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hands", [None, 2])
def test_a_left_capture_owns_its_mirrored_inputs(parts, hands):
    """The captured left=True step on fp32 frames mirrors into buffers whose addresses are baked into the graph: the engine
    keeps them for as long as the capture lives.  Tensors of the frames' sizes allocated and filled AFTER graphed() returned
    are untouched by later replays, and the replay still gives the step's bytes."""
    import gc
    eng = _engine(parts, hands, left=True)
    rgb, dep = _frames(1, first=1)
    first, _o = _host(eng, rgb, dep, graphed=True)
    held = [t for pair in eng._mirrored.values() for t in pair]
    assert any(t.shape == rgb.shape for t in held) and any(t.shape == dep.shape for t in held)
    gc.collect()
    later = [torch.full_like(rgb, 7.0) for _ in range(6)] + [torch.full_like(dep, 7.0) for _ in range(6)]
    assert not {t.data_ptr() for t in later} & {t.data_ptr() for t in held}
    torch.cuda.synchronize()
    for _ in range(3):
        again, _o = _host(eng, rgb, dep, graphed=True)
    assert torch.equal(again, first)
    assert all(bool((t == 7.0).all()) for t in later)


def test_dropin_forward_hands_hands_the_sides_over(parts, fcos_sd, a2j_sd):
    """HandNet.forward_hands(handed=True): a sixth result, the sides per slot on the CPU -- eagerly and after the call has
    switched to graph replay -- equal to the detections' sides gathered at the slots' ranks; mirrored slots' keypoints are the
    engine's handed step's."""
    import types
    from handnet_pipeline.handnet_pipeline import HandNet
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    net.detector.load_state_dict(fcos_sd, strict=False)
    net.a2j.load_state_dict(a2j_sd, strict=False)
    net = net.cuda().eval()
    rgb, depth = _frames(4)
    eng = net.engine()
    ref = eng.forward_hands(rgb, depth, max_hands=2, handed=True)
    idx = ref.det_index.reshape(4, 2).long()
    want = torch.where(idx >= 0, torch.gather(ref.detections.sides, 1, idx.clamp(min=0)), torch.full_like(idx, -1).int()).cpu()
    ref_kp, ref_mirror, ref_crops = ref.keypoints.clone().cpu(), ref.mirror.clone().cpu(), ref.crops_nhwc.clone()
    plain = eng.forward_hands(rgb, depth, max_hands=2).keypoints.clone().cpu()
    assert bool((want == 0).any()) and bool((want == 1).any()) and bool(ref_mirror.any())
    with torch.inference_mode():
        assert len(net.forward_hands(rgb, depth, max_hands=2)) == 5
        for call in range(net.AUTO_GRAPH_CALLS + 2):
            res = net.forward_hands(rgb, depth, max_hands=2, handed=True)
            assert len(res) == 6
            kp, db, _boxes, mask, _scores, sides = res
            assert sides.dtype == torch.int32 and sides.device.type == "cpu" and torch.equal(sides, want), call
            assert (kp - ref_kp).abs().max().item() < 3e-4
            assert torch.equal(db, ref_crops[mask.view(-1).cuda()][..., 0].unsqueeze(1))
    # a mirrored slot's keypoints are not the plain step's
    assert (ref_kp[ref_mirror != 0] - plain[ref_mirror != 0]).abs().max().item() > 1e-2
    assert eng.has_graph_hands(rgb.shape, depth.shape, 2, to_host=True, handed=True)
    assert not eng.has_graph_hands(rgb.shape, depth.shape, 2, to_host=True, handed=True, left_side=1)


def test_compacted_eager_step_carries_the_mirror_flags(parts, monkeypatch):
    """Fewer than half of the N*K = 16 slots filled: the next eager handed step runs A2J on the filled slots only, with their
    mirror flags -- another A2J batch size, so the suite's batch-consistency bounds apply (1e-4 on keypoints, 2e-3 on mesh
    vertices) against the dense step on the same slots; rows of the emptied slots are zeros."""
    from hn_amd import pipeline
    hand = parts[0]
    n, k = 8, 2
    rgb, depth = pc.noise_frames(n, seed=SEED).cuda(), pc.depth_noise(n, seed=SEED + 1000).cuda()
    keep = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    keep[:5, 0] = 1
    keep[2, 1] = 1
    real = pipeline.ops.crop_resize_hands

    def sparse_crop(*a, **kw):
        box, has, score, index, crops, side, mirror = real(*a, **kw)
        has.mul_(keep)
        mirror.mul_(keep)
        box.mul_(keep[..., None].to(box.dtype))
        crops.mul_(keep.view(-1, 1, 1, 1).to(crops.dtype))
        return box, has, score, index, crops, side, mirror
    monkeypatch.setattr(pipeline.ops, "crop_resize_hands", sparse_crop)
    calls = []
    real_fwd = hand.a2j.forward_nhwc

    def spy(x, valid=None, **kw):
        calls.append((x.shape[0], kw.get("convert", {}).get("mirror")))
        return real_fwd(x, valid=valid, **kw)
    monkeypatch.setattr(hand.a2j, "forward_nhwc", spy)
    eng = _engine(parts, k, handed=True)
    hand._sparse_hint, hand._hand_stat = False, None
    _h, out = _host(eng, rgb, depth)                  # masked full batch; its count arms the hint
    dense, dense_mirror = out.read(), out.mirror.clone().cpu()
    _h, out = _host(eng, rgb, depth)                  # compacted
    sparse = out.read()
    monkeypatch.setattr(hand.a2j, "forward_nhwc", real_fwd)
    hand._sparse_hint, hand._hand_stat = False, None
    assert [c[0] for c in calls] == [n * k, 6], calls
    sel = keep.bool().cpu()
    assert torch.equal(calls[1][1].cpu(), dense_mirror[sel]) and bool(dense_mirror[sel].any()) and not bool(dense_mirror[sel].all())
    assert torch.equal(sparse.has_hand, dense.has_hand) and torch.equal(sparse.side, dense.side)
    assert torch.equal(sparse.lifted, dense.lifted) and bool(dense.lifted[sel].any())
    for f in ("keypoints", "image_uvd", "xyz_mm", "mesh"):
        assert not getattr(sparse, f)[~sel].any(), f
    err_kp = (sparse.keypoints[sel] - dense.keypoints[sel]).abs().max().item()
    err_mesh = (sparse.mesh[sel] - dense.mesh[sel]).abs().max().item()
    print(f"compacted handed step vs dense: keypoints {err_kp:.3e}, mesh {err_mesh:.3e}")
    assert err_kp < 1e-4 and err_mesh < 2e-3
