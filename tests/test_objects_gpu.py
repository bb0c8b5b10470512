"""The held objects on the GPU (csrc/hand_object.hip through ops.hand_objects / ops.draw_object_labels and the C entries, and
the live steps with objects=True) against the rule in numpy float32 (tests/object_ref.py), bit for bit: no tolerance appears in
this file."""
import types

import numpy as np
import pytest
import torch

import object_cases as oc
import object_ref as orf
from test_occlude_gpu import H, LIVE_PARAS, W, _run, _same, inputs, parts  # noqa: F401  (the synthetic pipeline's fixtures)

pytestmark = pytest.mark.gpu

FIELDS = orf.FIELDS
SEED = 0                   # of the synthetic ext detector: the first of 0..15 whose step holds an object with a centroid
BAND = orf.OBJECT_BAND


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
    """outputs pre-filled with `fill` bytes, as the `out=` object of ops.hand_objects"""
    s = c.n * c.k
    raw = lambda words, dtype: torch.full((words * 4,), fill, dtype=torch.uint8, device="cuda").view(dtype)  # noqa: E731
    i32, f32 = torch.int32, torch.float32
    return types.SimpleNamespace(contact=raw(s, i32), object_index=raw(s, i32), object_box=raw(4 * s, f32).view(s, 4), object_score=raw(s, f32),
                                 object_point=raw(2 * s, f32).view(s, 2), object_xyz=raw(3 * s, f32).view(s, 3),
                                 object_extent=raw(6 * s, f32).view(s, 6), object_count=raw(2 * s, i32).view(s, 2))


def _device(c):
    from hn_amd import ops
    d = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731  (a copy: the cases are read-only)
    det = ops.Detections(d(c.boxes), d(c.scores), d(c.labels), None, None, None, d(c.count))
    depth = d(c.depth)
    if (c.n, c.k, c.h, c.w, c.cap) == oc.SHAPES[4]:      # the depth plane of an RGB-D tensor: frame stride 4 * H * W
        rgbd = torch.rand((c.n, 4, c.h, c.w), device="cuda")
        rgbd[:, 3] = depth
        depth = rgbd
    return dict(det=det, contacts=d(c.contacts), dxdymags=d(c.dxdymags), det_index=d(c.det_index), depth=depth, xyz_mm=d(c.xyz_mm))


# ---------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_against_the_rule(shape):
    """ops.hand_objects at the issue's five shapes on the seeded cases (tests/object_cases.py lists what they hold): the eight
    outputs equal object_ref bit for bit, written into buffers pre-filled with 0xFF; a second run gives the same bytes; so do
    a device camera table of equal rows in place of the host's four values and the C entry on raw pointers; without a
    silhouette the outputs equal the rule without the exclusion."""
    from hn_amd import _lib, ops
    c, want, bare = oc.case(*shape), oc.expected(*shape), oc.expected(*shape, with_silhouette=False)
    if shape == oc.SHAPES[0]:
        oc.check_conditions()
    t = _device(c)
    sil = torch.from_numpy(c.sil.copy()).cuda()
    kw = oc.kwargs(c)
    out = _filled(c)
    got = ops.hand_objects(**t, paras=c.paras, k=c.k, silhouette=sil, out=out, **kw)
    torch.cuda.synchronize()
    print(f"case {shape}: counts {want.object_count.reshape(-1, 2).tolist()}")
    assert got.object_count.data_ptr() == out.object_count.data_ptr()
    _differ(got, want, "op")
    again = ops.hand_objects(**t, paras=c.paras, k=c.k, silhouette=sil, out=_filled(c, 0x00), **kw)
    _differ(again, want, "second run")
    table = torch.tensor([c.paras] * c.n, dtype=torch.float32, device="cuda")
    _differ(ops.hand_objects(**t, paras=table, k=c.k, silhouette=sil, **kw), want, "camera table")
    _differ(ops.hand_objects(**t, paras=c.paras, k=c.k, **kw), bare, "no silhouette")
    # the C entry on raw pointers
    lib = _lib.load()
    need = lib.hn_hand_objects_scratch_bytes(c.n, c.k, c.h)
    assert need == ops.hand_objects_scratch_bytes(c.n, c.k, c.h) > 0
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    raw = _filled(c)
    depth = t["depth"]
    rgbd = depth.dim() == 4
    st = lib.hn_hand_objects_f32(t["det"].boxes.data_ptr(), t["det"].scores.data_ptr(), t["det"].labels.data_ptr(), t["det"].count.data_ptr(),
                                 t["contacts"].data_ptr(), t["dxdymags"].data_ptr(), t["det_index"].data_ptr(), c.cap, oc.OBJECT,
                                 depth.data_ptr() + (3 * c.h * c.w * 4 if rgbd else 0), (4 if rgbd else 1) * c.h * c.w, sil.data_ptr(),
                                 t["xyz_mm"].data_ptr(), 21, None, table.data_ptr(), c.n, c.k, c.h, c.w, c.stride, c.band, c.min_points,
                                 scratch.data_ptr(), need, *(getattr(raw, f).data_ptr() for f in FIELDS), None)
    torch.cuda.synchronize()
    assert st == 0, lib.hn_last_error()
    _differ(raw, want, "C entry")


def test_ops_refuse_bad_tensors_before_any_launch():
    from hn_amd import ops
    c = oc.case(*oc.SHAPES[1])
    good = dict(_device(c), paras=c.paras, k=c.k)
    sil = torch.from_numpy(c.sil.copy()).cuda()
    for kw, word in ((dict(k=17), "k = 17"), (dict(k=3), "det_index"), (dict(contacts=good["contacts"][:, :-1].contiguous()), "contacts"),
                     (dict(xyz_mm=good["xyz_mm"][1:].contiguous()), "xyz_mm"), (dict(depth=good["depth"][:1]), "scene_depth"),
                     (dict(silhouette=sil[:, 1:].contiguous()), "silhouette"), (dict(band=0), "object_band"), (dict(stride=0), "object_stride"),
                     (dict(min_points=0), "object_min_points"), (dict(paras=torch.zeros((3, 4), device="cuda")), "paras")):
        with pytest.raises(ValueError, match=word):
            ops.hand_objects(**{**good, **kw})
    with pytest.raises(ValueError, match="box_label"):
        ops.draw_object_labels(good["det"], good["det_index"], good["det_index"], torch.zeros((3, 5, 7, 3), dtype=torch.uint8, device="cuda"))


def test_label_draw_against_the_rule():
    """ops.draw_object_labels and the C entry on the (2,2,33,70,40) case, over an image of seeded bytes: the bytes equal the
    rule's, and every pixel off the rectangles and link lines keeps its own"""
    from hn_amd import _lib, ops
    c, want = oc.case(*oc.LABEL_SHAPE), oc.expected(*oc.LABEL_SHAPE)
    t = _device(c)
    img = np.random.default_rng(4).integers(0, 256, (c.n, c.h, c.w, 3)).astype(np.uint8)
    img[img[..., 2] == 255, 2] = 254                         # (no pixel holds the drawn colour beforehand)
    index = torch.from_numpy(want.object_index.copy()).cuda()
    expect, covered = orf.draw_object_labels(img, c.boxes, c.det_index, want.object_index)
    print(f"label draw: {int(covered.sum())} pixels covered, per frame {covered.reshape(c.n, -1).sum(1).tolist()}, slots "
          f"{want.object_index.tolist()}")
    assert int((want.object_index >= 0).sum()) >= 2 and covered.sum() >= 30 and not covered[1].any()
    got = ops.draw_object_labels(t["det"], t["det_index"], index, torch.from_numpy(img.copy()).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.tobytes() == expect.tobytes(), int((got != expect).sum())
    assert (got[~covered] == img[~covered]).all() and (got[covered] == orf.BLUE).all()
    raw = torch.from_numpy(img.copy()).cuda()
    lib = _lib.load()
    st = lib.hn_draw_object_labels_u8(t["det"].boxes.data_ptr(), t["det_index"].data_ptr(), index.data_ptr(), c.cap, c.n, c.k, c.h, c.w,
                                      raw.data_ptr(), None)
    torch.cuda.synchronize()
    assert st == 0 and raw.cpu().numpy().tobytes() == expect.tobytes()


# --------------------------------------------------------------------------------------------------------------- live steps
@pytest.fixture(scope="module")
def ext_sd():
    from hn_amd import synth
    return synth.make_fcos_state_dict(SEED, 3, ext=True)


@pytest.fixture(scope="module")
def ext_hand(ext_sd, a2j_sd):
    """the hand engine of the synthetic pipeline with the ext detector (the weights are keyed by name: seed 0's detections
    are the plain fixture's)"""
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    return HandNetEngine(FCOSEngine(ext_sd, 3, device="cuda", ext=True), A2JEngine(a2j_sd, device="cuda"), 3)


def _ext_net(ext_sd, a2j_sd):
    from fcos_utils.fcos import FCOS
    from handnet_pipeline.handnet_pipeline import HandNet
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    net.detector = FCOS(num_classes=3, ext=True, nms_thresh=0.5)
    net.detector.load_state_dict(ext_sd, strict=False)
    net.a2j.load_state_dict(a2j_sd, strict=False)
    return net.cuda().eval()


def _rule(out, r, depth, paras, sil=None, **kw):
    """object_ref on what the step itself left: its detections, contacts, dxdymags (device), its det_index, xyz_mm and
    silhouette (read()) and the depth map it ran on"""
    det, cpu = out.hands.detections, lambda t: t.cpu().numpy()  # noqa: E731
    return orf.hand_objects(cpu(det.boxes), cpu(det.scores), cpu(det.labels), cpu(det.count), cpu(out.hands.contacts), cpu(out.hands.dxdymags),
                            r.det_index.numpy(), cpu(depth), r.xyz_mm.numpy(), paras, object_label=1, silhouette=sil, **kw)


def _check_read(tag, out, r, depth, paras, sil=None, **kw):
    want = _rule(out, r, depth, paras, sil, **kw)
    print(f"{tag}: det_index {r.det_index.tolist()}, contacts {want.contact.tolist()}, object_index {want.object_index.tolist()}, "
          f"counts {want.object_count.tolist()}, xyz {want.object_xyz.round(3).tolist()}")
    _differ(r, want, tag)
    for name in FIELDS:
        assert torch.equal(getattr(out, name).cpu(), getattr(r, name)), (tag, name)
    return want


def test_live_step_end_to_end(parts, inputs, ext_sd, a2j_sd):  # noqa: F811
    """live_hands(max_hands=2, objects=True, occlude=True, faces=, labels=True) on the two synthetic frames with the ext
    detector: every field that exists without the option equals the same engine's with the option off, bit for bit (box_label
    only off the object rectangles and link lines, where it equals the rule's drawing over the plain step's image); the host
    buffer's prefix is unchanged but for those pixels; the eight new fields equal object_ref applied to what the step left;
    the device tensors equal read().  At least one slot holds an object and at least one has a centroid (seed 0 of the
    synthetic ext detector)."""
    _hand, lifter, perm, faces = parts
    rgb, depth = inputs
    net = _ext_net(ext_sd, a2j_sd)
    kw = dict(perm_reverse=perm, faces=faces, occlude=True, labels=True)
    with torch.inference_mode():
        out, r = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, objects=True, **kw), rgb, depth)
        host = out.host.clone()
        p_out, plain = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, **kw), rgb, depth)
    assert r._fields == plain._fields + FIELDS and type(r).__name__.endswith("ObjectsRead") and not type(plain).__name__.endswith("ObjectsRead")
    for name, tail, dtype in zip(FIELDS, ((), (), (4,), (), (2,), (3,), (6,), (2,)),
                                 (torch.int32, torch.int32) + (torch.float32,) * 5 + (torch.int32,)):
        for t in (getattr(r, name), getattr(out, name)):
            assert tuple(t.shape) == (2, 2) + tail and t.dtype == dtype, name
        assert getattr(p_out, name) is None
    assert out.hands.contacts is not None and p_out.hands.contacts is None
    want = _check_read("live_hands K = 2", out, r, depth, LIVE_PARAS, r.silhouette.numpy())
    assert (want.object_index >= 0).any() and (want.object_count[..., 1] == 0).any()          # not vacuous
    _same(plain, r, [f for f in plain._fields if f != "box_label"], "K = 2")
    boxes = out.hands.detections.boxes.cpu().numpy()
    expect, covered = orf.draw_object_labels(plain.box_label.numpy(), boxes, r.det_index.numpy(), want.object_index)
    print(f"box_label: {int(covered.sum())} pixels under object rectangles and link lines")
    assert covered.any() and r.box_label.numpy().tobytes() == expect.tobytes()
    assert (r.box_label.numpy()[~covered] == plain.box_label.numpy()[~covered]).all()
    lay, p_lay = out.layout, p_out.layout
    assert host.numel() == lay.nbytes > p_lay.nbytes == p_out.host.numel() and lay.contact_at >= p_lay.nbytes
    same = host[:p_lay.nbytes] == p_out.host
    same[lay.box_label_at:lay.box_label_at + covered.size * 3] |= torch.from_numpy(covered.reshape(-1).repeat(3))
    assert bool(same.all())


def test_graph_replay_and_raw_feed(parts, ext_hand, inputs):  # noqa: F811
    """One engine, one frame: the captured step equals the eager one; forward_raw with bgr8 + 16UC1 (millimetres) equals the
    fp32 feed of the same data; a replay after a copy of new inputs follows them"""
    from hn_amd.live import LiveHandsEngine
    _hand, lifter, perm, faces = parts
    eng = LiveHandsEngine(ext_hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, occlude=True, labels=True, objects=True)
    rng = np.random.default_rng(23)
    bgr = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    mm = rng.integers(300, 1500, size=(1, H, W)).astype(np.uint16)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    metres = torch.from_numpy(mm.astype(np.float32) / np.float32(1000.0)).unsqueeze(1).cuda()
    with torch.inference_mode():
        o_e, e = _run(eng, rgb, metres)
        _check_read("eager", o_e, e, metres, LIVE_PARAS, e.silhouette.numpy())
        o_g, g = _run(eng, rgb, metres, graphed=True)
        raw = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(mm))
        torch.cuda.synchronize()
        _same(e, g, e._fields, "graph replay")
        _same(e, raw.read(), e._fields, "16UC1")
        _check_read("16UC1", raw, raw.read(), metres, LIVE_PARAS, raw.read().silhouette.numpy())
        # new inputs into the same capture
        rgb2, depth2 = inputs[0][:1], inputs[1][:1]
        o_g2, g2 = _run(eng, rgb2, depth2, graphed=True)
        _o, e2 = _run(eng, rgb2, depth2)
    assert o_g2 is o_g and len([key for key in eng._graphs if "mirrored" not in key]) == 1
    _same(e2, g2, e2._fields, "replay on new inputs")
    _check_read("replay on new inputs", o_g2, g2, depth2, LIVE_PARAS, g2.silhouette.numpy())
    assert not torch.equal(g2.object_point, g.object_point) and eng._key_options()[-4:] == ("objects", BAND, 2, 50)


def test_left_works_in_the_mirrored_frame(parts, ext_hand, inputs):  # noqa: F811
    """left=True: every output equals the plain objects step's on frames and depth flipped along the width, and the rule
    applied to the mirrored depth map and the step's own (mirrored-frame) detections"""
    from hn_amd.live import LiveHandsEngine
    _hand, lifter, perm, _faces = parts
    rgb, depth = inputs[0][:1], inputs[1][:1]
    with torch.inference_mode():
        o_l, left = _run(LiveHandsEngine(ext_hand, lifter, LIVE_PARAS, 2, True, perm, left=True, objects=True), rgb, depth)
        flipped = depth.flip(3).contiguous()
        _o, want = _run(LiveHandsEngine(ext_hand, lifter, LIVE_PARAS, 2, True, perm, objects=True), rgb.flip(3).contiguous(), flipped)
    _same(want, left, want._fields, "left")
    _check_read("left", o_l, left, flipped, LIVE_PARAS)          # (a step without an overlay: no silhouette, no exclusion)


def test_per_frame_cameras_and_set_cameras(parts, ext_hand, inputs):  # noqa: F811
    """paras [N,4]: the captured step's objects equal the rule with a camera row per frame; after set_cameras the SAME graph's
    next replay gives the rule's centroids with the new rows"""
    from hn_amd.live import LiveHandsEngine
    _hand, lifter, perm, _faces = parts
    rgb, depth = inputs
    cams = np.array([LIVE_PARAS, (580.1, 600.7, 290.3, 260.9)])
    eng = LiveHandsEngine(ext_hand, lifter, cams, 2, True, perm, objects=True)
    with torch.inference_mode():
        out, r = _run(eng, rgb, depth, graphed=True)
        first = _check_read("cameras", out, r, depth, cams)
        graphs = len(eng._graphs)
        new = cams[::-1].copy()
        eng.set_cameras(new)
        eng.graphed(rgb, depth)[0]()
        torch.cuda.synchronize()
        moved = out.read()
    assert len(eng._graphs) == graphs
    after = _check_read("after set_cameras", out, moved, depth, new)
    assert (first.object_count[..., 1] == 0).any() and not np.array_equal(after.object_xyz, first.object_xyz)
    assert np.array_equal(after.object_index, first.object_index)
