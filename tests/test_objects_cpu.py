"""The held objects without a GPU: the rule (tests/object_ref.py) on a hand-computed case, its association against a float64
restatement of the reference's lines, its invariance under the order of the pixels; the cases' conditions; the layout of an
objects step's copy buffer; the public surfaces; and every refusal of the C entries and of the Python layer (all of them come
before any launch)."""
import ctypes as C
import inspect
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import object_cases as oc
import object_ref as orf

F = np.float32
FIELDS = ("contact", "object_index", "object_box", "object_score", "object_point", "object_xyz", "object_extent", "object_count")


# ----------------------------------------------------------------------------------------------------------------- the rule
def test_the_smallest_case_by_hand():
    """8 x 8, one hand (row 0, box 1 1 5 5, contact 3, vector (2^-13, 1, 0)), objects at rows 1 (3 2 7 6) and 2 (0 0 4 4):
    p = (3 + 1.220703125, 3); d(row 1) = (5 - p.x)^2 + 1, d(row 2) = (2 - p.x)^2 + 1: row 1.  Its box holds the 16 pixels
    c 3..6, r 2..5 (stride 1); (3, 4) is NaN, (4, 5) is 0, (2, 3) lies under a mesh (0x81), (2, 4) holds the bare hidden flag
    (0x80: no hand): 13 matches on a wall at z = 500 * 0.001f."""
    c = oc.case(*oc.SHAPES[0])
    got = oc.expected(*oc.SHAPES[0])
    assert got.contact.tolist() == [[3]] and got.object_index.tolist() == [[1]] and got.object_box.tolist() == [[[3.0, 2.0, 7.0, 6.0]]]
    assert got.object_score[0, 0] == c.scores[0, 1] and got.object_point.tolist() == [[[4.220703125, 3.0]]]
    assert got.object_count.tolist() == [[[13, 0]]]
    z = F(500.0) * F(0.001)
    pixels = [(r, col) for r in range(2, 6) for col in range(3, 7) if (r, col) not in ((3, 4), (4, 5), (2, 3))]
    fx, fy, cx, cy = (F(v) for v in c.paras)
    xs = [((F(col) + F(0.5)) - cx) * z / fx for _, col in pixels]
    ys = [((F(r) + F(0.5)) - cy) * z / fy for r, _ in pixels]
    for a, values in enumerate((xs, ys, [z] * 13)):
        total = sum(int(np.rint(F(v) * F(1e6))) for v in values)
        assert got.object_xyz[0, 0, a] == F(total / (13 * 1e6))
        assert got.object_extent[0, 0, a] == min(values) and got.object_extent[0, 0, 3 + a] == max(values)
    bare = oc.expected(*oc.SHAPES[0], with_silhouette=False)
    assert bare.object_count.tolist() == [[[14, 0]]]
    few = orf.hand_objects(c.boxes, c.scores, c.labels, c.count, c.contacts, c.dxdymags, c.det_index, c.depth, c.xyz_mm, c.paras,
                           silhouette=c.sil, band=c.band, stride=1, min_points=14)
    assert few.object_count.tolist() == [[[13, 2]]] and not few.object_xyz.any() and few.object_extent.tobytes() == got.object_extent.tobytes()


def _reference_lines(objects, hand):
    """voc_eval.py:687-699 restated in float64 on one hand [x1 y1 x2 y2 state m vx vy] and the objects' boxes -> position or None"""
    if hand[4] <= 0 or len(objects) == 0:
        return None
    centres = np.array([[(o[0] + o[2]) / 2, (o[1] + o[3]) / 2] for o in objects], np.float64)
    hand_cc = np.array([(hand[0] + hand[2]) / 2, (hand[1] + hand[3]) / 2])
    point_cc = np.array([hand_cc[0] + hand[5] * 10000 * hand[6], hand_cc[1] + hand[5] * 10000 * hand[7]])
    return int(np.argmin(np.sum((centres - point_cc) ** 2, axis=1)))


def test_the_association_is_the_references_on_exact_inputs():
    """integer boxes and dyadic vectors: every fp32 operation of the rule is exact, so its choice is the float64 lines' choice,
    ties included (np.argmin keeps the first minimum, as the scan does)"""
    rng = np.random.default_rng(5)
    ties = chosen = 0
    for trial in range(60):
        cap, k = 24, 4
        count = int(rng.integers(0, cap + 1))
        boxes = (rng.integers(0, 4, (1, cap, 4)) * 8).astype(F)           # (few distinct centres: equal distances do occur)
        boxes[..., 2:] += boxes[..., :2] + 8
        labels = rng.integers(1, 3, (1, cap)).astype(np.int32)
        contacts = rng.integers(0, 5, (1, cap)).astype(np.int32)
        vec = np.stack([rng.integers(0, 9, (1, cap)) * 2.0 ** -16, rng.integers(-4, 5, (1, cap)) / 4, rng.integers(-4, 5, (1, cap)) / 4], -1).astype(F)
        hands = [r for r in range(count) if labels[0, r] == oc.HAND][:k]
        det_index = np.full((1, k), -1, np.int32)
        det_index[0, :len(hands)] = hands
        contact, index, box, score, pt, status = orf.associate(boxes, rng.random((1, cap)).astype(F), labels, np.array([count]), contacts,
                                                               vec, det_index, oc.OBJECT)
        objects = [r for r in range(count) if labels[0, r] == oc.OBJECT]
        for kk, j in enumerate(hands):
            hand = [float(v) for v in boxes[0, j]] + [int(contacts[0, j])] + [float(v) for v in vec[0, j]]
            want = _reference_lines([boxes[0, r].astype(np.float64) for r in objects], hand)
            assert index[0, kk] == (-1 if want is None else objects[want]), (trial, kk)
            if want is not None:
                chosen += 1
                d = [orf.distance2(boxes[0, r], tuple(pt[0, kk])) for r in objects]
                ties += sum(v == min(d) for v in d) > 1
        assert (index[0, len(hands):] == -1).all() and (status[0, len(hands):] == -1).all()
    assert chosen >= 50 and ties >= 3, (chosen, ties)


def test_the_scan_keeps_the_earlier_of_a_tie_and_a_first_nan():
    nan = F(np.nan)
    assert orf.scan([F(3), F(1), F(1), F(2)]) == 1 and orf.scan([F(1), nan, F(0.5), F(0.5)]) == 2
    assert orf.scan([nan, F(0), F(1)]) == 0 and orf.scan([F(np.inf), F(np.inf)]) == 0 and orf.scan([F(np.inf), nan, F(7)]) == 2


@pytest.mark.parametrize("shape", oc.SHAPES[:3] + oc.SHAPES[4:])
def test_the_pixel_order_does_not_matter(shape):
    """integer sums, minima and maxima: any permutation of the matches gives the same bytes"""
    c, want = oc.case(*shape), oc.expected(*shape)
    rng = np.random.default_rng(11)
    for order in (lambda m: rng.permutation(m), lambda m: np.arange(m)[::-1]):
        got = orf.hand_objects(c.boxes, c.scores, c.labels, c.count, c.contacts, c.dxdymags, c.det_index, c.depth, c.xyz_mm, c.paras,
                               silhouette=c.sil, order=order, **oc.kwargs(c))
        for name in FIELDS:
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


def test_the_cases_hold_what_they_are_for():
    want = oc.check_conditions()
    c = oc.case(*oc.SHAPES[4])
    i, kk = c.notes["edges"]
    # the four stamped pixels: the two on the band's edges match, their outer neighbours do not
    box = want[oc.SHAPES[4]].object_box[i, kk]
    rows, cols = orf.candidates(box, c.depth[i], c.sil[i], F(500.0) * F(0.001), c.band, c.stride)
    matched = set(zip(rows.tolist(), cols.tolist()))
    assert [((r, col) in matched) for r, col, _ in c.notes["edge_pixels"]] == [inside for _, _, inside in c.notes["edge_pixels"]] == [True, False, True, False]


def test_the_label_rule_draws_a_rectangle_and_a_line():
    boxes = np.zeros((1, 3, 4), F)
    boxes[0, 0], boxes[0, 2] = (2.4, 1.6, 6.5, 5.5), (9.5, 6.0, 14.0, 9.49)          # the hand, the object
    img = np.full((1, 12, 16, 3), 7, np.uint8)
    out, covered = orf.draw_object_labels(img, boxes, np.array([[0, -1]], np.int32), np.array([[2, -1]], np.int32))
    assert orf.object_primitives(boxes, np.array([[0]]), np.array([[2]])) == [(0, (10, 6, 14, 9), (4, 4, 12, 8))]     # (ties to even: 9.5 -> 10, 6.5 -> 6)
    assert (out[covered] == orf.BLUE).all() and (out[~covered] == 7).all() and covered.sum() == (2 * 5 + 2 * 2) + 9 - 1      # (the line's (10, 7) lies on the rectangle)
    for x, y in ((4, 4), (6, 5), (8, 6), (10, 6), (14, 9), (12, 9)):
        assert covered[0, y, x], (x, y)
    none, nothing = orf.draw_object_labels(img, boxes, np.array([[0, 1]], np.int32), np.array([[-1, -1]], np.int32))
    assert not nothing.any() and none.tobytes() == img.tobytes()
    nan = boxes.copy()
    nan[0, 2, 0] = np.nan                                                            # NaN -> 0: still well defined
    assert orf.object_primitives(nan, np.array([[0]]), np.array([[2]]))[0][1] == (0, 6, 14, 9)
    far = boxes.copy()
    far[0, 2] = (1e9, -1e9, 2e9, 1e9)                                                # saturated at +-2^20
    (_, rect, line), = orf.object_primitives(far, np.array([[0]]), np.array([[2]]))
    assert rect == (2 ** 20, -2 ** 20, 2 ** 20, 2 ** 20) and line == (4, 4, 2 ** 20, 0)
    drawn, mask = orf.draw_object_labels(img, far, np.array([[0]], np.int32), np.array([[2]], np.int32))
    assert mask[0, 4, 4] and mask[0, 4, 15] and mask.sum() == 12                     # the link line leaves the frame to the right


# ------------------------------------------------------------------------------------------------------------------- layout
COMBOS = [(1, 1, 5, None, {}), (3, 2, 5, (5, 7), dict(labels=True, handed=True)),
          (2, 3, 778, (48, 64), dict(overlay=True, tracked=True, smoothed=True, occluded=True, cloud=7, fit=3)),
          (16, 16, 778, (33, 65), dict(overlay=True, handed=True, tracked=True, occluded=True, rig=True, fit=True))]


@pytest.mark.parametrize("n,k,v,hw,opts", COMBOS)
def test_objects_layout_appends_eight_aligned_parts_and_moves_nothing(n, k, v, hw, opts):
    from hn_amd.live import LiveLayout, LiveObjectsLayout
    plain, held = LiveLayout(n, k, v, hw, **opts), LiveObjectsLayout(n, k, v, hw, **opts)
    assert plain.objects is False and held.objects is True
    assert list(LiveObjectsLayout.__dataclass_fields__) == list(LiveLayout.__dataclass_fields__)
    assert list(inspect.signature(LiveObjectsLayout).parameters) == list(inspect.signature(LiveLayout).parameters)
    for f in LiveLayout.__dataclass_fields__:
        if f != "nbytes":
            assert getattr(plain, f) == getattr(held, f), f
    for name in ("cloud", "cloud_count", "cloud_resid", "fit_mesh", "fit_xyz", "fit_rt", "fit_count", "fit_cost", "fit_trace"):
        assert getattr(plain, name + "_at") == getattr(held, name + "_at"), name
    s = n * k
    sizes = dict(contact=4 * s, object_index=4 * s, object_box=16 * s, object_score=4 * s, object_point=8 * s, object_xyz=12 * s,
                 object_extent=24 * s, object_count=8 * s)
    end = plain.nbytes
    for name in FIELDS:                                     # behind every other part, one after the other, on dwords, to nbytes
        at = getattr(held, name + "_at")
        assert getattr(plain, name + "_at") is None and at == (end + 3) // 4 * 4, name
        end = at + sizes[name]
    assert held.nbytes == end
    buf = torch.arange(held.nbytes, dtype=torch.int64).to(torch.uint8)
    v0, v1 = plain.views(buf[:plain.nbytes]), held.views(buf)
    assert v1._fields == v0._fields + FIELDS and type(v1).__name__.endswith("ObjectsViews")
    for name in v0._fields:
        a, b = getattr(v0, name), getattr(v1, name)
        assert (a is None and b is None) or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype), name
    for name, dtype, shape in (("contact", torch.int32, (s,)), ("object_box", torch.float32, (s, 4)), ("object_extent", torch.float32, (s, 6)),
                               ("object_count", torch.int32, (s, 2))):
        t = getattr(v1, name)
        assert t.dtype == dtype and tuple(t.shape) == shape and t.data_ptr() == buf.data_ptr() + getattr(held, name + "_at")
    with pytest.raises(ValueError, match="K-hand step"):
        LiveObjectsLayout(2, None, 778)


def test_read_appends_the_eight_fields():
    from hn_amd.live import LiveHandsOutput, LiveLayout, LiveObjectsLayout
    n, k, v, hw = 2, 3, 5, (5, 7)
    for opts in ({}, dict(overlay=True, labels=True, occluded=True, cloud=4, fit=2)):
        plain, held = LiveLayout(n, k, v, hw, **opts), LiveObjectsLayout(n, k, v, hw, **opts)
        host = torch.from_numpy(np.random.default_rng(3).integers(0, 256, held.nbytes).astype(np.uint8))
        r = LiveHandsOutput(None, None, None, None, None, host, n, k, layout=held).read()
        p = LiveHandsOutput(None, None, None, None, None, host[:plain.nbytes], n, k, layout=plain).read()
        assert type(r).__name__ == type(p).__name__[:-len("Read")] + "ObjectsRead" and r._fields == p._fields + FIELDS
        for name in p._fields:
            a, b = getattr(p, name), getattr(r, name)
            assert (a == b) if not torch.is_tensor(a) else a.numpy().tobytes() == b.numpy().tobytes(), name
        views = held.views(host)
        for name, tail in zip(FIELDS, ((), (), (4,), (), (2,), (3,), (6,), (2,))):
            t = getattr(r, name)
            assert tuple(t.shape) == (n, k) + tail and t.numpy().tobytes() == getattr(views, name).numpy().tobytes(), name
        assert (r.overlay is None) == (not opts) and (r.box_label is None) == (not opts)


# ----------------------------------------------------------------------------------------------------------------- surfaces
def test_the_surfaces():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import live, ops
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandEngine, LiveHandsEngine, LiveHandsOutput
    from hn_amd.pipeline import HandNetEngine, HandsOutput
    assert (ops.OBJECT_BAND, ops.OBJECT_STRIDE, ops.OBJECT_MIN_POINTS) == (0.15, 2, 50) == (orf.OBJECT_BAND, orf.OBJECT_STRIDE, orf.OBJECT_MIN_POINTS)
    assert ops.OBJECT_FIELDS == FIELDS == orf.FIELDS == live.OBJECT_FIELDS == tuple(ops.HandObjects.__dataclass_fields__)
    sig = inspect.signature(ops.hand_objects).parameters
    assert list(sig) == ["det", "contacts", "dxdymags", "det_index", "depth", "xyz_mm", "paras", "k", "object_label", "band", "stride",
                         "min_points", "silhouette", "scratch", "out"]
    for name, default in (("object_label", 1), ("band", 0.15), ("stride", 2), ("min_points", 50), ("silhouette", None), ("scratch", None),
                          ("out", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    assert list(inspect.signature(ops.check_objects).parameters) == ["band", "stride", "min_points"]
    gather = inspect.signature(ops.fcos_ext_gather).parameters
    assert list(gather) == ["ext", "det", "cand", "out"] and gather["out"].kind is inspect.Parameter.KEYWORD_ONLY and gather["out"].default is None
    assert inspect.signature(FCOSEngine.detect_ext).parameters["zero"].default is True
    assert inspect.signature(HandNetEngine.forward_hands).parameters["objects"].default is False
    for fn in (HandNet.live_hands, LiveHandsEngine.__init__):
        d = {k: p.default for k, p in inspect.signature(fn).parameters.items()}
        assert (d["objects"], d["object_band"], d["object_stride"], d["object_min_points"]) == (False, 0.15, 2, 50), fn.__qualname__
    for fn in (HandNet.live, LiveHandEngine.__init__, HandNet.__init__):
        assert not any(p.startswith("object") for p in inspect.signature(fn).parameters), fn.__qualname__
    for doc in (ops.hand_objects.__doc__, ops.check_objects.__doc__, LiveHandsEngine.__init__.__doc__, HandNet.live_hands.__doc__):
        assert "NOT tuned on any model" in " ".join(doc.split()) and "starting values" in doc, doc[:40]
    for doc in (ops.hand_objects.__doc__, LiveHandsEngine.__init__.__doc__, HandNet.live_hands.__doc__):
        assert "100DOH's numbering" in " ".join(doc.split()) and "voc_eval.py:687-699" in doc
    assert "round trip" in ops.hand_objects.__doc__ and "left out on purpose" in " ".join(ops.hand_objects.__doc__.split())
    names = list(LiveHandsOutput.__dataclass_fields__)
    at = names.index("contact")
    assert tuple(names[at:at + 8]) == FIELDS and names[at - 1] == "fit_trace"
    names = list(HandsOutput.__dataclass_fields__)
    assert names[names.index("contacts"):][:2] == ["contacts", "dxdymags"]


def test_the_entries_are_declared_exported_and_bound():
    from hn_amd import _lib, build
    build.build_library()
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    for name, result, count in (("hn_hand_objects_f32", "int", 34), ("hn_hand_objects_scratch_bytes", "int64_t", 3),
                                ("hn_draw_object_labels_u8", "int", 10)):
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
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["hand_object.hip"]
    rows = (build.CSRC / "build" / "hand_object.resources.txt").read_text().splitlines()
    assert len(rows) == 4 and all(" vgpr_spill 0 " in r and r.endswith("sgpr_spill 0") and " scratch 0 " in r for r in rows)
    assert sum("hand_object_" in r for r in rows) == 3 and sum("object_label_kernel" in r for r in rows) == 1


def test_the_scratch_size():
    from hn_amd import _lib
    lib = _lib.load()
    size = lambda n, k, strips: n * k * strips * 64 + n * k * 32      # noqa: E731  a 64-byte partial per strip, a 32-byte record per slot
    assert lib.hn_hand_objects_scratch_bytes(1, 1, 1) == size(1, 1, 4) and lib.hn_hand_objects_scratch_bytes(1, 2, 480) == size(1, 2, 240)
    assert lib.hn_hand_objects_scratch_bytes(3, 3, 2050) == size(3, 3, 684) and lib.hn_hand_objects_scratch_bytes(2, 16, 16384) == size(2, 16, 1024)
    for bad in ((0, 1, 5), (1, 0, 5), (1, 17, 5), (1, 1, 0), (1, 1, 16385), (-1, 1, 5)):
        assert lib.hn_hand_objects_scratch_bytes(*bad) == 0, bad


def test_the_entries_check_their_arguments_before_any_launch():
    """no GPU here: every refusal comes back as HN_ERR_ARG with a message under the entry's name, before the device is touched"""
    from hn_amd import _lib
    lib = _lib.load()
    P = 4096        # stands for a device address
    host4 = (C.c_float * 4)(600.0, 600.0, 320.0, 240.0)
    nan, inf = float("nan"), float("inf")
    inputs = ("boxes", "scores", "labels", "count", "contacts", "dxdymags", "det_index", "depth", "xyz")
    outputs = ("out_contact", "out_index", "out_box", "out_score", "out_point", "out_xyz", "out_extent", "out_count")

    def call(n=2, k=2, h=48, w=64, cap=40, label=1, joints=21, stride=2, band=0.15, min_points=50, frame_stride=None, scratch_bytes=None,
             paras=host4, cams=None, **ptrs):
        p = dict({name: P for name in inputs + outputs + ("scratch",)}, sil=None)
        p.update(ptrs)
        need = lib.hn_hand_objects_scratch_bytes(n, k, h) if scratch_bytes is None else scratch_bytes
        return lib.hn_hand_objects_f32(*(p[name] for name in inputs[:7]), cap, label, p["depth"], h * w if frame_stride is None else frame_stride,
                                       p["sil"], p["xyz"], joints, paras, cams, n, k, h, w, stride, band, min_points, p["scratch"], need,
                                       *(p[name] for name in outputs), None)
    refusals = [(dict([(name, None)]), b"null pointer") for name in inputs + outputs + ("scratch",)]
    refusals += [(dict(cams=P), b"exactly one of paras"), (dict(paras=None), b"exactly one of paras"),
                 (dict(paras=None, cams=P + 2), b"cams must be aligned"),
                 (dict(n=0), b"n = 0"), (dict(n=65536), b"n = 65536"), (dict(k=0), b"k = 0"), (dict(k=17), b"k = 17"), (dict(k=-1), b"k = -1"),
                 (dict(h=0), b"frame size"), (dict(w=0), b"frame size"), (dict(h=16385), b"frame size"), (dict(w=16385), b"frame size"),
                 (dict(frame_stride=48 * 64 - 1), b"depth_frame_stride"), (dict(frame_stride=0), b"depth_frame_stride"),
                 (dict(cap=0), b"cap = 0"), (dict(cap=-3), b"cap = -3"), (dict(cap=2 ** 24 + 1), b"cap = "),
                 (dict(joints=0), b"joints = 0"), (dict(joints=4097), b"joints = 4097"),
                 (dict(stride=0), b"stride = 0"), (dict(stride=-2), b"stride = -2"),
                 (dict(band=0.0), b"band"), (dict(band=-0.15), b"band"), (dict(band=nan), b"band"), (dict(band=inf), b"band"),
                 (dict(band=100.5), b"band"),
                 (dict(min_points=0), b"min_points = 0"), (dict(min_points=-7), b"min_points = -7"),
                 (dict(scratch_bytes=lib.hn_hand_objects_scratch_bytes(2, 2, 48) - 1), b"scratch of"), (dict(scratch_bytes=0), b"scratch of"),
                 (dict(scratch=P + 4), b"8-byte aligned")]
    refusals += [(dict([(name, P + 2)]), b"aligned to 4 bytes") for name in outputs]
    for kw, word in refusals:
        assert call(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_hand_objects_f32: ") and word in err, (kw, err)

    def draw(n=2, k=2, h=48, w=64, cap=40, **ptrs):
        p = dict(boxes=P, det_index=P, object_index=P, image=P)
        p.update(ptrs)
        return lib.hn_draw_object_labels_u8(p["boxes"], p["det_index"], p["object_index"], cap, n, k, h, w, p["image"], None)
    for kw, word in [(dict([(name, None)]), b"null pointer") for name in ("boxes", "det_index", "object_index", "image")] + [
            (dict(n=0), b"n = 0"), (dict(k=17), b"k = 17"), (dict(k=0), b"k = 0"), (dict(h=0), b"frame size"), (dict(w=16385), b"frame size"),
            (dict(cap=0), b"cap = 0")]:
        assert draw(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_draw_object_labels_u8: ") and word in err, (kw, err)


# ---------------------------------------------------------------------------------------------------------- the Python layer
def test_check_objects():
    from hn_amd import ops
    assert ops.check_objects() == (0.15, 2, 50) and ops.check_objects(100, 1, 1) == (100.0, 1, 1)
    assert ops.check_objects(np.float32(0.5), np.int64(3), np.int32(7)) == (0.5, 3, 7)
    for bad in (0, -1, 2.0, True, "many", None, 2 ** 31):
        with pytest.raises(ValueError, match="object_stride"):
            ops.check_objects(stride=bad)
        with pytest.raises(ValueError, match="object_min_points"):
            ops.check_objects(min_points=bad)
    for bad in (0, -0.15, float("nan"), float("inf"), -float("inf"), 100.0001, 1e39, 1e-50, "wide", None, True):
        with pytest.raises(ValueError, match="object_band"):
            ops.check_objects(band=bad)


class _Fcos:
    def __init__(self, ext):
        self.ext = ext


class _Hand:
    device = "cpu"

    def __init__(self, ext=True):
        self.fcos = _Fcos(ext)

    def set_convert(self, **kw):
        pass


class _Graph:
    v = 1280


class _Lifter:
    device = "cpu"
    graphs = [_Graph()]


def test_the_engines_refuse_what_the_objects_cannot_do():
    """before anything touches a device"""
    from hn_amd.live import LiveHandEngine, LiveHandsEngine, LiveLayout, LiveObjectsLayout
    from hn_amd.pipeline import HandNetEngine
    paras, perm = (600.0, 600.0, 320.0, 240.0), np.arange(778)
    hands = lambda *a, ext=True, paras=paras, **kw: LiveHandsEngine(_Hand(ext), _Lifter(), paras, 2, True, *a, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="ext heads"):
        hands(perm, objects=True, ext=False)
    with pytest.raises(ValueError, match="objects=True needs paras="):
        hands(perm, objects=True, paras=None)
    for kw, word in ((dict(object_band=0), "object_band"), (dict(object_band=float("inf")), "object_band"), (dict(object_band=101), "object_band"),
                     (dict(object_stride=0), "object_stride"), (dict(object_stride=1.5), "object_stride"),
                     (dict(object_min_points=0), "object_min_points")):
        with pytest.raises(ValueError, match=word):
            hands(perm, objects=True, **kw)
    with pytest.raises(TypeError):
        LiveHandEngine(_Hand(), _Lifter(), paras, True, perm, objects=True)
    plain = hands(perm, ext=False, object_band=0)          # (the option off: its parameters are not looked at, nor the detector's heads)
    assert plain.objects is None and plain._key_options() == () and type(plain._layout(2, (5, 7))) is LiveLayout
    held = hands(perm, objects=True, object_band=0.2, object_stride=3, object_min_points=9)
    assert held.objects == (0.2, 3, 9) and held._key_options() == ("objects", 0.2, 3, 9)
    lay = held._layout(2, None)
    assert type(lay) is LiveObjectsLayout and lay.objects and lay.object_count_at is not None
    eng = HandNetEngine.__new__(HandNetEngine)
    eng.fcos = _Fcos(False)
    with pytest.raises(RuntimeError, match="ext heads"):
        HandNetEngine.forward_hands.__wrapped__(eng, None, None, 2, objects=True)


def test_live_hands_names_the_fix_for_a_detector_without_contact_heads():
    from handnet_pipeline.handnet_pipeline import HandNet
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    assert net.detector.ext is False
    with pytest.raises(ValueError, match=r"assign a FCOS\(num_classes=\.\.\., ext=True, nms_thresh=0\.5\) to net\.detector and load"):
        net.live_hands(None, (600.0, 600.0, 320.0, 240.0), objects=True)
