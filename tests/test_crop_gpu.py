"""hand_slots_kernel<SIDED> and hand_crop_gather_kernel<SIDED> behind every entry of the crop stage, the top-1 entry as their
one-slot case (csrc/crop_stage.hip),
convert_one in its three callers and the lifter's standardisation (csrc/a2j_ops.hip) against the rules of tests/crop_ref.py on the
cases of tests/crop_cases.py.  Boxes, flags, indices, crops and the fp32 conversion are compared bit for bit, no case excluded;
the only tolerances are crop_ref's two derived bounds (conversion and standardisation against float64), whose worst ratios are
printed.  Every output is filled with a sentinel first: an element the kernel does not write fails the comparison.  DESIGN.md
section 5, "The crop stage", holds what the MI355X returned."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import crop_cases as cc
import crop_ref as cr

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL_F, SENTINEL_I = -77.25, -7
FIELDS = ("crop_box", "has_hand", "score", "det_index")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _det(boxes, labels, scores, sides, counts):
    """[n, cap, 4] boxes, [n, cap] labels / scores / sides, [n] counts -> ops.Detections"""
    from hn_amd import ops
    n, cap = labels.shape
    det = ops.alloc_detections(n, cap, "cuda")
    det.boxes.copy_(_gpu(boxes.astype(F)))
    det.labels.copy_(_gpu(labels.astype(np.int32)))
    det.scores.copy_(_gpu(scores.astype(F)))
    det.sides.copy_(_gpu(sides.astype(np.int32)))
    det.count.copy_(_gpu(np.asarray(counts, np.int32)))
    return det


def _pack(boxes, k):
    """a flat list of boxes, k per frame, every row a hand -> (boxes [n, k, 4], labels, scores, sides, counts); the rows that pad
    the last frame lie beyond its count"""
    b = len(boxes)
    n = -(-b // k)
    full = np.zeros((n * k, 4), F)
    full[:b] = boxes
    labels = np.full((n, k), cc.HAND, np.int32)
    scores = (F(0.999) - F(1e-6) * np.arange(n * k, dtype=F)).reshape(n, k)
    sides = (np.arange(n * k) % 3 % 2).astype(np.int32).reshape(n, k)          # 0, 1, 0, 0, 1, 0, ...: left hands mixed in
    counts = np.full(n, k, np.int32)
    counts[-1] = b - (n - 1) * k
    return full.reshape(n, k, 4), labels, scores, sides, counts


def _outputs(n, k, out, cpad, handed):
    dev = "cuda"
    o = dict(crop_box=torch.full((n, k, 4), SENTINEL_I, device=dev, dtype=torch.int64),
             has_hand=torch.full((n, k), SENTINEL_I, device=dev, dtype=torch.int32),
             score=torch.full((n, k), SENTINEL_F, device=dev, dtype=torch.float32),
             det_index=torch.full((n, k), SENTINEL_I, device=dev, dtype=torch.int32),
             crops=torch.full((n * k, out, out, cpad), SENTINEL_F, device=dev, dtype=torch.float32))
    if handed:
        o["side"] = torch.full((n, k), SENTINEL_I, device=dev, dtype=torch.int32)
        o["mirror"] = torch.full((n, k), SENTINEL_I, device=dev, dtype=torch.int32)
    return o


def _keep_their_fill(o):
    torch.cuda.synchronize()
    for name, t in o.items():
        assert bool((t == (SENTINEL_F if t.is_floating_point() else SENTINEL_I)).all()), name


def _hands(det, depth, k, out, cpad=4, reorder=False, handed=False, left_side=0, in_ch=None):
    """ops.crop_resize_hands into sentinel-filled outputs -> numpy arrays.  in_ch: the C entry with the first in_ch channels of a
    [n, in_ch, h, w] image (ops takes 1 or 4 channels only)"""
    from hn_amd import ops
    n, c, h, w = depth.shape
    o = _outputs(n, k, out, cpad, handed)
    if in_ch is None:
        got = ops.crop_resize_hands(det, cc.HAND, depth, k, out_size=out, cpad=cpad, reorder_bgr=reorder, handed=handed,
                                    left_side=left_side, **o)
        assert all(g is o[name] for g, name in zip(got, ("crop_box", "has_hand", "score", "det_index", "crops", "side", "mirror")))
    else:
        assert not handed and c == in_ch
        p = ops.ptr
        ops.check(ops._lib.load().hn_crop_resize_hands(
            p(det.boxes), p(det.scores), p(det.labels), p(det.count), det.scores.shape[1], cc.HAND, k, p(depth), n, in_ch,
            1 if reorder else 0, h, w, out, cpad, p(o["crop_box"]), p(o["has_hand"]), p(o["score"]), p(o["det_index"]),
            p(o["crops"]), ops._stream()), "hn_crop_resize_hands")
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in o.items()}


def _want_slots(boxes, labels, scores, sides, counts, k, w, h, handed, left_side=0):
    n, cap = labels.shape
    per = [cr.slots(boxes[i], labels[i], scores[i], sides[i] if handed else None, counts[i], cap, cc.HAND, k, left_side, w, h)
           for i in range(n)]
    return {f: np.stack([p[f] for p in per]) for f in FIELDS + (("side", "mirror") if handed else ())}


def _want_crops(depth, want, out, cpad, reorder):
    n, k = want["has_hand"].shape
    mirror = want.get("mirror", np.zeros((n, k), np.int32))
    return np.stack([cr.gather(depth[i], want["crop_box"][i, s], want["has_hand"][i, s], mirror[i, s], out, cpad, reorder)
                     for i in range(n) for s in range(k)])


def _same(got, want, fields):
    for f in fields:
        assert got[f].dtype == want[f].dtype and cr.same_bits(got[f], want[f]), f


# --------------------------------------------------------------------------------------------------------------------------
# the box sweep
# --------------------------------------------------------------------------------------------------------------------------
@functools.cache
def _sweep_reference():
    """the sweep, 16 boxes per frame, every row a hand -> (tables, depth [n, 1, h, w], want, want crops at out = 4)"""
    h, w = cc.SWEEP_H, cc.SWEEP_W
    tables = _pack(cc.sweep_boxes(), 16)
    depth = cc.position_depth(1, h, w, n=len(tables[0]))
    want = _want_slots(*tables, 16, w, h, True)
    return tables, depth, want, _want_crops(depth, want, 4, 4, False)


@pytest.mark.parametrize("handed", [False, True], ids=["plain", "sided"])
def test_box_sweep_in_sixteen_slots(handed):
    """every box of the sweep as a slot of crop_resize_hands(out_size=4): box, flag, score, index (side, mirror) and the crop"""
    tables, depth, want, crops = _sweep_reference()
    got = _hands(_det(*tables), _gpu(depth), 16, 4, handed=handed)
    _same(got, want, FIELDS + (("side", "mirror") if handed else ()))
    plain = crops if handed else _want_crops(depth, {**want, "mirror": np.zeros_like(want["mirror"])}, 4, 4, False)
    assert cr.same_bits(got["crops"], plain)
    filled = want["has_hand"].astype(bool)
    assert filled.sum() > 1000 and (~filled).sum() > 1000
    # [0, 0, 0, 0] with a hand stays apart from `no hand`: its crop is the origin's pixel, not zeros
    origin = filled & ~want["crop_box"].any(axis=-1)
    assert origin.any() and (got["crops"].reshape(filled.shape + (4, 4, 4))[origin][..., 0] > 0).all()


def test_box_sweep_top1_and_one_slot():
    """one box per frame: ops.crop_resize and crop_resize_hands(max_hands=1) give the rule, and so each other"""
    from hn_amd import ops
    h, w = cc.SWEEP_H, cc.SWEEP_W
    boxes = cc.sweep_boxes()
    n = len(boxes)
    _, _, want16, crops16 = _sweep_reference()
    want = {f: want16[f].reshape((-1,) + want16[f].shape[2:])[:n, None] for f in FIELDS}       # the same boxes, one per frame
    want["det_index"] = np.where(want["has_hand"] == 1, 0, -1).astype(np.int32)
    tables = _pack(boxes, 1)
    det = _det(*tables)
    want["score"] = np.where(want["has_hand"] == 1, tables[2], 0).astype(F)
    depth1 = cc.position_depth(1, h, w)
    depth = _gpu(depth1)[None].expand(n, 1, h, w).contiguous()
    crops = np.stack([cr.gather(depth1, want["crop_box"][i, 0], want["has_hand"][i, 0], 0, 4, 4, False) for i in range(n)])
    one = _hands(det, depth, 1, 4)
    _same(one, want, FIELDS)
    assert cr.same_bits(one["crops"], crops)
    o = _outputs(n, 1, 4, 4, False)
    box, has, top = ops.crop_resize(det, cc.HAND, depth, 4, 4, crop_box=o["crop_box"].view(n, 4), has_hand=o["has_hand"].view(n),
                                    crops=o["crops"])
    torch.cuda.synchronize()
    assert cr.same_bits(box.cpu().numpy(), want["crop_box"][:, 0]) and cr.same_bits(has.cpu().numpy(), want["has_hand"][:, 0])
    assert cr.same_bits(top.cpu().numpy(), crops)


CANARY = 0x5A5A5A5A


@functools.cache
def _three_frames():
    """the top-1 entry's three answers on the sweep's frame at out = 4: frame 0 a hand behind a row of another label, frame 1
    none below its count, frame 2 a first hand whose padded slice is empty (the hand behind it must not take the slot) ->
    (tables, depth [3, 1, h, w], the rule's one slot per frame, its crops)"""
    h, w = cc.SWEEP_H, cc.SWEEP_W
    boxes = np.array([[(1.0, 2.0, 9.0, 8.0), (10.5, 5.25, 30.75, 20.5), (0.0, 0.0, 5.0, 5.0)],
                      [(3.0, 3.0, 12.0, 12.0), (4.0, 4.0, 20.0, 20.0), (10.5, 5.25, 30.75, 20.5)],
                      [cc.OUTSIDE["below"], (10.5, 5.25, 30.75, 20.5), (1.0, 1.0, 6.0, 6.0)]], F)
    labels = np.array([[1, cc.HAND, cc.HAND], [1, 1, cc.HAND], [cc.HAND, cc.HAND, 1]], np.int32)
    tables = (boxes, labels, _pack(boxes.reshape(-1, 4), 3)[2], np.zeros((3, 3), np.int32), np.array([3, 2, 3], np.int32))
    depth = cc.position_depth(1, h, w, n=3)
    want = _want_slots(*tables, 1, w, h, False)
    assert want["has_hand"][:, 0].tolist() == [1, 0, 0] and want["det_index"][:, 0].tolist() == [1, -1, -1]
    return tables, depth, want, _want_crops(depth, want, 4, 4, False)


def test_top1_entry_takes_a_crop_box_that_is_only_8_byte_aligned():
    """hn_crop_resize writes the C caller's own int64 array: crop_box at an address that is 8 mod 16 inside a canary-filled buffer.
    Boxes, flags and crops are the rule's, and no word around them is written."""
    from hn_amd import ops
    tables, depth, want, crops = _three_frames()
    det, n, (h, w) = _det(*tables), 3, depth.shape[2:]
    spans = dict(crop_box=(6, 6 + n * 8), has_hand=(32, 32 + n), crops=(40, 40 + n * 4 * 4 * 4))      # int32 words
    buf = torch.full((spans["crops"][1] + 4,), CANARY, dtype=torch.int32, device="cuda")
    cut = {name: buf[a:b] for name, (a, b) in spans.items()}
    box, has, out = cut["crop_box"].view(torch.int64).view(n, 4), cut["has_hand"], cut["crops"].view(torch.float32).view(n, 4, 4, 4)
    assert box.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 0
    p = ops.ptr
    ops.check(ops._lib.load().hn_crop_resize(p(det.boxes), p(det.labels), p(det.count), 3, cc.HAND, p(_gpu(depth)), n, 1, 0, h, w,
                                             4, 4, p(box), p(has), p(out), ops._stream()), "hn_crop_resize")
    torch.cuda.synchronize()
    outside = torch.ones(buf.shape, dtype=torch.bool)
    for a, b in spans.values():
        outside[a:b] = False
    assert bool((buf.cpu()[outside] == CANARY).all()), "a word outside the outputs was written"
    assert cr.same_bits(box.cpu().numpy(), want["crop_box"][:, 0]) and cr.same_bits(has.cpu().numpy(), want["has_hand"][:, 0])
    assert cr.same_bits(out.cpu().numpy(), crops)


def test_top1_entry_is_the_one_slot_entry():
    """the same three frames through hn_crop_resize_hands(max_hands = 1) and through hn_crop_resize: the rule's boxes, flags and
    crops from both, byte for byte; the scores and ranks, which only the first hands out, are the rule's too"""
    from hn_amd import ops
    tables, depth, want, crops = _three_frames()
    det = _det(*tables)
    one = _hands(det, _gpu(depth), 1, 4)
    _same(one, want, FIELDS)
    assert cr.same_bits(one["crops"], crops)
    o = _outputs(3, 1, 4, 4, False)
    box, has, top = ops.crop_resize(det, cc.HAND, _gpu(depth), 4, 4, crop_box=o["crop_box"].view(3, 4), has_hand=o["has_hand"].view(3),
                                    crops=o["crops"])
    torch.cuda.synchronize()
    assert box.cpu().numpy().tobytes() == one["crop_box"].tobytes() and has.cpu().numpy().tobytes() == one["has_hand"].tobytes()
    assert top.cpu().numpy().tobytes() == one["crops"].tobytes()
    _keep_their_fill({f: o[f] for f in ("score", "det_index")})        # (the top-1 entry has no such outputs)


# --------------------------------------------------------------------------------------------------------------------------
# the resize sweep
# --------------------------------------------------------------------------------------------------------------------------
def _resize_run(h, w, boxes, out, in_ch, cpad, reorder, k=16):
    """the boxes, k per frame, plain and (for images ops takes) sided: crops are gather's; a mirrored slot is the plain slot flipped"""
    tables = _pack(boxes, k)
    n = len(tables[0])
    depth = cc.position_depth(in_ch, h, w, n=n)
    det = _det(*tables)
    want = _want_slots(*tables, k, w, h, True)
    assert want["has_hand"].sum() == len(boxes) and want["mirror"].sum() > 0
    plain_want = _want_crops(depth, {**want, "mirror": np.zeros_like(want["mirror"])}, out, cpad, reorder)
    plain = _hands(det, _gpu(depth), k, out, cpad, reorder, in_ch=in_ch if in_ch == 3 else None)
    _same(plain, want, FIELDS)
    assert cr.same_bits(plain["crops"], plain_want)
    assert not plain["crops"][..., in_ch:].any()                                   # the padding channels
    if in_ch == 3:
        return
    sided = _hands(det, _gpu(depth), k, out, cpad, reorder, handed=True)
    _same(sided, want, FIELDS + ("side", "mirror"))
    assert cr.same_bits(sided["crops"], _want_crops(depth, want, out, cpad, reorder))
    m = want["mirror"].reshape(-1).astype(bool)
    assert cr.same_bits(sided["crops"][m], plain["crops"][m][:, :, ::-1]) and cr.same_bits(sided["crops"][~m], plain["crops"][~m])


def test_resize_sweep_every_crop_size_at_176():
    """every crop width 1 .. 300 and height 1 .. 200 (88, 176, 177 and the full frame among them) at out = 176"""
    _resize_run(cc.RESIZE_H, cc.RESIZE_W, cc.resize_boxes(cc.RESIZE_H, cc.RESIZE_W), 176, 1, 4, False)


@pytest.mark.parametrize("out", [7, 32])
@pytest.mark.parametrize("in_ch,cpad,reorder", cc.CHANNELS)
def test_resize_sweep_small_outputs_and_channels(out, in_ch, cpad, reorder):
    _resize_run(cc.SMALL_H, cc.SMALL_W, cc.resize_boxes(cc.SMALL_H, cc.SMALL_W), out, in_ch, cpad, reorder)


@pytest.mark.parametrize("hw", list(cc.TINY_FRAMES))
def test_resize_on_tiny_frames(hw):
    """frames smaller than the output: one pixel, one row, one column, 5 x 7"""
    _resize_run(hw[0], hw[1], np.asarray(cc.TINY_FRAMES[hw], F), 176, 1, 4, False, k=4)


@pytest.mark.parametrize("in_ch,cpad,reorder", cc.CHANNELS[:3])
def test_resize_top1(in_ch, cpad, reorder):
    """ops.crop_resize: one crop per frame over the small frame's sizes at out = 32, and the 176 sweep's shortcut sizes"""
    from hn_amd import ops
    for h, w, out, boxes in ((cc.SMALL_H, cc.SMALL_W, 32, cc.resize_boxes(cc.SMALL_H, cc.SMALL_W)),
                             (cc.RESIZE_H, cc.RESIZE_W, 176, cc.resize_boxes(cc.RESIZE_H, cc.RESIZE_W)[[0, 87, 175, 176, 299, 300]])):
        tables = _pack(boxes, 1)
        n = len(boxes)
        depth = cc.position_depth(in_ch, h, w, n=n)
        want, ok = cr.pad_boxes(boxes, w, h)
        o = _outputs(n, 1, out, cpad, False)
        box, has, crops = ops.crop_resize(_det(*tables), cc.HAND, _gpu(depth), out, cpad, crop_box=o["crop_box"].view(n, 4),
                                          has_hand=o["has_hand"].view(n), crops=o["crops"], reorder_bgr=reorder)
        torch.cuda.synchronize()
        assert ok.all() and cr.same_bits(box.cpu().numpy(), want) and (has.cpu().numpy() == 1).all()
        assert cr.same_bits(crops.cpu().numpy(), np.stack([cr.gather(depth[i], want[i], 1, 0, out, cpad, reorder) for i in range(n)]))


# --------------------------------------------------------------------------------------------------------------------------
# the slot walk and the second lap
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left_side", [None, 0, 1], ids=["plain", "left0", "left1"])
@pytest.mark.parametrize("k", cc.SLOT_KS)
def test_slot_walk(k, left_side):
    names, boxes, labels, scores, sides, counts = cc.slot_frames(k)
    h, w = cc.SWEEP_H, cc.SWEEP_W
    handed = left_side is not None
    depth = cc.position_depth(1, h, w, n=len(names))
    want = _want_slots(boxes, labels, scores, sides, counts, k, w, h, handed, left_side or 0)
    got = _hands(_det(boxes, labels, scores, sides, counts), _gpu(depth), k, 4, handed=handed, left_side=left_side or 0)
    for i, name in enumerate(names):
        for f in want:
            assert cr.same_bits(got[f][i], want[f][i]), (name, f, got[f][i], want[f][i])
    assert cr.same_bits(got["crops"], _want_crops(depth, want, 4, 4, False))


def test_gather_second_lap():
    """80 crops of 176 x 176: the grid-stride loop's second lap starts inside crop 67; the last slot is the frame's last pixel"""
    boxes = cc.lap_boxes()
    n, k = boxes.shape[:2]
    tables = (boxes, np.full((n, k), cc.HAND, np.int32), _pack(boxes.reshape(-1, 4), k)[2], np.zeros((n, k), np.int32), np.full(n, k))
    depth = cc.position_depth(1, cc.LAP_H, cc.LAP_W, n=n)
    want = _want_slots(*tables, k, cc.LAP_W, cc.LAP_H, False)
    got = _hands(_det(*tables), _gpu(depth), k, cc.LAP_OUT)
    _same(got, want, FIELDS)
    crops = _want_crops(depth, want, cc.LAP_OUT, 4, False)
    assert want["has_hand"].all() and cr.same_bits(got["crops"], crops)
    assert (crops[-1, ..., 0] == depth[-1, 0, -1, -1]).all()


# --------------------------------------------------------------------------------------------------------------------------
# the joint conversion
# --------------------------------------------------------------------------------------------------------------------------
def _paras_arg(paras):
    return (C.c_float * 4)(*[float(v) for v in paras]) if paras is not None else None


def _convert_joints(kp, box, valid, paras, cw, ch):
    """ops.convert_joints for a square crop, the C entry for crop_w != crop_h; into a sentinel-filled output"""
    from hn_amd import ops
    out = torch.full_like(kp, SENTINEL_F)
    if cw == ch:
        assert ops.convert_joints(kp, box, valid=valid, paras=paras, crop=cw, out=out) is out
    else:
        n, j, _ = kp.shape
        ops.check(ops._lib.load().hn_convert_joints_f32(ops.ptr(kp), ops.ptr(box), ops.ptr(valid), n, j, float(cw), float(ch),
                                                        _paras_arg(paras), ops.ptr(out), ops._stream()), "hn_convert_joints_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _convert_samples(kp, box_f32, sample_paras, valid, cw, ch):
    from hn_amd import ops
    if cw == ch:
        img, xyz = ops.convert_joints_samples(kp, box_f32, sample_paras, valid=valid, crop=cw)
    else:
        n, j, _ = kp.shape
        img, xyz = torch.full_like(kp, SENTINEL_F), torch.full_like(kp, SENTINEL_F)
        ops.check(ops._lib.load().hn_convert_joints_samples_f32(ops.ptr(kp), ops.ptr(box_f32), ops.ptr(sample_paras), ops.ptr(valid),
                                                                n, j, float(cw), float(ch), ops.ptr(img), ops.ptr(xyz),
                                                                ops._stream()), "hn_convert_joints_samples_f32")
    torch.cuda.synchronize()
    return img.cpu().numpy(), xyz.cpu().numpy()


def _check_converted(got, args, kw, worst):
    """got = (image uvd or None, xyz or None) against convert32 bit for bit and convert64 within the bound"""
    want32, want64, bound = cr.convert32(*args, **kw), cr.convert64(*args, **kw), cr.convert_bound(*args, **kw)
    for g, w32, w64, b in zip(got, want32, want64, bound):
        if g is None:
            continue
        assert cr.same_bits(g, w32)
        worst.append(cr.bound_ratio(g, w64, b))
        if kw.get("valid") is not None:
            assert not g[kw["valid"] == 0].any()


@pytest.mark.parametrize("name", [c[0] for c in cc.CONVERT_CASES])
def test_convert_joints_is_convert32(name):
    """ops.convert_joints (image uvd; camera xyz) and ops.convert_joints_samples, with and without valid"""
    _, j, n, cw, ch = cc.CONVERT_BY_NAME[name]
    d = cc.convert_inputs(name)
    kp, box, box_f32, sparas = _gpu(d["kp"]), _gpu(d["box"]), _gpu(d["box_f32"]), _gpu(d["sample_paras"])
    worst = []
    for valid in (d["valid"], None):
        tv = _gpu(valid) if valid is not None else None
        _check_converted((_convert_joints(kp, box, tv, None, cw, ch), None), (d["kp"], d["box"], None, cw, ch), dict(valid=valid), worst)
        _check_converted((None, _convert_joints(kp, box, tv, cc.PARAS, cw, ch)), (d["kp"], d["box"], cc.PARAS, cw, ch),
                         dict(valid=valid), worst)
        _check_converted(_convert_samples(kp, box_f32, sparas, tv, cw, ch), (d["kp"], d["box_f32"], d["sample_paras"], cw, ch),
                         dict(valid=valid), worst)
    print(f"crop gpu convert {name}: max |kernel - convert64| / bound = {max(worst):.4f}")
    assert 0.0 < max(worst) <= 1.0


AGG_CASES = (("J1", 1, 7, 176, 176), ("J21", 21, 13, 176, 176), ("J21-rect", 21, 13, 176, 96), ("J64", 64, 5, 176, 176),
             ("J64-rect", 64, 5, 176, 96))


@functools.cache
def _heads(j, k):
    """2 x 2 cells; the offsets of crop 0 lie around -250 px and those of crop 3 around +250 px, so its joints fall below 0 and
    beyond the crop; one NaN depth, one NaN offset"""
    rng = np.random.default_rng(7 * j + k)
    cls = rng.normal(0, 2, (k, 2, 2, 16 * j)).astype(F)
    reg = rng.uniform(-40, 40, (k, 2, 2, 32 * j)).astype(F)
    reg[0] -= 250
    reg[3] += 250
    dep = rng.uniform(0.0, 1.5, (k, 2, 2, 16 * j)).astype(F)
    dep[0, 0, 0, :j] = 0.0
    dep[1, 1, 0, j - 1] = np.nan
    reg[1, 0, 1, 0] = np.nan
    return cls, reg, dep


def _aggregate(cls, reg, dep, valid, j, box, cw, ch, paras, clamp_kp, clamp_box, sbox, sparas, mirror):
    """ops.a2j_aggregate(convert=...) for a square crop, the C entries for crop_w != crop_h -> (crop uvd, image uvd, xyz or None)"""
    from hn_amd import ops
    k = cls.shape[0]
    img = torch.full((k, j, 3), SENTINEL_F, device="cuda")
    xyz = torch.full((k, j, 3), SENTINEL_F, device="cuda") if paras is not None or sparas is not None else None
    out = torch.full((k, j, 3), SENTINEL_F, device="cuda")
    if cw == ch:
        conv = dict(paras=paras, crop=cw, clamp_keypoints=clamp_kp, clamp_box=clamp_box, image_uvd=img, xyz_mm=xyz, mirror=mirror)
        conv.update(dict(sample_box=sbox, sample_paras=sparas) if sbox is not None else dict(crop_box=box))
        got = ops.a2j_aggregate(cls, reg, dep, joints=j, stride=16, valid=valid, out=out, convert=conv)
        assert got[0] is out and got[1] is img and got[2] is xyz
    else:
        p, lib = ops.ptr, ops._lib.load()
        opts = ops._lib.ConvertOpts(1 if clamp_kp else 0, clamp_box[0] if clamp_box else 0, clamp_box[1] if clamp_box else 0, 0,
                                    p(sbox), p(sparas))
        head = (p(cls), p(reg), p(dep), p(valid))
        tail = (k, 2, 2, j, 16, p(box) if sbox is None else None, float(cw), float(ch), _paras_arg(paras), C.byref(opts), p(out), p(img),
                p(xyz), ops._stream())
        if mirror is not None:
            ops.check(lib.hn_a2j_aggregate_convert_mirror_f32(*head, p(mirror), *tail), "hn_a2j_aggregate_convert_mirror_f32")
        else:
            ops.check(lib.hn_a2j_aggregate_convert_f32(*head, *tail), "hn_a2j_aggregate_convert_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy(), img.cpu().numpy(), xyz.cpu().numpy() if xyz is not None else None


@pytest.mark.parametrize("name", [c[0] for c in AGG_CASES])
def test_fused_epilogue_is_convert32(name):
    """ops.a2j_aggregate(convert=...): image uvd and xyz are convert32 of the crop uvd the same launch returns -- plain, with the
    live caller's clamps (NaN kept), with the dataset's boxes and intrinsics, and mirrored"""
    _, j, k, cw, ch = next(c for c in AGG_CASES if c[0] == name)
    cls, reg, dep = _heads(j, k)
    rng = np.random.default_rng(j)
    valid = np.array([(1, 1, 0, 1, 2, 1)[i % 6] for i in range(k)], np.int32)
    box = cc.CONVERT_BOXES[np.arange(k) % len(cc.CONVERT_BOXES)].copy()
    box_f32 = (box + rng.uniform(-0.5, 0.5, box.shape)).astype(F)
    sparas = (np.asarray(cc.PARAS) * rng.uniform(0.9, 1.1, (k, 4))).astype(F)
    mirror = (np.arange(k) % 2).astype(np.int32)
    tc, tr, td, tv = _gpu(cls), _gpu(reg), _gpu(dep), _gpu(valid)
    frame = (cc.FRAME_H, cc.FRAME_W)
    worst, seen_nan = [], False
    for paras, clamp_kp, clamp_box, sampled, mirrored in ((cc.PARAS, False, None, False, False), (None, False, None, False, False),
                                                          (cc.PARAS, True, frame, False, False), (cc.PARAS, True, None, False, True),
                                                          (None, False, None, True, False), (None, True, frame, True, True)):
        uvd, img, xyz = _aggregate(tc, tr, td, tv, j, _gpu(box), cw, ch, paras, clamp_kp, clamp_box,
                                   _gpu(box_f32) if sampled else None, _gpu(sparas) if sampled else None,
                                   _gpu(mirror) if mirrored else None)
        assert not uvd[valid == 0].any() and np.isnan(uvd[valid == 2]).all() and np.isnan(img[valid == 2]).all()
        assert np.isfinite(uvd[0]).all() and (uvd[..., :2][np.isfinite(uvd[..., :2])] < 0).any() and np.nanmax(uvd[..., :2]) > 176
        args = (uvd, box_f32 if sampled else box, sparas if sampled else paras, cw, ch)
        _check_converted((img, xyz), args, dict(valid=valid, clamp_kp=clamp_kp, clamp_box=clamp_box), worst)
        if clamp_kp:                                        # NaN is preserved under clamp_keypoints, everything else is inside
            assert np.array_equal(np.isnan(img[..., 2]), np.isnan(uvd[..., 2])) and np.isnan(img[1, j - 1, 2])
            assert np.nanmin(img[..., 2]) >= 0 and np.nanmax(img[..., 2]) <= cw
            seen_nan = True
    print(f"crop gpu fused {name}: max |kernel - convert64| / bound = {max(worst):.4f}")
    assert seen_nan and 0.0 < max(worst) <= 1.0


# --------------------------------------------------------------------------------------------------------------------------
# the standardisation
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", cc.STD_JOINTS)
def test_standardisation_and_the_gated_form(j):
    from hn_amd import ops
    uvd, valid = cc.std_inputs(j)
    n = len(uvd)
    tu, tv = _gpu(uvd), _gpu(valid)
    want, bound = cr.standardize64(uvd[..., :2]), cr.standardize_bound(uvd[..., :2])
    gate = cr.gate32(uvd[..., :2])
    rows = dict(zip(cc.STD_ROWS, range(n)))
    for v in (valid, None):
        live = np.ones(n, bool) if v is None else v == 1
        out = torch.full((n, j, 2), SENTINEL_F, device="cuda")
        assert ops.joints2d_standardize(tu, valid=tv if v is not None else None, out=out) is out
        torch.cuda.synchronize()
        std = out.cpu().numpy()
        assert not std[~live].any()
        ratio = cr.bound_ratio(std[live], want[live], bound[live])
        print(f"crop gpu standardize J={j}{'' if v is not None else ' (no valid)'}: max |kernel - float64| / bound = {ratio:.4f}")
        assert ratio <= 1.0 and (ratio > 0.0 or j == 2)
        assert np.isnan(std[rows["same-u"], :, 0]).all() and np.isfinite(std[rows["same-u"], :, 1]).all()
        for mirror in (None, (np.arange(n) % 2).astype(np.int32)):
            gout = torch.full((n, j, 2), SENTINEL_F, device="cuda")
            lifted = torch.full((n,), SENTINEL_I, device="cuda", dtype=torch.int32)
            ops.lifter_input_gated(tu, valid=tv if v is not None else None, out=gout, lifted=lifted,
                                   mirror=_gpu(mirror) if mirror is not None else None)
            torch.cuda.synchronize()
            g, lf = gout.cpu().numpy(), lifted.cpu().numpy()
            assert lf.tolist() == (live & gate).astype(np.int32).tolist()
            accepted = std[live & gate].copy()
            if mirror is not None:
                flip = mirror[live & gate].astype(bool)
                accepted[flip, :, 0] = -accepted[flip, :, 0]
            assert cr.same_bits(g[live & gate], accepted) and not g[~(live & gate)].any()      # bit-identical rows; zeros
    assert (live & gate).sum() >= 2 and not gate[rows["clustered"]]


# --------------------------------------------------------------------------------------------------------------------------
# refusals
# --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    from hn_amd import ops
    h, w = cc.SWEEP_H, cc.SWEEP_W
    tables = _pack(cc.sweep_boxes()[:32], 16)
    det = _det(*tables)
    depth = _gpu(cc.position_depth(1, h, w, n=2))
    for k in (0, 17):                                      # max_hands
        o = _outputs(2, max(k, 1), 4, 4, True)
        with pytest.raises(ValueError, match="max_hands"):
            ops.crop_resize_hands(det, cc.HAND, depth, k, out_size=4, handed=True, **o)
        _keep_their_fill(o)
    o = _outputs(2, 16, 4, 4, False)
    p, lib = ops.ptr, ops._lib.load()

    def direct(k, in_ch, cpad, image):
        return lib.hn_crop_resize_hands(p(det.boxes), p(det.scores), p(det.labels), p(det.count), 16, cc.HAND, k, p(image), 2, in_ch, 0, h,
                                        w, 4, cpad, p(o["crop_box"]), p(o["has_hand"]), p(o["score"]), p(o["det_index"]), p(o["crops"]),
                                        ops._stream())
    five = _gpu(cc.position_depth(5, h, w, n=2))
    assert direct(0, 1, 4, depth) != 0 and direct(17, 1, 4, depth) != 0        # the library refuses them itself
    assert direct(16, 5, 4, five) != 0 and direct(16, 0, 4, depth) != 0          # in_ch = 5
    assert direct(16, 1, 6, depth) != 0 and direct(16, 1, 0, depth) != 0         # a cpad that is no multiple of 4
    with pytest.raises(ValueError, match="depth must be"):
        ops.crop_resize_hands(det, cc.HAND, five, 16, out_size=4, **o)
    with pytest.raises(RuntimeError, match="hn_crop_resize_hands"):
        ops.crop_resize_hands(det, cc.HAND, depth, 16, out_size=4, cpad=6, **o)
    _keep_their_fill(o)
    top = _outputs(2, 1, 4, 4, False)
    args = dict(crop_box=top["crop_box"].view(2, 4), has_hand=top["has_hand"].view(2), crops=top["crops"])
    with pytest.raises(ValueError, match="depth must be"):
        ops.crop_resize(det, cc.HAND, five, 4, 4, **args)
    with pytest.raises(RuntimeError, match="hn_crop_resize"):
        ops.crop_resize(det, cc.HAND, depth, 4, 6, **args)
    _keep_their_fill(top)
    uvd = _gpu(cc.std_inputs(2)[0][:, :1].copy())          # joints = 1: no standard deviation
    out = dict(out=torch.full((len(uvd), 1, 2), SENTINEL_F, device="cuda"))
    with pytest.raises(RuntimeError, match="hn_joints2d_standardize_f32"):
        ops.joints2d_standardize(uvd, out=out["out"])
    out["lifted"] = torch.full((len(uvd),), SENTINEL_I, device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError, match="hn_lifter_input_gated_f32"):
        ops.lifter_input_gated(uvd, **out)
    _keep_their_fill(out)
    got = _hands(det, depth, 16, 4)                        # and the next call is served
    assert (got["has_hand"] != SENTINEL_I).all()
