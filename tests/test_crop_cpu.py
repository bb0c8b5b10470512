"""The crop stage's and the joint conversion's rules (tests/crop_ref.py) without a GPU: the rules against the torch oracle
(oracle/handnet_ref.py: crop_box and crop_depth, which is F.interpolate; oracle/a2j_ref.convert_joints) on every case of
tests/crop_cases.py, the guards of the case tables, the negative-stop decision, the derived bounds around fp32 emulations, and
every mutant of the rules failing on its named case -- so the checks are known to be able to fail."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import crop_cases as cc
import crop_ref as cr

F = np.float32


# --------------------------------------------------------------------------------------------------------------------------
# the rules against the torch oracle
# --------------------------------------------------------------------------------------------------------------------------
def test_pad_box_is_the_oracle_on_every_box():
    """crop_box on every box of the sweep; ok is `crop_depth returns a crop`, and the crop is gather's (4 x 4)"""
    from oracle import handnet_ref
    boxes = cc.sweep_boxes()
    h, w = cc.SWEEP_H, cc.SWEEP_W
    depth = cc.position_depth(1, h, w)
    tdepth = torch.from_numpy(depth)
    got, ok = cr.pad_boxes(boxes, w, h)
    assert len(boxes) >= 82 * 82 and ok.any() and not ok.all()
    diff = 0
    for b, g, k in zip(boxes, got, ok):
        raw = handnet_ref.crop_box(torch.from_numpy(b), w, h)
        crop = handnet_ref.crop_depth(tdepth, raw, size=4)
        want = raw.numpy() if crop is not None else np.zeros(4, np.int64)
        diff += int(not np.array_equal(g, want) or bool(k) != (crop is not None))
        if crop is not None:
            diff += int(not np.array_equal(cr.gather(depth, g, True, False, 4, 4, False)[..., 0], crop[0].numpy()))
    print(f"crop cpu: {len(boxes)} boxes, {int(ok.sum())} with a hand, {diff} differences from the oracle")
    assert diff == 0


@pytest.mark.parametrize("out", [7, 32, 176])
def test_src_index_is_interpolate(out):
    for n_in in range(1, 700):
        want = TF.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), size=(1, out))[0, 0, 0].numpy()
        assert np.array_equal(cr.src_index(np.arange(out), n_in, out), want.astype(np.int64)), n_in


def _gather_vs_oracle(h, w, boxes, out, in_ch, cpad, reorder):
    from oracle import handnet_ref
    depth = cc.position_depth(in_ch, h, w)
    tdepth = torch.from_numpy(depth)
    padded, ok = cr.pad_boxes(boxes, w, h)
    assert ok.all()
    sizes = set()
    for b in padded:
        crop = handnet_ref.crop_depth(tdepth, torch.from_numpy(b), size=out)
        if reorder:
            crop = crop[[2, 1, 0, 3]]
        got = cr.gather(depth, b, True, False, out, cpad, reorder)
        assert np.array_equal(got[..., :in_ch], crop.permute(1, 2, 0).numpy()) and not got[..., in_ch:].any(), b
        assert np.array_equal(cr.gather(depth, b, True, True, out, cpad, reorder), got[:, ::-1]), b
        sizes.add(cr.crop_size(b, w, h))
    return sizes


def test_gather_is_crop_depth_over_every_crop_size():
    h, w = cc.RESIZE_H, cc.RESIZE_W
    sizes = _gather_vs_oracle(h, w, cc.resize_boxes(h, w), 176, 1, 4, False)
    assert {s[0] for s in sizes} == set(range(1, w + 1)) and {s[1] for s in sizes} == set(range(1, h + 1))
    for out in (7, 32):
        sizes = _gather_vs_oracle(cc.SMALL_H, cc.SMALL_W, cc.resize_boxes(cc.SMALL_H, cc.SMALL_W), out, 1, 4, False)
        assert {s[0] for s in sizes} == set(range(1, cc.SMALL_W + 1)) and {s[1] for s in sizes} == set(range(1, cc.SMALL_H + 1))


@pytest.mark.parametrize("in_ch,cpad,reorder", cc.CHANNELS[1:])
def test_gather_channels(in_ch, cpad, reorder):
    h, w = cc.SMALL_H, cc.SMALL_W
    _gather_vs_oracle(h, w, cc.resize_boxes(h, w), 32, in_ch, cpad, reorder)


@pytest.mark.parametrize("hw", list(cc.TINY_FRAMES))
def test_gather_on_tiny_frames(hw):
    sizes = _gather_vs_oracle(hw[0], hw[1], np.asarray(cc.TINY_FRAMES[hw], F), 176, 1, 4, False)
    assert (hw[1], hw[0]) in sizes                          # the whole frame is one of the crops


# --------------------------------------------------------------------------------------------------------------------------
# guards: the tables reach the bounds they claim
# --------------------------------------------------------------------------------------------------------------------------
def test_the_tables_hold_every_bound():
    h, w = cc.RESIZE_H, cc.RESIZE_W
    padded, ok = cr.pad_boxes(cc.resize_boxes(h, w), w, h)
    widths = [cr.crop_size(b, w, h)[0] for b in padded]
    assert ok.all() and {88, 176, 177, w} <= set(widths)              # out == 2 in, in == out, just beyond, the full frame
    assert any(int(b[2]) == w for b in padded) and any(int(b[3]) == h for b in padded)      # the key w + 1: b2 == w
    # the second lap
    total = cc.LAP_N * cc.LAP_K * cc.LAP_OUT ** 2
    assert cc.LAP_N * cc.LAP_K >= 68 and total > cc.GRID_THREADS and cc.GRID_THREADS // cc.LAP_OUT ** 2 == 67
    lap, lok = cr.pad_boxes(cc.lap_boxes(), cc.LAP_W, cc.LAP_H)
    assert lok.all() and lap[-1, -1].tolist() == [cc.LAP_W - 1, cc.LAP_H - 1, cc.LAP_W - 1, cc.LAP_H - 1]
    # the sweep: both axes exhaustive, and a box's two axes hold different pairs
    grid = cc.sweep_boxes()[:82 * 82]
    assert len({(a, c) for a, _, c, _ in grid.tolist()}) == 82 * 82 == len({(b, d) for _, b, _, d in grid.tolist()})
    assert (grid[:, 0] != grid[:, 1]).any() and not np.array_equal(grid[:, [0, 2]], grid[:, [1, 3]])
    assert np.isfinite(cc.sweep_boxes()).all() and np.abs(cc.sweep_boxes()).max() > 2 ** 24
    box, ok = cr.pad_box(cc.ORIGIN_PIXEL, cc.SWEEP_W, cc.SWEEP_H)
    assert ok and not box.any()                                        # [0, 0, 0, 0] WITH a hand


def _raw_pad(box, w, h):
    from oracle import handnet_ref
    return handnet_ref.crop_box(torch.tensor(box, dtype=torch.float32), w, h)


def test_outside_boxes_and_their_stops():
    """each of the four sides is rejected.  A box above or left of the frame has a negative stop, and so has an inverted box on
    either axis; one below or right of it cannot (t2 >= t0 > w there, so b2 clamps to w: the slice is empty from its start)"""
    h, w = cc.SWEEP_H, cc.SWEEP_W
    stops = {}
    for name, box in {**cc.OUTSIDE, **cc.INVERTED}.items():
        assert not cr.pad_box(box, w, h)[1], name
        raw = _raw_pad(box, w, h)
        stops[name] = (int(raw[2]) + 1, int(raw[3]) + 1)
    assert stops["above"][1] < 0 and stops["left"][0] < 0 and stops["inverted-x"][0] < 0 and stops["inverted-y"][1] < 0
    assert min(stops["below"]) > 0 and min(stops["right"]) > 0
    assert all(any(np.array_equal(np.asarray(b, F), r) for r in cc.sweep_boxes()[82 * 82:]) for b in cc.OUTSIDE.values())


# --------------------------------------------------------------------------------------------------------------------------
# the negative-stop decision
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box,frame", [((60, 0, 240, -20), (480, 640)), ((0, 60, -20, 240), (480, 640))])
def test_a_negative_stop_is_no_hand_in_the_oracle_and_the_rule(box, frame):
    from oracle import handnet_ref
    h, w = frame
    depth = torch.from_numpy(cc.position_depth(1, h, w))
    assert depth[:, box[1]:box[3] + 1, box[0]:box[2] + 1].numel() > 0        # what Python slicing would cut: not empty
    assert handnet_ref.crop_depth(depth, torch.tensor(box)) is None


def test_select_and_crop_agrees_with_the_rule_on_negative_stops():
    """the issue's example, its transpose, the sweep's outside and inverted boxes: oracle and rule say `no hand`; a frame with a
    hand between them keeps its place"""
    from oracle import handnet_ref
    h, w = 480, 640
    boxes = [(100.0, -300.0, 200.0, -100.0), (-300.0, 100.0, -100.0, 200.0), (100.0, 50.0, 300.0, 400.0), (400.0, 50.0, 20.0, 200.0)]
    assert _raw_pad(boxes[0], w, h).tolist() == [60, 0, 240, -20] and _raw_pad(boxes[1], w, h).tolist() == [0, 60, -20, 240]
    dets = [dict(boxes=torch.tensor([b]), labels=torch.tensor([2])) for b in boxes]
    depth = torch.from_numpy(np.stack([cc.position_depth(1, h, w)] * len(boxes)))
    mask, kept, crops = handnet_ref.select_and_crop(dets, depth, 3)
    want = [cr.pad_box(b, w, h) for b in boxes]
    assert mask.tolist() == [ok for _, ok in want] == [False, False, True, False]
    assert len(kept) == len(crops) == 1 and kept[0].tolist() == want[2][0].tolist()
    assert np.array_equal(crops[0][0].numpy(), cr.gather(depth[2].numpy(), want[2][0], True, False, 176, 4, False)[..., 0])


# --------------------------------------------------------------------------------------------------------------------------
# the slot walk
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cc.SLOT_KS)
def test_slot_tables_reach_their_branches(k):
    names, boxes, labels, scores, sides, counts = cc.slot_frames(k)
    h, w = cc.SWEEP_H, cc.SWEEP_W
    got = {n: cr.slots(boxes[i], labels[i], scores[i], sides[i], counts[i], cc.SLOT_CAP, cc.HAND, k, 0, w, h)
           for i, n in enumerate(names)}
    assert got["boundaries"]["det_index"].tolist() == ([0, 63, 64, 127, 128] + [-1] * 11)[:k]
    assert got["full-chunk"]["det_index"].tolist() == list(range(k))
    assert got["scattered"]["det_index"].tolist() == list(range(3, 61, 3))[:k]
    assert got["quota-at-63"]["det_index"].tolist() == list(range(64 - k, 64))
    assert not got["count-0"]["has_hand"].any() and not got["none"]["has_hand"].any()
    assert got["count-cap"]["det_index"].tolist() == got["count-above"]["det_index"].tolist() == ([5, 129] + [-1] * 14)[:k]
    assert got["count-short"]["det_index"].tolist() == ([1, 70] + [-1] * 14)[:k]
    assert got["rejected-first"]["det_index"].tolist() == ([-1, 9, 11, 64] + [-1] * 12)[:k]
    assert got["rejected-last"]["has_hand"].tolist() == [1] * (k - 1) + [0] and got["rejected-last"]["det_index"][-1] == -1
    g = got["scattered"]
    assert set(g["side"].tolist()) <= {0, 1} and g["mirror"].tolist() == [int(s == 0) for s in g["side"].tolist()]
    assert {int(s) for g in got.values() for s in g["side"][g["has_hand"] == 1]} == {0, 1}       # left hands are mixed in
    # one slot is the top-1 rule: the first hand row, and nothing else
    for i, n in enumerate(names):
        one = cr.slots(boxes[i], labels[i], scores[i], None, counts[i], cc.SLOT_CAP, cc.HAND, 1, 0, w, h)
        assert np.array_equal(one["crop_box"][0], got[n]["crop_box"][0]) and one["has_hand"][0] == got[n]["has_hand"][0]
        assert (one["side"] == -1).all() and not one["mirror"].any()


# --------------------------------------------------------------------------------------------------------------------------
# the conversion
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in cc.CONVERT_CASES])
def test_convert32_is_the_oracles_float32_branch(name):
    from oracle import a2j_ref
    _, j, n, cw, ch = cc.CONVERT_BY_NAME[name]
    d = cc.convert_inputs(name)
    img, xyz = cr.convert32(d["kp"], d["box_f32"], d["sample_paras"], cw, ch)
    for i in range(n):
        with np.errstate(all="ignore"):
            assert cr.same_bits(img[i], a2j_ref.convert_joints(d["kp"][i], d["box_f32"][i], None, cw, ch)), i
            assert cr.same_bits(xyz[i], a2j_ref.convert_joints(d["kp"][i], d["box_f32"][i], d["sample_paras"][i], cw, ch)), i
    # the detector's int64 boxes: the oracle promotes to float64 there -- the same formula, so convert64 is its value
    img64, xyz64 = cr.convert64(d["kp"], d["box"], cc.PARAS, cw, ch)
    for i in range(n):
        with np.errstate(all="ignore"):
            want = a2j_ref.convert_joints(d["kp"][i], d["box"][i], [float(F(v)) for v in cc.PARAS], cw, ch)
        assert cr.same_bits(xyz64[i].astype(F), want), i


CONVERT_OPTIONS = [dict(), dict(clamp_kp=True), dict(clamp_box=(cc.FRAME_H, cc.FRAME_W)),
                   dict(clamp_kp=True, clamp_box=(cc.FRAME_H, cc.FRAME_W))]


@pytest.mark.parametrize("name", [c[0] for c in cc.CONVERT_CASES])
def test_convert32_is_inside_the_bound_of_convert64(name):
    _, j, n, cw, ch = cc.CONVERT_BY_NAME[name]
    d = cc.convert_inputs(name)
    worst = 0.0
    for box, paras in ((d["box"], cc.PARAS), (d["box"], None), (d["box_f32"], d["sample_paras"])):
        for opt in CONVERT_OPTIONS:
            args = (d["kp"], box, paras, cw, ch)
            got, want, bound = cr.convert32(*args, valid=d["valid"], **opt), cr.convert64(*args, valid=d["valid"], **opt), \
                cr.convert_bound(*args, valid=d["valid"], **opt)
            for g, w_, b in zip(got, want, bound):
                if g is not None:
                    worst = max(worst, cr.bound_ratio(g, w_, b))
            assert not got[0][d["valid"] == 0].any()
            if opt.get("clamp_kp"):                                    # a NaN stays NaN under the clamp
                assert np.array_equal(np.isnan(got[0][..., 2]), np.isnan(d["kp"][..., 2]) & (d["valid"] != 0)[:, None])
    print(f"crop cpu convert {name}: max |convert32 - convert64| / bound = {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_the_ros_clamp_is_as_written():
    """x0 = 600 is clamped to H = 480 (not to W): as ros_demo.py writes it"""
    kp = np.zeros((1, 1, 3), F)
    img, _ = cr.convert32(kp, np.array([[600, 300, 640, 480]], np.int64), None, 176, 176, clamp_box=(480, 640))
    assert img[0, 0, 0] == 480.0 and img[0, 0, 1] == 300.0


# --------------------------------------------------------------------------------------------------------------------------
# the standardisation
# --------------------------------------------------------------------------------------------------------------------------
def _standardize_as_the_kernel(uv):
    """float64 sums in joint order, one fp32 rounding on store"""
    out = np.empty(uv.shape, F)
    with np.errstate(all="ignore"):
        for i in range(uv.shape[0]):
            for ax in range(2):
                x = uv[i, :, ax].astype(np.float64)
                m = 0.0
                for t in x:
                    m += t
                m /= len(x)
                v = 0.0
                for t in x:
                    v += (t - m) * (t - m)
                out[i, :, ax] = ((x - m) / np.sqrt(np.float64(v / len(x)))).astype(F)
    return out


@pytest.mark.parametrize("j", cc.STD_JOINTS)
def test_the_kernels_scheme_is_inside_the_standardisation_bound(j):
    uvd, valid = cc.std_inputs(j)
    uv = uvd[..., :2]
    want, bound = cr.standardize64(uv), cr.standardize_bound(uv)
    ratio = cr.bound_ratio(_standardize_as_the_kernel(uv), want, bound)
    print(f"crop cpu standardize J={j}: max |scheme - float64| / bound = {ratio:.4f}")
    assert ratio <= 1.0 and (ratio > 0.0 or j == 2)       # (two joints standardise to +-1 exactly)
    rows = dict(zip(cc.STD_ROWS, range(len(cc.STD_ROWS))))
    assert np.isnan(want[rows["same-u"], :, 0]).all() and np.isfinite(want[rows["same-u"], :, 1]).all()
    assert np.isnan(want[rows["same-v"], :, 1]).all() and np.isnan(want[rows["nan-joint"], :, 0]).all()
    assert np.abs(want[rows["spread"]].mean(axis=0)).max() < 1e-12 and np.abs(want[rows["spread"]].std(axis=0) - 1).max() < 1e-12
    # the gate: spread hands pass; clustered, collinear and NaN hands do not
    assert cr.gate32(uv).tolist() == [True, True, False, False, False, True, True, False]
    assert float(np.abs(uv[rows["clustered"]] - np.array([600, 400], F)).max()) <= 1e-3


def test_a_fp32_standardisation_is_outside_the_bound():
    """the bound is no wider than the scheme: the same statistics summed in fp32 miss it on the clustered row"""
    uvd, _ = cc.std_inputs(21)
    uv = uvd[2:3, :, :2]
    m = uv.mean(axis=1, keepdims=True, dtype=F)
    got = (uv - m) / np.sqrt(((uv - m) ** 2).mean(axis=1, keepdims=True, dtype=F))
    assert cr.bound_ratio(got.astype(F), cr.standardize64(uv), cr.standardize_bound(uv)) > 1.0


# --------------------------------------------------------------------------------------------------------------------------
# mutants: every check can fail
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["fma", "round"])
def test_box_mutants_fail_on_their_case(mutant):
    kind, box = cc.MUTANT_CASE[mutant]
    h, w = cc.SWEEP_H, cc.SWEEP_W
    assert kind == "box" and not np.array_equal(cr.pad_box(box, w, h, mutant)[0], cr.pad_box(box, w, h)[0])
    grid = cc.sweep_boxes()[:82 * 82]                      # the sweep holds the case's corners on each axis, and catches it
    assert ((grid[:, 0] == box[0]) & (grid[:, 2] == box[2])).any() and ((grid[:, 1] == box[1]) & (grid[:, 3] == box[3])).any()
    assert not np.array_equal(cr.pad_boxes(grid, w, h, mutant)[0], cr.pad_boxes(grid, w, h)[0])


def test_le_at_the_w_clamp_is_the_same_rule():
    """no case can catch `<=` for `<`: at t == (float)w the truncation is w itself"""
    assert cc.MUTANT_CASE["le_w"] is None
    h, w = cc.SWEEP_H, cc.SWEEP_W
    a, b = cr.pad_boxes(cc.sweep_boxes(), w, h, "le_w"), cr.pad_boxes(cc.sweep_boxes(), w, h)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    t2 = cc.sweep_boxes()[:, 2].astype(np.int64)
    bw = t2 - cc.sweep_boxes()[:, 0].astype(np.int64)
    assert ((t2.astype(F) + F(0.4) * bw.astype(F)) == F(w)).any()                    # the equality is reached in the sweep


@pytest.mark.parametrize("mutant", ["mul_first", "shift_2in1"])
def test_index_mutants_fail_on_their_case(mutant):
    kind, (n_in, n_out, dst) = cc.MUTANT_CASE[mutant]
    assert kind == "index" and n_out in (7, 32, 176) and n_in <= (cc.RESIZE_W if n_out == 176 else cc.SMALL_H)
    assert cr.src_index(dst, n_in, n_out, mutant) != cr.src_index(dst, n_in, n_out)


def test_the_clamp_to_in_minus_1_is_never_reached():
    """no case can catch a dropped clamp: floor(dst * fl(in / out)) <= in - 1 for every dst < out at these sizes (and for every
    out < 2^22: crop_cases.MUTANT_CASE) -- the clamp guards the arithmetic, it does not shape the result"""
    assert cc.MUTANT_CASE["no_clamp"] is None
    for out in (7, 32, 176):
        for n_in in range(1, 700):
            d = np.arange(out)
            assert np.array_equal(cr.src_index(d, n_in, out, "no_clamp"), cr.src_index(d, n_in, out))


def test_rank_mutant_fails_on_its_case():
    kind, name = cc.MUTANT_CASE["rank_skips_rejected"]
    names, boxes, labels, scores, sides, counts = cc.slot_frames(2)
    i = names.index(name)
    args = (boxes[i], labels[i], scores[i], sides[i], counts[i], cc.SLOT_CAP, cc.HAND, 2, 0, cc.SWEEP_W, cc.SWEEP_H)
    assert cr.slots(*args)["det_index"].tolist() == [-1, 9] and cr.slots(*args, mutant="rank_skips_rejected")["det_index"].tolist() == [9, 11]


def test_crop_w_for_v_fails_on_its_case_and_hides_on_a_square_crop():
    kind, name = cc.MUTANT_CASE["crop_w_for_v"]
    _, j, n, cw, ch = cc.CONVERT_BY_NAME[name]
    d = cc.convert_inputs(name)
    assert cw != ch
    assert not cr.same_bits(cr.convert32(d["kp"], d["box"], None, cw, ch, mutant="crop_w_for_v")[0], cr.convert32(d["kp"], d["box"], None, cw, ch)[0])
    d = cc.convert_inputs("J21-n13")
    assert cr.same_bits(cr.convert32(d["kp"], d["box"], None, 176, 176, mutant="crop_w_for_v")[0], cr.convert32(d["kp"], d["box"], None, 176, 176)[0])
