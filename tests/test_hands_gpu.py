"""Up to K hands per frame (HandNetEngine.forward_hands, HandNet.forward_hands, hn_handnet_forward_hands): slot k of a frame
is its k-th hand-label detection in score order, cropped exactly as the top-1 path crops the first."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 480, 640
PARAS = (617.343, 617.343, 312.42, 241.42)


def _dets_from_boxes(boxes, labels, cap=None, counts=None):
    """Pack per-image (boxes [k,4], labels [k]) lists into an ops.Detections; scores descend along each list."""
    from hn_amd import ops
    n = len(boxes)
    cap = cap or max(8, max(len(b) for b in boxes))
    det = ops.alloc_detections(n, cap, "cuda")
    for i, (b, l) in enumerate(zip(boxes, labels)):
        k = len(b)
        if k:
            det.boxes[i, :k] = torch.as_tensor(b, dtype=torch.float32).cuda()
            det.labels[i, :k] = torch.as_tensor(l, dtype=torch.int32).cuda()
            det.scores[i, :k] = 0.99 - 0.001 * torch.arange(k, dtype=torch.float32).cuda()
        det.count[i] = k if counts is None or counts[i] is None else counts[i]
    return det


def _engine(fcos_sd, a2j_sd, rgbd_sd=None):
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    a2j = A2JEngine(rgbd_sd, rgbd=True, device="cuda") if rgbd_sd is not None else A2JEngine(a2j_sd, device="cuda")
    return HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), a2j, 3)


def _hand_rule_cases():
    """Frames with 0, 1, 2, 3, 5 hand-label boxes (label 2) among other labels; a box out of the frame; an empty padded
    slice in slot 1; a list longer than one wave's chunk; det_count beyond cap."""
    other = [37.0, 40.0, 90.0, 99.0]
    boxes = [
        [other, [10.0, 10.0, 50.0, 60.0]],
        [other, [100.7, 50.2, 300.9, 400.5], other],
        [[600.1, 440.3, 700.0, 500.0], other, [-30.5, 200.2, 40.9, 260.0]],        # first hand sticks out bottom / right
        [[120.0, 80.0, 220.0, 200.0], other, [700.0, 100.0, 760.0, 200.0], [0.0, 0.0, 639.9, 479.9]],   # slot 1: empty slice
        [[5.0 + 30 * j, 7.0 + 20 * j, 60.0 + 31 * j, 90.0 + 21 * j] if j % 2 == 0 else other for j in range(9)],
    ]
    labels = [[0, 1], [0, 2, 1], [2, 0, 2], [2, 0, 2, 2], [2 if j % 2 == 0 else 1 for j in range(9)]]
    # frame 5: 70 non-hand rows, then hands at rows 70, 75, 129 -- a second chunk of 64, and det_count > cap (row 129 is the
    # last row the list holds)
    cap = 130
    b5 = [other] * cap
    l5 = [0] * cap
    for j, r in enumerate((70, 75, 129)):
        b5[r] = [50.0 + 40 * j, 60.0, 150.0 + 40 * j, 220.0]
        l5[r] = 2
    boxes.append(b5)
    labels.append(l5)
    return boxes, labels, cap, [None] * 5 + [cap + 57]


def _expected_slots(boxes, labels, counts, cap, depth, k_max, perm=None):
    """The reference rule (handnet_pipeline.py:84-105) per slot: (box int64 [4] or None, crop [C,176,176] or None, row)."""
    from oracle import handnet_ref
    out = []
    for i, (b, l) in enumerate(zip(boxes, labels)):
        cnt = min(len(b) if counts[i] is None else counts[i], cap)
        rows = [j for j in range(min(cnt, len(b))) if l[j] == 2]
        slots = []
        for k in range(k_max):
            if k >= len(rows):
                slots.append((None, None, -1))
                continue
            box = handnet_ref.crop_box(torch.tensor(b[rows[k]]), W, H)
            img = depth[i] if perm is None else depth[i][perm]
            dc = handnet_ref.crop_depth(img, box)
            slots.append((None, None, -1) if dc is None else (box, dc, rows[k]))
        out.append(slots)
    return out


@pytest.mark.parametrize("k_max", [1, 2, 4, 16])
def test_crop_resize_hands_matches_reference_rule(k_max):
    from hn_amd import ops
    g = torch.Generator().manual_seed(9)
    boxes, labels, cap, counts = _hand_rule_cases()
    depth = 0.3 + torch.rand((len(boxes), 1, H, W), generator=g)
    det = _dets_from_boxes(boxes, labels, cap=cap, counts=counts)
    box, has, score, index, crops = ops.crop_resize_hands(det, 2, depth.cuda(), k_max)
    torch.cuda.synchronize()
    assert box.shape == (len(boxes), k_max, 4) and crops.shape == (len(boxes) * k_max, 176, 176, 4)
    box, has, score, index, crops = box.cpu(), has.cpu(), score.cpu(), index.cpu(), crops.cpu()
    want = _expected_slots(boxes, labels, counts, cap, depth, k_max)
    filled = 0
    for i, slots in enumerate(want):
        for k, (wb, wc, row) in enumerate(slots):
            c = crops[i * k_max + k]
            if wb is None:
                assert int(has[i, k]) == 0 and int(index[i, k]) == -1 and float(score[i, k]) == 0.0, (i, k)
                assert not box[i, k].any() and not c.any(), (i, k)
                continue
            filled += 1
            assert int(has[i, k]) == 1 and int(index[i, k]) == row, (i, k)
            assert torch.equal(box[i, k], wb), (i, k, box[i, k], wb)
            assert float(score[i, k]) == float(det.scores[i, row]), (i, k)
            assert torch.equal(c[..., 0], wc[0]), (i, k)
            assert not c[..., 1:].any()
    # the rule's corner cases are in the data: slot 1 of frame 3 is empty and slot 2 is still the THIRD hand box
    if k_max >= 3:
        assert int(has[3, 1]) == 0 and int(index[3, 2]) == 3
    if k_max >= 3:
        assert index[5, :3].tolist() == [70, 75, 129]
    assert filled == sum(1 for s in want for x in s if x[0] is not None)


def test_crop_resize_hands_rgbd_permutation():
    from hn_amd import ops
    g = torch.Generator().manual_seed(11)
    boxes, labels, cap, counts = _hand_rule_cases()
    depth = torch.rand((len(boxes), 4, H, W), generator=g)
    det = _dets_from_boxes(boxes, labels, cap=cap, counts=counts)
    box, has, _, _, crops = ops.crop_resize_hands(det, 2, depth.cuda(), 3, reorder_bgr=True)
    box, crops = box.cpu(), crops.cpu()
    for i, slots in enumerate(_expected_slots(boxes, labels, counts, cap, depth, 3, perm=[2, 1, 0, 3])):
        for k, (wb, wc, _) in enumerate(slots):
            if wb is not None:
                assert torch.equal(crops[i * 3 + k].permute(2, 0, 1), wc), (i, k)


def test_one_hand_is_todays_path(fcos_sd, a2j_sd):
    """max_hands = 1 is forward_device: the same crop and the same A2J batch, so the same bits."""
    import types

    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import synth
    eng = _engine(fcos_sd, a2j_sd)
    rgb, depth = synth.make_rgb(3, seed=1000).cuda(), synth.make_depth(3, seed=2000).cuda()
    top = eng.forward_device(rgb, depth)
    one = eng.forward_hands(rgb, depth, max_hands=1)
    assert int(top.has_hand.sum()) >= 2
    assert torch.equal(one.crop_box[:, 0], top.crop_box) and torch.equal(one.has_hand[:, 0], top.has_hand)
    assert torch.equal(one.crops_nhwc, top.crops_nhwc) and torch.equal(one.keypoints[:, 0], top.keypoints)
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    net.detector.load_state_dict(fcos_sd, strict=False)
    net.a2j.load_state_dict(a2j_sd, strict=False)
    net = net.cuda().eval()
    with torch.inference_mode():
        kp, _, _ = net([f for f in rgb], depth_images=depth)
        hk, db, hb, mask, sc = net.forward_hands([f for f in rgb], depth, max_hands=1)
    assert torch.equal(hk[:, 0], kp)
    assert torch.equal(hb[:, 0], top.crop_box.cpu()) and torch.equal(mask[:, 0], top.has_hand.cpu() != 0)
    assert db.shape == (int(mask.sum()), 1, 176, 176)


def test_slot_k_is_the_top1_path_on_a_shifted_list(fcos_sd, a2j_sd):
    """Relabelling the first k hand detections to another class makes slot k the top-1 hand: ops.crop_resize on that list
    gives slot k's box and crop bit for bit, and A2J on that one crop gives slot k's keypoints (batch 1 vs batch N*K)."""
    import parity_cases as pc
    from hn_amd import ops
    eng = _engine(fcos_sd, a2j_sd)
    rgb, depth = pc.noise_frames(1).cuda(), pc.depth_noise(1).cuda()
    k_max = 3
    out = eng.forward_hands(rgb, depth, max_hands=k_max)
    det = dataclasses.replace(out.detections, **{f.name: getattr(out.detections, f.name).clone()
                                                 for f in dataclasses.fields(out.detections)})
    torch.cuda.synchronize()
    assert bool(out.has_hand.all()), out.has_hand
    hand_rows = [j for j in range(int(det.count[0])) if int(det.labels[0, j]) == 2]
    for k in range(k_max):
        labels = det.labels.clone()
        labels[0, hand_rows[:k]] = 0
        box, has, crop = ops.crop_resize(dataclasses.replace(det, labels=labels), 2, depth, 176, 4)
        assert torch.equal(box[0], out.crop_box[0, k]) and int(has[0]) == int(out.has_hand[0, k])
        assert torch.equal(crop[0], out.crops_nhwc[k])
        assert int(out.det_index[0, k]) == hand_rows[k]
        kp = eng.a2j.forward_nhwc(crop.contiguous(), valid=has.clone())
        assert (kp[0] - out.keypoints[0, k]).abs().max().item() < 1e-4


def test_end_to_end_matches_cpu_oracle(fcos_sd, a2j_sd):
    """Four noise frames, K = 4 (the oracle's detector leaves 22-44 hand survivors per frame): every slot whose rank and box
    agree with the oracle's has the identical int64 box and keypoints within 1e-3; near-tied scores may swap ranks, so a
    disagreeing slot is reported with its score margin, and at least 3 of the 4 frames must agree on all four slots."""
    import parity_cases as pc
    from oracle import a2j_ref, fcos_ref, handnet_ref
    k_max = 4
    rgb, depth = pc.noise_frames(4), pc.depth_noise(4)
    eng = _engine(fcos_sd, a2j_sd)
    out = eng.forward_hands(rgb.cuda(), depth.cuda(), max_hands=k_max)
    box, has, idx = out.crop_box.cpu(), out.has_hand.cpu(), out.det_index.cpu()
    kp, score = out.keypoints.cpu(), out.score.cpu()
    dets = fcos_ref.fcos_forward([f for f in rgb], fcos_sd, 3)
    whole, report = 0, []
    for i, d in enumerate(dets):
        rows = (d["labels"] == 2).nonzero().flatten().tolist()
        assert len(rows) >= k_max, (i, len(rows))
        agree = 0
        for k in range(k_max):
            wb = handnet_ref.crop_box(d["boxes"][rows[k]], W, H)
            dc = handnet_ref.crop_depth(depth[i], wb)
            if int(has[i, k]) == 1 and int(idx[i, k]) == rows[k] and torch.equal(box[i, k], wb):
                want = a2j_ref.a2j_forward(dc.unsqueeze(0), a2j_sd)[0]
                err = (kp[i, k] - want).abs().max().item()
                assert err < 1e-3, (i, k, err)
                agree += 1
            else:
                s = d["scores"]
                margin = float((s[:-1] - s[1:]).abs().min()) if len(s) > 1 else float("inf")
                report.append(f"frame {i} slot {k}: rank {int(idx[i, k])} vs {rows[k]}, score {float(score[i, k]):.6f} vs "
                              f"{float(d['scores'][rows[k]]):.6f}, smallest score gap of the list {margin:.2e}")
        whole += agree == k_max
    print("\n".join(report) or "all slots agree")
    assert whole >= 3, report


def test_graphed_hands_replay_and_frame_permutation(fcos_sd, a2j_sd):
    import parity_cases as pc
    eng = _engine(fcos_sd, a2j_sd)
    rgb, depth = pc.noise_frames(3).cuda(), pc.depth_noise(3).cuda()
    eager = eng.forward_hands(rgb, depth, max_hands=2)
    run, s_img, s_dep, out = eng.graphed_hands(rgb, depth, 2)
    assert eng.graph_count() == 1 and not eng.has_graph(rgb.shape, depth.shape)
    s_img.copy_(rgb)
    s_dep.copy_(depth)
    run()
    torch.cuda.synchronize()
    assert torch.equal(out.crop_box, eager.crop_box) and torch.equal(out.has_hand, eager.has_hand)
    assert (out.keypoints - eager.keypoints).abs().max().item() < 3e-4
    # frame permutation at N = 32, K = 2 permutes every output bit for bit (the slot scores are the detector's own scores,
    # whose last bits the detector does not promise across batch positions: to 1e-6)
    rgb, depth = pc.noise_frames(32, seed=3000).cuda(), pc.depth_noise(32, seed=4000).cuda()
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(5)).cuda()
    a = eng.forward_hands(rgb, depth, max_hands=2)
    a = {f: getattr(a, f).clone() for f in ("keypoints", "crop_box", "has_hand", "score", "crops_nhwc")}
    b = eng.forward_hands(rgb[perm].contiguous(), depth[perm].contiguous(), max_hands=2)
    for f, v in a.items():
        w = getattr(b, f)
        if f == "crops_nhwc":
            v, w = v.view(32, 2, *v.shape[1:]), w.view(32, 2, *w.shape[1:])
        if f == "score":
            d = (v[perm] - w).abs().max().item()
            print(f"slot scores under frame permutation: max |d| {d:.3e}")
            assert d < 1e-6, d
            continue
        assert torch.equal(v[perm], w), f


def test_sparse_slots_compact_a2j(fcos_sd, a2j_sd, monkeypatch):
    """Fewer than half of the N*K slots filled: the next eager step runs A2J on the filled slots only -- same keypoints there
    within 1e-4, zero rows elsewhere; a capture never takes that path."""
    import parity_cases as pc
    from hn_amd import pipeline
    eng = _engine(fcos_sd, a2j_sd)
    n, k_max = 4, 4
    rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
    dense = eng.forward_hands(rgb, depth, max_hands=k_max)
    torch.cuda.synchronize()
    assert int(dense.has_hand.sum()) == n * k_max and not eng._sparse_hint
    keep = torch.zeros((n, k_max), dtype=torch.int32, device="cuda")
    keep[0, 0] = keep[1, 2] = keep[3, 1] = 1
    real = pipeline.ops.crop_resize_hands
    calls = []

    def sparse_crop(*a, **k):
        box, has, score, index, crops = real(*a, **k)
        has.mul_(keep)
        box.mul_(keep[..., None].to(box.dtype))
        crops.mul_(keep.view(-1, 1, 1, 1).to(crops.dtype))
        return box, has, score, index, crops
    monkeypatch.setattr(pipeline.ops, "crop_resize_hands", sparse_crop)
    real_fwd = eng.a2j.forward_nhwc

    def spy(x, valid=None, **k):
        calls.append(x.shape[0])
        return real_fwd(x, valid=valid, **k)
    monkeypatch.setattr(eng.a2j, "forward_nhwc", spy)
    first = eng.forward_hands(rgb, depth, max_hands=k_max)     # masked full batch; its count arms the hint
    first = {f: getattr(first, f).clone() for f in ("keypoints", "has_hand")}
    torch.cuda.synchronize()
    second = eng.forward_hands(rgb, depth, max_hands=k_max)    # compacted
    assert calls == [n * k_max, 3], calls
    sel = keep.bool()
    assert torch.equal(second.has_hand, first["has_hand"])
    assert not second.keypoints[~sel].any()
    assert (second.keypoints[sel] - first["keypoints"][sel]).abs().max().item() < 1e-4
    assert (second.keypoints[sel] - dense.keypoints[sel]).abs().max().item() < 1e-4
    calls.clear()
    eng.graphed_hands(rgb, depth, k_max)
    assert calls[-1] == n * k_max, calls


def test_convert_and_host_record_per_slot(fcos_sd, a2j_sd):
    import parity_cases as pc
    from hn_amd import ops
    from hn_amd.pipeline import read_hands_tail, read_host_record
    eng = _engine(fcos_sd, a2j_sd).set_convert(PARAS)
    n, k_max = 2, 3
    rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
    out = eng.forward_hands(rgb, depth, max_hands=k_max, to_host=True)
    torch.cuda.synchronize()
    kp, box, has = out.keypoints.view(-1, 21, 3), out.crop_box.view(-1, 4), out.has_hand.view(-1)
    assert torch.equal(out.image_uvd.view(-1, 21, 3), ops.convert_joints(kp, box, has, None))
    assert torch.equal(out.xyz_mm.view(-1, 21, 3), ops.convert_joints(kp, box, has, PARAS))
    hk, hh, hb, words, more = read_host_record(out.host_record, n * k_max, 21, extras=True)
    assert torch.equal(hk, kp.cpu()) and torch.equal(hh, has.cpu()) and torch.equal(hb, box.cpu())
    assert torch.equal(more[0], out.image_uvd.view(-1, 21, 3).cpu()) and torch.equal(more[1], out.xyz_mm.view(-1, 21, 3).cpu())
    assert words == out.range_flags.cpu().tolist()
    sc, ix = read_hands_tail(out.host_record, n * k_max)
    assert torch.equal(sc, out.score.view(-1).cpu()) and torch.equal(ix, out.det_index.view(-1).cpu())


def test_dropin_forward_hands(fcos_sd, a2j_sd):
    """The drop-in's tuple, from one record: CPU keypoints / boxes / mask / scores per slot, the filled slots' crops on the
    device in frame-major order; repeated shapes switch to graph replay like forward()."""
    import types

    import parity_cases as pc
    from handnet_pipeline.handnet_pipeline import HandNet
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    net.detector.load_state_dict(fcos_sd, strict=False)
    net.a2j.load_state_dict(a2j_sd, strict=False)
    net = net.cuda().eval()
    rgb, depth = pc.noise_frames(2), pc.depth_noise(2)
    eng = net.engine()
    ref = eng.forward_hands(rgb.cuda(), depth.cuda(), max_hands=2)
    ref = {f: getattr(ref, f).clone() for f in ("keypoints", "crop_box", "has_hand", "score", "crops_nhwc")}
    with torch.inference_mode():
        for call in range(net.AUTO_GRAPH_CALLS + 2):      # CPU inputs; the later calls replay a capture
            kp, db, boxes, mask, scores = net.forward_hands([f for f in rgb], depth, max_hands=2)
            assert kp.device.type == "cpu" and boxes.dtype == torch.int64 and mask.dtype == torch.bool
            assert torch.equal(boxes, ref["crop_box"].cpu()) and torch.equal(mask, ref["has_hand"].cpu() != 0)
            assert torch.equal(scores, ref["score"].cpu())
            assert (kp - ref["keypoints"].cpu()).abs().max().item() < 3e-4
            sel = ref["has_hand"].view(-1) != 0
            assert torch.equal(db, ref["crops_nhwc"][sel][..., 0].unsqueeze(1))
    assert eng.has_graph_hands((2, 3, H, W), (2, 1, H, W), 2, to_host=True)


def test_native_hands_equal_python_engine(fcos_sd, a2j_sd):
    from hn_amd import synth
    from hn_amd.native_model import NativeModel
    eng = _engine(fcos_sd, a2j_sd)
    m = NativeModel(fcos_sd, a2j_sd, num_classes=3)
    try:
        for n, k_max, seed in ((2, 2, 1000), (5, 3, 1100), (2, 2, 1000)):   # a larger step re-sizes the arena; then a plan hit
            rgb, depth = synth.make_rgb(n, seed=seed).cuda(), synth.make_depth(n, seed=seed + 1000).cuda()
            ref = eng.forward_hands(rgb, depth, max_hands=k_max)
            kp, box, has, score = m.handnet_hands(rgb, depth, k_max)
            assert torch.equal(box, ref.crop_box) and torch.equal(has, ref.has_hand) and torch.equal(score, ref.score)
            assert torch.equal(kp, ref.keypoints)
        rgb, depth = synth.make_rgb(1, seed=1000).cuda(), synth.make_depth(1, seed=2000).cuda()
        for bad in (0, 17):
            with pytest.raises(RuntimeError, match="max_hands"):
                m.handnet_hands(rgb, depth, bad)
        assert m.lib.hn_abi_version() == 36
    finally:
        m.close()
