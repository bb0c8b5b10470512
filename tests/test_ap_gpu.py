"""The detector evaluation on the device (csrc/det_ap.hip) against the rule of tests/ap_ref.py, byte for
byte: the state (hand, obj, fed, overflow) through ops.det_ap_accumulate and through the C entry at every shape of
ap_cases.SHAPES; the golden's reference numbers through DetectionAP.compute(); the captured update; the evaluation loop end to
end with FCOS.device_metrics()."""
import ctypes as C

import numpy as np
import pytest
import torch

import ap_cases
import ap_ref as R
from test_ap_cpu import _golden_batch, _golden_recs

pytestmark = pytest.mark.gpu

_RULED = {}
KEYS = ("hand", "obj", "fed", "overflow")


def _case(shape, max_dets=None):
    """the batches of a shape and the rule on them, computed once and shared (never written to)"""
    key = (shape, max_dets)
    if key not in _RULED:
        case = ap_cases.cases(shape)
        table = R.table_from_recs(case["recs"], case["image_index"])
        want = None
        for batch in case["batches"]:
            want = R.accumulate(batch, table, want, max_dets=max_dets or case["cap"])
        _RULED[key] = (case, table, want)
    return _RULED[key]


def _upload(batch):
    """a numpy batch as (Detections, contacts, dxdymags, image_ids) on the GPU"""
    from hn_amd import ops
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}
    det = ops.Detections(t["boxes"], t["scores"], t["labels"], t["sides"], torch.zeros_like(t["labels"]), torch.zeros_like(t["labels"]),
                         t["count"])
    return det, t["contacts"], t["dxdymags"], t["image_ids"]


def _device_table(table):
    from hn_amd import ops
    return ops.det_ap_table(*(table[k] for k in ("hand_off", "hand_box", "hand_meta", "hand_obj", "obj_off", "obj_box", "obj_diff")),
                            device="cuda")


def _same(state, want):
    got = {k: getattr(state, k).cpu().numpy() for k in KEYS}
    return all(got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes() for k in KEYS)


def _c_entry(lib, up, table, state):
    det, contacts, dxdymags, ids = up
    n, cap = det.scores.shape
    p = lambda t: C.c_void_p(t.data_ptr())
    return lib.hn_det_ap_accumulate_f32(p(det.boxes), p(det.scores), p(det.labels), p(det.sides), p(det.count), p(contacts), p(dxdymags),
                                        p(ids), n, cap, p(table.hand_off), p(table.hand_box), p(table.hand_meta), p(table.hand_obj),
                                        table.hand_box.shape[0], p(table.obj_off), p(table.obj_box), p(table.obj_diff),
                                        table.obj_box.shape[0], table.num_images, 2, 1, 0.1, 0.5, p(state.hand), p(state.obj),
                                        p(state.fed), p(state.overflow), state.hand.shape[1],
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("shape", ap_cases.SHAPES, ids=lambda s: "N%d-cap%d-G%d" % s)
def test_the_kernel_equals_the_rule_byte_for_byte(shape):
    from hn_amd import _lib, ops
    case, table, want = _case(shape)
    lib = _lib.load()
    d_table = _device_table(table)
    assert (d_table.num_images, d_table.npos_hand, d_table.npos_obj) == (table["num_images"], table["npos_hand"], table["npos_obj"])
    uploads = [_upload(b) for b in case["batches"]]
    state = None
    for up in uploads:
        state = ops.det_ap_accumulate(*up, d_table, state=state, max_dets=case["cap"])
    assert tuple(state.hand.shape) == (table["num_images"], case["cap"]) and _same(state, want)
    through_c = ops.det_ap_state(table["num_images"], case["cap"], "cuda")
    for up in uploads:
        assert _c_entry(lib, up, d_table, through_c) == 0, lib.hn_last_error()
    assert _same(through_c, want)
    # twice into the same state: the records written over by themselves, every image fed twice
    twice = {k: v.copy() for k, v in want.items()}
    for batch in case["batches"]:
        twice = R.accumulate(batch, table, twice)
    assert twice["fed"].max() == 2 and twice["hand"].tobytes() == want["hand"].tobytes()
    for up in uploads:
        ops.det_ap_accumulate(*up, d_table, state=state)
    assert _same(state, twice)


def test_two_batches_into_one_state_equal_one_batch_of_both_in_any_order():
    from hn_amd import ops
    case, table, want = _case((2, 130, 64))
    d_table = _device_table(table)
    whole = ap_cases.concat(case["batches"])
    assert _same(ops.det_ap_accumulate(*_upload(whole), d_table, max_dets=130), want)
    perm = np.random.RandomState(5).permutation(whole["count"].shape[0])
    assert _same(ops.det_ap_accumulate(*_upload({k: v[perm] for k, v in whole.items()}), d_table, max_dets=130), want)
    state = None
    for lo, hi in ((0, 7), (7, 8), (8, whole["count"].shape[0])):           # uneven batches: 7 images, 1, the rest
        state = ops.det_ap_accumulate(*_upload({k: v[lo:hi] for k, v in whole.items()}), d_table, state=state, max_dets=130)
    assert _same(state, want)


def test_overflow_and_stray_ids_are_counted_on_the_device():
    from hn_amd import ops
    from hn_amd.metrics import DetectionAP
    case, table, want = _case(ap_cases.OVERFLOW_SHAPE, ap_cases.OVERFLOW_MAX_DETS)
    assert int(want["overflow"][0]) == 1
    ap = DetectionAP.from_recs(case["recs"], case["image_index"], device="cuda:0", max_dets=ap_cases.OVERFLOW_MAX_DETS)
    for batch in case["batches"]:
        ap.update(*_upload(batch))
    got = ap.state()
    assert all(got[k].tobytes() == want[k].tobytes() for k in KEYS)
    with pytest.raises(ValueError, match="did not fit"):
        ap.compute()
    ap.reset()
    stray = dict(case["batches"][0], image_ids=np.array([-1, table["num_images"]], np.int32))
    ap.update(*_upload(stray))
    got = ap.state()
    assert int(got["overflow"][0]) == 2 and not got["hand"].any() and not got["obj"].any() and not got["fed"].any()
    ap.reset()
    ap.update(*_upload(case["batches"][0]))
    ap.update(*_upload(case["batches"][0]))
    with pytest.raises(ValueError, match="fed 2 times"):
        ap.compute()


def test_the_goldens_reference_numbers_through_detection_ap(golden_dir):
    """DetectionAP on the golden's inputs in batches of 4 against the imported reference's rec, prec and ap for the six tables and
    both AP forms, under the CPU test's condition: equal arrays, the same float64 (the state is the rule's byte for byte, and the
    host part is the same numpy operations in the same order).  Two shards merged equal one pass."""
    from hn_amd.metrics import AP_NAMES, DetectionAP
    g = np.load(golden_dir / "det_ap.npz")
    recs, names = _golden_recs(g)
    batch = _golden_batch(g)
    table = R.table_from_recs(recs, names)
    want_state = R.accumulate(batch, table, max_dets=8)
    ap = DetectionAP.from_recs(recs, names, device="cuda:0", max_dets=8)
    shards = [DetectionAP.from_recs(recs, names, device="cuda:0", max_dets=8) for _ in range(2)]
    for i, lo in enumerate(range(0, batch["count"].shape[0], 4)):
        part = _upload({k: v[lo:lo + 4] for k, v in batch.items()})
        ap.update(*part)
        shards[i % 2].update(*part)
    state = ap.state()
    assert all(state[k].tobytes() == want_state[k].tobytes() for k in KEYS)
    for use_07, tag in ((False, "10"), (True, "07")):
        res = ap.compute(use_07_metric=use_07)
        for name in AP_NAMES:
            assert np.array_equal(res[name]["rec"], g[f"rec_{tag}_{name}"]) and np.array_equal(res[name]["prec"], g[f"prec_{tag}_{name}"]), name
            assert res[name]["ap"] == float(g[f"ap_{tag}_{name}"]), name
        assert res["mean_ap"] == float(np.mean([float(g[f"ap_{tag}_targetobject"]), float(g[f"ap_{tag}_hand"])]))
        assert res["fed"] == batch["count"].shape[0] and res["npos"] == {"targetobject": table["npos_obj"], "hand": table["npos_hand"]}
    shards[0].merge(shards[1])
    merged = shards[0].state()
    assert all(merged[k].tobytes() == state[k].tobytes() for k in KEYS)
    shards[1].merge(state)
    with pytest.raises(ValueError, match="fed 2 times"):
        shards[1].compute()


def test_the_op_checks_its_tensors():
    from hn_amd import ops
    case, table, _ = _case((3, 5, 2))
    d_table = _device_table(table)
    det, contacts, dxdymags, ids = _upload(case["batches"][0])
    state = ops.det_ap_state(table["num_images"], 5, "cuda")
    ops.det_ap_accumulate(det, contacts, dxdymags, ids, d_table, state=state)
    before = state.flat.clone()
    assert int(before[-table["num_images"] - 1:-1].sum()) == 3

    def changed(**kw):
        return ops.Detections(**{**{f: getattr(det, f) for f in ("boxes", "scores", "labels", "sides", "level", "keep", "count")}, **kw})
    bad = [(dict(det=changed(boxes=det.boxes[:, :, :3].contiguous())), ValueError, "det.boxes"),
           (dict(det=changed(scores=det.scores[:, :4].contiguous())), ValueError, "det.boxes"),
           (dict(det=changed(labels=det.labels[:2].contiguous())), ValueError, "det.labels"),
           (dict(det=changed(labels=det.labels.long())), TypeError, "det.labels"),
           (dict(det=changed(scores=det.scores.double())), TypeError, "det.scores"),
           (dict(det=changed(sides=det.sides.t().contiguous().t())), ValueError, "contiguous"),
           (dict(det=changed(count=det.count[:2].contiguous())), ValueError, "det.count"),
           (dict(contacts=contacts.float()), TypeError, "contacts"), (dict(contacts=contacts[:, :4].contiguous()), ValueError, "contacts"),
           (dict(dxdymags=dxdymags[:, :, :2].contiguous()), ValueError, "dxdymags"),
           (dict(ids=ids.long()), TypeError, "image_ids"), (dict(ids=ids[:2].contiguous()), ValueError, "image_ids"),
           (dict(ids=ids.cpu()), RuntimeError, "must live on the GPU"),
           (dict(table=table), TypeError, "det_ap_table"),
           (dict(state=ops.det_ap_state(table["num_images"] + 1, 5, "cuda")), ValueError, "state.hand"),
           (dict(state=ops.det_ap_state(table["num_images"], 5, "cuda")._replace(fed=state.fed[:3])), ValueError, "state.fed"),
           (dict(hand_label=1), ValueError, "both 1"), (dict(score_min=1.5), ValueError, "score_min"),
           (dict(ovthresh=float("nan")), ValueError, "threshold")]
    for kw, error, word in bad:
        a = dict(det=det, contacts=contacts, dxdymags=dxdymags, ids=ids, table=d_table, state=state)
        rule = {k: kw.pop(k) for k in ("hand_label", "score_min", "ovthresh") if k in kw}
        a.update(kw)
        with pytest.raises(error, match=word):
            ops.det_ap_accumulate(a["det"], a["contacts"], a["dxdymags"], a["ids"], a["table"], state=a["state"], **rule)
    assert torch.equal(state.flat, before)                                  # no refused call touched the state
    with pytest.raises(ValueError, match="65 obj boxes"):
        ops.det_ap_table([0, 0], np.zeros((0, 4)), np.zeros((0, 4)), np.zeros((0, 4)), [0, 65], np.zeros((65, 4)), np.zeros(65), "cuda")


def test_the_captured_update_replays_on_refilled_inputs():
    """`update` alone inside ops.capture_step: a synchronisation or a host copy in it would fail the capture.  Replayed on the
    static inputs refilled with each batch of the shape, into the zeroed state: the rule's bytes."""
    from hn_amd import ops
    from hn_amd.metrics import DetectionAP
    case, table, want = _case((3, 5, 2))
    ap = DetectionAP.from_recs(case["recs"], case["image_index"], device="cuda:0", max_dets=5)
    uploads = [_upload(b) for b in case["batches"]]
    static = _upload(case["batches"][0])
    graph, _ = ops.capture_step(lambda: ap.update(*static))
    ap.reset()                                                              # (the warm-up and the capture fed the first batch)
    for det, contacts, dxdymags, ids in uploads:
        for dst, src in zip((static[0].boxes, static[0].scores, static[0].labels, static[0].sides, static[0].count) + static[1:],
                            (det.boxes, det.scores, det.labels, det.sides, det.count, contacts, dxdymags, ids)):
            dst.copy_(src)
        graph.replay()
    torch.cuda.synchronize()
    got = ap.state()
    assert all(got[k].tobytes() == want[k].tobytes() for k in KEYS)


def _as_batch(dicts, ids):
    """the dicts `forward` returned -> the rule's batch (capacity = the longest list, never 0)"""
    cap = max(1, max(int(d["scores"].shape[0]) for d in dicts))
    n = len(dicts)
    batch = dict(boxes=np.zeros((n, cap, 4), np.float32), scores=np.zeros((n, cap), np.float32), labels=np.zeros((n, cap), np.int32),
                 sides=np.zeros((n, cap), np.int32), contacts=np.zeros((n, cap), np.int32), dxdymags=np.zeros((n, cap, 3), np.float32),
                 count=np.zeros((n,), np.int32), image_ids=np.asarray(ids, np.int32))
    for i, d in enumerate(dicts):
        k = int(d["scores"].shape[0])
        batch["count"][i] = k
        for key in ("boxes", "scores", "labels", "sides", "contacts", "dxdymags"):
            batch[key][i, :k] = d[key].cpu().numpy()
    return batch


def _annotations_from(dicts, names):
    """ground truth made from the detector's own output: of each class's detections (the first 40) every third box is kept as it
    is, every third moved off by its own width (no overlap), the rest kept with another state; one kept hand is difficult"""
    recs = {}
    for d, name in zip(dicts, names):
        rows, seen = [], {1: 0, 2: 0}
        boxes, labels = d["boxes"].cpu().numpy(), d["labels"].cpu().numpy()
        for k in range(boxes.shape[0]):
            label = int(labels[k])
            if label not in seen or seen[label] >= 40:
                continue
            j = seen[label]
            seen[label] += 1
            x1, y1, x2, y2 = (int(round(float(v) + 1.0)) for v in boxes[k])
            if j % 3 == 1:
                x1, x2 = x1 + (x2 - x1 + 2), x2 + (x2 - x1 + 2)
            state = int(d["contacts"][k]) + (1 if j % 3 == 2 else 0)
            rows.append({"name": "hand" if label == 2 else "targetobject", "bbox": [x1, y1, x2, y2], "difficult": int(label == 2 and j == 3),
                         "handstate": state, "leftright": int(d["sides"][k]), "objectbbox": None})
        recs[name] = rows
    return recs


def test_the_evaluation_loop_end_to_end():
    """FCOS(num_classes=3) with the synthetic ext weights on two synthetic frames, in batches of 1: the state after eval_step is
    the rule fed with forward's dicts, byte for byte; eval_results() is the rule's dict; a second epoch starts from zero; forward
    is what it was."""
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model = FCOS(num_classes=3).cuda().eval()
    model.load_state_dict(synth.make_fcos_state_dict(seed=0, num_classes=3, ext=True), strict=False)
    rgb = synth.make_rgb(2, seed=77).cuda()
    with pytest.raises(RuntimeError, match="call device_metrics"):
        model.eval_step([rgb[0]], [0])
    with torch.inference_mode():
        dicts = [model([rgb[i]])[0] for i in range(2)]
    names = ["frame_a", "frame_unfed", "frame_b"]
    ids = [2, 0]                                                            # frame 0 is image 2, frame 1 is image 0
    recs = _annotations_from(dicts, [names[i] for i in ids])
    recs["frame_unfed"] = [ap_cases.gt_hand(ap_cases.B), ap_cases.gt_obj(ap_cases.OB)]
    longest = max(1, max(int(d["scores"].shape[0]) for d in dicts))
    ap = model.device_metrics(recs, names, max_dets=longest)
    assert ap is model._detection_ap and ap.max_dets == longest
    with torch.inference_mode():
        for i in range(2):
            model.eval_step([rgb[i]], torch.tensor([ids[i]], dtype=torch.int32, device="cuda"))
    table = R.table_from_recs(recs, names)
    want_state = None
    for i in range(2):
        want_state = R.accumulate(_as_batch([dicts[i]], [ids[i]]), table, want_state, max_dets=longest)
    got = ap.state()
    assert want_state["fed"].tolist() == [1, 0, 1] and int(want_state["overflow"][0]) == 0
    assert all(got[k].tobytes() == want_state[k].tobytes() for k in KEYS)
    want = R.compute(want_state, table["npos_hand"], table["npos_obj"])
    tp, fp = (int(((want_state["hand"] >> shift) & 1).sum()) for shift in (R.TP_SHIFT, R.FP_SHIFT))
    assert tp > 0 and fp > 0, (tp, fp)                                      # TP and FP both occur
    res = model.eval_results()
    for name in R.NAMES:
        assert res[name]["ap"] == want[name]["ap"] and np.array_equal(res[name]["rec"], want[name]["rec"])
        assert np.array_equal(res[name]["prec"], want[name]["prec"])
    assert res["mean_ap"] == want["mean_ap"] and res["fed"] == 2 and 0.0 < res["hand"]["ap"] < 1.0
    # the second epoch starts from zero; ids given as a list are uploaded
    assert not ap.state()["hand"].any() and not ap.state()["fed"].any()
    with torch.inference_mode():
        model.eval_step([rgb[1]], [ids[1]])
    want_state = R.accumulate(_as_batch([dicts[1]], [ids[1]]), table, max_dets=longest)
    got = ap.state()
    assert all(got[k].tobytes() == want_state[k].tobytes() for k in KEYS)
    assert model.eval_results(use_07_metric=True)["hand"]["ap"] == R.compute(want_state, table["npos_hand"], table["npos_obj"], True)["hand"]["ap"]
    # forward is untouched: the same dicts, and targets are still refused
    with torch.inference_mode():
        again = model([rgb[0]])[0]
    assert all(torch.equal(again[k], dicts[0][k]) for k in dicts[0])
    with pytest.raises(NotImplementedError):
        model([rgb[0]], targets=[{}])
