"""The detector evaluation's rule (tests/ap_ref.py) against the imported reference's numbers
(tests/golden/det_ap.npz, made by tests/golden/make_golden_ap.py from lib/datasets/voc_eval.py), the file round trip's identity
against Python's own formatting, and the package's host side (hn_amd.metrics.compute_ap, flatten_recs, DetectionAP's merge and
refusals; the C entry's argument checks) -- all without a GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import ap_cases
import ap_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "det_ap.npz")


def _golden_recs(g):
    recs = {str(name): [] for name in g["image_index"]}
    for image, name, bbox, f, ob in zip(g["rec_image"], g["rec_name"], g["rec_bbox"], g["rec_fields"], g["rec_objectbbox"]):
        recs[str(image)].append({"name": str(name), "bbox": [int(v) for v in bbox], "difficult": int(f[0]), "handstate": int(f[1]),
                                 "leftright": int(f[2]), "objectbbox": [float(v) for v in ob] if f[3] else None})
    return recs, [str(n) for n in g["image_index"]]


def _golden_batch(g):
    return {k: g[k] for k in ("boxes", "scores", "labels", "sides", "contacts", "dxdymags", "count", "image_ids")}


@pytest.fixture(scope="module")
def golden_rule(golden):
    """the rule on the golden's inputs, computed once: (table, state)"""
    recs, names = _golden_recs(golden)
    table = R.table_from_recs(recs, names)
    return table, R.accumulate(_golden_batch(golden), table, max_dets=8)


def test_the_golden_holds_every_kind_but_the_ties(golden):
    kinds = set(str(k) for k in golden["kinds"])
    want = set(k.__name__ for k in ap_cases.KINDS) - set(ap_cases.TIE_KINDS)
    assert want <= kinds and not kinds & set(ap_cases.TIE_KINDS) and len(golden["image_index"]) >= 12
    # the condition that frees the reference's result from its sort's tie order: distinct rounded scores within each class
    for label in (1, 2):
        shown = []
        for n in range(golden["count"].shape[0]):
            for k in range(int(golden["count"][n])):
                if golden["scores"][n, k] > np.float32(0.1) and golden["labels"][n, k] == label:
                    shown.append(format(golden["scores"][n, k], ".3f"))
        assert len(shown) > 8 and len(set(shown)) == len(shown)


@pytest.mark.parametrize("use_07", [False, True], ids=["envelope", "11-point"])
def test_the_rule_equals_the_reference_on_the_golden(golden, golden_rule, use_07):
    """rec and prec are the cumulative TP over npos and over TP + FP: equal arrays are equal TP and FP flags in the reference's
    order; ap is the same float64, the host part being the same numpy operations in the same order (no bound needed: measured 0)."""
    table, state = golden_rule
    got = R.compute(state, table["npos_hand"], table["npos_obj"], use_07_metric=use_07)
    tag = "07" if use_07 else "10"
    for name in R.NAMES:
        rec, prec, ap = golden[f"rec_{tag}_{name}"], golden[f"prec_{tag}_{name}"], float(golden[f"ap_{tag}_{name}"])
        assert got[name]["rec"].shape == rec.shape and rec.shape[0] > 0, name
        assert np.array_equal(got[name]["rec"], rec), name
        assert np.array_equal(got[name]["prec"], prec), name
        print(name, tag, "ap", got[name]["ap"], "reference", ap, "difference", got[name]["ap"] - ap)
        assert got[name]["ap"] == ap, name
    assert got["mean_ap"] == float(np.mean([float(golden[f"ap_{tag}_targetobject"]), float(golden[f"ap_{tag}_hand"])]))
    # the tables differ from one another: every constraint costs something on this set
    aps = [got[n]["ap"] for n in R.NAMES[1:]]
    assert aps[0] > max(aps[1:4]) and min(aps[1:4]) > aps[4] > 0.0


def test_the_file_round_trip_is_one_rint_and_one_division():
    """float(format(x, '.1f')) == rint(double(x) * 10) / 10 and float(format(x, '.3f')) == rint(double(x) * 1000) / 1000 for a
    float32 x: over 2 x 520 000 seeded values of the ranges the evaluation sees, their neighbours in float32, and EVERY half-way
    case of the range -- x * 10 ends in .5 exactly when x is an odd number of quarters, x * 1000 when it is an odd number of
    sixteenths (the other factors of 20 and 2000 are odd) -- where Python's formatting rounds half to even, as rint does."""
    rng = np.random.RandomState(20261020)
    quarters = (np.arange(-4 * 4096, 4 * 4096 + 1, 2) + 1).astype(np.float64) / 4.0           # all odd quarters in +-4096
    coords = np.concatenate([rng.uniform(-200, 4096, 300000), rng.uniform(-1e6, 1e6, 100000), rng.uniform(-2, 2, 100000),
                             rng.uniform(0, 1e-3, 20000)]).astype(np.float32)
    coords = np.concatenate([coords, np.nextafter(coords[:50000], np.float32(np.inf)), quarters.astype(np.float32),
                             np.nextafter(quarters.astype(np.float32), np.float32(np.inf)),
                             np.nextafter(quarters.astype(np.float32), np.float32(-np.inf))])
    sixteenths = (np.arange(-16 * 64, 16 * 64 + 1, 2) + 1).astype(np.float64) / 16.0          # all odd sixteenths in +-64
    small = np.concatenate([rng.uniform(0, 1, 300000), rng.uniform(-64, 64, 200000), rng.uniform(0, 1e-3, 20000)]).astype(np.float32)
    small = np.concatenate([small, np.nextafter(small[:50000], np.float32(np.inf)), sixteenths.astype(np.float32),
                            np.nextafter(sixteenths.astype(np.float32), np.float32(np.inf)),
                            np.nextafter(sixteenths.astype(np.float32), np.float32(-np.inf)),
                            np.array([0.8125, 0.4375, 0.1, 0.0005, 0.0015, 1.0], np.float32)])
    assert coords.shape[0] + small.shape[0] >= 1000000
    assert np.array_equal(quarters.astype(np.float32).astype(np.float64), quarters)           # the half-way cases are float32 values
    for values, spec, rule in ((coords, ".1f", R.file_1f), (small, ".3f", R.file_3f)):
        want = np.array([float(format(x, spec)) for x in values.tolist()], np.float64)        # (tolist: the exact value as a double)
        got = rule(values)
        assert np.array_equal(got, want), (spec, values[got != want][:5])
    # the three the issue names, through the float32 add of the file writer
    assert R.file_3f(np.float32(0.8125)) == 0.812
    assert R.file_1f(np.float32(9.25) + np.float32(1.0)) == 10.2 and R.file_1f(np.float32(9.75) + np.float32(1.0)) == 10.8


@pytest.mark.parametrize("shape", ap_cases.SHAPES, ids=lambda s: "N%d-cap%d-G%d" % s)
def test_the_cases_hold_their_kinds_and_the_host_part_equals_the_rules(shape):
    from hn_amd import metrics
    case = ap_cases.cases(shape)
    assert set(ap_cases.kinds_that_fit(shape)) <= set(case["kinds"])
    if shape[1] >= 4 and shape[2] >= 2:
        assert set(k.__name__ for k in ap_cases.KINDS) <= set(case["kinds"])                   # every kind, from (3, 5, 2) on
    table = R.table_from_recs(case["recs"], case["image_index"])
    state = None
    for batch in case["batches"]:
        state = R.accumulate(batch, table, state, max_dets=case["cap"])
    assert int(state["overflow"][0]) == 0 and state["fed"].tolist() == [1] * (table["num_images"] - 1) + [0]
    for use_07 in (False, True):
        want = R.compute(state, table["npos_hand"], table["npos_obj"], use_07)
        got = metrics.compute_ap(state, table["npos_hand"], table["npos_obj"], use_07)
        assert list(got) == list(want)
        for name in R.NAMES:
            assert got[name]["ap"] == want[name]["ap"] or (np.isnan(got[name]["ap"]) and np.isnan(want[name]["ap"]))
            assert np.array_equal(got[name]["rec"], want[name]["rec"]) and np.array_equal(got[name]["prec"], want[name]["prec"])
        assert got["mean_ap"] == want["mean_ap"] and got["npos"] == want["npos"] and got["fed"] == want["fed"]
    assert tuple(metrics.AP_NAMES) == R.NAMES
    # one batch of everything, and the batches in reverse: the same bytes
    for batches in ([ap_cases.concat(case["batches"])], case["batches"][::-1]):
        again = None
        for batch in batches:
            again = R.accumulate(batch, table, again, max_dets=case["cap"])
        assert all(again[k].tobytes() == state[k].tobytes() for k in state)


def test_the_kinds_do_what_their_names_say():
    """the rule's verdicts on (3, 5, 2), record by record: (score in thousandths, TP bits, FP bits) with the tables '', handstate,
    handside, objectbbox, all as bits 0..4"""
    case = ap_cases.cases((3, 5, 2))
    table = R.table_from_recs(case["recs"], case["image_index"])
    state = None
    for batch in case["batches"]:
        state = R.accumulate(batch, table, state, max_dets=5)
    def records(key, kind, nth=0):
        image = [i for i, k in enumerate(case["kinds"]) if k == kind][nth]
        return [(int(w) & 1023, (int(w) >> R.TP_SHIFT) & 31, (int(w) >> R.FP_SHIFT) & 31) for w in state[key][image] if w & R.VALID]
    assert records("hand", "no_detections") == [] and records("obj", "objects_no_hand") == []   # the drop rule
    assert records("hand", "no_ground_truth") == [(900, 0, 31)] and records("obj", "no_ground_truth") == [(800, 0, 1)]
    assert records("hand", "difficult_hand") == [(900, 0, 0)]
    assert records("hand", "taken_twice") == [(900, 31, 0), (800, 0, 31), (700, 0, 31)]
    assert records("hand", "overlap_half") == [(900, 0, 31)]
    assert records("hand", "equal_overlap") == [(900, 31, 0), (800, 0, 31)]                      # the first box both times
    assert records("hand", "equal_distance") == [(950, 31, 0)]                                   # the first object
    assert records("hand", "state0_with_objects") == [(900, 31, 0)] and records("hand", "both_absent") == [(900, 31, 0)]
    assert records("hand", "wrong_state") == [(900, 0b01101, 0b10010)]
    assert records("hand", "wrong_side") == [(900, 0b01011, 0b10100)]
    for kind in ("wrong_object", "object_iou_half", "object_only_in_gt", "object_only_in_det"):
        assert records("hand", kind) == [(900, 0b00111, 0b11000)], kind
    assert records("hand", "low_score") == [(900, 31, 0)] and records("obj", "low_score") == []
    assert records("hand", "other_labels") == [(900, 31, 0)] and records("obj", "other_labels") == []
    assert records("hand", "halfway") == [(812, 0, 31), (438, 0b01101, 0b10010)]
    assert sorted(records("hand", "equal_scores_across_images", 0) + records("hand", "equal_scores_across_images", 1)) == [(900, 0, 31), (900, 31, 0)]
    assert [r[1:] for r in records("hand", "full_capacity")] == [(31, 0)] + [(0, 31)] * 4
    assert records("hand", "association_far") == [(970, 31, 0)]
    assert records("obj", "object_class_mix") == [(900, 1, 0), (850, 0, 1), (800, 0, 0), (700, 0, 1)]


def test_from_recs_flattens_the_cache_as_the_rule_does():
    import torch
    from hn_amd import metrics, ops
    case = ap_cases.cases((3, 5, 2))
    want = R.table_from_recs(case["recs"], case["image_index"])
    flat = metrics.flatten_recs(case["recs"], case["image_index"])
    for k, v in flat.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), k
    ap = metrics.DetectionAP.from_recs(case["recs"], case["image_index"], device="cpu", max_dets=7)
    assert (ap.table.num_images, ap.table.npos_hand, ap.table.npos_obj) == (want["num_images"], want["npos_hand"], want["npos_obj"])
    assert ap.table.hand_obj.dtype == torch.float64 and ap.table.hand_box.dtype == torch.int32
    assert np.array_equal(ap.table.hand_meta.numpy(), want["hand_meta"]) and ap.state()["hand"].shape == (want["num_images"], 7)
    same = metrics.DetectionAP("cpu", case["recs"], case["image_index"])                        # the dict itself is accepted too
    assert same.max_dets == 100 and np.array_equal(same.table.obj_box.numpy(), want["obj_box"])
    # refusals: a 65th box of a class, a fractional bbox, a wrong number of names, a state beyond the memory bound
    crowd = {"a": [ap_cases.gt_hand(ap_cases.B)] * 65}
    with pytest.raises(ValueError, match="65 hand boxes"):
        metrics.DetectionAP.from_recs(crowd, ["a"], device="cpu")
    with pytest.raises(ValueError, match="four integers"):
        metrics.flatten_recs({"a": [ap_cases.gt_hand([1.5, 2, 3, 4])]}, ["a"])
    with pytest.raises(ValueError, match="names in image_index"):
        metrics.DetectionAP("cpu", flat, case["image_index"][:-1])
    with pytest.raises(ValueError, match="num_images \\* max_dets"):
        ops.det_ap_state(1 << 20, 129, "cpu")
    with pytest.raises(ValueError, match="num_images \\* max_dets"):
        ops.det_ap_state(3, 0, "cpu")
    with pytest.raises(ValueError, match="rise from 0"):
        ops.det_ap_table([0, 2], np.zeros((1, 4)), np.zeros((1, 4)), np.zeros((1, 4)), [0, 0], np.zeros((0, 4)), [], "cpu")
    st = ops.det_ap_state(3, 5, "cpu")
    assert st.flat.dtype == torch.int32 and st.flat.numel() == 2 * 15 + 3 + 1 and st.hand.data_ptr() == st.flat.data_ptr()
    with pytest.raises(RuntimeError, match="must live on the GPU"):                              # no CPU fall-back
        ap.update(ops.alloc_detections(1, 4, "cpu"), torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 4, 3)),
                  torch.zeros((1,), dtype=torch.int32))


def test_merge_of_two_disjoint_shards_equals_one_pass_and_bad_states_raise():
    from hn_amd import metrics
    case = ap_cases.cases((2, 65, 3))
    table = R.table_from_recs(case["recs"], case["image_index"])
    whole, shards = None, [None, None]
    for i, batch in enumerate(case["batches"]):
        whole = R.accumulate(batch, table, whole, max_dets=65)
        shards[i % 2] = R.accumulate(batch, table, shards[i % 2], max_dets=65)
    ap = metrics.DetectionAP.from_recs(case["recs"], case["image_index"], device="cpu", max_dets=65)
    ap.merge(shards[0])
    other = metrics.DetectionAP.from_recs(case["recs"], case["image_index"], device="cpu", max_dets=65)
    other.merge(shards[1])
    ap.merge(other)
    got = ap.state()
    assert all(got[k].tobytes() == whole[k].tobytes() for k in whole)
    want = R.compute(whole, table["npos_hand"], table["npos_obj"])
    res = ap.compute()
    assert all(res[n]["ap"] == want[n]["ap"] for n in R.NAMES) and res["fed"] == table["num_images"] - 1
    assert res["npos"] == {"targetobject": table["npos_obj"], "hand": table["npos_hand"]}
    with pytest.raises(ValueError, match="does not fit"):
        ap.merge(R.new_state(table["num_images"], 64))
    # a doubly fed image
    ap.merge(shards[1])
    with pytest.raises(ValueError, match="fed 2 times"):
        ap.compute()
    with pytest.raises(ValueError, match="fed more than once"):
        R.compute(ap.state(), 1, 1)
    ap.reset()
    assert not ap.state()["hand"].any() and ap.compute()["fed"] == 0 and ap.compute()["hand"]["ap"] == 0.0
    # an overflow: the dedicated case, 65 hand records of one image into 64 places; and an image id outside the table
    case = ap_cases.cases(ap_cases.OVERFLOW_SHAPE)
    small = None
    for batch in case["batches"]:
        small = R.accumulate(batch, table, small, max_dets=ap_cases.OVERFLOW_MAX_DETS)
    assert int(small["overflow"][0]) == 1 and all(small[k][:, :64].tobytes() == whole[k][:, :64].tobytes() for k in ("hand", "obj"))
    for fn in (lambda: metrics.compute_ap(small, 1, 1), lambda: R.compute(small, 1, 1)):
        with pytest.raises(ValueError, match="did not fit|overflowed"):
            fn()
    stray = dict(case["batches"][0], image_ids=np.array([-1, table["num_images"]], np.int32))
    lost = R.accumulate(stray, table, max_dets=65)
    assert int(lost["overflow"][0]) == 2 and not lost["hand"].any() and not lost["fed"].any()
    with pytest.raises(ValueError, match="did not fit"):
        metrics.compute_ap(lost, 1, 1)


def test_the_c_entry_checks_its_arguments():
    from hn_amd import _lib
    lib = _lib.load()
    P = 0x10000
    names = ["boxes", "scores", "labels", "sides", "count", "contacts", "dxdymags", "image_ids", "n", "cap", "hand_off", "hand_box",
             "hand_meta", "hand_obj", "hand_total", "obj_off", "obj_box", "obj_diff", "obj_total", "images", "hand_label",
             "object_label", "score_min", "ovthresh", "hand", "obj", "fed", "overflow", "max_dets", "stream"]
    assert len(names) == len(_lib.SIGNATURES["hn_det_ap_accumulate_f32"][1])

    def call(**kw):
        a = {k: P for k in names}
        a.update(n=0, cap=4, hand_total=1, obj_total=1, images=3, hand_label=2, object_label=1, score_min=0.1, ovthresh=0.5,
                 max_dets=5, stream=None)
        a.update(kw)
        return lib.hn_det_ap_accumulate_f32(*[a[k] for k in names])

    refusals = [(dict(n=-1), b"n = -1"), (dict(cap=-2), b"cap = -2"), (dict(images=0), b"images = 0"), (dict(max_dets=0), b"max_dets = 0"),
                (dict(images=1 << 20, max_dets=129), b"at most 2^27"), (dict(n=1 << 20, cap=257), b"at most 2^28"),
                (dict(hand_total=-1), b"hand_total = -1"), (dict(hand_label=1), b"hand_label == object_label"),
                (dict(score_min=1.0), b"score_min"), (dict(score_min=-0.5), b"score_min"), (dict(ovthresh=float("nan")), b"NaN"),
                (dict(hand_obj=P + 4), b"aligned to 8"), (dict(hand=P + 2), b"aligned to 4"), (dict(obj_off=P + 1), b"aligned to 4"),
                (dict(hand_box=None), b"non-empty ground-truth table"), (dict(obj_diff=None), b"non-empty ground-truth table")]
    refusals += [(dict([(k, None)]), b"null pointer") for k in ("hand_off", "obj_off", "hand", "obj", "fed", "overflow")]
    for kw, word in refusals:
        assert call(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_det_ap_accumulate_f32: ") and word in err, (kw, err)
    # an empty batch is a successful no-op, with or without the batch's pointers, and with empty tables
    assert call() == 0 and call(boxes=None, scores=None, count=None, image_ids=None) == 0
    assert call(hand_total=0, hand_box=None, hand_meta=None, hand_obj=None, obj_total=0, obj_box=None, obj_diff=None) == 0


def test_the_drop_in_is_opt_in():
    from fcos_utils.fcos import FCOS
    assert list(inspect.signature(FCOS.device_metrics).parameters)[:3] == ["self", "annotations", "image_index"]
    net = FCOS(num_classes=3)
    assert net._detection_ap is None
    for call in (lambda: net.eval_step([], []), lambda: net.eval_results()):
        with pytest.raises(RuntimeError, match="call device_metrics"):
            call()
    with pytest.raises(RuntimeError, match="ext heads"):
        FCOS(num_classes=3, ext=False).device_metrics({}, [])
    with pytest.raises(NotImplementedError):                                                    # forward keeps raising on targets
        net.eval()(images=[], targets=[{}])
