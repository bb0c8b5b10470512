"""MPJPE, PCK and AUC of a hand-pose evaluation, accumulated on the device.

What the DexYCB toolkit's `HPEEvaluator.evaluate` reports for an epoch's text file (dex_ycb_toolkit/hpe_eval.py:198-265: three
`EvalUtil` accumulators -- absolute, root-relative, Procrustes-aligned through `align_w_scale` -- and `get_measures(0, 50, 100)`
of each), without the toolkit and without a host round trip per batch: `update` is one launch of `ops.hpe_accumulate` into an
integer state on the device, `compute` copies that state once and does the host's share in fp64.  The state is integer, so the
order of the samples, the batch size and a split over several devices (`merge`) do not change a byte of it.

    m = HPEMetrics("cuda:0")
    for batch in loader:
        m.update(pred_xyz_mm, gt_xyz_mm)          # fp32 [K,21,3] device tensors, camera millimetres; no synchronisation
    results = m.compute()                          # {'absolute': {'mpjpe', 'auc'}, 'root-relative': ..., 'procrustes': ..., 'pck', ...}

The median error is not offered: `evaluate()` computes it and drops it, and a histogram does not hold it.

The detector's evaluation loop has the same end: `DetectionAP` files the verdict of every detection record
on the device, one launch per batch, and `compute_ap` turns the records into the six AP tables of the legacy voc_eval.py.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

NAMES = ("absolute", "root-relative", "procrustes")
Q20 = 1048576.0            # the fixed point of the distance sums: 2^-20 mm


def _trapz(y, x):
    """np.trapz(y, x) along the last axis, written out (numpy 2 renamed it)"""
    return (np.diff(x) * (y[..., 1:] + y[..., :-1]) / 2.0).sum(axis=-1)


def compute(state, thresholds):
    """`EvalUtil.get_measures` for the three tables (tests/hpe_ref.py::compute is the rule; this is its copy inside the package).
    state: hist int64 [3,J,T+1], sum int64 [3,J], n int64 [2] as numpy arrays (a dict or an object with these names).
    -> the evaluator's `results` dict plus pck [3,T] (the mean over the joints), thresholds, fed, skipped.  fed == 0: NaN."""
    get = state.__getitem__ if isinstance(state, dict) else lambda k: getattr(state, k)
    thresholds = np.asarray(thresholds, np.float64).reshape(-1)
    hist, total, n = (np.asarray(get(k), np.int64) for k in ("hist", "sum", "n"))
    fed, skipped = int(n[0]), int(n[1])
    with np.errstate(all="ignore"):
        pck = np.cumsum(hist, axis=2)[:, :, :-1].astype(np.float64) / np.float64(fed)
        mean = (total.astype(np.float64) / Q20) / np.float64(fed)
        auc = _trapz(pck, thresholds) / _trapz(np.ones_like(thresholds), thresholds)
        out = {name: {"mpjpe": float(np.mean(mean[a])), "auc": float(np.mean(auc[a]))} for a, name in enumerate(NAMES)}
        out["pck"] = np.mean(pck, axis=1)
    out["thresholds"] = thresholds
    out["fed"], out["skipped"] = fed, skipped
    return out


class HPEMetrics:
    """The evaluator's accumulator for one device.  thresholds = np.linspace(val_min, val_max, steps) on the host (the toolkit's
    0, 50, 100: millimetres), uploaded once."""

    def __init__(self, device, joints: int = 21, val_min: float = 0.0, val_max: float = 50.0, steps: int = 100):
        self.device = torch.device(device)
        self.joints, self.steps = int(joints), int(steps)
        if not np.isfinite([val_min, val_max]).all() or not float(val_min) <= float(val_max):
            raise ValueError(f"thresholds from {val_min} to {val_max}: finite and non-decreasing")
        if self.device.type != "cuda":
            raise ValueError(f"HPEMetrics accumulates on a GPU, got {self.device}")
        self._state = ops.hpe_state(self.joints, self.steps, self.device)              # (checks joints and steps)
        self.thresholds = np.linspace(float(val_min), float(val_max), self.steps)
        self._thresholds = torch.from_numpy(self.thresholds).to(self.device)

    def update(self, pred_xyz_mm, gt_xyz_mm, valid=None):
        """One batch: fp32 [K,J,3] device tensors in camera millimetres (valid int32 [K], 0 = skip the sample).  One launch on
        the current stream; nothing is copied back and nothing waits."""
        with ops.on_device(self.device):
            ops.hpe_accumulate(pred_xyz_mm, gt_xyz_mm, self._thresholds, state=self._state, valid=valid)

    def state(self):
        """The state on the host: {'hist': int64 [3,J,T+1], 'sum': int64 [3,J], 'n': int64 [2]} from ONE device -> host copy."""
        flat = self._state.flat.cpu().numpy()
        a, b = 3 * self.joints * (self.steps + 1), 3 * self.joints
        return {"hist": flat[:a].reshape(3, self.joints, self.steps + 1), "sum": flat[a:a + b].reshape(3, self.joints),
                "n": flat[a + b:]}

    def merge(self, other_state):
        """Adds another accumulator's state (an HPEMetrics, or what its `state()` returned: a shard of the same evaluation)."""
        other = other_state.state() if isinstance(other_state, HPEMetrics) else other_state
        parts = [np.asarray(other[k], np.int64) for k in ("hist", "sum", "n")]
        want = [tuple(p.shape) for p in (self._state.hist, self._state.sum, self._state.n)]
        if [p.shape for p in parts] != want:
            raise ValueError(f"a state of shapes {[p.shape for p in parts]} does not fit this accumulator's {want}")
        flat = np.concatenate([p.reshape(-1) for p in parts])
        self._state.flat.add_(torch.from_numpy(flat).to(self.device))

    def reset(self):
        self._state.flat.zero_()

    def compute(self):
        return compute(self.state(), self.thresholds)


# ---------------------------------------------------------------------------------------------------------------------------
# The detector's evaluation: hand and object AP tables

AP_NAMES = ("targetobject", "hand", "hand+handstate", "hand+handside", "hand+objectbbox", "hand+all")
HAND_NAME, OBJECT_NAME = "hand", "targetobject"        # the two classes of the annotation cache (lower case, as voc_eval compares)


def flatten_recs(recs, image_index):
    """The reference's annotation cache -- {image name: [{name, bbox, difficult, handstate, leftright, objectbbox}, ...]}, what
    voc_eval.py pickles next to the annotations -- as the arrays of `ops.det_ap_table`, the images in `image_index` order (the
    position of a name there is the image id a batch carries).  bbox must hold integers, as parse_rec reads them."""
    hand_off, obj_off = [0], [0]
    hand_box, hand_meta, hand_obj, obj_box, obj_diff = [], [], [], [], []
    for name in image_index:
        for o in recs[name]:
            kind = str(o["name"]).lower()
            if kind not in (HAND_NAME, OBJECT_NAME):
                continue
            box = [int(v) for v in o["bbox"]]
            if len(box) != 4 or any(float(v) != b for v, b in zip(o["bbox"], box)):
                raise ValueError(f"{name}: bbox {o['bbox']} must be four integers")
            if kind == OBJECT_NAME:
                obj_box.append(box)
                obj_diff.append(int(bool(o["difficult"])))
                continue
            ob = o.get("objectbbox")
            hand_box.append(box)
            hand_meta.append([int(bool(o["difficult"])), int(o["handstate"]), int(o["leftright"]), int(ob is not None)])
            hand_obj.append([0.0, 0.0, 0.0, 0.0] if ob is None else [float(v) for v in ob])
        hand_off.append(len(hand_box))
        obj_off.append(len(obj_box))
    return {"hand_off": np.asarray(hand_off, np.int32), "hand_box": np.asarray(hand_box, np.int32).reshape(-1, 4),
            "hand_meta": np.asarray(hand_meta, np.int32).reshape(-1, 4), "hand_obj": np.asarray(hand_obj, np.float64).reshape(-1, 4),
            "obj_off": np.asarray(obj_off, np.int32), "obj_box": np.asarray(obj_box, np.int32).reshape(-1, 4),
            "obj_diff": np.asarray(obj_diff, np.int32).reshape(-1)}


def voc_ap(rec, prec, use_07_metric=False):
    """voc_eval.py:56-87: the 11-point form, or the area under the precision envelope"""
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def _ap_curve(words, tp_bit, fp_bit, npos, use_07_metric):
    w = np.asarray(words, np.int32).reshape(-1)                  # file order: image index, then the rank within the image
    w = w[(w & ops.DET_AP_VALID) != 0]
    confidence = (w & ((1 << ops.DET_AP_SCORE_BITS) - 1)).astype(np.float64) / 1000.0
    tp, fp = ((w >> tp_bit) & 1).astype(np.float64), ((w >> fp_bit) & 1).astype(np.float64)
    if w.shape[0] > 0:
        order = np.argsort(-confidence)                          # as the reference calls it
        tp, fp = tp[order], fp[order]
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    with np.errstate(all="ignore"):
        rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        ap = voc_ap(rec, prec, use_07_metric)
    return {"ap": float(ap), "rec": rec, "prec": prec}


def compute_ap(state, npos_hand, npos_obj, use_07_metric=False):
    """The epoch's end of the detector evaluation (tests/ap_ref.py::compute is the rule; this is its copy inside the package --
    under this name because `compute` above is the hand-pose evaluator's).  state: hand, obj int32 [I,max_dets], fed int32 [I],
    overflow int32 [1] as numpy arrays; npos: the non-difficult ground truths of ALL images of the table, fed or not.
    -> {name: {'ap', 'rec', 'prec'}} for AP_NAMES, plus mean_ap (the two class APs, as _do_python_eval prints it), npos, fed.
    Raises when an image was fed twice (its records were overwritten) or records did not fit (overflow)."""
    get = state.__getitem__ if isinstance(state, dict) else lambda k: getattr(state, k)
    hand, obj, fed, overflow = (np.asarray(get(k), np.int32) for k in ("hand", "obj", "fed", "overflow"))
    if fed.size and int(fed.max()) > 1:
        raise ValueError(f"image {int(np.argmax(fed))} was fed {int(fed.max())} times: every image once per evaluation")
    if int(overflow.reshape(-1)[0]) > 0:
        raise ValueError(f"{int(overflow.reshape(-1)[0])} records did not fit the state (more than max_dets = {hand.shape[1]} records "
                         "of a class in an image, a score above 1, or an image id outside the table)")
    out = {AP_NAMES[0]: _ap_curve(obj, ops.DET_AP_TP_SHIFT, ops.DET_AP_FP_SHIFT, npos_obj, use_07_metric)}
    for t in range(5):
        out[AP_NAMES[1 + t]] = _ap_curve(hand, ops.DET_AP_TP_SHIFT + t, ops.DET_AP_FP_SHIFT + t, npos_hand, use_07_metric)
    out["mean_ap"] = float(np.mean([out[AP_NAMES[0]]["ap"], out[AP_NAMES[1]]["ap"]]))
    out["npos"] = {OBJECT_NAME: int(npos_obj), HAND_NAME: int(npos_hand)}
    out["fed"] = int(fed.sum())
    return out


class DetectionAP:
    """The detector evaluation's accumulator for one device: what `evaluate()` of trainval_net_fcos.py and the legacy voc_eval.py
    report -- AP of targetobject, of hand, and of hand under the handstate, handside, objectbbox and all constraints -- without
    dicts, text files or a host round trip per batch.

        ap = DetectionAP.from_recs(recs, image_index, device="cuda:0")      # recs: the annotation cache dict
        for images, ids in loader:
            det, _, contacts, dxdymags = engine.detect_ext(images)
            ap.update(det, contacts, dxdymags, ids)                         # ids int32 [N] on the device; no synchronisation
        results = ap.compute()                                               # {'hand': {'ap', 'rec', 'prec'}, ..., 'mean_ap'}

    annotations: the flattened cache (`flatten_recs`), or the cache dict itself.  image_index: the image names, position = id.
    The state is position-addressed and integer: any order of the images, any batch size and any split over devices give the same
    bytes; `merge` adds the states of shards that were fed disjoint images (a DetectionAP on "cpu" can collect them: it merges,
    resets and computes, and has no `update` -- there is no CPU kernel)."""

    def __init__(self, device, annotations, image_index, max_dets: int = 100, hand_label: int = 2, object_label: int = 1,
                 score_min: float = 0.1, ovthresh: float = 0.5):
        self.device = torch.device(device)       # ("cpu": a host-side accumulator that merges shards and computes; `update` refuses)
        self.image_index = list(image_index)
        if not isinstance(annotations, dict):
            raise TypeError("annotations: the annotation cache dict, or what flatten_recs returned")
        if "hand_off" not in annotations:
            annotations = flatten_recs(annotations, self.image_index)
        self.rule = dict(hand_label=int(hand_label), object_label=int(object_label), score_min=float(score_min), ovthresh=float(ovthresh))
        self.max_dets = int(max_dets)
        keys = ("hand_off", "hand_box", "hand_meta", "hand_obj", "obj_off", "obj_box", "obj_diff")
        self.table = ops.det_ap_table(*(annotations[k] for k in keys), device=self.device)
        if self.table.num_images != len(self.image_index):
            raise ValueError(f"{self.table.num_images} images in the annotations, {len(self.image_index)} names in image_index")
        self._state = ops.det_ap_state(self.table.num_images, self.max_dets, self.device)     # (checks the memory bound)

    @classmethod
    def from_recs(cls, recs, image_index, device="cuda", **options):
        """From the reference's cache dict: name -> list of {name, bbox, difficult, handstate, leftright, objectbbox}."""
        return cls(device, flatten_recs(recs, image_index), image_index, **options)

    def update(self, det, contacts, dxdymags, image_ids):
        """One batch: the detector's `Detections` with the ext heads' contacts and dxdymags, and int32 [N] image ids, all on the
        device.  One launch on the current stream; nothing is copied back and nothing waits."""
        with ops.on_device(self.device):
            ops.det_ap_accumulate(det, contacts, dxdymags, image_ids, self.table, state=self._state, **self.rule)

    def state(self):
        """The state on the host: {'hand', 'obj': int32 [I,max_dets], 'fed': int32 [I], 'overflow': int32 [1]} from ONE copy."""
        flat = self._state.flat.cpu().numpy()
        i, a = self.table.num_images, self.table.num_images * self.max_dets
        return {"hand": flat[:a].reshape(i, self.max_dets), "obj": flat[a:2 * a].reshape(i, self.max_dets),
                "fed": flat[2 * a:2 * a + i], "overflow": flat[2 * a + i:]}

    def merge(self, other_state):
        """Adds another accumulator's state (a DetectionAP, or what its `state()` returned): a shard of the same evaluation that
        was fed OTHER images -- the words of an image nobody else fed are zero, so the sum is the union."""
        other = other_state.state() if isinstance(other_state, DetectionAP) else other_state
        parts = [np.asarray(other[k], np.int32) for k in ("hand", "obj", "fed", "overflow")]
        want = [tuple(p.shape) for p in (self._state.hand, self._state.obj, self._state.fed, self._state.overflow)]
        if [p.shape for p in parts] != want:
            raise ValueError(f"a state of shapes {[p.shape for p in parts]} does not fit this accumulator's {want}")
        flat = np.concatenate([p.reshape(-1) for p in parts])
        self._state.flat.add_(torch.from_numpy(flat).to(self.device))

    def reset(self):
        self._state.flat.zero_()

    def compute(self, use_07_metric: bool = False):
        return compute_ap(self.state(), self.table.npos_hand, self.table.npos_obj, use_07_metric)
