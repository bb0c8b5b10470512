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
