#!/usr/bin/env python3 -B
"""Golden vectors for the hand-pose evaluator's tables by IMPORTING the reference.

Runs only in the build container (needs /root/reference and scipy).  The functions under test are the DexYCB toolkit's own
`freihand.utils.eval_util.EvalUtil` (feed, get_measures) and `freihand.eval.align_w_scale` with scipy's `orthogonal_procrustes`,
fed exactly as `HPEEvaluator.evaluate` feeds them (dex_ycb_toolkit/hpe_eval.py:198-218).  Only imports that do no arithmetic here
are stubbed (matplotlib, pip -- the file would install what it misses --, open3d, skimage).

    python -B tests/golden/make_golden_hpe.py      ->  tests/golden/hpe_metrics.npz

Two sets of seeded float32 inputs in camera millimetres: hand-like ones (21 joints, 60-120 mm extent, prediction = ground truth
+ noise of 2-40 mm: a PCK curve that is neither all 0 nor all 1) and a few whose prediction is the ground truth rotated, scaled
and REFLECTED.  Two conditions are asserted, not measured: every M = A''^T B'' of the set has a smallest singular value above 1e-3
of its largest (R is then unique, whatever SVD finds it), and no reference pa distance lies within GUARD of a threshold (no PCK
cell depends on the last bits of the alignment).
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.dont_write_bytecode = True
GUARD = 1e-6               # mm; tests/test_hpe_cpu.py checks it against max(1e-6, 1000 x the rule's measured deviation)
HAND_LIKE, MOVED = 48, 8


def _mod(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _no_install(*a, **k):
    raise RuntimeError("the reference asked pip to install something: stub the missing module instead")


def main():
    mpl = _mod("matplotlib", use=lambda *a, **k: None)
    mpl.pyplot = _mod("matplotlib.pyplot")
    pip = _mod("pip", main=_no_install)
    pip._internal = _mod("pip._internal", main=_no_install)
    _mod("open3d")
    sk = _mod("skimage")
    sk.io = _mod("skimage.io")
    sys.path.insert(0, str(REF / "dex-ycb-toolkit"))
    from freihand.eval import align_w_scale                   # the reference's own (real module, stubbed imports)
    from freihand.utils.eval_util import EvalUtil
    from scipy.linalg import orthogonal_procrustes
    import freihand.eval as fe
    assert fe.orthogonal_procrustes is orthogonal_procrustes

    rng = np.random.RandomState(20261019)
    s = HAND_LIKE + MOVED
    gt = np.zeros((s, 21, 3), np.float32)
    pred = np.zeros((s, 21, 3), np.float32)
    reflected = np.zeros((s,), np.int32)
    for i in range(s):
        centre = np.array([rng.uniform(-250, 250), rng.uniform(-250, 250), rng.uniform(350, 950)])
        extent = rng.uniform(60, 120, 3)
        hand = centre + rng.uniform(-0.5, 0.5, (21, 3)) * extent
        gt[i] = hand.astype(np.float32)
        if i < HAND_LIKE:
            noise = rng.uniform(2, 40)                        # mm: the length scale of this sample's error
            pred[i] = (hand + rng.normal(0, noise / np.sqrt(3.0), (21, 3))).astype(np.float32)
        else:
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if (np.linalg.det(q) < 0) != (i % 4 != 3):        # three of four are reflections, the fourth a proper rotation
                q[:, 0] = -q[:, 0]
            reflected[i] = int(np.linalg.det(q) < 0)
            moved = (hand - hand.mean(0)) @ q.T * rng.uniform(0.5, 1.8) + centre + rng.uniform(-80, 80, 3)
            pred[i] = (moved + rng.normal(0, rng.uniform(1, 6), (21, 3))).astype(np.float32)
    assert reflected[HAND_LIKE:].sum() == MOVED - MOVED // 4

    utils = [EvalUtil(), EvalUtil(), EvalUtil()]
    aligned = np.zeros((s, 21, 3), np.float64)
    dist = np.zeros((s, 3, 21), np.float64)
    ratio = np.zeros((s,), np.float64)
    for i in range(s):
        kpt_gt, kpt_pred = gt[i].astype(np.float64), pred[i].astype(np.float64)       # hpe_eval.py:107-108,135: float64
        vis = np.ones_like(kpt_gt[:, 0])
        aligned[i] = align_w_scale(kpt_gt.copy(), kpt_pred.copy())
        utils[0].feed(kpt_gt, vis, kpt_pred)
        utils[1].feed(kpt_gt - kpt_gt[0], vis, kpt_pred - kpt_pred[0])
        utils[2].feed(kpt_gt, vis, aligned[i])
        for a in range(3):
            dist[i, a] = [utils[a].data[j][-1] for j in range(21)]
        # the condition on M (what orthogonal_procrustes factors)
        a1, b1 = kpt_gt - kpt_gt.mean(0), kpt_pred - kpt_pred.mean(0)
        sv = np.linalg.svd((a1 / (np.linalg.norm(a1) + 1e-8)).T @ (b1 / (np.linalg.norm(b1) + 1e-8)), compute_uv=False)
        ratio[i] = sv[-1] / sv[0]
    assert ratio.min() > 1e-3, ratio.min()
    out = dict(gt=gt, pred=pred, reflected=reflected, aligned=aligned, dist=dist, sv_ratio=ratio, guard=np.float64(GUARD))
    for a, name in enumerate(("ab", "rr", "pa")):
        mean, median, auc, pck, thresholds = utils[a].get_measures(0.0, 50.0, 100)
        out.update({f"mean_{name}": np.float64(mean), f"median_{name}": np.float64(median), f"auc_{name}": np.float64(auc),
                    f"pck_{name}": np.asarray(pck, np.float64)})
        # the integer PCK counts per joint and threshold, from the reference's own comparison (eval_util.py:40: data <= threshold)
        out[f"count_{name}"] = np.array([[int((np.array(utils[a].data[j]) <= t).sum()) for t in thresholds] for j in range(21)],
                                        np.int64)
    out["thresholds"] = np.asarray(thresholds, np.float64)
    gap = np.abs(dist[:, 2, :, None] - out["thresholds"][None, None, :]).min()
    assert gap > GUARD, gap
    curve = out["pck_ab"]
    assert 0.0 < curve[10] and curve[10] < 1.0 and curve[-1] > curve[10], curve
    np.savez_compressed(HERE / "hpe_metrics.npz", **out)
    print("wrote", HERE / "hpe_metrics.npz", "smallest sv ratio", float(ratio.min()), "nearest pa distance to a threshold", float(gap),
          "mpjpe", [float(out[f"mean_{n}"]) for n in ("ab", "rr", "pa")], "auc", [float(out[f"auc_{n}"]) for n in ("ab", "rr", "pa")])


if __name__ == "__main__":
    main()
