#!/usr/bin/env python3 -B
"""Golden vectors for the FCOS criterion by IMPORTING the reference.

Runs only in the build container (needs the reference checkout make_golden_fcos.py points at).  The functions under test are
the reference's own `FCOS.compute_loss` (fcos_utils/fcos.py:523-570, the matching) and `FCOSHead.compute_loss` (:44-178, the six
terms), with the reference's own AnchorGenerator, BoxLinearCoder and generalized_box_iou_loss.  No backbone runs: the head outputs
are seeded (tests/fcos_loss_cases.py heads_flat, stored as their seed only) and the targets are that file's handmade sets.

    python -B tests/golden/make_golden_fcos_loss.py      ->  tests/golden/fcos_loss.npz

torchvision is not installed: `torchvision.ops.sigmoid_focal_loss` is bound HERE to a stand-in written from torchvision's
published definition (ops/focal_loss.py: ce * (1 - p_t)^gamma * alpha_t, alpha 0.25, gamma 2), so the focal term is "parity
unpinned" like the other torchvision pieces (oracle/__init__.py); everything else is the reference's arithmetic.

Three runs per configuration: float32 throughout (its matched_idxs are recorded by wrapping head.compute_loss); the head's
compute_loss in float64 with those float32 matched_idxs (in_float64); and both again image by image as a batch of one.
  g1: C = 3, ext, levels 40x34 / 20x17 / 10x9 through AnchorGenerator.forward on a 320 x 288 canvas (strides 8 / 16 / 32), N = 3
  g2: C = 2, no ext, levels 5x7 / 3x4 / 2x2, N = 2, image 1 without boxes.  No canvas gives these grids equal strides on both
      axes, so the anchors come from the generator's grid_anchors with strides 8 / 16 / 32 handed in.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

from make_golden_fcos import _ImageList, install_fcos_shim  # noqa: E402
import fcos_loss_cases as lc  # noqa: E402
import fcos_loss_ref as fr  # noqa: E402


def sigmoid_focal_loss(inputs, targets, alpha: float = 0.25, gamma: float = 2, reduction: str = "none"):
    """torchvision.ops.sigmoid_focal_loss as published (a stand-in: unpinned)"""
    p = torch.sigmoid(inputs)
    ce_loss = torch.nn.functional.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce_loss * ((1 - p_t) ** gamma)
    if alpha >= 0:
        alpha_t = alpha * targets + (1 - alpha) * (1 - targets)
        loss = alpha_t * loss
    if reduction == "mean":
        loss = loss.mean()
    elif reduction == "sum":
        loss = loss.sum()
    return loss


def head_outputs(case, dtype):
    """the reference's head_outputs dict from the seeded values; hand_dxdy through the head's own normalisation (fcos.py:301-303)"""
    cls, reg, ex = lc.heads_flat(case.seed, case.n, lc.points(case), case.num_classes, case.ext)
    cls, reg = torch.from_numpy(cls).to(dtype), torch.from_numpy(reg).to(dtype)
    c = case.num_classes
    out = {"cls_logits": cls[..., :c], "hand_lr": cls[..., c:], "bbox_regression": reg[..., :4], "bbox_ctrness": reg[..., 4:]}
    if case.ext:
        ex = torch.from_numpy(ex).to(dtype)
        sub = 0.1 * torch.nn.functional.normalize(ex[..., 1:3], p=2, dim=2)
        out["hand_dxdy"] = torch.cat([ex[..., 0:1], sub], dim=2)
        out["hand_contact_state"] = ex[..., 3:]
    return out


def in_float64(fn, *a):
    """fn(*a) with the reference's `.float()` on the predicted boxes (fcos.py:139, "amp issue") bound to the identity: with it
    the float64 run would round the decoded boxes to float32 and then fail on the mixed dtypes in the GIoU loss"""
    keep = torch.Tensor.float
    torch.Tensor.float = lambda self, *k, **kw: self
    try:
        return fn(*a)
    finally:
        torch.Tensor.float = keep


def main():
    install_fcos_shim()
    sys.modules["torchvision.ops"].sigmoid_focal_loss = sigmoid_focal_loss
    from fcos_utils.fcos import FCOS                      # the reference's own
    out = {}
    for tag, name in lc.GOLDEN.items():
        case = lc.BY_NAME[name]
        model = FCOS(case.num_classes, ext=case.ext).train()
        feats = [torch.zeros((case.n, 1, h, w)) for h, w in case.sizes]
        if tag == "g1":
            anchors = model.anchor_generator(_ImageList(torch.zeros((case.n, 3, 320, 288)), [(320, 288)] * case.n), feats)
        else:
            model.anchor_generator.set_cell_anchors(torch.float32, torch.device("cpu"))
            per_level = model.anchor_generator.grid_anchors([f.shape[-2:] for f in feats],
                                                            [[torch.tensor(s), torch.tensor(s)] for s in case.strides])
            anchors = [torch.cat(per_level) for _ in range(case.n)]
        napl = [h * w for h, w in case.sizes]
        targets = [{"boxes": torch.from_numpy(b.copy()), "labels": torch.from_numpy(l.astype(np.int64)),
                    "box_info": torch.from_numpy(f.copy())} for b, l, f in case.targets]
        recorded = []
        inner = model.head.compute_loss

        def recording(t, h, a, matched):
            recorded.append([m.clone() for m in matched])
            return inner(t, h, a, matched)
        model.head.compute_loss = recording

        def values(d):
            assert list(d) == list(fr.KEYS[:len(d)]) and len(d) == (6 if case.ext else 4), list(d)
            return np.array([float(v) for v in d.values()] + [0.0] * (6 - len(d)), np.float64)

        ho32, ho64 = head_outputs(case, torch.float32), head_outputs(case, torch.float64)
        t64 = [{"boxes": t["boxes"].double(), "labels": t["labels"], "box_info": t["box_info"].double()} for t in targets]
        a64 = [a.double() for a in anchors]
        f32 = values(model.compute_loss(targets, ho32, anchors, napl))
        matched = recorded[-1]
        f64 = values(in_float64(inner, t64, ho64, a64, matched))
        img32, img64 = [], []
        for i in range(case.n):
            one = lambda d: {k: v[i:i + 1] for k, v in d.items()}
            img32.append(values(model.compute_loss(targets[i:i + 1], one(ho32), anchors[i:i + 1], napl)))
            assert torch.equal(recorded[-1][0], matched[i])
            img64.append(values(in_float64(inner, t64[i:i + 1], one(ho64), a64[i:i + 1], matched[i:i + 1])))
        out.update({f"{tag}_seed": np.int64(case.seed), f"{tag}_matched": torch.stack(matched).numpy().astype(np.int32),
                    f"{tag}_f32_losses": f32, f"{tag}_f64_losses": f64, f"{tag}_f32_image_losses": np.stack(img32),
                    f"{tag}_f64_image_losses": np.stack(img64)})
        print(tag, "foreground", [(int((m >= 0).sum())) for m in matched], "f64", f64, "f32 - f64", f32 - f64)
    np.savez_compressed(HERE / "fcos_loss.npz", **out)
    print("wrote", HERE / "fcos_loss.npz")


if __name__ == "__main__":
    main()
