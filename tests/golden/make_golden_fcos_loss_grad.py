#!/usr/bin/env python3 -B
"""Golden vectors for the FCOS criterion's backward by IMPORTING the reference.

Runs only in the build container (needs the reference checkout make_golden_fcos.py points at).  The function under test is the
reference's own `FCOSHead.compute_loss` (fcos_utils/fcos.py:44-178) in float64 under torch's autograd, with the float32
`matched_idxs` its `FCOS.compute_loss` gives; the shim, the stand-in `sigmoid_focal_loss` and `in_float64` are
make_golden_fcos_loss.py's, imported.  The leaves are the seeded head values as ops.fcos_loss receives them, BEFORE the
reference's own normalisation of (dx, dy) (fcos.py:301-303), so the chain through `normalize` is the reference's.

    python -B tests/golden/make_golden_fcos_loss_grad.py      ->  tests/golden/fcos_loss_grad.npz

The differentiated scalar is sum_k w_k loss_dict[k] for the two upstream settings of tests/fcos_loss_grad_cases.py.
  g1: tests/fcos_loss_cases.py's golden-1; every foreground row and every ROW_STRIDE-th other row of each image (`g1_rows`)
  g2: golden-2 in full
  g3: tests/fcos_loss_grad_cases.py's handmade non-smooth points, in full
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
from make_golden_fcos_loss import in_float64, sigmoid_focal_loss  # noqa: E402
import fcos_loss_cases as lc  # noqa: E402
import fcos_loss_grad_cases as gc  # noqa: E402
import fcos_loss_ref as fr  # noqa: E402

ROW_STRIDE = 37


def heads(case):
    if case.name == "g3":
        return gc.g3_heads_flat()
    return lc.heads_flat(case.seed, case.n, lc.points(case), case.num_classes, case.ext)


def head_outputs(case, cls, reg, ex):
    """the reference's head_outputs dict from the leaves; hand_dxdy through the head's own normalisation (fcos.py:301-303)"""
    c = case.num_classes
    out = {"cls_logits": cls[..., :c], "hand_lr": cls[..., c:], "bbox_regression": reg[..., :4], "bbox_ctrness": reg[..., 4:]}
    if case.ext:
        sub = 0.1 * torch.nn.functional.normalize(ex[..., 1:3], p=2, dim=2)
        out["hand_dxdy"] = torch.cat([ex[..., 0:1], sub], dim=2)
        out["hand_contact_state"] = ex[..., 3:]
    return out


def main():
    install_fcos_shim()
    sys.modules["torchvision.ops"].sigmoid_focal_loss = sigmoid_focal_loss
    from fcos_utils.fcos import FCOS                      # the reference's own
    out = {"torch": np.array(torch.__version__)}
    for tag, name in gc.GOLDEN.items():
        case = gc.BY_NAME[name]
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
        np_heads = heads(case)
        with torch.no_grad():
            model.compute_loss(targets, head_outputs(case, *[torch.from_numpy(t) if t is not None else None for t in np_heads]),
                               anchors, napl)
        matched = recorded[-1]
        t64 = [{"boxes": t["boxes"].double(), "labels": t["labels"], "box_info": t["box_info"].double()} for t in targets]
        a64 = [a.double() for a in anchors]
        m_np = torch.stack(matched).numpy().astype(np.int32)
        out[f"{tag}_matched"] = m_np
        rows = None
        if tag == "g1":
            keep = m_np >= 0
            keep[:, ::ROW_STRIDE] = True
            rows = np.argwhere(keep).astype(np.int32)
            out["g1_rows"] = rows
        for u, up in enumerate(gc.UPSTREAMS):
            leaves = [torch.from_numpy(t).double().requires_grad_(True) if t is not None else None for t in np_heads]
            d = in_float64(inner, t64, head_outputs(case, *leaves), a64, matched)
            assert list(d) == list(fr.KEYS[:len(d)]) and len(d) == (6 if case.ext else 4), list(d)
            w = [1.0] * 6 if up is None else list(up)
            sum(wk * v for wk, v in zip(w, d.values())).backward()
            for key, leaf in zip(("d_cls", "d_reg", "d_ext"), leaves):
                if leaf is None:
                    continue
                g = leaf.grad.numpy()
                assert g.dtype == np.float64 and np.isfinite(g).all()
                out[f"{tag}_up{u}_{key}"] = g[rows[:, 0], rows[:, 1]] if rows is not None else g
        print(tag, "foreground", [int((m >= 0).sum()) for m in matched], "rows", None if rows is None else len(rows))
    np.savez_compressed(HERE / "fcos_loss_grad.npz", **out)
    print("wrote", HERE / "fcos_loss_grad.npz", (HERE / "fcos_loss_grad.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
