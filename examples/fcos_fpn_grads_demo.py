#!/usr/bin/env python3
"""Fine-tuning the FCOS head and the FPN on a frozen ResNet-34, on the HIP kernels end to end: FCOS.fpn_grads(assign=True) computes
the criterion on the detector's own heads and its backward through the output convolutions, the four tower layers and the FPN (the
3x3 output convolutions, the top-down read, the 1x1 laterals) and sets .grad of every parameter outside the
ResNet body; torch.optim.SGD steps them; refresh_fpn(), refresh_towers() and refresh_outputs() copy the new values into the engine's
existing tensors.  Prints the losses for a few steps.

    python examples/fcos_fpn_grads_demo.py [--steps 3] [--lr 1e-3]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "handnet-pipeline_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from fcos_utils.fcos import FCOS  # noqa: E402
from hn_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()
    model = FCOS(num_classes=3, ext=True).cuda().eval()
    frame = synth.make_rgb(1, seed=1000).cuda()[0]
    targets = [{"boxes": torch.tensor([[100.0, 100, 130, 136], [300, 200, 360, 270]]), "labels": torch.tensor([1, 2]),
                "box_info": torch.tensor([[1.0, 0.0, 0.5, 0.06, -0.08], [3.0, 1.0, 0.2, 0.0, 0.1]])}]
    trained = [p for k, p in model.named_parameters() if k.startswith("head.") or k.startswith("backbone.fpn.")]
    opt = torch.optim.SGD(trained, lr=args.lr)
    for step in range(args.steps):
        with torch.inference_mode():
            losses, fg, grads = model.fpn_grads([frame], targets, assign=True)
        opt.step()
        model.refresh_fpn().refresh_towers().refresh_outputs()
        print(f"step {step}: fg {int(fg.sum())}, {len(grads)} gradients, "
              + ", ".join(f"{k} {float(v):.4f}" for k, v in losses.items()))


if __name__ == "__main__":
    main()
