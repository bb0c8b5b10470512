#!/usr/bin/env python3
"""The output layers of a torch-built detector on the HIP kernels, end to end: per level, a torch conv2d tower layer (+ ReLU) in
channels_last -> three hn_amd.autograd.ThinConv3x3Levels heads (forward: ops.conv3x3_thin_levels; backward: one
ops.conv3x3_thin_backward_levels call each) -> hn_amd.criterion.FCOSCriterion -> sum(losses).backward() -> one SGD step on the
heads' AND the tower's weights.  Prints the six losses for three steps.  (With torch heads instead: examples/fcos_head_grads_demo.py.)

A conv2d output [N,C,h,w] in channels_last memory format is [N,h,w,C] in memory: permute(0, 2, 3, 1) is a contiguous view in the
layout the heads take.  The heads apply the ReLU on the regressions and on the ext (mag, dx, dy) themselves (relu_cols) and mask
the gradient the way torch does.  One weight per head is shared over the levels, as in the reference.

    python examples/fcos_output_grads_demo.py [--images 2] [--steps 3] [--lr 1e-2]
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

from hn_amd import ops  # noqa: E402
from hn_amd.autograd import ThinConv3x3Levels  # noqa: E402
from hn_amd.criterion import FCOSCriterion  # noqa: E402

CLASSES, STRIDES, SIZES = 3, (8, 16, 32), ((40, 36), (20, 18), (10, 9))     # a 320 x 288 canvas


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-2)
    args = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda"
    feats = [torch.randn((args.images, 32, h, w), device=dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    tower = torch.nn.Conv2d(32, 64, 3, padding=1).to(dev).to(memory_format=torch.channels_last)
    heads = torch.nn.ModuleDict({"cls_lr": ThinConv3x3Levels(64, CLASSES + 2), "reg_ctr": ThinConv3x3Levels(64, 5, relu_cols=4),
                                 "ext": ThinConv3x3Levels(64, 8, relu_cols=3)}).to(dev)
    one = {"boxes": torch.tensor([[80.0, 70, 160, 170], [200, 40, 232, 72]]), "labels": torch.tensor([1, 2]),
           "box_info": torch.tensor([[3.0, 1.0, 0.5, 0.06, -0.08], [1.0, 0.0, 0.25, -0.1, 0.0]])}
    targets = ops.pack_fcos_targets([one] * args.images, (1.0, 1.0), num_classes=CLASSES, ext=True, device=dev)
    crit = FCOSCriterion(CLASSES, STRIDES, ext=True)
    opt = torch.optim.SGD(list(heads.parameters()) + list(tower.parameters()), lr=args.lr)
    for step in range(args.steps):
        opt.zero_grad()
        acts = [nhwc(torch.relu(tower(f))) for f in feats]          # [N,h,w,64] per level: what the heads read
        losses, fg = crit(heads["cls_lr"](acts), heads["reg_ctr"](acts), targets, ext=heads["ext"](acts))
        sum(losses.values()).backward()
        opt.step()
        print(f"step {step}: fg {int(fg.sum())}, " + ", ".join(f"{k} {float(v.detach()):.4f}" for k, v in losses.items()))


if __name__ == "__main__":
    main()
