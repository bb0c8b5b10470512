#!/usr/bin/env python3
"""The FCOS criterion under torch-built detector heads: per level, three torch conv2d output layers in channels_last on a random
feature map -> hn_amd.criterion.FCOSCriterion (forward: ops.fcos_loss; backward: one ops.fcos_loss_grad call) ->
sum(losses).backward() -> one SGD step on the heads' weights.  Prints the six losses for three steps.  (The A2J counterpart is
examples/head_grads_demo.py.)

A conv2d output [N,C,h,w] in channels_last memory format is [N,h,w,C] in memory: permute(0, 2, 3, 1) is a contiguous view in the
layout the criterion takes.  The regressions and the ext (mag, dx, dy) are a ReLU's outputs; the ReLU stays in torch, so autograd
masks the criterion's gradient at those outputs.

    python examples/fcos_head_grads_demo.py [--images 2] [--steps 3] [--lr 1e-2]
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
from hn_amd.criterion import FCOSCriterion  # noqa: E402

CLASSES, STRIDES, SIZES = 3, (8, 16, 32), ((40, 36), (20, 18), (10, 9))     # a 320 x 288 canvas


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)


def relu_head(t, cols):
    """relu on the first `cols` channels of an NHWC head"""
    return torch.cat([torch.relu(t[..., :cols]), t[..., cols:]], dim=3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-2)
    args = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda"
    feats = [torch.randn((args.images, 32, h, w), device=dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    heads = torch.nn.ModuleDict({"cls_lr": torch.nn.Conv2d(32, CLASSES + 2, 3, padding=1), "reg_ctr": torch.nn.Conv2d(32, 5, 3, padding=1),
                                 "ext": torch.nn.Conv2d(32, 8, 3, padding=1)}).to(dev).to(memory_format=torch.channels_last)
    one = {"boxes": torch.tensor([[80.0, 70, 160, 170], [200, 40, 232, 72]]), "labels": torch.tensor([1, 2]),
           "box_info": torch.tensor([[3.0, 1.0, 0.5, 0.06, -0.08], [1.0, 0.0, 0.25, -0.1, 0.0]])}
    targets = ops.pack_fcos_targets([one] * args.images, (1.0, 1.0), num_classes=CLASSES, ext=True, device=dev)
    crit = FCOSCriterion(CLASSES, STRIDES, ext=True)
    opt = torch.optim.SGD(heads.parameters(), lr=args.lr)
    for step in range(args.steps):
        opt.zero_grad()
        cls_lr = [nhwc(heads["cls_lr"](f)) for f in feats]
        reg_ctr = [relu_head(nhwc(heads["reg_ctr"](f)), 4) for f in feats]
        ext = [relu_head(nhwc(heads["ext"](f)), 3) for f in feats]
        losses, fg = crit(cls_lr, reg_ctr, targets, ext=ext)
        sum(losses.values()).backward()
        opt.step()
        print(f"step {step}: fg {int(fg.sum())}, " + ", ".join(f"{k} {float(v.detach()):.4f}" for k, v in losses.items()))


if __name__ == "__main__":
    main()
