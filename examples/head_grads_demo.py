#!/usr/bin/env python3
"""The fused A2J criterion under a torch-built head: three torch conv2d output layers in channels_last on a random feature map
-> hn_amd.criterion.A2JCriterion (forward: ops.a2j_loss; backward: one ops.a2j_loss_grad launch) -> total_loss.backward() -> one
SGD step on the heads' weights.  Prints the loss for three steps.

A conv2d output [K,C,fh,fw] in channels_last memory format is [K,fh,fw,C] in memory: permute(0, 2, 3, 1) is a contiguous view
in exactly the layout the criterion takes (channel = anchor * J + joint; the regression head with (h, w) innermost).

    python examples/head_grads_demo.py [--crops 4] [--steps 3] [--lr 1e-3]
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

from hn_amd.criterion import A2JCriterion  # noqa: E402

JOINTS = 21


def nhwc(t):
    """the criterion's layout from a conv2d output (a view when the output already is channels_last)"""
    return t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda"
    features = torch.randn((args.crops, 64, 11, 11), device=dev).contiguous(memory_format=torch.channels_last)
    heads = torch.nn.ModuleDict({"cls": torch.nn.Conv2d(64, 16 * JOINTS, 3, padding=1), "reg": torch.nn.Conv2d(64, 32 * JOINTS, 3, padding=1),
                                 "dep": torch.nn.Conv2d(64, 16 * JOINTS, 3, padding=1)}).to(dev).to(memory_format=torch.channels_last)
    gt = torch.rand((args.crops, JOINTS, 3), device=dev) * torch.tensor([176.0, 176.0, 0.8], device=dev)
    crit = A2JCriterion(joints=JOINTS, stride=16, spatial_factor=0.5, reg_loss_factor=3.0)
    opt = torch.optim.SGD(heads.parameters(), lr=args.lr)
    for step in range(args.steps):
        opt.zero_grad()
        losses, _uvd = crit(nhwc(heads["cls"](features)), nhwc(heads["reg"](features)), nhwc(heads["dep"](features)), gt)
        losses["total_loss"].backward()
        opt.step()
        host = {name: float(v.detach()) for name, v in losses.items()}
        print(f"step {step}: total_loss {host['total_loss']:.4f} (classification {host['classification']:.4f}, "
              f"regression {host['regression']:.4f})")


if __name__ == "__main__":
    main()
