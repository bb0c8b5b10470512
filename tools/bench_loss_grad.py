"""Cost of the A2J criterion's backward on the device (ops.a2j_loss_grad: csrc/a2j_ops.hip a2j_loss_grad_kernel) against the
forward alone and against torch's autograd through a restatement of the criterion.

At each of `--crops` (1 and 64: one hand, and the reference's training batch) three arms run in this process on the same seeded
heads of the model's shape and are timed alternately: `rounds` rounds, each `iters` calls between two device events after `warmup`
calls; a row reports the median per-call time of each arm, each arm's spread (max - min over the rounds) and torch / fused.
  loss        ops.a2j_loss alone (the launch pair of tools/bench_loss.py's op row: the same code, so the same time);
  loss_grad   ops.a2j_loss, then ops.a2j_loss_grad (three launches: the fused forward + backward);
  torch       the criterion restated in torch as the reference writes it (a2j/anchor.py:99-153: a Python loop over the batch,
              softmax, weighted sums, torch.where smooth-L1, means) on the same device tensors, total_loss.backward().  This arm
              lives only in this tool: the product never imports it.
Before timing, the torch arm's gradients are compared with the kernel's (a sanity check of the tool, not a test).  One JSON line
per row.

    python tools/bench_loss_grad.py [--crops 1 64] [--iters 20] [--warmup 5] [--rounds 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "handnet-pipeline_amd"), str(ROOT / "tests"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_occlude import _alternate  # noqa: E402

JOINTS, STRIDE, SF, R = 21, 16, 0.5, 3.0


def _anchors(fh, fw, device):
    """[fh*fw*16, 2] in the heads' NHWC order (cell-major, then anchor)"""
    h, w, a = torch.meshgrid(torch.arange(fh), torch.arange(fw), torch.arange(16), indexing="ij")
    return torch.stack([h * STRIDE + 2 + 4 * (a >> 2), w * STRIDE + 2 + 4 * (a & 3)], -1).reshape(-1, 2).float().to(device)


def torch_criterion(cls, reg, dep, gt, anchor):
    """tests/loss_ref.py's rule in torch, sample by sample as the reference's criterion loops (a2j/anchor.py:99-153: about 25
    small operations per sample), on NHWC heads viewed as [K, anchors, J(, 2)]; -> total_loss [1]"""
    k = cls.shape[0]
    c, r, d = cls.reshape(k, -1, JOINTS), reg.reshape(k, -1, JOINTS, 2), dep.reshape(k, -1, JOINTS)

    def sl1(x):
        return torch.where(x <= 1, 0.5 * x * x, x - 0.5)
    la, lr = [], []
    for i in range(k):
        w = torch.softmax(c[i], dim=0)
        w2 = w.unsqueeze(2).expand(-1, -1, 2)
        uv = gt[i, :, :2]
        la.append(sl1((uv - (w2 * anchor.unsqueeze(1)).sum(0)).abs()).mean())
        spatial = sl1((uv - (w2 * (anchor.unsqueeze(1) + r[i])).sum(0)).abs()).mean() * SF
        lr.append(spatial + (gt[i, :, 2] - (w * d[i]).sum(0)).abs().mean())
    return torch.stack(la).mean(dim=0, keepdim=True) + R * torch.stack(lr).mean(dim=0, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hn_amd import ops
    rows = []
    for k in args.crops:
        g = torch.Generator().manual_seed(9 + k)
        cls = (torch.randn((k, 11, 11, 336), generator=g) * 2.0).cuda()
        reg = (torch.randn((k, 11, 11, 672), generator=g) * 8.0).cuda()
        dep = (0.8 + 0.2 * torch.randn((k, 11, 11, 336), generator=g)).cuda()
        gt = (torch.rand((k, 21, 3), generator=g) * torch.tensor([176.0, 176.0, 0.8]) + torch.tensor([0.0, 0.0, 0.4])).cuda().contiguous()
        out = torch.empty((k, 21, 3), device="cuda")
        anchor = _anchors(11, 11, "cuda")
        leaves = [t.clone().requires_grad_(True) for t in (cls, reg, dep)]

        def torch_arm():
            for t in leaves:
                t.grad = None
            torch_criterion(*leaves, gt, anchor).backward()

        def fused_arm():
            ops.a2j_loss(cls, reg, dep, gt, out=out)
            return ops.a2j_loss_grad(cls, reg, dep, gt)
        torch_arm()
        worst = max(float((t.grad - w).abs().max() / w.abs().max()) for t, w in zip(leaves, fused_arm()))
        assert worst < 1e-4, worst
        t = _alternate({"loss": lambda: ops.a2j_loss(cls, reg, dep, gt, out=out), "loss_grad": fused_arm, "torch": torch_arm}, args)
        rows.append({"row": f"b{k}", "crops": k, "what": "ops.a2j_loss; ops.a2j_loss + ops.a2j_loss_grad; torch restatement forward + backward",
                     "loss_ms": round(t["loss"][0], 5), "loss_grad_ms": round(t["loss_grad"][0], 5), "torch_ms": round(t["torch"][0], 4),
                     "grad_cost_ms": round(t["loss_grad"][0] - t["loss"][0], 5), "torch_over_fused": round(t["torch"][0] / t["loss_grad"][0], 1),
                     "loss_spread_ms": round(t["loss"][1], 5), "loss_grad_spread_ms": round(t["loss_grad"][1], 5),
                     "torch_spread_ms": round(t["torch"][1], 4), "torch_vs_kernel_max_rel": worst})
        print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
