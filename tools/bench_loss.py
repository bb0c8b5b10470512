"""Cost of the A2J criterion on the device (ops.a2j_loss: csrc/a2j_ops.hip's aggregation in its loss form + the reduction launch)
against the plain aggregation, and of forward(x, gt) against forward(x).

At each of `--crops` (1 and 64: one hand, and BASELINE config 2's batch) two pairs of arms run in this process on the same
buffers and are timed alternately: `rounds` rounds, each `iters` calls between two device events after `warmup` calls; a row
reports the median per-call time of each arm, their difference and each arm's spread (max - min over the rounds).
  op row       ops.a2j_aggregate (the plain launch: the code of the commit before the criterion, so its time is that commit's
               baseline) against ops.a2j_loss (the loss launch pair) on seeded heads of the model's shape, launches back to back;
  forward row  A2JEngine.forward(x) against forward(x, gt=...), eager launches as the drop-in issues them.
Synthetic weights, crops and heads.  One JSON line per row.

    python tools/bench_loss.py [--crops 1 64] [--iters 50] [--warmup 10] [--rounds 7] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hn_amd import ops, synth
    from hn_amd.a2j_engine import A2JEngine
    eng = A2JEngine(synth.make_a2j_state_dict(0), device="cuda")
    rows = []
    with torch.inference_mode():
        for k in args.crops:
            g = torch.Generator().manual_seed(9 + k)
            cls = (torch.randn((k, 11, 11, 336), generator=g) * 2.0).cuda()
            reg = (torch.randn((k, 11, 11, 672), generator=g) * 8.0).cuda()
            dep = (0.8 + 0.2 * torch.randn((k, 11, 11, 336), generator=g)).cuda()
            gt = (torch.rand((k, 21, 3), generator=g) * torch.tensor([176.0, 176.0, 0.8]) + torch.tensor([0.0, 0.0, 0.4])).cuda().contiguous()
            out = torch.empty((k, 21, 3), device="cuda")
            assert torch.equal(ops.a2j_loss(cls, reg, dep, gt)[0], ops.a2j_aggregate(cls, reg, dep))
            t = _alternate({"plain": lambda: ops.a2j_aggregate(cls, reg, dep, out=out),
                            "loss": lambda: ops.a2j_loss(cls, reg, dep, gt, out=out)}, args)
            rows.append({"row": f"op_b{k}", "crops": k, "what": "ops.a2j_aggregate against ops.a2j_loss (two launches), back to back",
                         "plain_ms": round(t["plain"][0], 5), "loss_ms": round(t["loss"][0], 5),
                         "loss_cost_ms": round(t["loss"][0] - t["plain"][0], 5),
                         "plain_spread_ms": round(t["plain"][1], 5), "loss_spread_ms": round(t["loss"][1], 5)})
            print(json.dumps(rows[-1]), flush=True)
            crops = synth.make_crops(k, 176, seed=9).cuda()
            t = _alternate({"forward": lambda: eng.forward(crops), "forward_gt": lambda: eng.forward(crops, gt=gt)}, args)
            rows.append({"row": f"forward_b{k}", "crops": k, "what": "A2JEngine.forward(x) against forward(x, gt), eager",
                         "forward_ms": round(t["forward"][0], 4), "forward_gt_ms": round(t["forward_gt"][0], 4),
                         "gt_cost_ms": round(t["forward_gt"][0] - t["forward"][0], 4),
                         "forward_spread_ms": round(t["forward"][1], 4), "forward_gt_spread_ms": round(t["forward_gt"][1], 4)})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
