"""Cost of device_metrics (HPEMetrics.update: one launch of csrc/hpe_metrics.hip per batch) against the same evaluation step
without it.

The step is the device side of A2JModelLightning.test_step at `--crops` crops (64: BASELINE config 2's batch): the A2J forward
with the conversion in its epilogue, and the ground truth's conversion -- eager launches, as the loop issues them.  BOTH arms run
in this process on the same engine and the same buffers and are timed alternately: `rounds` rounds of (step, step + update), each
`iters` calls between two device events after `warmup` calls; the row reports the median per-call time of each arm, their
difference and each arm's spread.  The op row times ops.hpe_accumulate alone on the step's tensors.  Synthetic weights and crops.
One JSON line per row.

    python tools/bench_metrics.py [--crops 64] [--iters 20] [--warmup 5] [--rounds 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
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
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hn_amd import ops, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.metrics import HPEMetrics
    k = args.crops
    g = torch.Generator().manual_seed(9)
    eng = A2JEngine(synth.make_a2j_state_dict(0), device="cuda")
    crops = synth.make_crops(k, 176, seed=9).cuda()
    gt = (torch.rand((k, 21, 3), generator=g) * torch.tensor([176.0, 176.0, 0.8]) + torch.tensor([0.0, 0.0, 0.4])).cuda().contiguous()
    x1, y1 = torch.rand((k,), generator=g) * 380, torch.rand((k,), generator=g) * 260
    box = torch.stack([x1, y1, x1 + 40 + torch.rand((k,), generator=g) * 200, y1 + 40 + torch.rand((k,), generator=g) * 170], dim=1).float().cuda()
    paras = (torch.tensor([[617.343, 617.343, 312.42, 241.42]]).repeat(k, 1) + torch.rand((k, 4), generator=g) * 20).float().cuda()
    metrics = HPEMetrics("cuda:0")
    conv = dict(sample_box=box, sample_paras=paras)

    def step():
        _kp, _img, xyz = eng.forward(crops, convert=conv)
        _, gt_xyz = ops.convert_joints_samples(gt, box, paras, want_image=False)
        return xyz, gt_xyz

    def step_update():
        xyz, gt_xyz = step()
        metrics.update(xyz, gt_xyz)

    rows = []
    with torch.inference_mode():
        xyz, gt_xyz = step()
        xyz, gt_xyz = xyz.clone(), gt_xyz.clone()
        t = _alternate({"step": step, "step_update": step_update}, args)
        rows.append({"row": f"eval_step_b{k}", "crops": k, "what": "A2J forward + conversion + ground-truth conversion, eager",
                     "step_ms": round(t["step"][0], 4), "step_update_ms": round(t["step_update"][0], 4),
                     "update_cost_ms": round(t["step_update"][0] - t["step"][0], 4),
                     "step_spread_ms": round(t["step"][1], 4), "step_update_spread_ms": round(t["step_update"][1], 4)})
        print(json.dumps(rows[-1]), flush=True)
        t = _alternate({"update": lambda: metrics.update(xyz, gt_xyz)}, args)
        res = metrics.compute()
        rows.append({"row": f"op_b{k}", "crops": k, "what": "HPEMetrics.update alone, launches back to back",
                     "update_ms": round(t["update"][0], 4), "update_spread_ms": round(t["update"][1], 4), "fed": res["fed"],
                     "skipped": res["skipped"]})
        print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
