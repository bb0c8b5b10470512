"""What the FCOS criterion's backward at the heads costs on the device, at `--batches` 480 x 640 frames per
batch (1 and 16), by the protocol of tools/bench_fcos_loss.py:

  op / op_grad          ops.fcos_loss (two launches) against ops.fcos_loss_grad (the same two and the gradient launch) on the
                        batch's head tensors, into preallocated outputs, launches back to back
  loss_step / head_grads   FCOS.loss_step against FCOS.head_grads on targets packed once: the detector's heads, then the
                        criterion's launches (head_grads allocates its gradient tensors per call)

The arms of a row run in this process on the same model and frames and are timed alternately (tools/bench_occlude.py _alternate):
`rounds` rounds of each arm, each `iters` calls between two device events after `warmup` calls; a row reports each arm's median
per-call time, the difference and each arm's spread.  The `op` arm is the forward's unchanged code: compare it with
profiles/bench_fcos_loss.json's op rows to see that the session is sane.  Synthetic weights and frames, eight fixed boxes per
image.  One JSON line per row.

    python tools/bench_fcos_loss_grad.py [--batches 1 16] [--iters 10] [--warmup 3] [--rounds 7] [--out FILE]
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

from bench_fcos_loss import _targets  # noqa: E402
from bench_occlude import _alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fcos_utils.fcos import FCOS
    from hn_amd import ops, synth
    model = FCOS(num_classes=3).cuda().eval()
    model.load_state_dict(synth.make_fcos_state_dict(seed=0, num_classes=3, ext=True), strict=False)
    engine = model.engine()
    rows = []
    with torch.inference_mode():
        for n in args.batches:
            rgb = synth.make_rgb(n, seed=500 + n).cuda()
            frames = [rgb[i] for i in range(n)]
            cls_lr, reg_ctr, strides, (oh, ow, _, _) = engine.forward_heads(rgb)
            ext = engine._ext_levels
            packed = ops.pack_fcos_targets(_targets(n), ops.fcos_target_ratios([(480, 640)] * n, [(oh, ow)] * n), num_classes=3, ext=True)
            points = sum(a.shape[1] * a.shape[2] for a in cls_lr)
            out = ops.alloc_fcos_loss(n, points, "cuda")
            grads = tuple([torch.empty_like(t) for t in h] for h in (cls_lr, reg_ctr, ext))
            upstream = torch.ones((6,), device="cuda")
            t = _alternate({"op": lambda: ops.fcos_loss(cls_lr, reg_ctr, strides, 3, packed, ext=ext, out=out),
                            "op_grad": lambda: ops.fcos_loss_grad(cls_lr, reg_ctr, strides, 3, packed, ext=ext, upstream=upstream, out=grads)},
                           args)
            rows.append({"row": f"op_b{n}", "batch": n, "points": points, "gradient_bytes": sum(t_.numel() * 4 for g in grads for t_ in g),
                         "op_ms": round(t["op"][0], 4), "op_grad_ms": round(t["op_grad"][0], 4),
                         "grad_launch_ms": round(t["op_grad"][0] - t["op"][0], 4), "op_spread_ms": round(t["op"][1], 4),
                         "op_grad_spread_ms": round(t["op_grad"][1], 4)})
            print(json.dumps(rows[-1]), flush=True)
            t = _alternate({"loss_step": lambda: model.loss_step(frames, packed), "head_grads": lambda: model.head_grads(frames, packed)}, args)
            _, fg, _ = model.head_grads(frames, packed)
            rows.append({"row": f"step_b{n}", "batch": n, "loss_step_ms": round(t["loss_step"][0], 4),
                         "head_grads_ms": round(t["head_grads"][0], 4), "backward_cost_ms": round(t["head_grads"][0] - t["loss_step"][0], 4),
                         "loss_step_spread_ms": round(t["loss_step"][1], 4), "head_grads_spread_ms": round(t["head_grads"][1], 4),
                         "fg": int(fg.sum())})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
