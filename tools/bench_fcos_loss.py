"""What the FCOS criterion costs on the device, at `--batches` images per batch (1 and 16):

  heads       FCOSEngine.forward_heads alone: the detector up to its head tensors, nothing copied back
  loss_step   FCOS.loss_step on targets packed once (ops.FcosTargets): forward_heads + the criterion's two launches
  loss_dicts  FCOS.loss_step on the reference's list of target dicts: the host packing and its upload on top
  mixed_heads / mixed_step  the same on a list of two image sizes (480 x 640 and 480 x 648, one canvas): forward_heads on the
              list as one batch, against loss_step, which runs such a list image by image (FCOSEngine.forward_heads_each)

All arms run in this process on the same model and frames and are timed alternately (tools/bench_occlude.py _alternate): `rounds`
rounds of each arm, each `iters` calls between two device events after `warmup` calls; a row reports each arm's median per-call
time, loss_step's difference to heads (the two added launches) and each arm's spread.  The op row times ops.fcos_loss alone on the
batch's head tensors, launches back to back.  Synthetic weights and frames, eight fixed boxes per image.  One JSON line per row.

    python tools/bench_fcos_loss.py [--batches 1 16] [--iters 10] [--warmup 3] [--rounds 7] [--out FILE]
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


def _targets(n):
    boxes = torch.tensor([[100.0, 100, 130, 136], [300, 200, 360, 270], [50, 40, 400, 420], [420, 300, 470, 330],
                          [10, 10, 60, 50], [500, 60, 620, 200], [200, 300, 330, 460], [240, 20, 280, 70]])
    info = torch.tensor([[1.0, 0.0, 0.5, 0.06, -0.08], [3.0, 1.0, 0.2, 0.0, 0.1], [0.0, 1.0, 0.0, 0.0, 0.0], [-1.0, -1.0, 0.0, 0.0, 0.0]] * 2)
    return [{"boxes": boxes, "labels": torch.tensor([1, 2, 1, 0] * 2), "box_info": info} for _ in range(n)]


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
            dicts = _targets(n)
            cls_lr, reg_ctr, strides, (oh, ow, _, _) = engine.forward_heads(rgb)
            ext = engine._ext_levels
            packed = ops.pack_fcos_targets(dicts, ops.fcos_target_ratios([(480, 640)] * n, [(oh, ow)] * n), num_classes=3, ext=True)
            t = _alternate({"heads": lambda: engine.forward_heads(model._batch(frames)),
                            "loss_step": lambda: model.loss_step(frames, packed),
                            "loss_dicts": lambda: model.loss_step(frames, dicts)}, args)
            losses, fg = model.loss_step(frames, packed)
            mixed = [torch.cat([f, f[:, :, :8]], dim=2).contiguous() if i % 2 else f for i, f in enumerate(frames)]
            if n > 1:
                tm = _alternate({"mixed_heads": lambda: engine.forward_heads(mixed), "mixed_step": lambda: model.loss_step(mixed, dicts)}, args)
            rows.append({"row": f"loss_batch_b{n}", "batch": n, "points": sum(a.shape[1] * a.shape[2] for a in cls_lr),
                         "heads_ms": round(t["heads"][0], 4), "loss_step_ms": round(t["loss_step"][0], 4),
                         "loss_dicts_ms": round(t["loss_dicts"][0], 4), "criterion_cost_ms": round(t["loss_step"][0] - t["heads"][0], 4),
                         "heads_spread_ms": round(t["heads"][1], 4), "loss_step_spread_ms": round(t["loss_step"][1], 4),
                         "loss_dicts_spread_ms": round(t["loss_dicts"][1], 4), "fg": int(fg.sum()),
                         "losses": {k: round(float(v), 6) for k, v in losses.items()}})
            if n > 1:
                rows[-1].update({"mixed_heads_ms": round(tm["mixed_heads"][0], 4), "mixed_step_ms": round(tm["mixed_step"][0], 4)})
            print(json.dumps(rows[-1]), flush=True)
            out = ops.alloc_fcos_loss(n, rows[-1]["points"], "cuda")
            t = _alternate({"op": lambda: ops.fcos_loss(cls_lr, reg_ctr, strides, 3, packed, ext=ext, out=out)}, args)
            rows.append({"row": f"op_b{n}", "batch": n, "what": "ops.fcos_loss alone (two launches), back to back",
                         "op_ms": round(t["op"][0], 4), "op_spread_ms": round(t["op"][1], 4)})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
