"""What a batch of the detector's evaluation loop costs, at `--batches` images per batch (1 and 16):

  detect      FCOSEngine.detect_ext alone: the detector's launches, nothing copied back
  eval_step   FCOS.eval_step: detect_ext + ONE launch of csrc/det_ap.hip (DetectionAP.update); no copy, no synchronisation
  forward     what eval_step replaces: FCOS.forward (one count copy, the list of dicts) + the host assembly of
              trainval_net_fcos.py:132-169 -- the two index lists, the [k, 11] rows per image and class copied to numpy, filed
              under the image ids (the text files and voc_eval.py at the epoch's end are NOT in this arm)

All three run in this process on the same model and the same frames and are timed alternately: `rounds` rounds of each arm, each
`iters` calls between two device events after `warmup` calls; a row reports the median per-call time of each arm, eval_step's
difference to detect (the added launch) and to forward, and each arm's spread.  The op row times DetectionAP.update alone on the
batch's detections, launches back to back.  Synthetic weights and frames; the annotations are
the detector's own boxes, so every image has ground truth to match.  One JSON line per row.

    python tools/bench_ap.py [--batches 1 16] [--iters 10] [--warmup 3] [--rounds 7] [--out FILE]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_occlude import _alternate  # noqa: E402


def _host_assembly(outputs, ids, all_boxes):
    """the loop's host side for one batch: select, gather [k, 11] rows per class, copy, file under the image id"""
    empty = np.zeros((0, 11), np.float32)
    for out, image in zip(outputs, ids):
        rows = {}
        for label in (1, 2):
            pick = torch.nonzero((out["scores"] > 0.1) & (out["labels"] == label)).reshape(-1)
            k = pick.shape[0]
            rows[label] = torch.cat((out["boxes"][pick].reshape(k, 4), out["scores"][pick].reshape(k, 1),
                                     out["contacts"][pick].reshape(k, 1), out["dxdymags"][pick].reshape(k, 3),
                                     out["sides"][pick].reshape(k, 1), torch.ones((k, 1), device=pick.device)), -1).cpu().numpy()
        if rows[1].size == 0:
            all_boxes[1][image] = empty
        if rows[2].size == 0:
            all_boxes[2][image] = empty
        else:
            all_boxes[1][image], all_boxes[2][image] = rows[1], rows[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model = FCOS(num_classes=3).cuda().eval()
    model.load_state_dict(synth.make_fcos_state_dict(seed=0, num_classes=3, ext=True), strict=False)
    rows = []
    with torch.inference_mode():
        for n in args.batches:
            rgb = synth.make_rgb(n, seed=500 + n).cuda()
            frames = [rgb[i] for i in range(n)]
            dicts = model(frames)
            names = ["frame_%03d" % i for i in range(n)]
            recs = {}
            for name, d in zip(names, dicts):
                recs[name] = [{"name": "hand" if int(l) == 2 else "targetobject", "bbox": [int(round(float(v) + 1.0)) for v in b],
                               "difficult": 0, "handstate": int(c), "leftright": int(s), "objectbbox": None}
                              for b, l, c, s in list(zip(d["boxes"].cpu(), d["labels"].cpu(), d["contacts"].cpu(), d["sides"].cpu()))[:64]
                              if int(l) in (1, 2)]
            longest = max(1, max(int(d["scores"].shape[0]) for d in dicts))
            acc = model.device_metrics(recs, names, max_dets=longest)
            ids = torch.arange(n, dtype=torch.int32, device="cuda")
            host_ids = list(range(n))
            all_boxes = [[[] for _ in range(n)] for _ in range(3)]
            engine = model.engine()

            def detect():
                return engine.detect_ext(model._batch(frames))      # (stacks the frames, as forward and eval_step do)

            def eval_step():
                model.eval_step(frames, ids)      # (the same images every call: `fed` counts up, the records are rewritten)

            def forward():
                _host_assembly(model(frames), host_ids, all_boxes)

            t = _alternate({"detect": detect, "eval_step": eval_step, "forward": forward}, args)
            acc.reset()
            model.eval_step(frames, ids)
            res = model.eval_results()
            rows.append({"row": f"eval_batch_b{n}", "batch": n, "detections": [int(d["scores"].shape[0]) for d in dicts][:4],
                         "detect_ms": round(t["detect"][0], 4), "eval_step_ms": round(t["eval_step"][0], 4),
                         "forward_host_ms": round(t["forward"][0], 4),
                         "update_cost_ms": round(t["eval_step"][0] - t["detect"][0], 4),
                         "saved_vs_forward_ms": round(t["forward"][0] - t["eval_step"][0], 4),
                         "detect_spread_ms": round(t["detect"][1], 4), "eval_step_spread_ms": round(t["eval_step"][1], 4),
                         "forward_spread_ms": round(t["forward"][1], 4), "hand_ap": res["hand"]["ap"], "fed": res["fed"]})
            print(json.dumps(rows[-1]), flush=True)
            det, _, contacts, dxdymags = engine.detect_ext(model._batch(frames))
            t = _alternate({"update": lambda: acc.update(det, contacts, dxdymags, ids)}, args)
            rows.append({"row": f"op_b{n}", "batch": n, "what": "DetectionAP.update alone, launches back to back",
                         "update_ms": round(t["update"][0], 4), "update_spread_ms": round(t["update"][1], 4)})
            print(json.dumps(rows[-1]), flush=True)
            acc.reset()
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
