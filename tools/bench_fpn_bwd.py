"""What the FPN's backward costs on the device, at `--batches` 480 x 640 frames per batch (1 and 16; the
800 x 1088 canvas, levels 100 x 136, 50 x 68, 25 x 34), by the protocol of tools/bench_tower_bwd.py:

  tower_grads / fpn_grads   FCOS.tower_grads (the parent's step: heads, criterion, its backward, the output convolutions' and the
                        towers' backward) against FCOS.fpn_grads on targets packed once: the same, then the walk over the FPN and
                        the reference's parameter names
  wgrad1x1 / wgrad3x3 / dgrad / upT   the launches of that walk alone, on the engine's own captured tensors: the three lateral
                        weight-gradient calls (ops.conv1x1_wgrad, Cin 128 / 256 / 512), the three output-convolution weight-gradient
                        calls (ops.conv3x3_wgrad_levels, one level each), the three 3x3 input-gradient calls with their residuals
                        plus the three 1x1 ones for d_body (banks transposed once, outside the arm), the two adjoint calls
                        (ops.upsample_nearest_backward)

The arms of a row run in this process on the same model and frames and are timed alternately (tools/bench_occlude.py _alternate):
`rounds` rounds of each arm, each `iters` calls between two device events after `warmup` calls; a row reports each arm's median
per-call time and spread.  Synthetic weights and frames, eight fixed boxes per image.  One JSON line per row.

    python tools/bench_fpn_bwd.py [--batches 1 16] [--iters 10] [--warmup 3] [--rounds 7] [--out FILE]
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
    from hn_amd.weights import dgrad_bank, dgrad_bank_1x1
    model = FCOS(num_classes=3).cuda().eval()
    model.load_state_dict(synth.make_fcos_state_dict(seed=0, num_classes=3, ext=True), strict=False)
    engine = model.engine()
    rows = []
    med = lambda t, k: round(t[k][0], 4)                                                         # noqa: E731
    with torch.no_grad():
        for n in args.batches:
            rgb = synth.make_rgb(n, seed=500 + n).cuda()
            frames = [rgb[i] for i in range(n)]
            oh, ow, _, _ = engine.geometry(480, 640)
            packed = ops.pack_fcos_targets(_targets(n), ops.fcos_target_ratios([(480, 640)] * n, [(oh, ow)] * n), num_classes=3, ext=True)
            t = _alternate({"tower_grads": lambda: model.tower_grads(frames, packed), "fpn_grads": lambda: model.fpn_grads(frames, packed)},
                           args)
            res = engine.fpn_grads(rgb, packed, want_inputs=True)
            d_feats, inp = res[6], res[9]
            points = sum(a.shape[1] * a.shape[2] for a in inp["lat"])
            rows.append({"row": f"step_b{n}", "batch": n, "points": points, "tower_grads_ms": med(t, "tower_grads"),
                         "fpn_grads_ms": med(t, "fpn_grads"), "added_cost_ms": round(t["fpn_grads"][0] - t["tower_grads"][0], 4),
                         "tower_grads_spread_ms": round(t["tower_grads"][1], 4), "fpn_grads_spread_ms": round(t["fpn_grads"][1], 4)})
            print(json.dumps(rows[-1]), flush=True)
            cs, lats, ds, ups = inp["c"], inp["lat"], inp["D"], inp["U"]
            banks3 = [dgrad_bank(cw.w) for cw in engine.layer]
            banks1 = [dgrad_bank_1x1(cw.w) for cw in engine.inner]

            def wgrad1x1():
                for c, d in zip(cs, ds):
                    ops.conv1x1_wgrad(c, d)

            def wgrad3x3():
                for lat, g in zip(lats, d_feats):
                    ops.conv3x3_wgrad_levels([lat], [g])

            def dgrad():
                for g, bank, u in zip(d_feats, banks3, ups):
                    ops.conv3x3_dgrad_levels([g], bank, residuals=[u])
                for d, bank in zip(ds, banks1):
                    ops.conv2d_nhwc(d, bank)

            def upt():
                for d, lat in zip(ds[:-1], lats[1:]):
                    ops.upsample_nearest_backward(d, tuple(lat.shape[1:3]))

            t = _alternate({"wgrad1x1": wgrad1x1, "wgrad3x3": wgrad3x3, "dgrad": dgrad, "upT": upt}, args)
            fma1 = n * sum(a.shape[1] * a.shape[2] * ops.channels(a) * 256 for a in cs)
            fma3 = n * points * 9 * 256 * 256
            rows.append({"row": f"op_b{n}", "batch": n, "points": points, "fma_wgrad1x1": fma1, "fma_wgrad3x3": fma3,
                         "fma_dgrad": fma3 + fma1, "wgrad1x1_ms": med(t, "wgrad1x1"), "wgrad3x3_ms": med(t, "wgrad3x3"),
                         "dgrad_ms": med(t, "dgrad"), "upT_ms": med(t, "upT"),
                         "wgrad1x1_tflops": round(2 * fma1 / (t["wgrad1x1"][0] * 1e-3) / 1e12, 2),
                         "wgrad3x3_tflops": round(2 * fma3 / (t["wgrad3x3"][0] * 1e-3) / 1e12, 2),
                         "dgrad_tflops": round(2 * (fma3 + fma1) / (t["dgrad"][0] * 1e-3) / 1e12, 2),
                         **{f"{k}_spread_ms": round(t[k][1], 4) for k in ("wgrad1x1", "wgrad3x3", "dgrad", "upT")}})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
