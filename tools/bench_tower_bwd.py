"""What the tower layers' backward costs on the device, at `--batches` 480 x 640 frames per batch (1 and 16;
the 800 x 1088 canvas), by the protocol of tools/bench_thin_bwd.py:

  output_grads / tower_grads   FCOS.output_grads (the parent's step: heads, criterion, its backward, the output convolutions'
                        backward) against FCOS.tower_grads on targets packed once: the same, then the walk over the four tower
                        layers and the un-concatenation into the reference's parameter names
  wgrad / dgrad / gn    the launches of that walk alone, on the engine's own captured tensors: the seven weight-gradient calls
                        (ops.conv3x3_wgrad_levels: tower0's 256 -> 512 bank, six 256 -> 256 banks), the seven input-gradient calls
                        (ops.conv3x3_dgrad_levels with banks flipped once, outside the arm), the four statistics + four
                        GroupNorm backward calls
  torch                 torch fp32 autograd through F.conv2d / F.group_norm / relu (channels_last) on the same FPN outputs,
                        parameters and upstream gradients: forward + backward of the eight tower layers (`torch_fwd`: forward alone)

The arms of a row run in this process on the same model and frames and are timed alternately (tools/bench_occlude.py _alternate):
`rounds` rounds of each arm, each `iters` calls between two device events after `warmup` calls; a row reports each arm's median
per-call time and spread.  Synthetic weights and frames, eight fixed boxes per image.  One JSON line per row.

    python tools/bench_tower_bwd.py [--batches 1 16] [--iters 10] [--warmup 3] [--rounds 7] [--out FILE]
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
import torch.nn.functional as fn  # noqa: E402

from bench_fcos_loss import _targets  # noqa: E402
from bench_occlude import _alternate  # noqa: E402


def _torch_arm(feats, towers, ups):
    """feats: FPN outputs NCHW channels_last; towers = [[(w, b, gamma, beta)] x 4] x 2; ups[l] = gradient at the stacked
    [N,512,h,w] output of the last layer -> (forward, forward + backward)"""
    def forward():
        outs = []
        for x0, up in zip(feats, ups):
            for h, layers in enumerate(towers):
                x = x0
                for w, b, gamma, beta in layers:
                    x = torch.relu(fn.group_norm(fn.conv2d(x, w, b, padding=1), 32, gamma, beta, eps=1e-5))
                outs.append((x, up[:, 256 * h:256 * (h + 1)]))
        return outs

    def both():
        with torch.enable_grad():
            outs = forward()
            leaves = [t for layers in towers for group in layers for t in group] + list(feats)
            torch.autograd.grad([y for y, _ in outs], leaves, [g for _, g in outs])
    return (lambda: forward()), both


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
    from hn_amd.weights import dgrad_bank
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
            t = _alternate({"output_grads": lambda: model.output_grads(frames, packed), "tower_grads": lambda: model.tower_grads(frames, packed)},
                           args)
            *_, d_towers, _, _, inp = engine.tower_grads(rgb, packed, want_inputs=True)
            points = sum(a.shape[1] * a.shape[2] for a in inp["cls_lr"])
            rows.append({"row": f"step_b{n}", "batch": n, "points": points, "output_grads_ms": med(t, "output_grads"),
                         "tower_grads_ms": med(t, "tower_grads"), "added_cost_ms": round(t["tower_grads"][0] - t["output_grads"][0], 4),
                         "output_grads_spread_ms": round(t["output_grads"][1], 4), "tower_grads_spread_ms": round(t["tower_grads"][1], 4)})
            print(json.dumps(rows[-1]), flush=True)
            layers = inp["layers"]
            half = lambda ts, h: [x[..., 256 * h:256 * (h + 1)] for x in ts]                        # noqa: E731
            blocks = lambda ts, h: [x[:, :, :, 8 * h:8 * (h + 1)] for x in ts]                      # noqa: E731
            jobs = [(layers[0]["a"], layers[0]["dy"], dgrad_bank(engine.tower0.w), None)]
            for k in (1, 2, 3):
                for h, tower in enumerate((engine.cls_tower, engine.reg_tower)):
                    jobs.append((blocks(layers[k]["a"], h), half(layers[k]["dy"], h), dgrad_bank(tower[k - 1].w), h))
            scratch = [torch.empty_like(x) for x in d_towers]

            def wgrad():
                for a, dy, _, _ in jobs:
                    ops.conv3x3_wgrad_levels(a, dy)

            def dgrad():
                for _, dy, bank, h in jobs:
                    if h is None:
                        ops.conv3x3_dgrad_levels(dy, bank)
                    else:
                        ops.conv3x3_dgrad_levels(dy, bank, outs=scratch, out_channel_offset=256 * h)

            def gn():
                for k in range(4):
                    lay = layers[k]
                    gamma = engine.gn0_gamma if k == 0 else engine.both_gn[k - 1][0]
                    stats = ops.groupnorm_stats_levels(lay["y"], 64)
                    ops.groupnorm_relu_backward_levels(lay["y"], lay["g"], lay["aff"], stats, gamma, 64)

            nchw = lambda x: x.permute(0, 3, 1, 2)                                               # noqa: E731
            leaf = lambda x: x.clone().requires_grad_(True)                                      # noqa: E731
            feats = [leaf(nchw(ops.from_split(f))) for f in inp["feats"]]
            sd = model.state_dict()
            towers = [[(leaf(sd[f"{hd}.conv.{3 * i}.weight"].contiguous(memory_format=torch.channels_last)), leaf(sd[f"{hd}.conv.{3 * i}.bias"]),
                        leaf(sd[f"{hd}.conv.{3 * i + 1}.weight"]), leaf(sd[f"{hd}.conv.{3 * i + 1}.bias"])) for i in range(4)]
                      for hd in ("head.classification_head", "head.regression_head")]
            fwd, both = _torch_arm(feats, towers, [nchw(x) for x in d_towers])
            t = _alternate({"wgrad": wgrad, "dgrad": dgrad, "gn": gn, "torch": both, "torch_fwd": fwd}, args)
            fma = n * points * 9 * 256 * 256 * 8
            rows.append({"row": f"op_b{n}", "batch": n, "points": points, "fma_wgrad": fma, "fma_dgrad": fma,
                         "wgrad_ms": med(t, "wgrad"), "dgrad_ms": med(t, "dgrad"), "gn_ms": med(t, "gn"), "torch_ms": med(t, "torch"),
                         "torch_fwd_ms": med(t, "torch_fwd"), "wgrad_tflops": round(2 * fma / (t["wgrad"][0] * 1e-3) / 1e12, 2),
                         "dgrad_tflops": round(2 * fma / (t["dgrad"][0] * 1e-3) / 1e12, 2),
                         **{f"{k}_spread_ms": round(t[k][1], 4) for k in ("wgrad", "dgrad", "gn", "torch")}})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
