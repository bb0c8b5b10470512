"""What the output convolutions' backward costs on the device, at `--batches` 480 x 640 frames per batch (1
and 16; the 800 x 1088 canvas), by the protocol of tools/bench_fcos_loss_grad.py:

  head_grads / output_grads   FCOS.head_grads against FCOS.output_grads on targets packed once: the detector's heads and the
                        criterion with its backward at the heads, then (output_grads) the two backward calls of the output banks
                        and the un-concatenation into the reference's parameter names
  op / torch            the two ops.conv3x3_thin_backward_levels calls (cls + ext banks on the cls tower's map, reg bank on the
                        reg tower's) on the engine's own tensors, against torch autograd through F.conv2d (fp32, channels_last)
                        on the same activations, weights, masks and upstream gradients: forward + backward, since autograd has
                        no backward without its forward (`torch_fwd` is the forward alone)

The arms of a row run in this process on the same model and frames and are timed alternately (tools/bench_occlude.py _alternate):
`rounds` rounds of each arm, each `iters` calls between two device events after `warmup` calls; a row reports each arm's median
per-call time, the difference and each arm's spread.  The head_grads arm is the parent's unchanged step.  Synthetic weights and
frames, eight fixed boxes per image.  One JSON line per row.

    python tools/bench_thin_bwd.py [--batches 1 16] [--iters 10] [--warmup 3] [--rounds 7] [--out FILE]
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


def _torch_arm(maps):
    """maps = [(a levels fp32 NCHW channels_last, [(w [Cout,Cin,3,3], relu_cols, g levels NCHW)])] -> (forward, forward + backward)"""
    def forward():
        outs = []
        for xs, members in maps:
            for w, relu, gs in members:
                for x, g in zip(xs, gs):
                    y = fn.conv2d(x, w, None, padding=1)
                    outs.append((torch.cat([torch.relu(y[:, :relu]), y[:, relu:]], dim=1) if relu else y, g))
        return outs

    def both():
        with torch.enable_grad():
            outs = forward()
            leaves = [w for _, members in maps for w, _, _ in members] + [x for xs, _ in maps for x in xs]
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
    model = FCOS(num_classes=3).cuda().eval()
    model.load_state_dict(synth.make_fcos_state_dict(seed=0, num_classes=3, ext=True), strict=False)
    engine = model.engine()
    rows = []
    with torch.no_grad():
        for n in args.batches:
            rgb = synth.make_rgb(n, seed=500 + n).cuda()
            frames = [rgb[i] for i in range(n)]
            oh, ow, _, _ = engine.geometry(480, 640)
            packed = ops.pack_fcos_targets(_targets(n), ops.fcos_target_ratios([(480, 640)] * n, [(oh, ow)] * n), num_classes=3, ext=True)
            t = _alternate({"head_grads": lambda: model.head_grads(frames, packed), "output_grads": lambda: model.output_grads(frames, packed)},
                           args)
            _, fg, grads, _, d_towers, inp = engine.output_grads(rgb, packed, want_inputs=True)
            points = sum(a.shape[1] * a.shape[2] for a in inp["cls_lr"])
            rows.append({"row": f"step_b{n}", "batch": n, "points": points, "head_grads_ms": round(t["head_grads"][0], 4),
                         "output_grads_ms": round(t["output_grads"][0], 4),
                         "added_cost_ms": round(t["output_grads"][0] - t["head_grads"][0], 4),
                         "head_grads_spread_ms": round(t["head_grads"][1], 4), "output_grads_spread_ms": round(t["output_grads"][1], 4),
                         "fg": int(fg.sum())})
            print(json.dumps(rows[-1]), flush=True)
            cls_members = [(engine.cls_out, 0, inp["cls_lr"], grads[0]), (engine.ext_out, 3, inp["ext"], grads[2])]
            reg_members = [(engine.reg_out, 4, inp["reg_ctr"], grads[1])]

            def op():
                ops.conv3x3_thin_backward_levels(inp["a_cls"], cls_members, dx_out=d_towers, dx_channel_offset=0)
                ops.conv3x3_thin_backward_levels(inp["a_reg"], reg_members, dx_out=d_towers, dx_channel_offset=256)
            nchw = lambda ts: [x.permute(0, 3, 1, 2) for x in ts]                                   # noqa: E731
            maps = []
            for a16, members in ((inp["a_cls"], cls_members), (inp["a_reg"], reg_members)):
                xs = [x.requires_grad_(True) for x in nchw([ops.from_split(a) for a in a16])]
                maps.append((xs, [(cw.w.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_(True), relu,
                                   nchw(gs)) for cw, relu, _ys, gs in members]))
            fwd, both = _torch_arm(maps)
            t = _alternate({"op": op, "torch": both, "torch_fwd": fwd}, args)
            act_bytes = sum(a.numel() * 2 for a in inp["a_cls"] + inp["a_reg"])
            rows.append({"row": f"op_b{n}", "batch": n, "points": points, "activation_bytes": act_bytes,
                         "fma": 2 * n * points * 9 * 256 * (5 + 8 + 5), "op_ms": round(t["op"][0], 4), "torch_ms": round(t["torch"][0], 4),
                         "torch_fwd_ms": round(t["torch_fwd"][0], 4), "op_spread_ms": round(t["op"][1], 4),
                         "torch_spread_ms": round(t["torch"][1], 4)})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
