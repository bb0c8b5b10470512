"""Cost of the K-hands step (HandNetEngine.forward_hands) next to the top-1 step (forward_device).

For (N, K) in (1,1), (1,2), (32,1), (32,2), eager and captured: the per-call time of both steps from device events after
warm-up, the slot fill rate, and the largest keypoint difference between slot 0 and forward_device.  Synthetic weights
(hn_amd.synth) and noise frames; one JSON line per row.

    python tools/bench_hands.py [--iters 20] [--warmup 5] [--out profiles/bench_hands.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "handnet-pipeline_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="1x1,1x2,32x1,32x2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import parity_cases as pc
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    eng = HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                        A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows = []
    with torch.inference_mode():
        for shape in args.shapes.split(","):
            n, k = (int(v) for v in shape.split("x"))
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            top = eng.forward_device(rgb, depth)
            hands = eng.forward_hands(rgb, depth, max_hands=k)
            torch.cuda.synchronize()
            diff = (hands.keypoints[:, 0] - top.keypoints).abs().max().item()
            fill = float((hands.has_hand != 0).float().mean())
            for mode in ("eager", "graph"):
                if mode == "eager":
                    t_top = _time(lambda: eng.forward_device(rgb, depth), args.iters, args.warmup)
                    t_hands = _time(lambda: eng.forward_hands(rgb, depth, max_hands=k), args.iters, args.warmup)
                else:
                    run_top, si, sd, _ = eng.graphed(rgb, depth)
                    si.copy_(rgb)
                    sd.copy_(depth)
                    run_hands, hi, hd, _ = eng.graphed_hands(rgb, depth, k)
                    hi.copy_(rgb)
                    hd.copy_(depth)
                    t_top = _time(run_top, args.iters, args.warmup)
                    t_hands = _time(run_hands, args.iters, args.warmup)
                row = {"n": n, "k": k, "mode": mode, "forward_device_ms": round(t_top, 4),
                       "forward_hands_ms": round(t_hands, 4), "extra_ms": round(t_hands - t_top, 4),
                       "slot_fill": round(fill, 4), "max_abs_dkp_slot0": diff}
                print(json.dumps(row), flush=True)
                rows.append(row)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
