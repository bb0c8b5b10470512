"""Cost of the smoothed live step (track=True, smooth=True: hn_amd.live.LiveHandsEngine) against the tracked step IN THE SAME
PROCESS.

For N x K = 1 x 2, 32 x 2 and 32 x 16: both steps are captured first; then 5 windows of 20 replays each ALTERNATE between the two
(tracked, smoothed, tracked, ...), timed with device events; a row reports the medians of the windows, their spread (max - min)
and the difference of the medians.  The eager launch counts of the two steps (torch profiler, kernels only) go into the row: one
mesh_finish_smooth_kernel stands in place of one mesh_finish_kernel, so they must be equal.  Synthetic weights (hn_amd.synth),
noise frames.  One JSON line per row.

    python tools/bench_smooth.py [--windows 5] [--replays 20] [--shapes 1x2,32x2,32x16] [--out FILE] [--trace]

--trace: no timing -- 10 replays of each captured step at every shape, for a kernel trace taken from outside
(tools/bench_smooth.sh: rocprofv3 --kernel-trace --stats, the two mesh kernels' times).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "handnet-pipeline_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PARAS = (617.343, 617.343, 312.42, 241.42)
SEED = 3000


def _window(fn, replays):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / replays


def _pair(plain, variant, windows, replays):
    for fn in (plain, variant):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {"plain": [], "variant": []}
    for _ in range(windows):
        t["plain"].append(_window(plain, replays))
        t["variant"].append(_window(variant, replays))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"tracked_ms": round(med["plain"], 4), "smoothed_ms": round(med["variant"], 4),
            "delta_ms": round(med["variant"] - med["plain"], 4),
            "tracked_spread_ms": round(max(t["plain"]) - min(t["plain"]), 4),
            "smoothed_spread_ms": round(max(t["variant"]) - min(t["variant"]), 4)}


def _launches(eng, rgb, depth):
    """Kernel launches of one eager step (memcpys and memsets not counted)."""
    from torch.profiler import ProfilerActivity, profile
    eng.forward_device(rgb, depth)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        eng.forward_device(rgb, depth)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
             and not e.name.lower().startswith(("memcpy", "memset"))]
    return len(names), sum("mesh_finish_smooth_kernel" in x for x in names), sum("mesh_finish_kernel" in x for x in names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--shapes", default="1x2,32x2,32x16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import parity_cases as pc
    from hn_amd import pipeline, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandsEngine
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    g = np.load(ROOT / "tests" / "golden" / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    perm = g["perm_reverse"][:778]
    lifter = Pose2MeshEngine(synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs]),
                             graphs, device="cuda")
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows = []
    with torch.inference_mode():
        for n, k in (tuple(int(x) for x in shape.split("x")) for shape in args.shapes.split(",")):
            rgb, depth = pc.noise_frames(n, seed=SEED).cuda(), pc.depth_noise(n, seed=SEED + 1000).cuda()
            engines = {"tracked": LiveHandsEngine(hand, lifter, PARAS, k, True, perm, track=True),
                       "smoothed": LiveHandsEngine(hand, lifter, PARAS, k, True, perm, track=True, smooth=True)}
            counts = None if args.trace else {name: _launches(eng, rgb, depth) for name, eng in engines.items()}
            runs, outs = {}, {}
            for name, eng in engines.items():
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                runs[name], outs[name] = run, out
            torch.cuda.synchronize()
            if args.trace:
                for fn in runs.values():
                    for _ in range(10):
                        fn()
                torch.cuda.synchronize()
                continue
            row = {"pair": "smoothed", "n": n, "k": k, **_pair(runs["tracked"], runs["smoothed"], args.windows, args.replays)}
            r = outs["smoothed"].read()
            row.update(filled=int((r.has_hand != 0).sum()), lifted=int(r.lifted.sum()), ids=int((r.track_id != 0).sum()),
                       launches_tracked=counts["tracked"][0], launches_smoothed=counts["smoothed"][0],
                       mesh_kernels_tracked=list(counts["tracked"][1:]), mesh_kernels_smoothed=list(counts["smoothed"][1:]))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out and not args.trace:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "windows": args.windows,
                                              "replays": args.replays, "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
