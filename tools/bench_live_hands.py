"""Cost of the K-hand live step (hn_amd.live.LiveHandsEngine) next to the one-hand live step (LiveHandEngine).

Rows: batch 1 with LiveHandEngine and with LiveHandsEngine at K = 1 and K = 2; batch 32 with LiveHandEngine, and at K = 2
with every slot filled and with half of them filled (slot 1 of every frame emptied after the crop stage, as
tests/test_hands_gpu.py's sparse test does: its few extra elementwise launches are counted in that row).
Each row: the captured step's time per call from device events after warm-up, the kernel launches of one eager step
(torch.profiler's device activity; null where the profiler records none), the bytes of the step's one device -> host copy,
and the slot / lifted counts.  Synthetic weights (hn_amd.synth), the live fixture's lifter graphs, noise frames; one JSON line
per row.

    python tools/bench_live_hands.py [--iters 20] [--warmup 5] [--rows b1_live,b1_k1,b1_k2,b32_live,b32_k2,b32_k2_half] [--out FILE]
"""
from __future__ import annotations

import argparse
import contextlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "handnet-pipeline_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PARAS = (617.343, 617.343, 312.42, 241.42)
ROWS = {"b1_live": (1, None, False), "b1_k1": (1, 1, False), "b1_k2": (1, 2, False), "b32_live": (32, None, False),
        "b32_k2": (32, 2, False), "b32_k2_half": (32, 2, True)}


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


def _launches(fn):
    """Kernel launches of one call (device activity of torch.profiler), or None when the profiler records no device work."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    return len(kernels) or None


@contextlib.contextmanager
def _half_filled(pipeline):
    """Empty slot 1 of every frame after the crop stage (box, flag and crop zeroed)."""
    real = pipeline.ops.crop_resize_hands

    def crop(*a, **k):
        box, has, score, index, crops = real(*a, **k)
        keep = torch.zeros_like(has)
        keep[:, 0] = 1
        has.mul_(keep)
        box.mul_(keep[..., None].to(box.dtype))
        crops.mul_(keep.view(-1, 1, 1, 1).to(crops.dtype))
        return box, has, score, index, crops
    pipeline.ops.crop_resize_hands = crop
    try:
        yield
    finally:
        pipeline.ops.crop_resize_hands = real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import parity_cases as pc
    from hn_amd import pipeline, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandEngine, LiveHandsEngine
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
        for name in args.rows.split(","):
            n, k, half = ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            with _half_filled(pipeline) if half else contextlib.nullcontext():
                eng = (LiveHandEngine(hand, lifter, PARAS, True, perm) if k is None
                       else LiveHandsEngine(hand, lifter, PARAS, k, True, perm))
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                ms = _time(run, args.iters, args.warmup)
                torch.cuda.synchronize()
                res = out.read()
                launches = None if args.no_launch_count else _launches(lambda: eng.forward_device(rgb, depth))
            if k is None:
                slots, filled, lifted = n, int((res[1] != 0).sum()), int((res[1] == 1).sum())
            else:
                slots, filled, lifted = n * k, int((res.has_hand != 0).sum()), int(res.lifted.sum())
            row = {"row": name, "n": n, "k": k, "engine": type(eng).__name__, "graph_ms": round(ms, 4),
                   "launches_per_step": launches, "host_bytes": int(out.host.numel()), "slots": slots,
                   "filled": filled, "lifted": lifted}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters,
                                              "warmup": args.warmup, "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
