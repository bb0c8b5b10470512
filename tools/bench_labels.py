"""Cost of the label images (labels=: csrc/label_draw.hip at the end of the live step) against the same step without them.

Rows b1_k1, b1_k2, b32_k2: each builds BOTH K-hand engines (without and with labels) in this process, captures both and
times them alternately: `rounds` rounds of (plain, labels), each `iters` replays between two device events after `warmup`
replays; the row reports the median per-call time of each arm, their difference and the bytes of the step's one device -> host
copy in both arms (expected growth: N H W 3 + N K 92928).
Rows op_b1_k1, op_b1_k2, op_b32_k2: the kernels alone on the step's own shapes (noise frames, boxes of 150..250 pixels, every
slot drawn), in event windows: box_label alone, pose_label alone, and the yardstick of DESIGN.md 9b -- the overlay's tile kernel
with nothing to draw (ops.mesh_render with every slot's flag 0: one pixel per lane, three byte stores) -- on the same frames,
and the ratio box_label / yardstick.  Kernel times proper come from a kernel trace of these rows.
Synthetic weights (hn_amd.synth), the live fixture's lifter graphs, noise frames; one JSON line per row.

    python tools/bench_labels.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b1_k2,b32_k2,op_b1_k1,op_b1_k2,op_b32_k2] [--out FILE]
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
ROWS = {"b1_k1": (1, 1), "b1_k2": (1, 2), "b32_k2": (32, 2), "op_b1_k1": (1, 1), "op_b1_k2": (1, 2), "op_b32_k2": (32, 2)}
H, W = 480, 640


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _median(fn, args):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(_window(fn, args.iters) for _ in range(args.rounds))


def _op_row(name, n, k, args):
    from hn_amd import ops
    rng = np.random.default_rng(5)
    s = n * k
    rgb = torch.from_numpy(rng.random((n, 3, H, W), dtype=np.float32)).cuda()
    x1, y1 = rng.integers(0, W - 260, size=s), rng.integers(0, H - 260, size=s)
    side = rng.integers(150, 251, size=(s, 2))
    box = torch.from_numpy(np.stack([x1, y1, x1 + side[:, 0], y1 + side[:, 1]], axis=1).astype(np.int64)).cuda()
    kp = torch.from_numpy(rng.uniform(10, 166, size=(s, 21, 3)).astype(np.float32)).cuda()
    out_box = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    out_pose = torch.empty((s, 176, 176, 3), dtype=torch.uint8, device="cuda")
    # the yardstick: the overlay's tile kernel on frames where no slot is drawn (its set-up launch has nothing to do either)
    mesh = torch.zeros((s, 778, 3), device="cuda")
    faces = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
    nothing = torch.zeros((s,), dtype=torch.int32, device="cuda")
    overlay = torch.empty_like(out_box)
    scratch = torch.empty((ops.mesh_render_scratch_bytes(s, 16),), dtype=torch.uint8, device="cuda")
    box_ms = _median(lambda: ops.draw_labels(kp, box, rgb, k=k, out_box=out_box, pose=False), args)
    pose_ms = _median(lambda: ops.draw_labels(kp, box, rgb, k=k, out_pose=out_pose, box=False), args)
    both_ms = _median(lambda: ops.draw_labels(kp, box, rgb, k=k, out_box=out_box, out_pose=out_pose), args)
    tile_ms = _median(lambda: ops.mesh_render(mesh, faces, PARAS, rgb, lifted=nothing, k=k, out=overlay, scratch=scratch), args)
    assert torch.equal(overlay, torch.where((out_box == torch.tensor([0, 255, 0], dtype=torch.uint8, device="cuda")).all(dim=3, keepdim=True),
                                            overlay, out_box))         # off the rectangles both are the converted frame
    return {"row": name, "n": n, "k": k, "what": "eager event windows, launch included", "box_label_ms": round(box_ms, 4),
            "pose_label_ms": round(pose_ms, 4), "both_ms": round(both_ms, 4), "nothing_to_draw_two_launches_ms": round(tile_ms, 4),
            "box_over_yardstick": round(box_ms / tile_ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = args.rows.split(",")
    rows = []
    for name in [r for r in names if r.startswith("op_")]:
        rows.append(_op_row(name, *ROWS[name], args))
        print(json.dumps(rows[-1]), flush=True)
    names = [r for r in names if not r.startswith("op_")]
    if names:
        rows += _step_rows(names, args)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def _step_rows(names, args):
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
    sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    lifter = Pose2MeshEngine(sd, graphs, device="cuda")
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows = []
    with torch.inference_mode():
        for name in names:
            n, k = ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            arms = {}
            for arm in ("plain", "labels"):
                eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, labels=arm == "labels")
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                for _ in range(args.warmup):
                    run()
                torch.cuda.synchronize()
                arms[arm] = (eng, run, out)
            times = {"plain": [], "labels": []}
            for _ in range(args.rounds):
                for arm in ("plain", "labels"):
                    times[arm].append(_window(arms[arm][1], args.iters))
            torch.cuda.synchronize()
            out = arms["labels"][2]
            res = out.read()
            plain_ms, labels_ms = statistics.median(times["plain"]), statistics.median(times["labels"])
            plain_bytes, labels_bytes = int(arms["plain"][2].host.numel()), int(out.host.numel())
            row = {"row": name, "n": n, "k": k, "plain_graph_ms": round(plain_ms, 4), "labels_graph_ms": round(labels_ms, 4),
                   "labels_cost_ms": round(labels_ms - plain_ms, 4),
                   "plain_spread_ms": round(max(times["plain"]) - min(times["plain"]), 4),
                   "labels_spread_ms": round(max(times["labels"]) - min(times["labels"]), 4),
                   "plain_host_bytes": plain_bytes, "labels_host_bytes": labels_bytes,
                   "expected_growth_bytes": n * H * W * 3 + n * k * 92928, "growth_bytes": labels_bytes - plain_bytes,
                   "lifted": int(res.lifted.sum()), "pose_labels_drawn": int(res.pose_label.reshape(n * k, -1).any(dim=1).sum())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


if __name__ == "__main__":
    main()
