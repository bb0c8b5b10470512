"""Cost of the overlay (faces=: csrc/mesh_raster.hip at the end of the K-hand live step) against the same step without it.

Rows: batch 1 with K = 1 and K = 2, batch 32 with K = 2.  Each row builds BOTH engines (without and with faces) in this
process, captures both, and times them alternately: `rounds` rounds of (plain, overlay), each `iters` replays between two
device events after `warmup` replays; the row reports the median per-call time of each arm and their difference.  Also per
row: the two raster launches alone (ops.mesh_render on the step's own mesh / lifted / frames, device events), the bytes of
the step's one device -> host copy in both arms, and the slots lifted / pixels drawn.  Synthetic weights (hn_amd.synth), the
live fixture's lifter graphs, a seeded Delaunay face list over the 778 vertices, noise frames; one JSON line per row.
The seeded lifter's vertices spread over metres and hardly any face would be drawn, so the lifter's last graph convolution is
scaled by --lifter-scale (0.01: vertices within centimetres of the wrist); "pixels_changed" says how much each row drew.  That
mesh is a triangle soup, not a hand's surface, so the op_* rows measure the rasteriser on closed hand-sized meshes as well:
ops.mesh_render alone on hand-sized closed meshes (the ellipsoids of tests/raster_ref.py, 777 vertices / 1550 faces, ~16-20
thousand pixels per frame) over noise frames at the same three shapes, in event windows; their kernel times are read from a
kernel trace of one row at a time.
--depth-check adds the largest relative difference of the GPU's fp32 depth to the float64 statement of the rule
(tests/raster_ref.py) over its scenes(), the ones tests/test_render_gpu.py checks ("depth_max_rel").

    python tools/bench_render.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b1_k2,b32_k2,op_b1_k1,op_b1_k2,op_b32_k2] [--depth-check] [--out FILE]
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


def synthetic_faces(seed=7, nv=778):
    from scipy.spatial import Delaunay
    return Delaunay(np.random.default_rng(seed).random((nv, 2))).simplices.astype(np.int64)


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _op_row(name, n, k, args):
    """ops.mesh_render alone on n frames x k hand-sized ellipsoids (every frame the same two meshes over its own noise frame)."""
    import raster_ref as rr
    from hn_amd import ops
    e1, f = rr.ellipsoid((0.02, -0.01, 0.55), (0.05, 0.08, 0.03))
    e2, _ = rr.ellipsoid((0.06, 0.02, 0.56), (0.06, 0.04, 0.04))
    mesh = torch.from_numpy(np.stack([np.stack([e1, e2][:k])] * n)).cuda()
    faces = ops.mesh_faces(f, e1.shape[0], "cuda")
    bgr = rr.frame_bgr8(n, 480, 640, seed=11)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    img = torch.empty((n, 480, 640, 3), dtype=torch.uint8, device="cuda")
    dep = torch.zeros((n, 480, 640), device="cuda")
    scratch = torch.empty((ops.mesh_render_scratch_bytes(n * k, f.shape[0]),), dtype=torch.uint8, device="cuda")
    ops.mesh_render(mesh, faces, rr.PARAS, rgb, k=k, out=img, depth_out=dep, scratch=scratch)
    torch.cuda.synchronize()
    drawn = int((dep > 0).sum())
    call = lambda: ops.mesh_render(mesh, faces, rr.PARAS, rgb, k=k, out=img, scratch=scratch)  # noqa: E731
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    windows = [_window(call, args.iters) for _ in range(args.rounds)]
    return {"row": name, "n": n, "k": k, "what": "ops.mesh_render alone, hand-sized ellipsoids",
            "raster_two_launches_eager_ms": round(statistics.median(windows), 4),
            "spread_ms": round(max(windows) - min(windows), 4), "faces": int(f.shape[0]), "pixels_drawn": drawn,
            "pixels_drawn_per_frame": drawn // n}


def _depth_check():
    import raster_ref as rr
    from hn_amd import ops
    worst = {}
    for name, (meshes, faces, lifted, paras, (h, w)) in rr.scenes().items():
        n, k = meshes.shape[:2]
        bgr = rr.frame_bgr8(n, h, w, seed=len(name))
        depth = torch.zeros((n, h, w), device="cuda")
        ops.mesh_render(torch.from_numpy(np.ascontiguousarray(meshes)).cuda(), faces, paras, torch.from_numpy(bgr).cuda(),
                        lifted=None if lifted is None else torch.from_numpy(lifted.reshape(-1).astype(np.int32)).cuda(), k=k,
                        depth_out=depth)
        torch.cuda.synchronize()
        dep = depth.cpu().numpy()
        rel = 0.0
        for i in range(n):
            _w, want, covered, amb = rr.render(meshes[i], faces, paras, bgr[i], None if lifted is None else lifted[i])
            clear = covered & ~amb
            if clear.any():
                rel = max(rel, float((np.abs(dep[i][clear].astype(np.float64) - want[clear]) / want[clear]).max()))
        worst[name] = rel
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--lifter-scale", type=float, default=0.01)
    ap.add_argument("--depth-check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import parity_cases as pc
    from hn_amd import ops, pipeline, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandsEngine
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    names = args.rows.split(",")
    rows = []
    for name in [r for r in names if r.startswith("op_")]:
        rows.append(_op_row(name, *ROWS[name], args))
        print(json.dumps(rows[-1]), flush=True)
    names = [r for r in names if not r.startswith("op_")]
    if names:
        rows += _step_rows(names, args, pc, ops, pipeline, synth, A2JEngine, FCOSEngine, LiveHandsEngine, Pose2MeshEngine,
                           pose2mesh_ref)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.depth_check:
        worst = _depth_check()
        doc["depth_rel_by_scene"] = worst
        doc["depth_max_rel"] = max(worst.values())
        print(json.dumps({"depth_max_rel": doc["depth_max_rel"]}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def _step_rows(names, args, pc, ops, pipeline, synth, A2JEngine, FCOSEngine, LiveHandsEngine, Pose2MeshEngine, pose2mesh_ref):
    g = np.load(ROOT / "tests" / "golden" / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    perm = g["perm_reverse"][:778]
    faces = synthetic_faces()
    sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    last = max(int(key.split(".")[2]) for key in sd if key.startswith("pose2mesh.cl."))
    for key in (f"pose2mesh.cl.{last}.weight", f"pose2mesh.cl.{last}.bias"):        # a hand-sized mesh (see the module docstring)
        sd[key] = sd[key] * args.lifter_scale
    lifter = Pose2MeshEngine(sd, graphs, device="cuda")
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows = []
    with torch.inference_mode():
        for name in names:
            n, k = ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            arms = {}
            for arm, f in (("plain", None), ("overlay", faces)):
                eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, faces=f)
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                for _ in range(args.warmup):
                    run()
                torch.cuda.synchronize()
                arms[arm] = (eng, run, out)
            times = {"plain": [], "overlay": []}
            for _ in range(args.rounds):
                for arm in ("plain", "overlay"):
                    times[arm].append(_window(arms[arm][1], args.iters))
            torch.cuda.synchronize()
            eng, _run, out = arms["overlay"]
            res = out.read()
            frame_u8 = torch.from_numpy(np.stack([np.rint(255.0 * rgb[i].cpu().numpy()).astype(np.uint8).transpose(1, 2, 0)
                                                  for i in range(n)]))
            drawn = int((res.overlay != frame_u8).any(dim=3).sum())
            dev_faces = ops.mesh_faces(faces, 778, "cuda")
            img = torch.empty_like(out.overlay)
            raster = lambda: ops.mesh_render(out.mesh, dev_faces, PARAS, rgb, lifted=out.lifted.reshape(-1), k=k, out=img)  # noqa: E731
            for _ in range(args.warmup):
                raster()
            torch.cuda.synchronize()
            raster_ms = statistics.median(_window(raster, args.iters) for _ in range(args.rounds))
            plain_ms, overlay_ms = statistics.median(times["plain"]), statistics.median(times["overlay"])
            row = {"row": name, "n": n, "k": k, "plain_graph_ms": round(plain_ms, 4), "overlay_graph_ms": round(overlay_ms, 4),
                   "overlay_cost_ms": round(overlay_ms - plain_ms, 4),
                   "plain_spread_ms": round(max(times["plain"]) - min(times["plain"]), 4),
                   "overlay_spread_ms": round(max(times["overlay"]) - min(times["overlay"]), 4),
                   "raster_two_launches_eager_ms": round(raster_ms, 4),
                   "plain_host_bytes": int(arms["plain"][2].host.numel()), "overlay_host_bytes": int(out.host.numel()),
                   "faces": int(faces.shape[0]), "lifted": int(res.lifted.sum()), "pixels_changed": drawn}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


if __name__ == "__main__":
    main()
