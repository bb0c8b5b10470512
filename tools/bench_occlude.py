"""Cost of occlude= (the overlay tested against the step's depth map, plus silhouette and coverage: csrc/mesh_raster.hip with
its switch) against the same K-hand live step with faces= alone.

Rows: batch 1 with K = 1 and K = 2, batch 32 with K = 2.  Each row builds BOTH engines (faces=, and faces= + occlude) in this
process, captures both, and times them alternately: `rounds` rounds of (overlay, occluded), each `iters` replays between two
device events after `warmup` replays; the row reports the median per-call time of each arm and their difference, the bytes of
the step's one device -> host copy in both arms, and the pixels under a mesh / hidden.  Synthetic weights, graphs, faces and
frames as tools/bench_render.py (the lifter's last graph convolution scaled by --lifter-scale); the depth map is per-pixel
noise in 0.3-1.5 m, so the default margin hides a part of every mesh.
The op_* rows time the two raster launches alone, plain against occluded, on hand-sized closed meshes (the ellipsoids of
tests/raster_ref.py) under a noise depth map around them, alternating in event windows; the kernels' own times are read from a
kernel trace of one such row at a time.  One JSON line per row.

    python tools/bench_occlude.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b1_k2,b32_k2,op_b1_k1,op_b1_k2,op_b32_k2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "handnet-pipeline_amd"), str(ROOT / "tests"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_render import PARAS, ROWS, _window, synthetic_faces  # noqa: E402


def _alternate(arms, args):
    """arms: name -> callable; -> name -> (median ms, spread ms) over `rounds` alternating windows"""
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            times[name].append(_window(fn, args.iters))
    return {name: (statistics.median(t), max(t) - min(t)) for name, t in times.items()}


def _op_row(name, n, k, args):
    import raster_ref as rr
    from hn_amd import ops
    e1, f = rr.ellipsoid((0.02, -0.01, 0.55), (0.05, 0.08, 0.03))
    e2, _ = rr.ellipsoid((0.06, 0.02, 0.56), (0.06, 0.04, 0.04))
    mesh = torch.from_numpy(np.stack([np.stack([e1, e2][:k])] * n)).cuda()
    faces = ops.mesh_faces(f, e1.shape[0], "cuda")
    bgr = rr.frame_bgr8(n, 480, 640, seed=11)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    depth = (0.43 + 0.2 * torch.rand((n, 1, 480, 640), generator=torch.Generator().manual_seed(5))).cuda()
    img = torch.empty((n, 480, 640, 3), dtype=torch.uint8, device="cuda")
    sil = torch.empty((n, 480, 640), dtype=torch.uint8, device="cuda")
    cov = torch.empty((n * k, 2), dtype=torch.int32, device="cuda")
    scratch = torch.empty((ops.mesh_render_scratch_bytes(n * k, f.shape[0]),), dtype=torch.uint8, device="cuda")
    plain = lambda: ops.mesh_render(mesh, faces, rr.PARAS, rgb, k=k, out=img, scratch=scratch)  # noqa: E731
    occluded = lambda: ops.mesh_render(mesh, faces, rr.PARAS, rgb, k=k, out=img, scratch=scratch, scene_depth=depth,  # noqa: E731
                                       margin=args.margin, silhouette_out=sil, coverage_out=cov)
    t = _alternate({"plain": plain, "occluded": occluded}, args)
    torch.cuda.synchronize()
    c = cov.cpu()
    return {"row": name, "n": n, "k": k, "what": "ops.mesh_render alone, hand-sized ellipsoids",
            "plain_two_launches_eager_ms": round(t["plain"][0], 4), "occluded_two_launches_eager_ms": round(t["occluded"][0], 4),
            "plain_spread_ms": round(t["plain"][1], 4), "occluded_spread_ms": round(t["occluded"][1], 4),
            "faces": int(f.shape[0]), "pixels_under_a_mesh": int(c[:, 0].sum()), "pixels_hidden": int((c[:, 0] - c[:, 1]).sum())}


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
    faces = synthetic_faces()
    sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    last = max(int(key.split(".")[2]) for key in sd if key.startswith("pose2mesh.cl."))
    for key in (f"pose2mesh.cl.{last}.weight", f"pose2mesh.cl.{last}.bias"):        # a hand-sized mesh (tools/bench_render.py)
        sd[key] = sd[key] * args.lifter_scale
    lifter = Pose2MeshEngine(sd, graphs, device="cuda")
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows = []
    with torch.inference_mode():
        for name in names:
            n, k = ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            arms, outs = {}, {}
            for arm, occlude in (("overlay", False), ("occluded", True)):
                eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, faces=faces, occlude=occlude, occlude_margin=args.margin)
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                arms[arm], outs[arm] = run, out
            t = _alternate(arms, args)
            torch.cuda.synchronize()
            res = outs["occluded"].read()
            row = {"row": name, "n": n, "k": k, "overlay_graph_ms": round(t["overlay"][0], 4),
                   "occluded_graph_ms": round(t["occluded"][0], 4), "occlude_cost_ms": round(t["occluded"][0] - t["overlay"][0], 4),
                   "overlay_spread_ms": round(t["overlay"][1], 4), "occluded_spread_ms": round(t["occluded"][1], 4),
                   "overlay_host_bytes": int(outs["overlay"].host.numel()), "occluded_host_bytes": int(outs["occluded"].host.numel()),
                   "faces": int(faces.shape[0]), "lifted": int(res.lifted.sum()), "margin_m": args.margin,
                   "pixels_under_a_mesh": int(res.coverage[..., 0].sum()),
                   "pixels_hidden": int((res.coverage[..., 0] - res.coverage[..., 1]).sum())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--lifter-scale", type=float, default=0.01)
    ap.add_argument("--margin", type=float, default=0.03)
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


if __name__ == "__main__":
    main()
