"""Cost of fit= (each hand's mesh fitted to its measured depth: two more launches -- mesh_fit_accumulate, mesh_fit_apply,
csrc/mesh_fit.hip --, the raster's depth output switched on, and five more parts in the step's one copy) against the same
captured live_hands step with faces= + occlude alone.

Rows: N x K = 1 x 1, 1 x 2 and 32 x 2.  Each row builds BOTH engines in this process, captures both, and times them
alternately: `rounds` rounds of (occluded, fit), each `iters` replays between two device events after `warmup` replays; the
row reports the median per-call time of each arm, their difference and each arm's spread over the rounds, with the matches
and statuses the fit step found and the bytes of the one device -> host copy in both arms.  Synthetic weights, graphs, faces and
frames as tools/bench_cloud.py (the depth map is per-pixel noise in 0.3-1.5 m, so --band, default the engines' 0.03 m, keeps a
part of every hand's pixels; --min-points, default the engines' 200).
The op_* rows time ops.mesh_fit's two launches alone, eager, on the silhouette and mesh depth that the occluded raster leaves
for hand-sized ellipsoids under a depth map 5 mm behind them.  One JSON line per row.

    python tools/bench_fit.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b1_k2,b32_k2,op_b1_k1,op_b1_k2,op_b32_k2] [--out FILE]
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

from bench_cams import _lifter, _times  # noqa: E402
from bench_occlude import _alternate  # noqa: E402
from bench_render import PARAS, ROWS, _window  # noqa: E402


def _op_row(name, n, k, args):
    import raster_ref as rr
    from hn_amd import ops
    e1, f = rr.ellipsoid((0.02, -0.01, 0.55), (0.05, 0.08, 0.03))
    e2, _ = rr.ellipsoid((0.06, 0.02, 0.56), (0.06, 0.04, 0.04))
    mesh = torch.from_numpy(np.stack([np.stack([e1, e2][:k])] * n)).cuda()
    faces = ops.mesh_faces(f, e1.shape[0], "cuda")
    bgr = rr.frame_bgr8(n, 480, 640, seed=11)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    far = torch.full((n, 1, 480, 640), 2.0, device="cuda")
    best = torch.empty((n, 480, 640), dtype=torch.float32, device="cuda")
    _img, sil, _cov = ops.mesh_render(mesh, faces, rr.PARAS, rgb, k=k, depth_out=best, scene_depth=far)
    # the measured surface: the drawn one 5 mm farther, 1 mm of noise
    depth = (best + 0.005 + 0.001 * torch.randn((n, 480, 640), generator=torch.Generator().manual_seed(5)).cuda()).unsqueeze(1).contiguous()
    slots = mesh.reshape(n * k, -1, 3).contiguous()
    xyz = torch.zeros((n * k, 21, 3), device="cuda")
    xyz[:] = (slots.mean(dim=1) * torch.tensor([1000.0, -1000.0, -1000.0], device="cuda"))[:, None, :]      # (camera millimetres)
    out = ops.mesh_fit(best, sil, depth, rr.PARAS, slots, xyz, k, band=args.band, min_points=args.min_points)
    scratch = torch.empty((ops.mesh_fit_scratch_bytes(n, k, 480),), dtype=torch.uint8, device="cuda")
    holder = argparse.Namespace(fit_mesh=out.mesh, fit_xyz=out.xyz, fit_rt=out.rt, fit_count=out.count, fit_cost=out.cost)
    call = lambda: ops.mesh_fit(best, sil, depth, rr.PARAS, slots, xyz, k, band=args.band, min_points=args.min_points,  # noqa: E731
                                out=holder, scratch=scratch)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    t = [_window(call, args.iters) for _ in range(args.rounds)]
    count, cost, rt = out.count.cpu(), out.cost.cpu(), out.rt.cpu()
    total = int(count[:, 0].sum())
    return {"row": name, "n": n, "k": k, "what": "ops.mesh_fit alone (two launches, eager), hand-sized ellipsoids, 480 x 640",
            "fit_two_launches_eager_ms": round(statistics.median(t), 4), "spread_ms": round(max(t) - min(t), 4), "band_m": args.band,
            "silhouette_pixels": int((sil != 0).sum()), "matches": total, "statuses": sorted(set(count[:, 1].tolist())),
            "rms_residual_mm": round(1000.0 * float(np.sqrt(float(cost.sum()) / 2.0 ** 30 / max(1, total))), 3),
            "shift_slot0_mm": [round(1000.0 * float(v), 3) for v in rt[0, 9:]]}


def _step_rows(names, args):
    import parity_cases as pc
    from hn_amd import pipeline, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandsEngine
    lifter, perm, faces = _lifter(args)
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows, engines = [], []
    with torch.inference_mode():
        for name in names:
            n, k = ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            arms, outs = {}, {}
            for arm, more in (("occluded", {}), ("fit", dict(fit=True, fit_band=args.band, fit_min_points=args.min_points))):
                eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, faces=faces, occlude=True, **more)
                # (an engine owns what its captures' addresses point at -- static inputs, face list, scratch --: every engine
                # of this process stays alive, or the next capture's cache flush could unmap what an earlier graph replays on)
                engines.append(eng)
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                arms[arm], outs[arm] = run, out
            t = _alternate(arms, args)
            torch.cuda.synchronize()
            res = outs["fit"].read()
            row = {"row": name, "n": n, "k": k, **_times(t, "occluded", "fit"), "launches_added": 2, "band_m": args.band,
                   "min_points": args.min_points, "lifted": int(res.lifted.sum()), "silhouette_pixels": int((res.silhouette != 0).sum()),
                   "matches": int(res.fit_count[..., 0].sum()),
                   "slots_by_status": [int((res.fit_count[..., 1] == s).sum()) for s in range(4)],
                   "occluded_host_bytes": int(outs["occluded"].host.numel()), "fit_host_bytes": int(outs["fit"].host.numel())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    from hn_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default="b1_k1,b1_k2,b32_k2,op_b1_k1,op_b1_k2,op_b32_k2")
    ap.add_argument("--band", type=float, default=ops.FIT_BAND)
    ap.add_argument("--min-points", type=int, default=ops.FIT_MIN_POINTS)
    ap.add_argument("--lifter-scale", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = args.rows.split(",")
    rows = _step_rows([r for r in names if not r.startswith("op_")], args)
    with torch.inference_mode():
        for name in (r for r in names if r.startswith("op_")):
            row = _op_row(name, *ROWS[name], args)
            print(json.dumps(row), flush=True)
            rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
