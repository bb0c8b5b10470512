"""Cost of fit_iters= and fit_draw= (the depth fit iterated, the moved mesh drawn again by the raster's
geometry pass before every further step -- 4 (I - 1) + 1 more launches --, and the overlay, silhouette, coverage and cloud drawn
from the fitted mesh) against the captured live_hands step with faces= + occlude + fit=True, which at fit_iters = 1 is that
step launch for launch.

Rows: N x K = 1 x 1, 1 x 2 and 32 x 2.  Each row builds ALL engines in this process -- fit_iters = 1, 2, 3, 4 and fit_draw=True
at 1 and 3 --, captures them, and times them alternately: `rounds` rounds over the arms, each `iters` replays between two device
events after `warmup` replays; the row reports each arm's median per-call time, its difference to the fit_iters = 1 arm and its
spread over the rounds, with the matches and statuses per iteration that the fit_iters = 4 arm found.  Synthetic weights, graphs,
faces and frames as tools/bench_fit.py.
The op_* rows time, eager and alone, the geometry pass (ops.mesh_geometry: two launches) against the occluded raster
(ops.mesh_render with scene_depth: two launches) on the closed hand-sized ellipsoids, alternately.  One JSON line per row.

    python tools/bench_refit.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b1_k2,b32_k2,op_b1_k1,op_b1_k2,op_b32_k2] [--out FILE]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_cams import _lifter  # noqa: E402
from bench_occlude import _alternate  # noqa: E402
from bench_render import PARAS, ROWS  # noqa: E402

ARMS = (("iters1", dict()), ("iters2", dict(fit_iters=2)), ("iters3", dict(fit_iters=3)), ("iters4", dict(fit_iters=4)),
        ("draw1", dict(fit_draw=True)), ("draw3", dict(fit_iters=3, fit_draw=True)))


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
    z, sil = torch.empty((n, 480, 640), device="cuda"), torch.empty((n, 480, 640), dtype=torch.uint8, device="cuda")
    cov = torch.empty((n * k, 2), dtype=torch.int32, device="cuda")
    gz, who = torch.empty((n, 480, 640), device="cuda"), torch.empty((n, 480, 640), dtype=torch.uint8, device="cuda")
    scratch = torch.empty((ops.mesh_render_scratch_bytes(n * k, f.shape[0]),), dtype=torch.uint8, device="cuda")
    arms = {"occluded_raster": lambda: ops.mesh_render(mesh, faces, rr.PARAS, rgb, k=k, out=img, depth_out=z, scratch=scratch,
                                                       scene_depth=depth, silhouette_out=sil, coverage_out=cov),
            "geometry": lambda: ops.mesh_geometry(mesh, faces, rr.PARAS, (480, 640), k=k, out_depth=gz, out_who=who, scratch=scratch)}
    t = _alternate(arms, args)
    torch.cuda.synchronize()
    assert torch.equal(gz, z) and torch.equal(who, sil & 0x7F)
    return {"row": name, "n": n, "k": k, "what": "two launches each, eager, hand-sized closed ellipsoids, 480 x 640",
            "occluded_raster_eager_ms": round(t["occluded_raster"][0], 4), "geometry_eager_ms": round(t["geometry"][0], 4),
            "difference_ms": round(t["geometry"][0] - t["occluded_raster"][0], 4),
            "occluded_raster_spread_ms": round(t["occluded_raster"][1], 4), "geometry_spread_ms": round(t["geometry"][1], 4),
            "covered_pixels": int((who != 0).sum())}


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
            for arm, more in ARMS:
                eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, faces=faces, occlude=True, fit=True, fit_band=args.band,
                                      fit_min_points=args.min_points, **more)
                engines.append(eng)      # (every engine of this process stays alive: its captures' addresses point into it)
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                arms[arm], outs[arm] = run, out
            t = _alternate(arms, args)
            torch.cuda.synchronize()
            res = outs["iters4"].read()
            base = t["iters1"][0]
            row = {"row": name, "n": n, "k": k, "band_m": args.band, "min_points": args.min_points}
            for arm, _more in ARMS:
                row[f"{arm}_graph_ms"] = round(t[arm][0], 4)
                row[f"{arm}_spread_ms"] = round(t[arm][1], 4)
                if arm != "iters1":
                    row[f"{arm}_minus_iters1_ms"] = round(t[arm][0] - base, 4)
            trace = res.fit_trace.reshape(-1, 4, 3)
            row.update(lifted=int(res.lifted.sum()), matches_per_iteration=[int(v) for v in trace[:, :, 0].sum(dim=0)],
                       fitted_slots_per_iteration=[int(v) for v in (trace[:, :, 1] == 0).sum(dim=0)],
                       cost_per_iteration=[int(v) for v in trace[:, :, 2].sum(dim=0)],
                       iters1_host_bytes=int(outs["iters1"].host.numel()), iters4_host_bytes=int(outs["iters4"].host.numel()))
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
