"""Cost of cloud= (each hand's depth pixels as a point cloud: two more launches -- hand_cloud_count, hand_cloud_write,
csrc/hand_cloud.hip --, the raster's depth output switched on, and three more parts in the step's one copy) against the same
captured live_hands step with faces= + occlude alone.

Rows: N x K = 1 x 1, 1 x 2 and 32 x 2.  Each row builds BOTH engines in this process, captures both, and times them
alternately: `rounds` rounds of (occluded, cloud), each `iters` replays between two device events after `warmup` replays; the
row reports the median per-call time of each arm, their difference and each arm's spread over the rounds, with the matches the
cloud step found and the bytes of the one device -> host copy in both arms.  Synthetic weights, graphs, faces and frames as
tools/bench_occlude.py (the lifter's last graph convolution scaled by --lifter-scale; the depth map is per-pixel noise in
0.3-1.5 m, so --band, default the engines' 0.03 m, keeps a part of every hand's pixels).
The op_* rows time ops.hand_cloud's two launches alone, eager, on the silhouette and mesh depth that the occluded raster
leaves for hand-sized ellipsoids under a noise depth map around them.  One JSON line per row.

    python tools/bench_cloud.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b1_k2,b32_k2,op_b1_k1,op_b1_k2,op_b32_k2] [--out FILE]
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
    depth = (0.43 + 0.2 * torch.rand((n, 1, 480, 640), generator=torch.Generator().manual_seed(5))).cuda()
    best = torch.empty((n, 480, 640), dtype=torch.float32, device="cuda")
    _img, sil, _cov = ops.mesh_render(mesh, faces, rr.PARAS, rgb, k=k, depth_out=best, scene_depth=depth)
    out = ops.hand_cloud(best, sil, depth, rr.PARAS, k, band=args.band)
    scratch = torch.empty((ops.hand_cloud_scratch_bytes(n, k, 480),), dtype=torch.uint8, device="cuda")
    holder = argparse.Namespace(cloud=out.cloud, cloud_count=out.count, cloud_resid=out.resid)
    call = lambda: ops.hand_cloud(best, sil, depth, rr.PARAS, k, band=args.band, out=holder, scratch=scratch)  # noqa: E731
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    t = [_window(call, args.iters) for _ in range(args.rounds)]
    count = out.count.cpu()
    return {"row": name, "n": n, "k": k, "what": "ops.hand_cloud alone (two launches, eager), hand-sized ellipsoids, 480 x 640",
            "cloud_two_launches_eager_ms": round(statistics.median(t), 4), "spread_ms": round(max(t) - min(t), 4), "band_m": args.band,
            "silhouette_pixels": int((sil != 0).sum()), "matches": int(count[:, 0].sum()), "rows_written": int(count[:, 1].sum())}


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
            for arm, more in (("occluded", {}), ("cloud", dict(cloud=True, cloud_band=args.band))):
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
            res = outs["cloud"].read()
            row = {"row": name, "n": n, "k": k, **_times(t, "occluded", "cloud"), "launches_added": 2, "band_m": args.band,
                   "lifted": int(res.lifted.sum()), "silhouette_pixels": int((res.silhouette != 0).sum()),
                   "matches": int(res.cloud_count[..., 0].sum()), "rows_written": int(res.cloud_count[..., 1].sum()),
                   "mean_residual_mm": round(float(res.cloud_resid.sum()) / max(1, int(res.cloud_count[..., 0].sum())) / 1000.0, 3),
                   "occluded_host_bytes": int(outs["occluded"].host.numel()), "cloud_host_bytes": int(outs["cloud"].host.numel())}
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
    ap.add_argument("--band", type=float, default=ops.CLOUD_BAND)
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
