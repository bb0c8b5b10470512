"""Cost of a camera per frame (paras [N,4]: the raster's setup kernel and the aggregation's epilogue read their intrinsics from
device tables, csrc/mesh_raster.hip's table form) against the same captured live step with one camera (four kernel arguments),
and of CropMeshEngine's overlay (faces= + frames) against the same captured step without it.

Step rows: batch 1 with K = 1 and K = 2, batch 32 with K = 2.  Each row builds BOTH engines (the 4-tuple, and a table of N
slightly different cameras; faces= in both) in this process, captures both, and times them alternately: `rounds` rounds of
(one, table), each `iters` replays between two device events after `warmup` replays; the row reports the median per-call time
of each arm, their difference and each arm's spread over the rounds.  crop_* rows: the stand-alone mesh demo's step over K
crops, without faces and with faces + K full images (480 x 640 bgr8), the same way.  Synthetic weights, graphs, faces and frames
as tools/bench_render.py (the lifter's last graph convolution scaled by --lifter-scale).  One JSON line per row.

    python tools/bench_cams.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b1_k2,b32_k2,crop_k2,crop_k32] [--out FILE]
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

from bench_occlude import _alternate  # noqa: E402
from bench_render import PARAS, ROWS, synthetic_faces  # noqa: E402

STEP_ROWS = ("b1_k1", "b1_k2", "b32_k2")
CROP_ROWS = {"crop_k2": 2, "crop_k32": 32}


def cameras(n):
    """n slightly different cameras around PARAS, fp32 [n,4]"""
    rng = np.random.default_rng(3)
    return (np.asarray(PARAS, np.float64)[None] + rng.uniform(-15.0, 15.0, (n, 4))).astype(np.float32)


def _lifter(args):
    from hn_amd import synth
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    g = np.load(ROOT / "tests" / "golden" / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    last = max(int(key.split(".")[2]) for key in sd if key.startswith("pose2mesh.cl."))
    for key in (f"pose2mesh.cl.{last}.weight", f"pose2mesh.cl.{last}.bias"):        # a hand-sized mesh (tools/bench_render.py)
        sd[key] = sd[key] * args.lifter_scale
    return Pose2MeshEngine(sd, graphs, device="cuda"), g["perm_reverse"][:778], synthetic_faces()


def _times(t, a, b):
    return {f"{a}_graph_ms": round(t[a][0], 4), f"{b}_graph_ms": round(t[b][0], 4), "difference_ms": round(t[b][0] - t[a][0], 4),
            f"{a}_spread_ms": round(t[a][1], 4), f"{b}_spread_ms": round(t[b][1], 4)}


def _step_rows(names, args, lifter, perm, faces):
    import parity_cases as pc
    from hn_amd import pipeline, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandsEngine
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows = []
    with torch.inference_mode():
        for name in names:
            n, k = ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            arms, outs = {}, {}
            # (the engines share the hand engine, whose conversion the one built last owns: build, capture, then the next)
            for arm, paras in (("one_camera", PARAS), ("camera_table", cameras(n))):
                eng = LiveHandsEngine(hand, lifter, paras, k, True, perm, faces=faces)
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                arms[arm], outs[arm] = run, out
            t = _alternate(arms, args)
            torch.cuda.synchronize()
            res = outs["camera_table"].read()
            row = {"row": name, "n": n, "k": k, **_times(t, "one_camera", "camera_table"), "faces": int(faces.shape[0]),
                   "lifted": int(res.lifted.sum()), "host_bytes": int(outs["camera_table"].host.numel())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def _crop_rows(names, args, lifter, perm, faces):
    import raster_ref as rr
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.live import CropMeshEngine
    a2j = A2JEngine(synth.make_a2j_state_dict(0), device="cuda")
    rows = []
    with torch.inference_mode():
        for name in names:
            k = CROP_ROWS[name]
            g = torch.Generator().manual_seed(k)
            crops = synth.make_crops(k, 176, seed=k).cuda()
            x1, y1 = 150 + torch.rand((k,), generator=g) * 150, 100 + torch.rand((k,), generator=g) * 100
            box = torch.stack([x1, y1, x1 + 150, y1 + 150], dim=1).float().cuda()
            paras = torch.from_numpy(cameras(k)).cuda()
            frames = torch.from_numpy(rr.frame_bgr8(k, 480, 640, seed=k)).cuda()
            plain = CropMeshEngine(a2j, lifter, True, perm).graphed(crops, box, paras)
            drawn = CropMeshEngine(a2j, lifter, True, perm, faces).graphed(crops, box, paras, frames)
            t = _alternate({"mesh_only": plain[0], "with_overlay": drawn[0]}, args)
            torch.cuda.synchronize()
            overlay = drawn[-1].read().overlay
            row = {"row": name, "k": k, **_times(t, "mesh_only", "with_overlay"), "faces": int(faces.shape[0]),
                   "host_bytes": int(drawn[-1].host.numel() * 4), "overlay_bytes": int(overlay.numel()),
                   "pixels_drawn": int((overlay != torch.from_numpy(rr.frame_bgr8(k, 480, 640, seed=k)[..., ::-1].copy())).any(dim=-1).sum())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default=",".join(STEP_ROWS + tuple(CROP_ROWS)))
    ap.add_argument("--lifter-scale", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = args.rows.split(",")
    lifter, perm, faces = _lifter(args)
    rows = _step_rows([r for r in names if r in STEP_ROWS], args, lifter, perm, faces)
    rows += _crop_rows([r for r in names if r in CROP_ROWS], args, lifter, perm, faces)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
