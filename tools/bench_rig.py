"""Cost of the rig frame (extrinsics=: three more launches -- rig_transform_kernel, rig_associate_kernel, rig_fuse_kernel,
csrc/rig_ops.hip -- and eight more parts in the step's one copy) against the same captured live_hands step without it.

Rows: N x K = 2 x 2, 8 x 2 and 16 x 16 (the 256-slot limit).  Each row builds BOTH engines (without extrinsics, and with N
cameras turned and moved against each other) in this process, captures both, and times them alternately: `rounds` rounds of
(plain, rig), each `iters` replays between two device events after `warmup` replays; the row reports the median per-call time of
each arm, their difference and each arm's spread over the rounds.  Synthetic weights, graphs and frames as tools/bench_cams.py
(the lifter's last graph convolution scaled by --lifter-scale).  One JSON line per row.

    python tools/bench_rig.py [--iters 20] [--warmup 5] [--rounds 5] [--rows n2_k2,n8_k2,n16_k16] [--out FILE]
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

from bench_cams import _lifter, _times  # noqa: E402
from bench_occlude import _alternate  # noqa: E402
from bench_render import PARAS  # noqa: E402

RIG_ROWS = {"n2_k2": (2, 2), "n8_k2": (8, 2), "n16_k16": (16, 16)}


def rig(n):
    """n camera -> rig transforms [n,3,4]: camera i turned by i * 0.3 rad about the vertical and moved along a line"""
    e = np.zeros((n, 3, 4))
    for i in range(n):
        c, s = np.cos(0.3 * i), np.sin(0.3 * i)
        e[i, :, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        e[i, :, 3] = (0.25 * i, 0.0, 0.05 * i)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default=",".join(RIG_ROWS))
    ap.add_argument("--lifter-scale", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import parity_cases as pc
    from hn_amd import pipeline, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandsEngine
    lifter, perm, _faces = _lifter(args)
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3), 3, device="cuda"),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows = []
    with torch.inference_mode():
        for name in args.rows.split(","):
            n, k = RIG_ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            arms, outs = {}, {}
            for arm, ext in (("plain", None), ("rig", rig(n))):
                eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, extrinsics=ext)
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                arms[arm], outs[arm] = run, out
            t = _alternate(arms, args)
            torch.cuda.synchronize()
            res = outs["rig"].read()
            row = {"row": name, "n": n, "k": k, **_times(t, "plain", "rig"), "launches_added": 3, "lifted": int(res.lifted.sum()),
                   "rig_count": res.rig_count, "max_views": int(res.rig_views.max()), "plain_host_bytes": int(outs["plain"].host.numel()),
                   "rig_host_bytes": int(outs["rig"].host.numel())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
