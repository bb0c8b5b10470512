"""Cost of objects= (what each hand holds: the detector pass through detect_ext -- one more launch, hn_fcos_ext_gather --, three
more launches -- hand_object_associate, hand_object_walk, hand_object_finish, csrc/hand_object.hip --, one more with labels --
object_label_kernel --, and eight more parts in the step's one copy) against the same captured live_hands step of the same
engine (a detector WITH the ext heads in both arms) with the option off.

Rows: N x K = 1 x 1 and 2 x 2 (the shape of tests/test_objects_gpu.py's live step), each with faces= + occlude + labels.  Each
row builds BOTH engines in this process, captures both, and times them alternately: `rounds` rounds of (plain, objects), each
`iters` replays between two device events after `warmup` replays; the row reports the median per-call time of each arm, their
difference and each arm's spread over the rounds, with what the objects step found and the bytes of the one device -> host copy
in both arms.  Synthetic weights, graphs, faces and frames as tools/bench_cloud.py (the depth map is per-pixel noise in 0.3-1.5
m, so the default band of 0.15 m keeps a part of every object's pixels).  One JSON line per row.

    python tools/bench_objects.py [--iters 20] [--warmup 5] [--rounds 5] [--rows b1_k1,b2_k2] [--out FILE]
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

import torch  # noqa: E402

from bench_cams import _lifter, _times  # noqa: E402
from bench_occlude import _alternate  # noqa: E402
from bench_render import PARAS  # noqa: E402

ROWS = {"b1_k1": (1, 1), "b2_k2": (2, 2)}


def _step_rows(names, args):
    import parity_cases as pc
    from hn_amd import pipeline, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.live import LiveHandsEngine
    lifter, perm, faces = _lifter(args)
    hand = pipeline.HandNetEngine(FCOSEngine(synth.make_fcos_state_dict(0, 3, ext=True), 3, device="cuda", ext=True),
                                  A2JEngine(synth.make_a2j_state_dict(0), device="cuda"), 3)
    rows, engines = [], []
    with torch.inference_mode():
        for name in names:
            n, k = ROWS[name]
            rgb, depth = pc.noise_frames(n).cuda(), pc.depth_noise(n).cuda()
            arms, outs = {}, {}
            for arm, more in (("plain", {}), ("objects", dict(objects=True, object_band=args.band))):
                eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, faces=faces, occlude=True, labels=True, **more)
                engines.append(eng)      # (every engine of this process stays alive: its captures' addresses point into it)
                run, s_img, s_dep, out = eng.graphed(rgb, depth)
                s_img.copy_(rgb)
                s_dep.copy_(depth)
                arms[arm], outs[arm] = run, out
            t = _alternate(arms, args)
            torch.cuda.synchronize()
            res = outs["objects"].read()
            row = {"row": name, "n": n, "k": k, **_times(t, "plain", "objects"), "launches_added": 5, "band_m": args.band,
                   "filled_slots": int((res.det_index >= 0).sum()), "in_contact": int((res.contact > 0).sum()),
                   "objects_held": int((res.object_index >= 0).sum()), "with_centroid": int((res.object_count[..., 1] == 0).sum()),
                   "matches": int(res.object_count[..., 0].sum()), "detection_rows": int(outs["objects"].hands.detections.count.sum()),
                   "plain_host_bytes": int(outs["plain"].host.numel()), "objects_host_bytes": int(outs["objects"].host.numel())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    from hn_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default="b1_k1,b2_k2")
    ap.add_argument("--band", type=float, default=ops.OBJECT_BAND)
    ap.add_argument("--lifter-scale", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = _step_rows(args.rows.split(","), args)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
