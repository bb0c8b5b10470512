#!/usr/bin/env python3
"""The reference's live loop (ros_demo.py:260-337) on the MI355X path, without ROS: synthetic 640x480 RGB-D frames go through

  1. the drop-in callable exactly as ros_demo.py:270 calls it            -> (keypoints on the CPU, depth crop, crop box)
  2. the same call with the caller's convert_joints folded into the step   -> net.last_converted (image uv, camera xyz in mm)
  3. the whole chain as ONE captured step (network -> convert -> Pose2Mesh lifter -> one copy)  -> mesh vertices

Weights are the seeded synthetic checkpoints of the tests (the published models/*.pth are not redistributable); with real
checkpoints pass their paths in `args` and reload_detector / reload_a2j = True, as ros_demo.py:370-388 does.
With --overlay out.png the step also draws the mesh over the frame (the caller's render(), ros_demo.py:86-116,341) and the last
frame's overlay is written with PIL; --mano FILE reads the face list from a MANO pickle's 'f' entry, else a synthetic face list
over the 778 vertices is used (a seeded Delaunay triangulation, as tests/golden/make_golden_p2m.py builds one).
With --labels PREFIX the step also draws the loop's other two images (ros_demo.py:310-326): the last frame's box_label (the
frame with the crop box) and pose_label (the 176 x 176 colour crop with the skeleton) are written as PREFIX_box.npy / PREFIX_pose.npy.
With --left the step runs in the caller's mirror mode for a left-handed subject (ImageListener(left=True), ros_demo.py:259-262):
frame and depth map are mirrored before anything else and every result is in the mirrored frame.  With --handed the last frame
also goes through the K = 2 step with per-slot handedness: the detector's side of each slot, and which slots ran mirrored
through the right-handed pose network and lifter (side == left_side; 0 is an assumption about the checkpoint's convention).
With --track a few frames go through the K = 2 step with tracked slots (live_hands(track=True)): the track id and age of every
slot are printed per frame -- a hand keeps its slot and id whatever its score rank, a slot whose hand is missing is held.
With --smooth the same frames go through the tracked K = 2 step with the filter on (live_hands(track=True, smooth=True)): per
frame, how far the filtered mesh and joints lie from the raw ones (0 on a slot's first frame and on a repeated frame); the
filter's parameters are the paper's starting values, not tuned on this model.
With --occlude the last frame also goes through the K = 2 step with faces= and occlude=True: the overlay leaves out what lies
more than 3 cm (a starting value, not tuned) behind the frame's depth map, and for every slot the share of its mesh's pixels that
the camera sees is printed (read().coverage), with the silhouette's pixel counts.
With --cameras N the last frame goes N times through ONE captured K = 2 step built with N slightly different intrinsics
(paras [N,4]: a rig of N cameras), and once more after set_cameras() swapped them, without a recapture.
With --rig the last frame goes twice, as two cameras, through ONE captured K = 2 step built with extrinsics= (camera -> rig
transforms): first with both cameras at one place -- every hand is seen twice and fused into one rig hand --, then, after
set_extrinsics() moved camera 1 a metre aside without a recapture, as two hands a metre apart.  The association radius of
8 cm is a starting value, not tuned on this model.
With --cloud the last frame also goes through the K = 2 step with faces=, occlude=True and cloud=True: every slot's measured
depth pixels (every second row and column under its silhouette, within 3 cm of the mesh; at most 4096 points; starting values,
not tuned) as 3-D points in the camera frame -- per slot, the number of matching pixels, the rows written and the mean residual
depth - mesh Z in millimetres (how far the mesh sits from the surface the camera sees).
With --fit the last frame also goes through the K = 2 step with faces=, occlude=True and fit=True: every slot's mesh and joints
moved onto its measured depth pixels by one Gauss-Newton step of point-to-plane alignment (starting values, not tuned) -- per
slot, the matching pixels, the status, the RMS residual along the normals before the step and the shift found, in millimetres.
--fit-iters I (1..8) runs I such steps, the moved mesh drawn again before every further one, and prints every step's matches,
status and RMS residual (the trace); --fit-draw draws the overlay and the silhouette from the fitted mesh and prints how many
silhouette pixels that changed.  Both imply --fit.
usage (GPU box): python examples/live_demo.py [frames] [--overlay out.png] [--mano MANO_RIGHT.pkl] [--labels PREFIX] [--left]
                 [--handed] [--track] [--smooth] [--occlude] [--cameras N] [--rig] [--cloud] [--fit] [--fit-iters I] [--fit-draw]"""
import sys
import time
import types
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "handnet-pipeline_amd"))                       # the drop-in tree in front of a reference checkout
sys.path.insert(0, str(REPO / "handnet-pipeline_amd" / "pose2mesh" / "lib"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

import models  # noqa: E402  (pose2mesh/lib/models, ros_demo.py:30)
from handnet_pipeline.handnet_pipeline import HandNet  # noqa: E402  (ros_demo.py:10)
from hn_amd import synth  # noqa: E402

PARAS = (617.343, 617.343, 312.42, 241.42)        # fx, fy, cx, cy of the depth camera (ros_demo.py:191-196)


def _faces(mano_file):
    if mano_file:
        import pickle
        with open(mano_file, "rb") as f:
            return np.asarray(pickle.load(f, encoding="latin1")["f"], dtype=np.int64)
    from scipy.spatial import Delaunay
    return Delaunay(np.random.default_rng(7).random((778, 2))).simplices.astype(np.int64)


def main():
    argv = sys.argv[1:]
    opt = {}
    for flag in ("--overlay", "--mano", "--labels", "--cameras", "--fit-iters"):
        if flag in argv:
            i = argv.index(flag)
            opt[flag] = argv[i + 1]
            del argv[i:i + 2]
    left, handed, track, smooth = "--left" in argv, "--handed" in argv, "--track" in argv, "--smooth" in argv
    occlude, rig_frame, cloud, fit = "--occlude" in argv, "--rig" in argv, "--cloud" in argv, "--fit" in argv
    fit_iters, fit_draw = int(opt.get("--fit-iters", 1)), "--fit-draw" in argv
    fit = fit or fit_draw or "--fit-iters" in opt
    argv = [a for a in argv if a not in ("--left", "--handed", "--track", "--smooth", "--occlude", "--rig", "--cloud", "--fit", "--fit-draw")]
    frames = int(argv[0]) if argv else 20
    faces = _faces(opt.get("--mano")) if "--overlay" in opt else None
    args = types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-")
    net = HandNet(args, reload_detector=False, num_classes=3, reload_a2j=False)           # ros_demo.py:374-388
    net.detector.load_state_dict(synth.make_fcos_state_dict(0, 3), strict=False)
    net.a2j.load_state_dict(synth.make_a2j_state_dict(0), strict=False)
    net = net.cuda().eval()
    g = np.load(REPO / "tests" / "golden" / "pose2mesh_forward.npz")                      # graph hierarchy (data fixture)
    graph_L = [sp.csr_matrix((g[f"L{i}_data"], g[f"L{i}_indices"], g[f"L{i}_indptr"]), shape=tuple(int(v) for v in g[f"L{i}_shape"]))
               for i in range(int(g["num_levels"]))]
    model = models.pose2mesh_net.get_model(21, graph_L)                                  # ros_demo.py:142
    model.load_state_dict(synth.make_pose2mesh_state_dict(0, graph_sizes=[m.shape[0] for m in graph_L]), strict=False)
    model = model.cuda().eval()

    rgb, depth = synth.make_rgb(1, seed=1000).cuda(), synth.make_depth(1, seed=2000).cuda()
    with torch.inference_mode():
        # 1. ros_demo.py:270
        keypoint_pred, depth_im, detections = net([rgb[0]], depth_images=depth)
        print("1. HandNet.forward:", tuple(keypoint_pred.shape), keypoint_pred.device, tuple(depth_im.shape), detections[0].tolist())
        # 2. the caller's clamp + convert_joints (ros_demo.py:279-290,329-330) as part of the step
        net.set_convert(PARAS, clamp=True)
        net([rgb[0]], depth_images=depth)
        conv = net.last_converted
        print("2. set_convert: joints2d[0] =", conv["image_uvd"][0, 0, :2].tolist(), " joints3d[0] (mm) =", conv["xyz_mm"][0, 0].tolist())
        # 3. the live chain as one captured step
        rev = torch.from_numpy(g["perm_reverse"][:778].astype(np.int64))                  # graph_perm_reverse[:V], ros_demo.py:162
        live = net.live(model, PARAS, clamp=True, perm_reverse=rev, faces=faces,          # -> the step hands over out['mesh']
                        labels="--labels" in opt, left=left)
        run, s_img, s_dep, out = live.graphed(rgb, depth)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            s_img.copy_(synth.make_rgb(1, seed=1000 + i).cuda())                           # (a camera would write here)
            s_dep.copy_(synth.make_depth(1, seed=2000 + i).cuda())
            run()
            torch.cuda.current_stream().synchronize()
            res = out.read()
            kp, has_hand, crop_box, _words, (image_uvd, xyz_mm), mesh = res[:6]
        dt = time.perf_counter() - t0
        cam_mesh = mesh[0]                                                                # out['mesh'] of ros_demo.py:332-337
        print(f"3. live step: {frames} frames, {1e3 * dt / frames:.2f} ms per frame incl. synthetic frame generation; "
              f"mesh {tuple(out.raw_mesh.shape)} -> {tuple(cam_mesh.shape)} camera-frame vertices; has_hand = {has_hand.tolist()}")
        if faces is not None:                                                             # ros_demo.py:341: the mesh_label image
            from PIL import Image
            Image.fromarray(res.overlay[0].numpy()).save(opt["--overlay"])
            shown = s_img[0].flip(-1) if left else s_img[0]                                # (--left: the mirrored frame is drawn on)
            changed = int((res.overlay[0] != (shown * 255).round().byte().permute(1, 2, 0).cpu()).any(dim=2).sum())
            print(f"4. overlay: {tuple(res.overlay.shape)} uint8 RGB in the same copy, {changed} pixels drawn -> {opt['--overlay']}")
        if "--labels" in opt:                                                             # ros_demo.py:310-326: box_label, pose_label
            np.save(opt["--labels"] + "_box.npy", res.box_label[0].numpy())
            np.save(opt["--labels"] + "_pose.npy", res.pose_label[0].numpy())
            print(f"5. labels: box_label {tuple(res.box_label.shape)}, pose_label {tuple(res.pose_label.shape)} uint8 RGB in the same "
                  f"copy -> {opt['--labels']}_box.npy, {opt['--labels']}_pose.npy")
        if handed:                                                                        # a left and a right hand in one frame
            two = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev, handed=True, left_side=0)
            o2 = two.forward_device(s_img, s_dep)
            torch.cuda.current_stream().synchronize()
            r2 = o2.read()
            print(f"6. handed: side per slot {r2.side.tolist()} (-1: empty), mirrored {o2.mirror.tolist()}, lifted {r2.lifted.tolist()}; "
                  f"mesh {tuple(r2.mesh.shape)} in the frame's own coordinates")
        if track:                                                                         # stable slots and ids across frames
            tracked = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev, track=True, track_iou=0.3,
                                     track_hold=5)
            tracked.track_reset()
            run, t_img, t_dep, o3 = tracked.graphed(rgb, depth)
            for i in range(min(frames, 6)):
                t_img.copy_(synth.make_rgb(1, seed=1000 + i // 2).cuda())                  # (every frame twice: ages count up)
                t_dep.copy_(synth.make_depth(1, seed=2000 + i // 2).cuda())
                run()
                torch.cuda.current_stream().synchronize()
                r3 = o3.read()
                print(f"7. track, frame {i}: id per slot {r3.track_id[0].tolist()} (0: free), age {r3.track_age[0].tolist()}, "
                      f"filled {(r3.has_hand[0] != 0).tolist()}, detection {r3.det_index[0].tolist()}")
        if smooth:                                                                        # ... and their signals filtered over time
            smoothed = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev, track=True, smooth=True,
                                      smooth_min_cutoff=1.0, smooth_beta=0.007, smooth_d_cutoff=1.0, smooth_rate=30.0)
            smoothed.track_reset()                                                        # (empties the filters too)
            run, t_img, t_dep, o4 = smoothed.graphed(rgb, depth)
            for i in range(min(frames, 6)):
                t_img.copy_(synth.make_rgb(1, seed=1000 + i // 2).cuda())
                t_dep.copy_(synth.make_depth(1, seed=2000 + i // 2).cuda())
                smoothed.smooth_dt(1 / 30)                                                 # (a camera would give its frame time)
                run()
                torch.cuda.current_stream().synchronize()
                r4 = o4.read()
                print(f"8. smooth, frame {i}: id per slot {r4.track_id[0].tolist()}, |smooth_mesh - mesh| max "
                      f"{1e3 * float((r4.smooth_mesh - r4.mesh).abs().max()):.3f} mm, |smooth_xyz - xyz_mm| max "
                      f"{float((r4.smooth_xyz - r4.xyz_mm).abs().max()):.3f} mm")
        if occlude:                                                                       # the mesh behind nearer scene depth
            hidden = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev,
                                    faces=faces if faces is not None else _faces(opt.get("--mano")), occlude=True,
                                    occlude_margin=0.03)
            o5 = hidden.forward_device(s_img, s_dep)
            torch.cuda.current_stream().synchronize()
            r5 = o5.read()
            for k, (under, seen) in enumerate(r5.coverage[0].tolist()):
                share = f"{seen / under:.1%} shown" if under else "nothing drawn"
                print(f"9. occlude, slot {k}: lifted {bool(r5.lifted[0, k])}, {under} pixels where its mesh is the nearest, {share}")
            print(f"   silhouette {tuple(r5.silhouette.shape)} uint8: {int((r5.silhouette != 0).sum())} pixels under a mesh, "
                  f"{int((r5.silhouette & 0x80 != 0).sum())} of them hidden")
        if "--cameras" in opt:                                                            # a rig of N cameras in ONE step
            n = int(opt["--cameras"])
            cams = np.asarray(PARAS)[None] + 12.0 * np.arange(n)[:, None] * np.array([1.0, -1.0, 1.5, -0.5])     # [N,4]
            rig = net.live_hands(model, cams, max_hands=2, clamp=True, perm_reverse=rev)
            run, c_img, c_dep, o6 = rig.graphed(s_img.expand(n, -1, -1, -1).contiguous(), s_dep.expand(n, -1, -1, -1).contiguous())
            for label, values in (("as built", None), ("after set_cameras", cams[::-1].copy())):
                if values is not None:
                    rig.set_cameras(values)                                               # (no recapture: the kernels read tables)
                run()
                torch.cuda.current_stream().synchronize()
                r6 = o6.read()
                print(f"10. cameras {label}: the same frame through {n} intrinsics in one captured step: wrist x (mm) per camera "
                      f"{[round(float(v), 1) for v in r6.xyz_mm[:, 0, 0, 0]]}, image u {[round(float(v), 1) for v in r6.image_uvd[:, 0, 0, 0]]}")
        if rig_frame:                                                                     # two cameras, one entry per physical hand
            same = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (2, 1, 1))           # camera -> rig [R | t], [N,3,4]
            aside = same.copy()
            aside[1, 0, 3] = 1.0
            two_cams = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev, extrinsics=same, rig_radius=0.08)
            run, r_img, r_dep, o7 = two_cams.graphed(s_img.expand(2, -1, -1, -1).contiguous(), s_dep.expand(2, -1, -1, -1).contiguous())
            for label, values in (("both cameras at one place", None), ("camera 1 a metre aside (set_extrinsics)", aside)):
                if values is not None:
                    two_cams.set_extrinsics(values)                                       # (no recapture: the kernels read the table)
                run()
                torch.cuda.current_stream().synchronize()
                r7 = o7.read()
                wrists = [[round(float(v), 3) for v in r7.fused_xyz[g, 0]] for g in range(r7.rig_count)]
                print(f"11. rig, {label}: {int(r7.lifted.sum())} lifted slots -> {r7.rig_count} rig hands, views "
                      f"{r7.rig_views[:r7.rig_count].tolist()}, rig hand per slot {r7.rig_hand.tolist()}, fused wrist (m, rig frame) {wrists}")
        if cloud:                                                                         # each hand's measured depth points
            cut = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev,
                                 faces=faces if faces is not None else _faces(opt.get("--mano")), occlude=True, cloud=True,
                                 cloud_points=4096, cloud_band=0.03, cloud_stride=2)
            o8 = cut.forward_device(s_img, s_dep)
            torch.cuda.current_stream().synchronize()
            r8 = o8.read()
            for k, ((total, written), resid) in enumerate(zip(r8.cloud_count[0].tolist(), r8.cloud_resid[0].tolist())):
                mean = f"mean residual {resid / total / 1000.0:+.2f} mm" if total else "no point"
                print(f"12. cloud, slot {k}: {total} matching pixels, {written} points written, {mean}")
            print(f"    cloud {tuple(r8.cloud.shape)} fp32 metres (x right, y down, z forward), first point of slot 0 "
                  f"{[round(float(v), 4) for v in r8.cloud[0, 0, 0]]}")
        if fit:                                                                           # each hand's mesh moved onto its depth pixels
            fitted = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev,
                                    faces=faces if faces is not None else _faces(opt.get("--mano")), occlude=True, fit=True,
                                    fit_iters=fit_iters, fit_draw=fit_draw)
            o9 = fitted.forward_device(s_img, s_dep)
            torch.cuda.current_stream().synchronize()
            r9 = o9.read()
            words = {0: "fitted", 1: "too few matches", 2: "no solution", 3: "beyond the caps"}
            for k, ((matches, status), cost) in enumerate(zip(r9.fit_count[0].tolist(), r9.fit_cost[0].tolist())):
                rms = f"{1000.0 * (cost / 2 ** 30 / matches) ** 0.5:.2f} mm" if matches else "-"
                print(f"13. fit, slot {k}: {matches} matching pixels, {words[status]}, RMS residual before {rms}, shift (mm) "
                      f"{[round(1000.0 * float(v), 2) for v in r9.fit_rt[0, k, 9:]]}")
                for t, (m, st, c) in enumerate(r9.fit_trace[0, k].tolist() if fit_iters > 1 else ()):
                    print(f"    step {t + 1}: {m} matching pixels, {words[st]}, RMS residual before "
                          + (f"{1000.0 * (c / 2 ** 30 / m) ** 0.5:.2f} mm" if m else "-"))
            if fit_draw:
                plain = net.live_hands(model, PARAS, max_hands=2, clamp=True, perm_reverse=rev, faces=fitted.faces.cpu().numpy(),
                                       occlude=True, fit=True, fit_iters=fit_iters).forward_device(s_img, s_dep)
                torch.cuda.current_stream().synchronize()
                moved = int((plain.read().silhouette != r9.silhouette).sum())
                print(f"    fit_draw: overlay and silhouette are drawn from the fitted mesh; {moved} silhouette pixels differ from "
                      "the unfitted mesh's")


if __name__ == "__main__":
    main()
