"""Drop-in `handnet_pipeline.handnet_pipeline.HandNet` (alias `HandNetPipeline`) on MI355X.

Constructor and call contract of handnet_pipeline/handnet_pipeline.py:38-116:

    net = HandNet(args, reload_detector=True, num_classes=3, reload_a2j=True, RGBD=False).cuda().eval()
    keypoints, depth_batch, crops = net(images, depth_images=depth)        # ros_demo.py:270,388

  keypoints   FloatTensor [N,21,3] on the CPU (zero rows for frames without a hand)
  depth_batch [K,1,176,176] on the model device, K = frames with a hand
  crops       [K,4] int64 on the model device (padded, clamped x1,y1,x2,y2)
  no frame with a hand: (zeros[N,21,3], zeros_like(depth_images), zeros[N,4] float32 on the CPU)
  is_detect or is_3D: returns None (the reference has no such branch either).

Beyond the reference: net.forward_hands(images, depth, max_hands=K) poses the first K hand detections of every frame
(the reference keeps the first, :84-85) -> keypoints [N,K,21,3], depth_batch of the filled slots, boxes [N,K,4], hand_mask
[N,K], scores [N,K].

Documented deviations: a batch that MIXES frames with and without a hand raises in the
reference (torch.stack of a list containing None, :82,111) and an empty crop slice reuses
the previous frame's crop (:100-105); here such frames simply count as "no hand".
"""
from __future__ import annotations

import math
import os

import torch

from a2j.a2j import A2JModel
from fcos_utils.fcos import FCOS
from a2j.a2j import A2JModelLightning
from hn_amd import ops
from hn_amd.pipeline import HandNetEngine, check_range_contract
from hn_amd.state import EngineOwner


def load_pretrained_fcos(args, reload_detector=False, num_classes=2):
    detector = FCOS(num_classes=num_classes, ext=False, nms_thresh=0.5)
    if reload_detector:
        checkpoint = torch.load(args.pretrained_fcos, map_location="cpu")
        detector.load_state_dict(checkpoint["model"], strict=False)
    for p in detector.parameters():
        p.requires_grad = False
    return detector


def load_pretrained_a2j(args, reload_a2j=False, RGBD=False):
    """handnet_pipeline.py:25-36: RGBD or a path containing 'ckpt' -> Lightning checkpoint through
    A2JModelLightning.load_from_checkpoint (the file's hyper_parameters decide the stem width); else A2JModel +
    optional {"model": sd}."""
    if RGBD or "ckpt" in str(args.pretrained_a2j):
        return A2JModelLightning.load_from_checkpoint(args.pretrained_a2j).eval()
    a2j = A2JModel(21, crop_height=176, crop_width=176, is_RGBD=False)
    if reload_a2j:
        checkpoint = torch.load(args.pretrained_a2j, map_location="cpu")
        a2j.load_state_dict(checkpoint["model"], strict=False)
    for p in a2j.parameters():
        p.requires_grad = False
    return a2j


class HandNet(EngineOwner):
    """End-to-End HandNet: FCOS hand detector -> depth crop -> A2J keypoints."""

    def __init__(self, args, reload_detector: bool = False, num_classes: int = 2, reload_a2j: bool = False,
                 RGBD: bool = False):
        super().__init__()
        self.detector = load_pretrained_fcos(args, reload_detector, num_classes)
        self.detector.eval()
        self.a2j = load_pretrained_a2j(args, reload_a2j, RGBD)
        # the reference keeps the caller's flag (handnet_pipeline.py:55); a Lightning checkpoint knows its own stem
        self.RGBD = bool(self.a2j.rgbd) if isinstance(self.a2j, A2JModelLightning) else bool(RGBD)
        self.num_classes = num_classes
        self._auto_graph_allowed = os.environ.get("HN_AUTO_GRAPH", "1") != "0"

    def engine(self) -> HandNetEngine:
        # the per-call path: the engines stand and belong to the sub-modules' CURRENT state -- load_state_dict() and every
        # device / dtype move (nn.Module._apply) reset a sub-module's engine (hn_amd/state.py), which this test sees.  (Walking
        # the three parameter trees for their device on every call was 20 us of the ~90 us the call costs beyond its GPU time.)
        eng = self._engine
        if (eng is not None and getattr(self.detector, "_engine", None) is eng.fcos
                and getattr(self.a2j, "_engine", None) is eng.a2j):
            return eng
        self._require_gpu()
        fcos, a2j = self.detector.engine(), self.a2j.engine()
        # the sub-modules rebuild their engines when THEIR weights change (net.detector.load_state_dict(...)):
        # never keep running a holder of stale ones
        if self._engine is None or self._engine.fcos is not fcos or self._engine.a2j is not a2j:
            self._engine = HandNetEngine(fcos, a2j, self.num_classes)
            if getattr(self, "_convert_cfg", None) is not None:
                self._engine.set_convert(*self._convert_cfg)
        return self._engine

    def set_convert(self, paras=None, clamp: bool = False, on: bool = True):
        """What the reference's caller does with every result (ros_demo.py:279-290,329-330: clamp, convert_joints to image
        (u,v,d), uvd2xyz to camera millimetres) as part of the step: the aggregation's own launch writes them and the call's one
        device -> host record carries them.  After each forward(): `net.last_converted` = {"image_uvd": [N,21,3] CPU,
        "xyz_mm": [N,21,3] CPU or None (no intrinsics)}; forward()'s tuple itself is unchanged.  paras = (fx, fy, cx, cy), or a
        camera per frame [N,4] (frame i is converted with row i; a call over another number of frames raises ValueError)."""
        paras = ops.camera_paras(paras)
        self._convert_cfg = (paras, bool(clamp)) if on else None
        if self._engine is not None:
            self._engine.set_convert(paras, clamp, on)
        self.last_converted = None
        return self

    def live(self, lifter, paras, clamp: bool = True, perm_reverse=None, faces=None, labels: bool = False, left: bool = False,
             occlude: bool = False, occlude_margin: float = 0.03, fit_iters: int = 1, fit_draw: bool = False,
             cloud: bool = False, cloud_points: int = 4096,
             cloud_band: float = 0.03, cloud_stride: int = 2, fit: bool = False, fit_band: float = 0.03, fit_stride: int = 2,
             fit_min_points: int = 200, fit_damp: float = 1e-3, fit_max_shift: float = 0.05, fit_max_angle: float = 0.35):
        """The live caller's chain as ONE step (hn_amd.live.LiveHandEngine; ros_demo.py:270-290,329-337): this network, the
        caller's clamp + convert_joints (in the aggregation's epilogue), the lifter's input, Pose2Mesh, one device -> host copy.
        lifter: the drop-in `models.pose2mesh_net.get_model(...)` module (on the GPU) or a Pose2MeshEngine; paras = (fx, fy,
        cx, cy), or a camera per frame [N,4] (a nested sequence, an ndarray or a tensor, rounded to fp32): the step then takes
        exactly N frames, frame i is converted and drawn with row i, and engine.set_cameras(new [N,4]) changes the values
        without recapturing anything; perm_reverse = graph_perm_reverse[:V]: the step then also does ros_demo.py:162,332-337 and hands over out['mesh'].
        faces = mesh_model.face (needs perm_reverse): the step also draws the mesh over the frame, the caller's render()
        (ros_demo.py:86-116,341): out.overlay on the device, read().overlay on the host.
        labels: the step also draws the caller's other two images (ros_demo.py:310-326): box_label (the frame with the crop
        box) and pose_label (the 176 x 176 colour crop with the skeleton), out.box_label / .pose_label, read() likewise.
        left: the caller's ImageListener(left=True) (ros_demo.py:259-262): frame and depth map are mirrored along the width
        before anything else runs -- inside the ingest kernel for forward_raw -- and every result is in the mirrored frame.
        occlude (needs faces): the overlay leaves out the mesh where it lies more than occlude_margin metres behind the step's
        own depth map (holes -- 0, NaN -- hide nothing), and read() ends with silhouette [N,H,W] uint8 (0 no mesh, 1 shown,
        0x81 hidden) and coverage [N,2] int32 (pixels under the mesh, of those shown).  0.03 m is a starting value, NOT tuned.
        cloud (needs occlude): the step also cuts the hand's measured depth pixels out of its depth map --
        every cloud_stride-th row and column under the silhouette whose depth lies within cloud_band metres of the mesh --
        and read() ends with cloud [N,P,3] fp32 (P = cloud_points; metres in the camera frame of xyz_mm, x right, y down, z
        forward, the pixel centre at +0.5; the first P matches in row-major order, zero rows behind them), cloud_count [N,2]
        int32 (matches, rows written) and cloud_resid [N] int64 (the summed depth - mesh Z over all matches, micrometres).
        cloud_points = 4096, cloud_band = 0.03 m and cloud_stride = 2 are starting values, NOT tuned on this model.
        fit (needs occlude): the step also fits the hand's mesh to its measured depth -- one Gauss-Newton
        step of point-to-plane alignment over every fit_stride-th row and column under the silhouette whose depth lies within
        fit_band metres of the mesh -- and read() ends with fit_mesh [N,V,3], fit_xyz [N,21,3] (camera millimetres), fit_rt
        [N,12] fp32 (R row-major, then t in metres: the motion about the root joint, camera frame), fit_count [N,2] int32
        (matches, status: 0 fitted, 1 fewer than fit_min_points matches, 2 no solution, 3 beyond fit_max_shift metres or
        fit_max_angle radians: the mesh is left as it is) and fit_cost [N] int64 (the summed squared residual, 2^-30 m^2).
        fit_iters = I (1..8) runs I such steps, the moved mesh drawn again before every further one;
        read() then also ends with fit_trace [N,I,3] int64 (matches, status, cost of every step; I >= 2).  fit_draw=True draws
        the overlay, silhouette and coverage, and cuts the cloud, from the fitted mesh.  Either without fit=True: ValueError.
        fit_band = 0.03 m, fit_stride = 2, fit_min_points = 200, fit_damp = 1e-3, fit_max_shift = 0.05 m and fit_max_angle =
        0.35 rad are starting values, NOT tuned on this model.
        The returned engine owns this network's step from then on (forward() of this module keeps working and
        carries the converted joints: set_convert)."""
        from hn_amd.live import LiveHandEngine
        paras = ops.camera_paras(paras)
        self._convert_cfg = (paras, bool(clamp))
        return LiveHandEngine(self.engine(), lifter.engine() if hasattr(lifter, "engine") else lifter, paras, clamp, perm_reverse,
                              faces, labels, left, occlude, occlude_margin, fit_iters=fit_iters, fit_draw=fit_draw, cloud=cloud,
                              cloud_points=cloud_points, cloud_band=cloud_band, cloud_stride=cloud_stride, fit=fit,
                              fit_band=fit_band, fit_stride=fit_stride, fit_min_points=fit_min_points, fit_damp=fit_damp,
                              fit_max_shift=fit_max_shift, fit_max_angle=fit_max_angle)

    def live_hands(self, lifter, paras, max_hands: int = 2, clamp: bool = True, perm_reverse=None, faces=None,
                   labels: bool = False, left: bool = False, handed: bool = False, left_side: int = 0, track: bool = False,
                   track_iou: float = 0.3, track_hold: int = 5, occlude: bool = False, occlude_margin: float = 0.03,
                   objects: bool = False, object_band: float = 0.15, object_stride: int = 2, object_min_points: int = 50,
                   extrinsics=None, rig_radius: float = 0.08, fit_iters: int = 1, fit_draw: bool = False, cloud: bool = False,
                   cloud_points: int = 4096,
                   cloud_band: float = 0.03, cloud_stride: int = 2, cloud_frame: str = "camera", fit: bool = False,
                   fit_band: float = 0.03, fit_stride: int = 2, fit_min_points: int = 200, fit_damp: float = 1e-3,
                   fit_max_shift: float = 0.05, fit_max_angle: float = 0.35,
                   smooth: bool = False, smooth_min_cutoff: float = 1.0, smooth_beta: float = 0.007, smooth_d_cutoff: float = 1.0,
                   smooth_rate: float = 30.0):
        """live() for up to max_hands (1..16) hands per frame (hn_amd.live.LiveHandsEngine): forward_hands' slots, the
        caller's clamp + convert_joints, the lifter's input with the caller's skip rule per slot (a hand whose 2D box
        process_bbox refuses is not lifted: ros_demo.py:288-300), Pose2Mesh on every slot, one device -> host copy.
        read() of a step's output gives keypoints / boxes / scores per slot, `lifted` [N,K] and the mesh [N,K,V,3].
        paras: as for live(); with a camera per frame [N,4], all K slots of frame i use row i.
        faces = mesh_model.face (needs perm_reverse): every lifted mesh of a frame is drawn over it (one depth buffer per frame):
        out.overlay / read().overlay [N,H,W,3] uint8 RGB.
        labels: as for live(): box_label [N,H,W,3] with the crop box of every lifted slot, pose_label [N,K,176,176,3] (zeros
        where the slot is not lifted).
        left: as for live().  handed: per-slot handedness instead -- read().side is the detector's side of every slot and a
        slot whose side equals left_side goes mirrored through the right-handed A2J and Pose2Mesh and comes back un-mirrored, so
        a left hand's mesh has its thumb on the right side; no launch is added.  left_side = 0 assumes the 100DOH
        convention of the detector's training targets, which the reference does not state.  left with handed: ValueError.
        track: the slots are tracked from step to step (batch row i = one camera stream): a hand keeps its slot and its
        read().track_id while its padded box overlaps the slot's last one with IoU >= track_iou, a slot whose hand is missing is
        held empty for track_hold steps, and max_hands=1 sticks to its hand instead of jumping to the top score
        (engine.track_reset() starts over).
        smooth (needs track and perm_reverse): the tracked slots' xyz_mm and final mesh are also filtered over time on the
        device (a One Euro filter per coordinate, inside the step's last mesh launch): read().smooth_xyz [N,K,21,3] and
        read().smooth_mesh [N,K,V,3] behind track_id, and the overlay is drawn from smooth_mesh; everything else stays
        unfiltered.  smooth_min_cutoff, smooth_beta (per mm/s), smooth_d_cutoff and smooth_rate (steps per second) are the
        paper's starting values, NOT tuned on this model; engine.smooth_dt(seconds) follows the camera's real frame time and
        engine.smooth_reset() restarts the filters.  max_hands=1, track=True, smooth=True is the smoothed sticky top-1.
        occlude (needs faces): as live()'s, for all K slots against the frame's one depth map: read() ends with silhouette
        [N,H,W] uint8 (0 no mesh, k + 1 slot k shown, 0x80 | (k + 1) hidden) and coverage [N,K,2] int32 (per slot: pixels where
        its mesh is the nearest, of those shown).  occlude_margin = 0.03 m is a starting value, NOT tuned on this model.
        extrinsics (needs perm_reverse): a rig of N cameras -- one camera -> rig transform [R | t] per
        frame, [N,3,4] or [N,4,4] (t in metres), N * max_hands <= 256.  read() then ends with the hands in the rig frame
        (rig_xyz [N,K,21,3], rig_mesh [N,K,V,3], metres), one entry per physical hand (rig_hand [N,K], rig_count, rig_views,
        rig_seed: lifted slots of different frames within rig_radius metres of each other, with handed=True of one side) and
        their score-weighted fusion (fused_xyz, fused_mesh [N*K,...]); engine.set_extrinsics(new) changes the values without
        recapturing anything.  rig_radius = 0.08 m is a starting value, NOT tuned on this model.  left=True: ValueError.
        cloud (needs occlude): as live()'s, per slot: read() ends with cloud [N,K,P,3], cloud_count
        [N,K,2] and cloud_resid [N,K]; cloud_frame="rig" (needs extrinsics) hands the points out in the rig frame.
        cloud_points = 4096, cloud_band = 0.03 m and cloud_stride = 2 are starting values, NOT tuned on this model.
        fit (needs occlude): as live()'s, per slot: read() ends with fit_mesh [N,K,V,3], fit_xyz
        [N,K,21,3], fit_rt [N,K,12], fit_count [N,K,2] and fit_cost [N,K]; fit_iters / fit_draw as
        live()'s, fit_trace [N,K,I,3].  fit_band = 0.03 m, fit_stride = 2, fit_min_points =
        200, fit_damp = 1e-3, fit_max_shift = 0.05 m and fit_max_angle = 0.35 rad are starting values, NOT tuned on this model.
        objects (needs paras and a detector built with ext=True): the step also says what every hand holds
        -- read() ends with contact and object_index [N,K], object_box [N,K,4], object_score [N,K], object_point [N,K,2],
        object_xyz [N,K,3], object_extent [N,K,6] and object_count [N,K,2]: each slot's contact state, the detector's object its
        offset vector points at (the reference's evaluation rule, voc_eval.py:687-699) and the centroid and extent of that
        object's depth pixels in the camera frame, inside the captured step and its one copy; with labels, box_label also shows
        the object's rectangle and the link line.  object_band = 0.15 m, object_stride = 2 and object_min_points = 50 are
        starting values, NOT tuned on any model; contact state > 0 = in contact is 100DOH's numbering, to be checked against the
        checkpoint.  A detector without the ext heads: ValueError."""
        from hn_amd.live import LiveHandsEngine
        k = ops.check_max_hands(max_hands)
        if objects and not getattr(self.detector, "ext", False):
            raise ValueError("live_hands(objects=True) needs the detector's contact heads: assign a FCOS(num_classes=..., ext=True, "
                             "nms_thresh=0.5) to net.detector and load its weights")
        if left and handed:
            raise ValueError("left=True mirrors the whole frame and handed=True mirrors the left-hand slots: give one of them")
        paras = ops.camera_paras(paras)
        self._convert_cfg = (paras, bool(clamp))
        return LiveHandsEngine(self.engine(), lifter.engine() if hasattr(lifter, "engine") else lifter, paras, k, clamp,
                               perm_reverse, faces, labels, left, handed, left_side, track, track_iou, track_hold,
                               occlude=occlude, occlude_margin=occlude_margin, extrinsics=extrinsics, rig_radius=rig_radius,
                               fit_iters=fit_iters, fit_draw=fit_draw, cloud=cloud, cloud_points=cloud_points, cloud_band=cloud_band, cloud_stride=cloud_stride,
                               cloud_frame=cloud_frame, fit=fit, fit_band=fit_band, fit_stride=fit_stride,
                               fit_min_points=fit_min_points, fit_damp=fit_damp, fit_max_shift=fit_max_shift,
                               fit_max_angle=fit_max_angle,
                               smooth=smooth, smooth_min_cutoff=smooth_min_cutoff,
                               smooth_beta=smooth_beta, smooth_d_cutoff=smooth_d_cutoff, smooth_rate=smooth_rate,
                               objects=objects, object_band=object_band, object_stride=object_stride,
                               object_min_points=object_min_points)

    # forward() switches ITSELF to hipGraph replay once the same input shapes have come in a few times in a row -- the live
    # caller's case (ros_demo.py:270-273: one 640x480 frame per call, ~150 dependent launches whose host cost is 8 % of the
    # call; at batch 32 the replay saves the ~0.3 ms the GPU idles while Python issues the first launches after the sync).
    # forward() hands out fresh tensors (keypoints on the CPU, copies of the crops), so replaying into captured buffers is
    # invisible to the caller; enable_graph(False) turns it off, enable_graph(True) forces it from the first call and also for
    # forward_device().
    AUTO_GRAPH_CALLS = 3        # same-shape calls in a row before forward() captures
    AUTO_GRAPH_MAX_SHAPES = 4   # captured steps kept at a time (each holds its own static activation pool): one more input
    #                             shape EVICTS the least recently used capture (a batch-size-sweeping caller stays bounded)
    # HN_AUTO_GRAPH=0 in the environment keeps forward() eager; a capture that FAILS (no memory for the static pool, a
    # capture-unsafe call from another thread of the host) is not an error of the call: forward() runs that call eagerly and
    # never tries again (self._auto_graph_allowed = False), see _forward_auto.
    # A SPARSE stream (a hand in fewer than half of the frames of a batch of >= 8: forward() sees the flags on the CPU anyway)
    # stays eager, because the engine then runs A2J on the frames with a hand only and that path is data dependent.

    def enable_graph(self, on=True):
        """hipGraph replay: the first call with a given input shape captures the whole step, later calls copy the inputs
        into the captured buffers and replay (no per-launch host cost; the launch sequence is static by construction).
        on=True: always (results of forward_device() then alias the captured output buffers and are overwritten by the next
        call; forward() returns fresh tensors either way); on=False: never; on=None: the default -- forward() decides by
        itself (see AUTO_GRAPH_*), forward_device() stays eager."""
        self.use_graph = None if on is None else bool(on)
        if on:
            self._auto_graph_allowed = True
        return self

    def _auto_graph(self, image_shape, depth_shape, on_gpu=True, hands=None, handed=(False, 0), tracked=None) -> bool:
        """Whether this call of forward() (hands = K: of forward_hands()) should run as a graph replay (capturing first if
        need be)."""
        eng = self.engine()
        sparse = getattr(self, "_last_sparse" if hands is None else "_last_sparse_hands", False)
        if not self._auto_graph_allowed or eng.check_range or sparse or not on_gpu:
            return False
        if (eng.has_graph(image_shape, depth_shape, to_host=True) if hands is None
                else eng.has_graph_hands(image_shape, depth_shape, hands, to_host=True, handed=handed[0], left_side=handed[1],
                                         **(tracked or {}))):
            return True
        key = (tuple(image_shape), tuple(depth_shape)) + (() if hands is None else (hands,)) + (handed if handed[0] else ())
        key += tuple(sorted((tracked or {}).items()))
        if key == getattr(self, "_streak_key", None):
            self._streak += 1
        else:
            self._streak_key, self._streak = key, 1
        return self._streak > self.AUTO_GRAPH_CALLS

    def forward_device(self, images, depth_images, _graph=None, _to_host=False):
        """Sync-free variant: returns hn_amd.pipeline.HandNetOutput with everything on the GPU."""
        batch = images if torch.is_tensor(images) else torch.stack([i.float() for i in images])
        if getattr(self, "use_graph", None) if _graph is None else _graph:
            batch, depth = batch.float().contiguous(), depth_images.float().contiguous()
            run, s_img, s_dep, out = self.engine().graphed(batch, depth, to_host=_to_host, limit=self.AUTO_GRAPH_MAX_SHAPES)
            s_img.copy_(batch)
            s_dep.copy_(depth)
            run()
            return out
        return self.engine().forward_device(batch, depth_images, to_host=_to_host)

    def _forward_auto(self, images, depth_images, n):
        """forward() in its default mode: replay when a captured step fits, capture when the shapes have repeated, else eager."""
        eng = self.engine()
        if (self._auto_graph_allowed and not torch.is_tensor(images) and n and depth_images.is_cuda
                and depth_images.dtype == torch.float32 and all(i.dtype == torch.float32 and i.is_cuda for i in images)
                and not eng.check_range and not getattr(self, "_last_sparse", False)):
            out = eng.replay_frames(images, depth_images, to_host=True)
            if out is not None:
                return out
        batch = images if torch.is_tensor(images) else torch.stack([i.float() for i in images])
        return self._graph_or_eager(self._auto_graph(batch.shape, depth_images.shape, batch.is_cuda and depth_images.is_cuda),
                                    lambda: self.forward_device(batch, depth_images, _graph=True, _to_host=True),
                                    lambda: self.forward_device(batch, depth_images, _graph=False, _to_host=True))

    def _graph_or_eager(self, graph, captured, eager, passing=()):
        """The one capture ladder of forward(), forward_hands() and forward_raw(): graph -> captured() (capture if need be, and
        replay), else eager().  A RangeError (and the caller's `passing`: errors of its arguments) always propagates, and so
        does every failure in the forced mode (enable_graph(True)); in the automatic mode any other failure of captured()
        ends capturing for good (_capture_failed) and the call runs eagerly."""
        if graph:
            try:
                return captured()
            except (ops.RangeError,) + passing:
                raise
            except Exception as e:  # noqa: BLE001 -- whatever made the capture fail, this call would succeed eagerly
                if getattr(self, "use_graph", None):
                    raise
                self._capture_failed(e)
        return eager()

    def _capture_failed(self, e):
        import warnings
        self._auto_graph_allowed = False
        torch.cuda.synchronize()
        warnings.warn(f"HandNet: automatic hipGraph capture failed ({type(e).__name__}: {e}); "
                      "staying eager from now on (enable_graph(True) forces a new attempt)")

    def forward(self, images, depth_images=None, is_3D: bool = False, is_detect: bool = False):
        if is_detect or is_3D:
            return None
        if depth_images is None:
            raise ValueError("depth_images is required for the ensemble inference branch")
        n = len(images)
        mode = getattr(self, "use_graph", None)
        if mode is None and torch.is_tensor(depth_images):
            out = self._forward_auto(images, depth_images, n)
        else:
            out = self.forward_device(images, depth_images, _to_host=True)
        return self._finish(out, n, depth_images)

    def forward_hands(self, images, depth_images, max_hands: int = 2, is_3D: bool = False, is_detect: bool = False,
                      handed: bool = False, left_side: int = 0, track: bool = False, track_iou: float = 0.3,
                      track_hold: int = 5):
        """forward() for up to max_hands (1..16) hands per frame.  Slot k of frame i is the k-th hand-class detection of
        frame i in the detector's score order (the reference keeps slot 0 only, handnet_pipeline.py:84-85), padded and
        cropped as forward() crops it.  images / depth_images as forward() takes them.  Returns
          keypoints   [N,K,21,3] fp32 on the CPU (zero rows for empty slots)
          depth_batch [M,1,176,176] (RGB-D: [M,4,176,176]) on the model device: the crops of the M filled slots, frame-major
                      then rank order ([0,...] when no slot is filled)
          boxes       [N,K,4] int64 on the CPU (padded, clamped x1,y1,x2,y2; zeros for empty slots)
          hand_mask   [N,K] bool on the CPU
          scores      [N,K] fp32 on the CPU (the detections' scores; 0 for empty slots)
        One device -> host copy and one sync per call; repeated shapes switch to graph replay as forward() does.
        handed: a sixth result, sides [N,K] int32 on the CPU (the detector's side of the slot's detection, -1 for empty slots),
        and a slot whose side equals left_side goes through the right-handed A2J mirrored (its crop in depth_batch is flipped
        along the width) and its keypoints come back un-mirrored (u = 176 - u).  left_side = 0 assumes the 100DOH convention
        of the detector's training targets, which the reference does not state.
        track: the slots are tracked from call to call (engine().forward_hands(track=True); engine().track_reset() starts
        over) and two more results end the tuple: track_id and track_age [N,K] int32 on the CPU."""
        if is_detect or is_3D:
            return None
        if depth_images is None:
            raise ValueError("depth_images is required for the ensemble inference branch")
        k = ops.check_max_hands(max_hands)
        handed, left_side = bool(handed), int(left_side)
        tracked = dict(track=True, track_iou=track_iou, track_hold=track_hold) if track else {}
        if track:
            ops.check_track_options(track_iou, track_hold)
        eng = self.engine()
        n = len(images)
        dev = eng.device
        batch = images if torch.is_tensor(images) else torch.stack([i.float() for i in images])
        batch, depth = batch.to(dev).float().contiguous(), depth_images.to(dev).float().contiguous()
        mode = getattr(self, "use_graph", None)
        graph = bool(mode) if mode is not None else self._auto_graph(batch.shape, depth.shape, True, hands=k,
                                                                     handed=(handed, left_side), tracked=tracked)

        def captured():
            run, s_img, s_dep, out = eng.graphed_hands(batch, depth, k, to_host=True, limit=self.AUTO_GRAPH_MAX_SHAPES,
                                                       handed=handed, left_side=left_side, **tracked)
            s_img.copy_(batch)
            s_dep.copy_(depth)
            run()
            return out
        out = self._graph_or_eager(graph, captured, lambda: eng.forward_hands(batch, depth, k, to_host=True, handed=handed,
                                                                              left_side=left_side, **tracked))
        return self._finish_hands(out, n, k, depth, handed, bool(track))

    def _finish_hands(self, out, n, k, depth, handed=False, tracked=False):
        """forward_hands()'s tuple from the step's one host record (see _finish)."""
        from hn_amd.pipeline import read_hands_tail
        rows = n * k
        sel = out.crops_nhwc
        depth_all = (sel.permute(0, 3, 1, 2) if self.RGBD else sel[..., 0].unsqueeze(1)).contiguous()
        kp, box, mask, filled = self._read_step(out, (n, k), "_last_sparse_hands", depth)
        scores, _, *sides = read_hands_tail(out.host_record, rows, handed, tracked)      # (sides: + the track ids and ages)
        if filled == rows:
            depth_batch = depth_all
        else:
            depth_batch = depth_all.index_select(0, mask.nonzero().flatten().to(depth_all.device))
        return (kp, depth_batch, box, mask.view(n, k), scores.view(n, k)) + tuple(sd.view(n, k) for sd in sides)

    def forward_raw(self, bgr_u8, depth_raw, is_3D: bool = False, is_detect: bool = False):
        """The reference caller's ingest AND its network call in one (ros_demo.py:227-231,266-273): bgr_u8 = the cv_bridge
        'bgr8' frames, uint8 [N,H,W,3] (or one [H,W,3] frame); depth_raw = 16UC1 millimetres as uint16 [N,H,W] or 32FC1 metres
        as float32 -- numpy arrays or torch tensors, on the host (pinned memory is read in place over PCIe, pageable memory is
        staged once) or on the GPU.  One kernel does `astype(float32) / 255.0`, BGR -> RGB, HWC -> CHW and `/ 1000.0` (bit-identical
        to the host arithmetic; 1.5 MB per frame cross PCIe instead of 4.9 MB) and the step runs exactly as forward() runs it.
        Returns forward()'s tuple; its no-hand placeholder `zeros_like(depth_images)` has the fp32 [N,1|4,H,W] shape forward()
        would have been given."""
        if is_detect or is_3D:
            return None
        bgr = torch.as_tensor(bgr_u8)
        dep = torch.as_tensor(depth_raw)
        if bgr.dim() == 3:
            bgr = bgr.unsqueeze(0)
        if dep.dim() == 2:
            dep = dep.unsqueeze(0)
        if dep.dim() == 4 and dep.shape[1] == 1:
            dep = dep[:, 0]
        n, h, w = bgr.shape[0], bgr.shape[1], bgr.shape[2]
        eng = self.engine()
        shapes = ((n, 3, h, w), (n, 4 if self.RGBD else 1, h, w))
        mode = getattr(self, "use_graph", None)
        graph = bool(mode) if mode is not None else self._auto_graph(*shapes)
        out = self._graph_or_eager(
            graph, lambda: eng.forward_raw(bgr, dep, to_host=True, use_graph=True, limit=self.AUTO_GRAPH_MAX_SHAPES),
            lambda: eng.forward_raw(bgr, dep, to_host=True), passing=(TypeError, ValueError))
        return self._finish(out, n, None, placeholder_shape=shapes[1])

    def _read_step(self, out, lead, sparse_hint, inputs):
        """What _finish and _finish_hands share: wait for the step, read its host record (rows = the product of `lead`: (N,) or
        (N, K)), fill last_converted after set_convert(), set the sparse hint `sparse_hint` for the next call and apply the
        f16x3 range contract to what has just been copied (hn_amd.pipeline.check_range_contract: overflow raises, non-finite
        depth pixels give NaN rows like the reference).  -> (keypoints lead + [J,3], boxes lead + [4], mask [rows], filled)."""
        from hn_amd.pipeline import read_host_record
        torch.cuda.current_stream(out.keypoints.device).synchronize()
        rows, per = math.prod(lead), lead + tuple(out.keypoints.shape[-2:])
        kp, has, box, words, more = read_host_record(out.host_record, rows, per[-2], extras=True)
        if out.image_uvd is not None:
            self.last_converted = {"image_uvd": more[0].view(per), "xyz_mm": more[1].view(per) if len(more) > 1 else None}
        mask = has != 0
        filled = int(mask.sum())
        setattr(self, sparse_hint, rows >= 8 and filled * 2 < rows)      # (the engine's own threshold for compaction)
        check_range_contract(kp, words if out.range_flags is not None else None, inputs, has_hand=has)
        return kp.view(per), box.view(lead + (4,)), mask, filled

    def _finish(self, out, n, depth_images, placeholder_shape=None):
        """The reference's return tuple from a step's device results: ONE device -> host copy (and sync) per call -- the
        step's record buffer (keypoints, has-hand flags, crop boxes, range-contract words), which the step has already enqueued
        into pinned memory."""
        # the usual case -- every frame has a hand -- needs fresh copies of the crop boxes and the depth crops; they are
        # enqueued BEFORE the sync (hidden behind the step instead of trailing it) and thrown away in the other cases
        # (.contiguous() of the permuted / sliced view is a copy: the caller never holds a view of a captured buffer)
        sel = out.crops_nhwc
        crops_all = out.crop_box.clone()
        depth_all = (sel.permute(0, 3, 1, 2) if self.RGBD else sel[..., 0].unsqueeze(1)).contiguous()
        final_results, _box, mask_cpu, hands = self._read_step(out, (n,), "_last_sparse", depth_images)
        if hands == 0:  # handnet_pipeline.py:107-108: the crops placeholder is a CPU float tensor
            zeros = torch.zeros_like(depth_images) if depth_images is not None else torch.zeros(
                placeholder_shape, device=out.keypoints.device)
            return torch.zeros((n, 21, 3)), zeros, torch.zeros((n, 4))
        if hands == n:
            return final_results, depth_all, crops_all
        idx = mask_cpu.nonzero().flatten().to(out.crop_box.device)
        return final_results, depth_all.index_select(0, idx), crops_all.index_select(0, idx)


HandNetPipeline = HandNet
