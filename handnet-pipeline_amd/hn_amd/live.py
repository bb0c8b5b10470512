"""The live caller's whole chain as ONE captured step (ros_demo.py:270-290,329-337):

    HandNet (FCOS -> crop -> A2J)                                  handnet_pipeline.py:58-116
      -> clamp + convert_joints: image (u,v), camera xyz in mm     ros_demo.py:279-283,329-330 -- the aggregation's epilogue
      -> the lifter's input (bbox / affine / standardisation)      ros_demo.py:148-157        -- hn_joints2d_standardize_f32
      -> Pose2Mesh (PoseNet MLP + Chebyshev graph convolutions)    ros_demo.py:161, pose2mesh/lib/models/*
      -> ONE device -> host copy: the wide per-frame records (crop box, flags, crop uvd, image uvd, xyz) + the mesh vertices

Everything between the frame and the copy is a static launch sequence on the device: one hipGraph, no host round trip between
the pose network and the lifter (the reference copies the keypoints to the CPU, converts them in numpy and uploads the
normalised joints again, per frame).  What stays the caller's: the vertex permutation / camera offset of the final mesh
(`pred_mesh[:, graph_perm_reverse[:V]]`, `mesh * 1000 + joints3d[0]`, ros_demo.py:162,332-337) -- the step hands over what
`model(joint_img)` and `convert_joints` return.

`CropMeshEngine` is the same chain without the detector, for the reference's stand-alone mesh demo (a2j_mesh.py:58-80): dataset
crops + the dataset's float32 boxes + per-sample intrinsics -> A2J -> clip + convert -> lifter input -> Pose2Mesh -> final mesh.
"""
from __future__ import annotations

import collections
from dataclasses import dataclass

import torch

from . import ops
from .pipeline import (HandNetEngine, HandNetOutput, HandsOutput, hands_record_rows, read_hands_tail, read_host_record,
                       record_bytes)
from .pose2mesh_engine import Pose2MeshEngine


def _same_device(a, b) -> bool:
    """"cuda" and "cuda:<current device>" name the same card"""
    a, b = torch.device(a), torch.device(b)
    index = lambda d: d.index if d.index is not None else torch.cuda.current_device()
    return a.type == b.type and (a.type != "cuda" or index(a) == index(b))


def _final_mesh_perm(perm_reverse, lifter, device):
    """(perm_reverse as int64 on the device -- None stays None --, vertices of the mesh the step hands over): the indices must
    lie inside the lifter's finest graph."""
    if perm_reverse is None:
        return None, lifter.graphs[0].v
    perm = torch.as_tensor(perm_reverse).to(torch.int64).to(device).contiguous()
    if int(perm.max()) >= lifter.graphs[0].v or int(perm.min()) < 0:
        raise ValueError("perm_reverse points outside the lifter's finest graph")
    return perm, int(perm.shape[0])


def _read_type(name, fields, doc, **absent):
    """A namedtuple whose absent images (overlay / box_label / pose_label) read as None class attributes."""
    return type(name, (collections.namedtuple(name, fields),), dict(absent, __slots__=(), __doc__=doc))


_NO_LABELS = dict(box_label=None, pose_label=None)
_LABEL_FIELDS = ("box_label", "pose_label")
LiveRead = _read_type("LiveRead", "keypoints has_hand crop_box words more mesh",
                      "LiveOutput.read() of a step without images: unpacks as the six results it always had.",
                      overlay=None, **_NO_LABELS)
LiveOverlayRead = _read_type("LiveOverlayRead", LiveRead._fields + ("overlay",), "... of a step with faces=.", **_NO_LABELS)
LiveLabelsRead = _read_type("LiveLabelsRead", LiveRead._fields + _LABEL_FIELDS, "... of a step with labels.", overlay=None)
LiveOverlayLabelsRead = _read_type("LiveOverlayLabelsRead", LiveRead._fields + ("overlay",) + _LABEL_FIELDS,
                                   "... of a step with faces= and labels.")

POSE_LABEL = ops.LABEL_CROP                           # side of a pose_label image
POSE_LABEL_BYTES = POSE_LABEL * POSE_LABEL * 3


def _labels_behind(end: int, frames: int, slots: int, h: int, w: int, labels: bool):
    """(offset of box_label, offset of pose_label, total bytes) of the two label images appended at byte `end` of a step's
    buffer (each starts on a dword: the kernels store three dwords per four pixels); labels False: (end, end, end)."""
    if not labels:
        return end, end, end
    box = (end + 3) // 4 * 4
    pose = (box + frames * h * w * 3 + 3) // 4 * 4
    return box, pose, pose + slots * POSE_LABEL_BYTES


def live_overlay_layout(n: int, vertices: int, h: int, w: int):
    """Byte layout of the one-hand live step's buffer with an overlay: (offset of the mesh, offset of the overlay (uint8
    [n,h,w,3], appended: the records and the mesh stay where a step without one has them), total bytes)."""
    mesh = (n + 1) * record_bytes(3)
    overlay = mesh + n * vertices * 12
    return mesh, overlay, overlay + n * h * w * 3


def live_labels_layout(n: int, vertices: int, h: int, w: int, overlay: bool = False, labels: bool = True):
    """Byte layout of the one-hand live step's buffer with the label images: (offset of the mesh, offset of the overlay, offset
    of box_label (uint8 [n,h,w,3]), offset of pose_label (uint8 [n,176,176,3]), total bytes).  The images are appended behind
    the mesh, and behind the overlay when there is one: without `labels` the first two offsets and the total are
    live_overlay_layout's (h = w = 0 there for a step without an overlay)."""
    mesh, oo, end = live_overlay_layout(n, vertices, h if overlay else 0, w if overlay else 0)
    return (mesh, oo) + _labels_behind(end, n, n, h, w, labels)


@dataclass
class LiveOutput:
    hand: HandNetOutput          # the step's detector / pose results (image_uvd and xyz_mm included), on the device
    pose2d: torch.Tensor         # [N,21,2] the lifter's standardised input
    mesh: torch.Tensor           # [N,V0,3] Pose2Mesh vertices (finest level of the graph hierarchy, coarsening order), or --
    #                              with perm_reverse -- [N,V,3] = out['mesh'] of ros_demo.py:337 (camera frame, original order)
    pose3d: torch.Tensor         # [N,21,3] PoseNet's lifted joints (millimetre scale of the lifter's training set)
    host: torch.Tensor           # pinned uint8: (N + 1) wide records, then the mesh as fp32 -- ONE copy, enqueued by the step
    n: int = 0
    raw_mesh: torch.Tensor = None   # [N,V0,3] the lifter's own output on the device (= mesh without perm_reverse)
    overlay: torch.Tensor = None    # [N,H,W,3] uint8 RGB on the device: the mesh drawn over the frame (engines with faces=)
    box_label: torch.Tensor = None  # [N,H,W,3] uint8 RGB on the device: the frame with the hand's crop box (engines with labels)
    pose_label: torch.Tensor = None  # [N,176,176,3] uint8 RGB on the device: the colour crop with the skeleton (zeros: no hand)

    def read(self):
        """After the stream is synchronised: (keypoints, has_hand, crop_box, range words, [image_uvd, xyz_mm], mesh) as fresh CPU
        tensors (LiveRead; `.overlay`, `.box_label`, `.pose_label` are None).  A step with faces= appends the overlay [N,H,W,3]
        uint8 (LiveOverlayRead); a step with labels appends box_label [N,H,W,3] and pose_label [N,176,176,3] (LiveLabelsRead,
        LiveOverlayLabelsRead)."""
        rb = record_bytes(3)
        n = self.n
        rec = self.host[: (n + 1) * rb].view(n + 1, rb)
        kp, has, box, words, more = read_host_record(rec, n, extras=True)
        # (h = w = 0: a step without images has the records and the mesh at the same offsets, and nothing behind them)
        image = self.overlay if self.overlay is not None else self.box_label
        h, w = (0, 0) if image is None else image.shape[1:3]
        mo, oo, bo, po, end = live_labels_layout(n, self.mesh.shape[1], h, w, self.overlay is not None, self.box_label is not None)
        mesh = self.host[mo:oo].view(torch.float32).reshape(n, -1, 3).clone()
        fields = (kp, has, box, words, more, mesh)
        if self.overlay is not None:
            fields += (self.host[oo:oo + self.overlay.numel()].reshape(self.overlay.shape).clone(),)
        if self.box_label is None:
            return (LiveRead if self.overlay is None else LiveOverlayRead)(*fields)
        fields += (self.host[bo:bo + self.box_label.numel()].reshape(self.box_label.shape).clone(),
                   self.host[po:end].reshape(self.pose_label.shape).clone())
        return (LiveLabelsRead if self.overlay is None else LiveOverlayLabelsRead)(*fields)


class _LiveStep:
    """What the one-hand and the K-hand live steps share: the engines, the caller's conversion, the final-mesh permutation,
    the output buffers of a batch size, the camera feed (forward_raw) and the capture (graphed).  A subclass gives _nbytes(n)
    and forward_device(images, depth, _buffers)."""

    def __init__(self, hand: HandNetEngine, lifter: Pose2MeshEngine, paras, clamp: bool = True, perm_reverse=None, faces=None,
                 labels: bool = False, left: bool = False):
        if not _same_device(hand.device, lifter.device):
            raise ValueError(f"HandNet on {hand.device} but the lifter on {lifter.device}")
        self.hand, self.lifter, self.device = hand, lifter, hand.device
        hand.set_convert(paras=paras, clamp=clamp)
        self.perm, self.vertices = _final_mesh_perm(perm_reverse, lifter, self.device)
        # faces: the mesh's triangles (mesh_model.face) -- given, the step ends with the overlay (ops.mesh_render: the caller's
        # render(), ros_demo.py:86-116) and the image rides behind the mesh in the step's one copy
        self.faces, self.paras = None, tuple(float(p) for p in paras)
        if faces is not None:
            if self.perm is None:
                raise ValueError("faces= needs perm_reverse=: the overlay projects out['mesh'] (camera frame, the real mesh's "
                                 "vertex order); the lifter's raw output has no camera offset to project")
            with ops.on_device(self.device):
                self.faces = ops.mesh_faces(faces, self.vertices, self.device)
        # labels: the step ends with the caller's other two images (ops.draw_labels: ros_demo.py:310-326), behind the overlay
        self.labels, self.clamp = bool(labels), bool(clamp)
        # left: the caller's mirror mode (ImageListener(left=True), ros_demo.py:259-262): the step runs on the frame and the
        # depth map flipped along the width, and every result is in that mirrored frame, as the reference publishes it
        self.left = bool(left)
        self._mirrored = {}
        self._render_scratch = {}
        self._graphs = {}
        self._buffers = {}

    def _frames(self, images):
        """The step's input frames as one fp32 [N,3,H,W] tensor (the background of the overlay and of the label images), or
        None for a step that draws nothing."""
        if self.faces is None and not self.labels:
            return None
        frames = images if torch.is_tensor(images) else torch.stack(list(images))
        return frames.contiguous()

    def _hw(self, frames):
        return None if frames is None else (int(frames.shape[2]), int(frames.shape[3]))

    def _mirror_inputs(self, images, depth, owned=None):
        """The `left` step's inputs: frames and depth map mirrored along the width into buffers of the engine (`owned`: of a
        capture) by ONE launch (ops.flip_w)."""
        images = (images if torch.is_tensor(images) else torch.stack(list(images))).float().contiguous()
        depth = depth.float().contiguous()
        if owned is None:
            key = (tuple(images.shape), tuple(depth.shape))
            owned = self._mirrored.get(key)
            if owned is None:
                with torch.inference_mode(False):
                    owned = self._mirrored[key] = (torch.empty_like(images), torch.empty_like(depth))
        return ops.flip_w(images, depth, out=owned[0], out_other=owned[1])

    def _draw(self, mesh, lifted, frames, k, out):
        s = mesh.shape[0]
        scratch = self._render_scratch.get(s)
        if scratch is None:
            with torch.inference_mode(False):
                scratch = self._render_scratch[s] = torch.empty(
                    (ops.mesh_render_scratch_bytes(s, self.faces.shape[0]),), dtype=torch.uint8, device=self.device)
        return ops.mesh_render(mesh, self.faces, self.paras, frames, lifted=lifted, k=k, out=out, scratch=scratch)

    def _draw_labels(self, kp, crop_box, drawn, frames, k, dev, box_at, pose_at):
        """The step's two label images, written into its copy buffer `dev` at the layout's offsets."""
        n, _, h, w = frames.shape
        return ops.draw_labels(kp, crop_box, frames, drawn=drawn, k=k, clamp=self.clamp,
                               out_box=dev[box_at:box_at + n * h * w * 3], out_pose=dev[pose_at:pose_at + n * k * POSE_LABEL_BYTES])

    def _new_buffers(self, n, hw=None):
        """A fresh (device, pinned host) pair of a step over n frames (hw: with images of that frame size)."""
        nbytes = self._nbytes(n, hw)
        return (torch.zeros((nbytes,), dtype=torch.uint8, device=self.device),
                torch.zeros((nbytes,), dtype=torch.uint8, pin_memory=True))

    def _out_buffers(self, n, v0, hw=None):
        key = (n, v0, hw)
        b = self._buffers.get(key)
        if b is None:
            with torch.inference_mode(False):
                b = self._buffers[key] = self._new_buffers(n, hw)
        return b

    @ops.device_guarded
    def forward_raw(self, bgr_u8, depth_raw) -> LiveOutput:
        """The camera's buffers in, the mesh out: bgr_u8 uint8 [N,H,W,3] (cv_bridge 'bgr8'), depth_raw [N,H,W] uint16 millimetres
        (16UC1) or float32 metres (32FC1), on the GPU or on the host (pinned: read in place; pageable: staged) -- ONE ingest
        kernel writes the captured step's input buffers (ros_demo.py:227-231,266-269) and the live step replays (captured at
        the first call with these shapes).  Returns the capture's static LiveOutput (overwritten by the next call); no sync."""
        staged = []
        bgr, dep = self.hand._device_readable(bgr_u8, staged), self.hand._device_readable(depth_raw, staged)
        n, h, w, _ = bgr.shape
        # (a `left` step: the ingest kernel mirrors while it converts, so this capture -- keyed apart from graphed()'s -- takes
        # its inputs as already mirrored and holds no mirror launch)
        key = ((n, 3, h, w), (n, 1, h, w)) + (("mirrored",) if self.left else ())
        if key not in self._graphs:
            rgb, d1, _ = ops.ingest_raw(bgr, dep, device=self.device, flip_w=self.left)
            self.graphed(rgb, d1, _mirrored=self.left)
        return self.hand._ingest_replay(self._graphs[key], bgr, dep, staged, flip_w=self.left)

    @ops.device_guarded
    def graphed(self, images: torch.Tensor, depth: torch.Tensor, _mirrored: bool = False):
        """(run, static images, static depth, static LiveOutput): copy new frames into the static inputs and call run().
        (A `left` step: the captured step mirrors the static inputs itself, one launch.)"""
        key = (tuple(images.shape), tuple(depth.shape)) + (("mirrored",) if _mirrored else ())
        hit = self._graphs.get(key)
        if hit is None:
            with torch.inference_mode(False), torch.no_grad():
                s_img, s_dep = torch.empty_like(images), torch.empty_like(depth)
                s_img.copy_(images)
                s_dep.copy_(depth)
                # the capture's own pair, never the eager cache's (addresses are baked into the graph)
                bufs = self._new_buffers(images.shape[0], self._hw(self._frames(images)))
                flipped = None
                if self.left and not _mirrored:
                    # the capture's mirrored inputs: owned by the engine for as long as the capture lives (their addresses are
                    # baked into the graph, and nothing the step hands out refers to them)
                    flipped = self._mirrored[("capture",) + key] = (torch.empty_like(s_img), torch.empty_like(s_dep))
                g, out = ops.capture_step(lambda: self.forward_device(s_img, s_dep, _buffers=bufs,
                                                                      _mirror=False if _mirrored else flipped))
            hit = self._graphs[key] = (g, s_img, s_dep, out)
        g, s_img, s_dep, out = hit
        return g.replay, s_img, s_dep, out


class LiveHandEngine(_LiveStep):
    def __init__(self, hand: HandNetEngine, lifter: Pose2MeshEngine, paras, clamp: bool = True, perm_reverse=None, faces=None,
                 labels: bool = False, left: bool = False):
        """paras = (fx, fy, cx, cy) of the depth camera (ros_demo.py:191-196); clamp: the caller's clamps before the
        conversion (ros_demo.py:279-283).  perm_reverse: graph_perm_reverse[:V] (int64, V = vertices of the real mesh,
        ros_demo.py:162) -- given, the step also does the caller's last three lines (vertex order, camera offset by the first
        joint, y / z negated: ros_demo.py:332-337) and `mesh` of the outputs IS out['mesh'], [N,V,3]; else the lifter's raw
        [N,V0,3] vertices in coarsening order.  faces: mesh_model.face ([F,3] vertex indices of the real mesh; needs perm_reverse) --
        given, the step also draws the mesh over the frame (ros_demo.py:86-116 render(): LiveOutput.overlay, read().overlay).
        labels: the step also draws box_label and pose_label (ros_demo.py:310-326: LiveOutput.box_label / .pose_label, read()
        likewise); a frame without a hand (has_hand != 1) keeps its plain frame and a zero pose_label.
        left: the reference's mirror mode for a left-handed subject (ImageListener(left=True), ros_demo.py:259-262) -- every
        output equals the one of this engine without `left` on frames and depth flipped along the width, bit for bit (boxes,
        keypoints, mesh and images are in the mirrored frame, as the reference publishes them).  forward_raw mirrors inside the
        ingest kernel (no launch added); fp32 feeds (forward_device / graphed) cost one launch."""
        super().__init__(hand, lifter, paras, clamp, perm_reverse, faces, labels, left)

    def _nbytes(self, n, hw=None):
        if hw is None:
            return (n + 1) * record_bytes(3) + n * self.vertices * 12
        return live_labels_layout(n, self.vertices, *hw, overlay=self.faces is not None, labels=self.labels)[4]

    @ops.device_guarded
    def forward_device(self, images, depth, _buffers=None, _mirror=None) -> LiveOutput:
        """images [N,3,H,W] 0..1 (or a list), depth [N,1,H,W] metres on the GPU -> LiveOutput (no sync).
        (_mirror: a `left` capture's own mirrored-input buffers; False: the inputs are mirrored already.)"""
        n = len(images)
        if self.left and _mirror is not False:
            images, depth = self._mirror_inputs(images, depth, _mirror)
        v0 = self.vertices
        frames = self._frames(images)
        dev, host = _buffers if _buffers is not None else self._out_buffers(n, v0, self._hw(frames))
        rb = record_bytes(3)
        rec = dev[: (n + 1) * rb].view(n + 1, rb)
        mesh_buf = dev[(n + 1) * rb:(n + 1) * rb + n * v0 * 12].view(torch.float32).view(n, v0, 3)

        def lift(_kp, image_uvd, xyz, has_hand):
            # (inside the step's range scope: the lifter's split producers note into the step's flag words, which the step's one
            # collect launch hands over -- an overflowing activation of the lifter raises like one of the pose network)
            p2d = ops.joints2d_standardize(image_uvd, valid=has_hand)
            if self.perm is None:
                mesh, pose3d = self.lifter.forward(p2d, mesh_out=mesh_buf)          # the last layer writes into the copy buffer
                return p2d, mesh, pose3d, mesh
            raw, pose3d = self.lifter.forward(p2d)
            return p2d, ops.mesh_finish(raw, self.perm, xyz, valid=has_hand, out=mesh_buf), pose3d, raw
        # the step packs its wide records and its range words straight into `rec`; ONE copy moves records + mesh
        out = self.hand.forward_device(images, depth, _record=(None, rec), _tail=lift)
        p2d, mesh, pose3d, raw = out.tail
        overlay = box_label = pose_label = None
        if frames is not None:
            h, w = frames.shape[2:]
            _, oo, bo, po, _ = live_labels_layout(n, v0, h, w, self.faces is not None, self.labels)
            if self.faces is not None:
                overlay = self._draw(mesh, out.has_hand.view(-1), frames, 1, dev[oo:oo + n * h * w * 3])
            if self.labels:
                box_label, pose_label = self._draw_labels(out.keypoints, out.crop_box, out.has_hand.view(-1), frames, 1, dev, bo, po)
        host.copy_(dev, non_blocking=True)
        return LiveOutput(out, p2d, mesh, pose3d, host, n, raw, overlay, box_label, pose_label)


def live_hands_layout(slots: int, vertices: int, handed: bool = False):
    """Byte layout of the K-hand live step's one buffer for `slots` = N*K hand slots: (record rows, record bytes, offset of
    `lifted` (int32 [slots]), offset of the mesh (fp32 [slots,V,3]), total bytes).  The record is forward_hands' wide record
    unchanged (one row per slot, the range-word row, the scores and detection ranks: hands_record_rows).  handed: the
    slots' sides (int32 [slots]) sit behind the score and rank rows, at `rows * record bytes` -- `lifted` and everything behind
    it move up by 4 * slots bytes, nothing else changes."""
    rb = record_bytes(3)
    rows = hands_record_rows(slots, rb)
    lifted = rows * rb + (4 * slots if handed else 0)
    mesh = lifted + 4 * slots
    return rows, rb, lifted, mesh, mesh + slots * vertices * 12


def live_hands_overlay_layout(slots: int, vertices: int, frames: int, h: int, w: int, handed: bool = False):
    """live_hands_layout with the overlay appended: the same five values (every offset where a step without an overlay has
    it; the fifth is now the overlay's offset) + the total bytes; the overlay is uint8 [frames,h,w,3]."""
    rows, rb, lifted, mesh, overlay = live_hands_layout(slots, vertices, handed)
    return rows, rb, lifted, mesh, overlay, overlay + frames * h * w * 3


def live_hands_labels_layout(slots: int, vertices: int, frames: int, h: int, w: int, overlay: bool = False, labels: bool = True,
                             handed: bool = False):
    """live_hands_overlay_layout with the label images appended behind the mesh, and behind the overlay when there is one: its
    first five values (the overlay's offset: the end of the mesh), then the offset of box_label (uint8 [frames,h,w,3]), the
    offset of pose_label (uint8 [slots,176,176,3]) and the total bytes.  Without `labels` the total is the one of
    live_hands_overlay_layout / live_hands_layout."""
    rows, rb, lifted, mesh, oo, end = live_hands_overlay_layout(slots, vertices, frames, h if overlay else 0, w if overlay else 0,
                                                                handed)
    return (rows, rb, lifted, mesh, oo) + _labels_behind(end, frames, slots, h, w, labels)


LiveHandsRead = _read_type("LiveHandsRead", "keypoints has_hand crop_box score det_index image_uvd xyz_mm lifted mesh words",
                           "LiveHandsOutput.read() of a step without images (the fields are the ten it always had).",
                           overlay=None, **_NO_LABELS)
LiveHandsOverlayRead = _read_type("LiveHandsOverlayRead", LiveHandsRead._fields + ("overlay",), "... of a step with faces=.",
                                  **_NO_LABELS)
LiveHandsLabelsRead = _read_type("LiveHandsLabelsRead", LiveHandsRead._fields + _LABEL_FIELDS, "... of a step with labels.",
                                 overlay=None)
LiveHandsOverlayLabelsRead = _read_type("LiveHandsOverlayLabelsRead", LiveHandsRead._fields + ("overlay",) + _LABEL_FIELDS,
                                        "... of a step with faces= and labels.")
# ... and of a handed step: the same fields + `side` [N,K] int32 (the detector's side of the slot's detection, -1: empty slot)
_SIDED_READS = {t: _read_type(t.__name__.replace("Read", "SidedRead"), t._fields + ("side",), t.__doc__ + "  Handed: + side.",
                              **{f: None for f in ("overlay",) + _LABEL_FIELDS if f not in t._fields})
                for t in (LiveHandsRead, LiveHandsOverlayRead, LiveHandsLabelsRead, LiveHandsOverlayLabelsRead)}


@dataclass
class LiveHandsOutput:
    hands: HandsOutput           # the step's forward_hands results (image_uvd and xyz_mm included), on the device
    pose2d: torch.Tensor         # [N*K,21,2] the lifter's input; zero rows where not lifted
    lifted: torch.Tensor         # [N,K] int32: 1 where the slot's hand went through the lifter (the caller's skip rule)
    mesh: torch.Tensor           # [N,K,V,3] as LiveOutput.mesh, per slot; zero rows where not lifted
    pose3d: torch.Tensor         # [N*K,21,3] PoseNet's lifted joints (every row: rows not lifted are the lifter on zeros)
    host: torch.Tensor           # pinned uint8 (live_hands_layout): records, lifted, mesh -- ONE copy, enqueued by the step
    n: int = 0
    k: int = 0
    raw_mesh: torch.Tensor = None   # [N*K,V0,3] the lifter's own output on the device
    overlay: torch.Tensor = None    # [N,H,W,3] uint8 RGB on the device: all lifted meshes of a frame drawn over it (faces=)
    box_label: torch.Tensor = None  # [N,H,W,3] uint8 RGB on the device: the frame with the crop box of every lifted slot (labels)
    pose_label: torch.Tensor = None  # [N*K,176,176,3] uint8 RGB on the device: per slot, the colour crop with the skeleton
    side: torch.Tensor = None        # handed steps: [N,K] int32 on the device, the detector's side per slot (-1: empty slot)
    mirror: torch.Tensor = None      # handed steps: [N,K] int32 on the device, 1 where the slot ran mirrored (a left hand)

    def read(self) -> LiveHandsRead:
        """After the stream is synchronised: the step's results per frame and slot as fresh CPU tensors (LiveHandsRead;
        lifted as bool, words = the step's range words; a step with faces=: LiveHandsOverlayRead, + overlay [N,H,W,3] uint8; a
        step with labels: + box_label [N,H,W,3], pose_label [N,K,176,176,3] -- LiveHandsLabelsRead, LiveHandsOverlayLabelsRead;
        a handed step: the same with `side` [N,K] int32 as the last field)."""
        n, k, s = self.n, self.k, self.n * self.k
        handed = self.side is not None
        rows, rb, lo, mo, nbytes = live_hands_layout(s, self.mesh.shape[2], handed)

        def sided(kind, values):
            if not handed:
                return kind(*values)
            return _SIDED_READS[kind](*values, self.host[rows * rb:lo].view(torch.int32).reshape(n, k).clone())
        rec = self.host[:rows * rb].view(rows, rb)
        kp, has, box, words, (img, xyz) = read_host_record(rec, s, extras=True)
        score, index = read_hands_tail(rec, s)
        lifted = self.host[lo:mo].view(torch.int32).reshape(n, k) != 0
        mesh = self.host[mo:nbytes].view(torch.float32).reshape(n, k, -1, 3).clone()
        per = lambda t: t.reshape((n, k) + tuple(t.shape[1:]))
        fields = (per(kp), per(has), per(box), per(score), per(index), per(img), per(xyz), lifted, mesh, words)
        if self.overlay is not None:
            fields += (self.host[nbytes:nbytes + self.overlay.numel()].reshape(self.overlay.shape).clone(),)
        if self.box_label is None:
            return sided(LiveHandsRead if self.overlay is None else LiveHandsOverlayRead, fields)
        h, w = self.box_label.shape[1:3]
        bo, po, end = live_hands_labels_layout(s, self.mesh.shape[2], n, h, w, self.overlay is not None, handed=handed)[5:]
        fields += (self.host[bo:bo + self.box_label.numel()].reshape(self.box_label.shape).clone(),
                   self.host[po:end].reshape(n, k, POSE_LABEL, POSE_LABEL, 3).clone())
        return sided(LiveHandsLabelsRead if self.overlay is None else LiveHandsOverlayLabelsRead, fields)


class LiveHandsEngine(_LiveStep):
    """LiveHandEngine for up to max_hands hands per frame: HandNet's forward_hands step (slot k of frame i = frame i's k-th
    hand detection) -> clamp + convert in the aggregation's epilogue -> the lifter's input WITH the caller's skip rule per
    slot (ros_demo.py:288-300: a hand whose 2D box process_bbox refuses is not lifted; hn_lifter_input_gated_f32) ->
    Pose2Mesh on all N*K rows (dense: rejected rows are zeros, so the step stays capturable and its activations finite) ->
    the final mesh (perm_reverse) -> ONE device -> host copy of records + lifted + mesh (live_hands_layout)."""

    def __init__(self, hand: HandNetEngine, lifter: Pose2MeshEngine, paras, max_hands: int = 2, clamp: bool = True,
                 perm_reverse=None, faces=None, labels: bool = False, left: bool = False, handed: bool = False,
                 left_side: int = 0):
        """faces: mesh_model.face ([F,3]; needs perm_reverse) -- given, the step ends with the overlay: every lifted mesh of a
        frame drawn over it with one depth buffer per frame (LiveHandsOutput.overlay, read().overlay), in the same copy.
        labels: the step ends with box_label (the crop box of every lifted slot on its frame) and one pose_label per slot
        (zeros where the slot is not lifted: the reference's condition, ros_demo.py:294), in the same copy.
        left: the reference's whole-frame mirror mode, as LiveHandEngine's.
        handed: the per-slot form of that mirror, for frames that hold a left AND a right hand.  The detector's side of every
        slot is handed over (LiveHandsOutput.side, read().side; -1: empty slot) and a filled slot whose side equals left_side
        goes MIRRORED through the right-handed pose network and lifter and comes back un-mirrored: its crop is flipped along
        the width, the aggregation writes u = 176 - u, the lifter's input has column 0 negated and the x of the lifter's raw
        vertices is negated before the final mesh's arithmetic -- all flags on launches the step makes anyway.  Keypoints,
        mesh and images are in the frame's own coordinates; slots that are not mirrored are the plain step's, bit for bit.
        left_side = 0 is an ASSUMPTION: the detector's side targets are box_info[:, 1] of its training set, whose convention
        (100DOH: 0 = left) the reference does not state -- it never reads `sides`.  Check it on your checkpoint.
        left and handed together: ValueError (a mirrored frame swaps the sides)."""
        self.max_hands = ops.check_max_hands(max_hands)
        if left and handed:
            raise ValueError("left=True mirrors the whole frame and handed=True mirrors the left-hand slots: give one of them")
        self.handed, self.left_side = bool(handed), int(left_side)
        super().__init__(hand, lifter, paras, clamp, perm_reverse, faces, labels, left)

    def _nbytes(self, n, hw=None):
        if hw is None:
            return live_hands_layout(n * self.max_hands, self.vertices, self.handed)[4]
        return live_hands_labels_layout(n * self.max_hands, self.vertices, n, *hw, overlay=self.faces is not None,
                                        labels=self.labels, handed=self.handed)[7]

    @ops.device_guarded
    def forward_device(self, images, depth, _buffers=None, _mirror=None) -> LiveHandsOutput:
        """images [N,3,H,W] 0..1 (or a list), depth [N,1,H,W] metres on the GPU -> LiveHandsOutput (no sync).  Eager steps
        may run A2J on the filled slots only (HandNetEngine.forward_hands); the lifter always runs on all N*K rows.
        (_mirror: as LiveHandEngine.forward_device's.)"""
        n, k = len(images), self.max_hands
        if self.left and _mirror is not False:
            images, depth = self._mirror_inputs(images, depth, _mirror)
        s, v = n * k, self.vertices
        frames = self._frames(images)
        dev, host = _buffers if _buffers is not None else self._out_buffers(n, v, self._hw(frames))
        rows, rb, lo, mo, nbytes = live_hands_layout(s, v, self.handed)
        rec = dev[:rows * rb].view(rows, rb)
        side = dev[rows * rb:lo].view(torch.int32) if self.handed else None
        lifted = dev[lo:mo].view(torch.int32)
        mesh_buf = dev[mo:nbytes].view(torch.float32).view(s, v, 3)

        def lift(_kp, image_uvd, xyz, has_hand, mirror=None):
            # (inside the step's range scope, as LiveHandEngine's lifter; mirror: the handed step's per-slot flags)
            p2d, _ = ops.lifter_input_gated(image_uvd, valid=has_hand, lifted=lifted, mirror=mirror)
            raw, pose3d = self.lifter.forward(p2d)
            if mirror is not None:      # (also without perm_reverse: the raw vertices, x negated where mirrored)
                mesh = ops.mesh_finish(raw, self.perm, xyz if self.perm is not None else None, valid=lifted, out=mesh_buf,
                                       mirror=mirror)
            elif self.perm is None:
                mesh = torch.mul(raw, lifted.view(s, 1, 1), out=mesh_buf)       # (x * 1 is x: rows not lifted -> zeros)
            else:
                mesh = ops.mesh_finish(raw, self.perm, xyz, valid=lifted, out=mesh_buf)
            return p2d, mesh, pose3d, raw
        # the step packs its per-slot records, range words, scores and ranks straight into `rec`; ONE copy moves it all
        out = self.hand.forward_hands(images, depth, k, _record=(None, rec), _tail=lift, handed=self.handed,
                                      left_side=self.left_side, _side=side)
        p2d, mesh, pose3d, raw = out.tail
        overlay = box_label = pose_label = None
        if frames is not None:
            h, w = frames.shape[2:]
            bo, po, _ = live_hands_labels_layout(s, v, n, h, w, self.faces is not None, self.labels, self.handed)[5:]
            if self.faces is not None:
                overlay = self._draw(mesh, lifted, frames, k, dev[nbytes:nbytes + n * h * w * 3])
            if self.labels:
                box_label, pose_label = self._draw_labels(out.keypoints, out.crop_box, lifted, frames, k, dev, bo, po)
        host.copy_(dev, non_blocking=True)
        return LiveHandsOutput(out, p2d, lifted.view(n, k), mesh.view(n, k, v, 3), pose3d, host, n, k, raw, overlay, box_label,
                               pose_label, out.side, out.mirror)


@dataclass
class CropMeshOutput:
    keypoints: torch.Tensor      # [K,21,3] crop (u,v,d) as the network returns it, on the device
    image_uvd: torch.Tensor      # [K,21,3] image (u,v,d) of the (clipped) joints
    xyz_mm: torch.Tensor         # [K,21,3] camera xyz in millimetres
    pose2d: torch.Tensor         # [K,21,2] the lifter's input
    mesh: torch.Tensor           # [K,V,3]: out['mesh'] of a2j_mesh.py:77-80 with perm_reverse, else the lifter's raw [K,V0,3]
    pose3d: torch.Tensor         # [K,21,3]
    raw_mesh: torch.Tensor       # [K,V0,3] the lifter's own output
    host: torch.Tensor           # pinned fp32: keypoints | image_uvd | xyz_mm | mesh | 4 range words (as bits) -- ONE copy; the
    #                              engine's buffer for this batch size: the next call overwrites it (read() returns copies)
    k: int = 0

    def read(self):
        """After the stream is synchronised: (keypoints, image_uvd, xyz_mm, mesh, range words) as fresh CPU tensors."""
        k, j3 = self.k, self.keypoints.shape[1] * 3
        h = self.host
        parts = [h[i * k * j3:(i + 1) * k * j3].reshape(k, -1, 3).clone() for i in range(3)]
        mesh = h[3 * k * j3:-4].reshape(k, -1, 3).clone()
        return parts[0], parts[1], parts[2], mesh, h[-4:].view(torch.int32).tolist()


class CropMeshEngine:
    """The stand-alone mesh demo's loop body (a2j_mesh.py:58-80) as one step on the device: dataset crops -> A2J -> np.clip to
    [0, 176] + convert_joints twice (image uv; camera xyz with the sample's intrinsics -- the dataset's float32 box, fractional
    corners: a2jdataset.py:293) in the aggregation's epilogue -> the lifter's input (predict_mesh, ros_demo.py:148-157) ->
    Pose2Mesh -> the caller's last lines (vertex order, camera offset by the first joint, y / z negated: a2j_mesh.py:77-80) ->
    ONE device -> host copy.  The reference goes to the CPU after A2J, converts in numpy and uploads the normalised joints."""

    def __init__(self, a2j, lifter: Pose2MeshEngine, clamp: bool = True, perm_reverse=None):
        if not _same_device(a2j.device, lifter.device):
            raise ValueError(f"A2J on {a2j.device} but the lifter on {lifter.device}")
        self.a2j, self.lifter, self.device, self.clamp = a2j, lifter, a2j.device, bool(clamp)
        self.perm, self.vertices = _final_mesh_perm(perm_reverse, lifter, self.device)
        self._block = None
        self._graphs = {}
        self._hosts = {}

    @ops.device_guarded
    def forward_device(self, crops, box_f32, paras, _host=None) -> CropMeshOutput:
        """crops [K,1,176,176] (or [K,4,..] for the RGB-D network), box_f32 [K,4] float32, paras [K,4] float32, on the GPU."""
        k = crops.shape[0]
        if self._block is None:
            self._block = torch.zeros((4,), device=self.device, dtype=torch.int32)
        conv = dict(sample_box=box_f32, sample_paras=paras, clamp_keypoints=self.clamp)
        with ops.range_scope(self._block, on=self.a2j.precision == "f16x3" and self.a2j.note_range):
            kp, img, xyz = self.a2j.forward(crops, convert=conv)
            p2d = ops.joints2d_standardize(img)
            raw, pose3d = self.lifter.forward(p2d)
            mesh = raw if self.perm is None else ops.mesh_finish(raw, self.perm, xyz)
            words = ops.range_check_collect(self._block)
        dev = torch.cat([kp.reshape(-1), img.reshape(-1), xyz.reshape(-1), mesh.reshape(-1), words.view(torch.float32)])
        if _host is None:     # one pinned buffer per batch size, like the live step's: the NEXT eager call with this batch size
            _host = self._hosts.get(dev.numel())      # overwrites it (read() hands out copies)
            if _host is None:
                with torch.inference_mode(False):
                    _host = self._hosts[dev.numel()] = self._new_host(k)
        _host.copy_(dev, non_blocking=True)
        return CropMeshOutput(kp, img, xyz, p2d, mesh, pose3d, raw, _host, k)

    def _new_host(self, k):
        """The pinned buffer of a step over k crops, as forward_device's torch.cat fills it: three [k,J,3] fields (keypoints,
        image_uvd, xyz_mm), the mesh [k,V,3], 4 range words."""
        return torch.zeros((3 * k * self.a2j.joints * 3 + k * self.vertices * 3 + 4,), dtype=torch.float32, pin_memory=True)

    @ops.device_guarded
    def graphed(self, crops, box_f32, paras):
        """(run, static crops, static boxes, static intrinsics, static CropMeshOutput): copy a new batch into the static inputs and
        call run() -- every launch of the step and its copy replay from one hipGraph."""
        key = (tuple(crops.shape),)
        hit = self._graphs.get(key)
        if hit is None:
            with torch.inference_mode(False), torch.no_grad():
                s = [torch.empty_like(t) for t in (crops, box_f32, paras)]
                for a, b in zip(s, (crops, box_f32, paras)):
                    a.copy_(b)
                host = self._new_host(crops.shape[0])
                g, out = ops.capture_step(lambda: self.forward_device(*s, _host=host))
            hit = self._graphs[key] = (g, s[0], s[1], s[2], out)
        g, s_crops, s_box, s_paras, out = hit
        return g.replay, s_crops, s_box, s_paras, out
