"""End-to-end HandNet on the device: FCOS -> top-1 hand box -> depth crop -> A2J.

Restates handnet_pipeline/handnet_pipeline.py:58-116 without its per-image Python loop
and its ~10 device->host syncs per frame: box selection, int truncation, 40 % padding,
clamping and the nearest-neighbour 176x176 gather run in hn_crop_resize (csrc/crop_stage.hip:
the one-slot case of the K-hand stage that forward_hands runs); A2J then runs on
ALL N frames with a validity mask (frames without a hand produce zero rows), so the whole
step has a static launch sequence and can be captured into a hipGraph.
"""
from __future__ import annotations

import collections
from dataclasses import dataclass

import os

import numpy as np
import torch

from . import ops
from .a2j_engine import A2JEngine
from .fcos_engine import FCOSEngine

CROP = 176


class CameraTables:
    """A camera per frame as the kernels read it: the caller's [N,4] fp32 values and, per number of slots per frame, a device
    table with one row per slot (frame-major: slot i * k + j holds row i), made on first use.  update() copies new values
    into the SAME tables, so a captured step that holds their addresses uses them at its next replay; whoever captured such a
    step keeps this object, and with it the tables, alive."""

    def __init__(self, values, device):
        self.values, self.device, self.tables = values, device, {}

    @property
    def frames(self) -> int:
        return self.values.shape[0]

    def _expanded(self, k):
        return torch.from_numpy(np.repeat(self.values, k, axis=0))

    def rows(self, k=1):
        table = self.tables.get(k)
        if table is None:
            with torch.inference_mode(False):
                table = self.tables[k] = self._expanded(k).to(self.device)
        return table

    def update(self, paras):
        new = ops.camera_paras(paras)
        if not isinstance(new, np.ndarray) or new.shape != self.values.shape:
            raise ValueError(f"set_cameras: expected [{self.frames},4] values, one row per frame")
        self.values = new
        for k, table in self.tables.items():
            table.copy_(self._expanded(k))
        return self


@dataclass
class HandNetOutput:
    keypoints: torch.Tensor   # [N,21,3] fp32 device; zero rows where has_hand == 0
    crops_nhwc: torch.Tensor  # [N,176,176,4] fp32 device; channel 0 = cropped depth
    crop_box: torch.Tensor    # [N,4] int64 device (x1,y1,x2,y2 after padding)
    has_hand: torch.Tensor    # [N] int32 device: 0 no hand, 1 hand, 2 hand whose depth crop holds non-finite pixels (NaN row)
    detections: ops.Detections
    candidates: ops.Candidates   # rows at or beyond count[i] are undefined (never zero-filled)
    range_flags: torch.Tensor = None   # [4] int32 device: the step's f16x3 range-contract words (ops.range_bits), or None
    image_uvd: torch.Tensor = None     # [N,21,3] fp32 device, after HandNetEngine.set_convert(): image (u,v,d) per joint
    xyz_mm: torch.Tensor = None        # [N,21,3] fp32 device, set_convert(paras=...): camera xyz in millimetres
    tail: object = None                # what forward_device's `_tail` callable returned (the live step: the lifter's mesh, pose3d)
    host_record: torch.Tensor = None   # to_host steps: PINNED uint8 [N+1, 296] the step copies its results into (device -> host
    #                                    copy enqueued by the step itself; valid after the stream is synchronised): rows 0..N-1 =
    #                                    hn_pack_records rows (crop box 32 B | has_hand | 1 | keypoints), row N = the range words


@dataclass
class HandsOutput:
    """HandNetEngine.forward_hands: up to K hands per frame.  Slot k of frame i is the k-th hand-label detection of frame i
    (score order); empty slots (fewer hand detections, or an empty padded slice) are zeros with det_index -1."""
    keypoints: torch.Tensor   # [N,K,21,3] fp32 device, crop (u,v,d); zero rows for empty slots
    crops_nhwc: torch.Tensor  # [N*K,176,176,4] fp32 device, frame-major (crop i*K + k = slot k of frame i)
    crop_box: torch.Tensor    # [N,K,4] int64 device
    has_hand: torch.Tensor    # [N,K] int32 device: 0 empty, 1 hand, 2 hand whose crop holds non-finite pixels (NaN row)
    score: torch.Tensor       # [N,K] fp32 device: the slot's detection score (0 when empty)
    det_index: torch.Tensor   # [N,K] int32 device: the slot's row in `detections` (-1 when empty)
    #                           (to_host steps: both are views of the device record, rewritten by the engine's next such step)
    detections: ops.Detections
    candidates: ops.Candidates
    range_flags: torch.Tensor = None
    image_uvd: torch.Tensor = None     # [N,K,21,3] after set_convert()
    xyz_mm: torch.Tensor = None        # [N,K,21,3] after set_convert(paras=...)
    host_record: torch.Tensor = None   # to_host steps: pinned uint8; rows 0..N*K-1 = one record per slot, row N*K = the range
    #                                    words, then score [N*K] fp32 and det_index [N*K] int32 (read_hands_tail)
    tail: object = None                # what forward_hands' `_tail` callable returned (the multi-hand live step, hn_amd/live.py)
    side: torch.Tensor = None          # handed steps: [N,K] int32 device, detections.sides of the slot's detection (-1 when empty)
    mirror: torch.Tensor = None        # handed steps: [N,K] int32 device, 1 where the slot went through A2J mirrored (a left hand)
    contacts: torch.Tensor = None      # objects steps: [N,cap] int32 device, the contact state of every detection row below count
    dxdymags: torch.Tensor = None      # objects steps: [N,cap,3] fp32 device, (magnitude, x, y) of every such row's offset vector
    track_id: torch.Tensor = None      # tracked steps: [N,K] int32 device, the slot's track id (held slots included; 0: free)
    track_age: torch.Tensor = None     # tracked steps: [N,K] int32 device, the steps on which the slot's track was seen again


RECORD_BYTES = 296      # hn_amd.dist's per-frame record (box 32 + flags 8 + 21 x 3 fp32 keypoints, padded to 8)
RECORD_FIELD = 252      # one [21,3] fp32 field; the WIDE record of a converting step appends image (u,v,d) and camera xyz


def record_bytes(fields: int = 1) -> int:
    return (40 + RECORD_FIELD * fields + 7) // 8 * 8


def read_host_record(rec: torch.Tensor, n: int, joints: int = 21, extras: bool = False):
    """A synchronised host_record -> (keypoints [n,J,3] fp32, has_hand [n] int32, crop_box [n,4] int64, range words [4] list);
    all fresh CPU tensors (the pinned buffer is overwritten by the engine's next step).  numpy slicing: a handful of torch
    ops on 300-byte tensors would cost more host time than the copy itself (batch 1: the call is 2.3 ms in all).
    extras: also the further [n,J,3] fields of a wide record (image uvd, camera xyz) as a list, appended to the tuple."""
    import numpy as np
    a = rec.numpy()
    j3 = joints * 3
    # (.copy(), not np.ascontiguousarray: a ONE-row slice is already contiguous and would come back as a VIEW of the pinned
    # buffer -- at batch 1, the live caller's batch, the "fresh" keypoints of round 5 aliased the record the next call overwrites)
    kp = torch.from_numpy(a[:n, 40:40 + 4 * j3].copy().view(np.float32).reshape(n, joints, 3))
    has = torch.from_numpy(a[:n, 32:36].copy().view(np.int32).reshape(n))
    box = torch.from_numpy(a[:n, :32].copy().view(np.int64).reshape(n, 4))
    words = a[n, :16].view(np.int32).tolist()
    if not extras:
        return kp, has, box, words
    more = []
    for f in range(1, (a.shape[1] - 40) // (4 * j3)):
        lo = 40 + 4 * j3 * f
        more.append(torch.from_numpy(a[:n, lo:lo + 4 * j3].copy().view(np.float32).reshape(n, joints, 3)))
    return kp, has, box, words, more


def hands_record_rows(slots: int, rec_bytes: int, handed: bool = False, tracked: bool = False) -> int:
    """Rows of a forward_hands record: one per slot, the range-word row, then the slots' scores and detection ranks -- and,
    for a handed step, their sides behind those; for a tracked step, the track ids and ages behind all of them."""
    return slots + 1 + ((8 + 4 * bool(handed) + 8 * bool(tracked)) * slots + rec_bytes - 1) // rec_bytes


def _hands_tail(rec: torch.Tensor, slots: int, handed: bool = False, tracked: bool = False):
    """(score [slots] fp32, det_index [slots] int32) views of a forward_hands record (device or host); handed: + side [slots]
    int32, behind them; tracked: + track_id, track_age [slots] int32, last."""
    flat = rec.view(-1)
    base = (slots + 1) * rec.shape[1]
    tail = (flat[base:base + 4 * slots].view(torch.float32), flat[base + 4 * slots:base + 8 * slots].view(torch.int32))
    end = base + 8 * slots
    for _ in range(bool(handed) + 2 * bool(tracked)):
        tail += (flat[end:end + 4 * slots].view(torch.int32),)
        end += 4 * slots
    return tail


def read_hands_tail(rec: torch.Tensor, slots: int, handed: bool = False, tracked: bool = False):
    """A synchronised forward_hands host_record -> (score [slots] fp32, det_index [slots] int32), fresh CPU tensors; handed
    (the record of a handed step): + side [slots] int32; tracked: + track_id, track_age [slots] int32."""
    return tuple(t.clone() for t in _hands_tail(rec, slots, handed, tracked))


def range_message(bits: int) -> str:
    """What the f16x3 range-contract bits of a step (ops.range_bits) mean for its caller."""
    from ._lib import RANGE_ACTIVATION, RANGE_INPUT, RANGE_INPUT_NONFINITE
    if bits & RANGE_INPUT_NONFINITE:
        return ("the inputs hold non-finite values (NaN / inf pixels): frames whose depth crop holds one return NaN "
                "keypoints, as the reference does; a non-finite RGB pixel raises RangeError (its NaN reaches the activation "
                "flag through the NaN-propagating ReLUs)")
    if bits & RANGE_INPUT:
        return ("an input value lies outside the range of the f16x3 split format (|v| > 65504): RGB must be 0..1 and depth "
                "METRES (ros_demo.py:230-231 divides 16UC1 millimetres by 1000); or build the engines with precision='f32'")
    if bits & RANGE_ACTIVATION:
        return ("an activation left the range of the f16x3 split format (|v| > 65504) although the inputs are in range: "
                "results would be inf / NaN or silently wrong.  Build the engines with precision='f32' for this checkpoint")
    return "in range"


def check_range_contract(keypoints_cpu, words, inputs=None, has_hand=None):
    """The f16x3 range contract of a step, decided on values the caller has copied to the host anyway.  words: the collected
    flag words (ops.range_check_collect) as a host list, or None when noting is off (HN_CHECK_RANGE=0); has_hand: the step's
    per-frame flags on the host (2 = a frame whose crop holds non-finite pixels; None: A2J-only callers).
    Non-finite INPUTS are the reference's business -- ROS 32FC1 depth marks invalid pixels with NaN and ros_demo.py:227-231
    passes them on; its network then returns NaN keypoints for the crops that hold one, and so does this one -- so they never
    raise.  A finite input beyond +-65504 or an activation that overflows with in-range inputs WOULD give inf / NaN or (ReLU
    maps NaN to 0) silently wrong keypoints: those raise ops.RangeError."""
    from ._lib import RANGE_ACTIVATION, RANGE_INPUT, RANGE_INPUT_NONFINITE
    if words is not None:
        bits = ops.range_bits(words)
        # an overflow raises whether or not the step ALSO saw non-finite input pixels (one NaN depth pixel in one frame of a
        # batch must not switch the safety net off for the other frames)
        if bits & (RANGE_ACTIVATION | RANGE_INPUT):
            msg = range_message(bits & (RANGE_ACTIVATION | RANGE_INPUT))
            if bits & RANGE_INPUT_NONFINITE:
                msg += ("  (The step also saw non-finite input pixels.  NaN / inf DEPTH pixels are kept out of the network and "
                        "give NaN keypoints for their frame, like the reference; non-finite RGB pixels are not supported: "
                        "they propagate as NaN activations, which is what was flagged if the checkpoint is sound.)")
            raise ops.RangeError(msg)
        finite = torch.isfinite(keypoints_cpu)
        if bits & RANGE_INPUT_NONFINITE:
            # rows of frames whose crop holds a non-finite pixel are NaN by contract (has_hand == 2); the others must be finite
            if has_hand is not None:
                marked = torch.as_tensor(has_hand).reshape(-1) == 2
            elif inputs is not None and inputs.shape[0] == finite.shape[0]:   # the A2J-only entry: one crop per row
                marked = ~torch.isfinite(inputs).flatten(1).all(dim=1).cpu()
            else:
                return
            finite = finite.reshape(finite.shape[0], -1)[~marked]
        if not bool(finite.all()):    # (e.g. a non-finite bias of an output convolution)
            raise ops.RangeError("non-finite keypoints from finite, in-range inputs: the checkpoint holds non-finite or "
                                 "extreme values; build the engines with precision='f32' to compare")
        return
    # noting is off: only the symptom is left -- non-finite keypoints from finite inputs
    if not bool(torch.isfinite(keypoints_cpu).all()) and (inputs is None or bool(torch.isfinite(inputs).all())):
        raise ops.RangeError("non-finite keypoints from finite inputs: a value left the range of the f16x3 split format "
                             "(|v| > 65504).  Unset HN_CHECK_RANGE=0 to locate the kind, or build the engines with "
                             "precision='f32'")


class HandNetEngine:
    def __init__(self, fcos: FCOSEngine, a2j: A2JEngine, num_classes: int):
        if fcos.device != a2j.device:
            raise ValueError(f"detector on {fcos.device} but A2J on {a2j.device}")
        self.fcos, self.a2j, self.num_classes = fcos, a2j, num_classes
        self.device = fcos.device
        # captured steps, least recently used first: key -> (graph, static images, static depth, static HandNetOutput)
        self._graphs = collections.OrderedDict()
        self._host_records = {}     # eager to_host steps: batch -> (pinned record, device record)
        self._raw_staging = {}      # forward_raw from pageable host memory: (shape, dtype) -> two rotating pinned buffers + their events
        # f16x3 range contract.  Always on (HN_CHECK_RANGE=0 turns it off for A/B timing): every split producer of a step
        # notes values outside the fp16 range into this engine's flag block and the step ends with ONE tiny launch that
        # hands the words over as HandNetOutput.range_flags -- no sync; the drop-in HandNet.forward reads them with the
        # copy of the keypoints it makes anyway.  check_range (HN_CHECK_RANGE=1) is the synchronous debug form:
        # forward_device itself reads the words (one device -> host sync per call) and raises.
        self.note_range = os.environ.get("HN_CHECK_RANGE", "1") != "0"
        self.check_range = os.environ.get("HN_CHECK_RANGE", "") == "1"
        self._range_block = torch.zeros((4,), device=self.device, dtype=torch.int32) if self.note_range else None
        # Sparse streams: A2J runs on all N frames with a validity mask (static launch sequence, capturable), which wastes
        # its time on frames without a hand.  When the PREVIOUS step had a hand in fewer than half of its frames (read
        # back asynchronously: no sync on the dense path), this step reads its own count (one sync) and runs A2J on the
        # frames with a hand only.  Never under graph capture; HN_COMPACT_SPARSE=0 turns it off.
        self.compact_sparse = os.environ.get("HN_COMPACT_SPARSE", "1") != "0"
        self._hand_stat = None      # (event, pinned count tensor, frames) of the last eager step
        self._sparse_hint = False
        self._convert = None        # set_convert(): the aggregation's epilogue also writes image (u,v,d) / camera xyz
        self._track_states = {}     # tracked steps: (N, K) -> the tracker's state (ops.track_state), shared by eager steps and captures

    def set_convert(self, paras=None, clamp: bool = False, on: bool = True):
        """convert_joints + uvd2xyz as part of the step (a2j/a2j.py:17-43, what ros_demo.py:289,329-330 does with
        every result): HandNetOutput.image_uvd, and .xyz_mm when the camera intrinsics paras = (fx, fy, cx, cy) are given, are
        written by the aggregation's own launch, and to_host steps carry them in a wide record.  clamp: the live caller's
        clamps before the conversion (keypoints to [0, 176], box to the frame: ros_demo.py:279-283).  Captured steps are
        dropped (their launch sequence changes).
        paras may also be a camera per frame, [N,4] (a nested sequence, an ndarray or a tensor; rounded to fp32 as the one
        camera's values are): frame i -- every slot of frame i in forward_hands -- is converted with row i.
        The rows live in a table on the device that the aggregation reads (sample_paras of its conversion spec, one row per
        slot), so set_cameras() changes them under captured steps; a step over another number of frames raises ValueError."""
        paras = ops.camera_paras(paras)
        table = isinstance(paras, np.ndarray)
        self._convert = None if not on else {"paras": None if table else paras, "clamp": bool(clamp),
                                             "cams": CameraTables(paras, self.device) if table else None}
        self._graphs.clear()
        self._host_records.clear()
        return self

    @ops.device_guarded
    def set_cameras(self, paras):
        """New values for the per-frame cameras of set_convert(paras=[N,4]): copied into the same device tables (on the current
        stream), so eager steps and every already captured step convert with them from the next step on -- nothing is
        recaptured.  Same N; ValueError on an engine whose conversion has one camera or none."""
        c = self._convert
        if c is None or c["cams"] is None:
            raise ValueError("set_cameras needs a camera per frame: set_convert(paras=[N,4])")
        c["cams"].update(paras)
        return self

    def _convert_spec(self, crop_box, frame_hw, n=None, hands=None):
        c = self._convert
        if c is None:
            return None
        spec = {"crop_box": crop_box, "paras": c["paras"], "crop": CROP}
        if c["cams"] is not None:
            if n != c["cams"].frames:
                raise ValueError(f"a step over {n} frames, but set_convert was given {c['cams'].frames} cameras, one per frame")
            spec["sample_paras"] = c["cams"].rows(hands or 1)
        if c["clamp"]:
            spec.update(clamp_keypoints=True, clamp_box=frame_hw)
        return spec

    def _fields(self) -> int:
        c = self._convert
        return 1 if c is None else (3 if c["paras"] is not None or c["cams"] is not None else 2)

    @ops.device_guarded
    def forward_device(self, images, depth: torch.Tensor, to_host: bool = False, _record=None, _tail=None) -> HandNetOutput:
        """images [N,3,H,W] 0..1 (or a list of [3,h_i,w_i] tensors of different sizes), depth [N,1,H,W] metres
        (RGBD model: [N,4,H,W] = RGB + depth), fp32 on the GPU.  to_host: the step also packs its per-frame results and the
        range words into one record buffer and enqueues ONE device -> host copy of it into pinned memory
        (HandNetOutput.host_record; the reference returns its keypoints on the CPU, a2j/a2j.py:229) -- no sync here.
        _tail(keypoints, image_uvd, xyz_mm, has_hand): more launches of the SAME step, issued inside its range scope -- before
        the flag words are collected, so their split producers are covered by the step's range contract (the live step's
        lifter, hn_amd/live.py); its return value is HandNetOutput.tail."""
        return self._step(images, depth, None, to_host, _record, _tail)

    @ops.device_guarded
    def forward_hands(self, images, depth: torch.Tensor, max_hands: int = 2, to_host: bool = False, _record=None,
                      _tail=None, handed: bool = False, left_side: int = 0, _side=None, track: bool = False,
                      track_iou: float = 0.3, track_hold: int = 5, _track_out=None, objects: bool = False) -> HandsOutput:
        """forward_device for up to max_hands (1..16) hands per frame: slot k of frame i is the k-th hand-label detection of
        frame i in the detector's score order, cropped as forward_device crops the first (max_hands = 1 IS forward_device's
        crop); A2J runs on the N * max_hands crops with the slots' has_hand mask (capturable), or -- eager, when the previous
        step filled fewer than half of its slots -- on the filled slots only.  to_host: one record row per slot, the range
        words, then the scores and detection ranks, in ONE device -> host copy (HandsOutput.host_record; read_host_record /
        read_hands_tail after a sync).  _tail(keypoints, image_uvd, xyz_mm, has_hand), all per slot ([N*K,...]): as for
        forward_device; its return value is HandsOutput.tail.
        handed: per-slot handedness.  HandsOutput.side = detections.sides of the slot's detection (-1: empty slot); a filled
        slot whose side equals left_side (HandsOutput.mirror) goes through the right-handed pose network MIRRORED -- its crop
        is flipped along the width and the aggregation writes u = 176 - u -- so keypoints, image_uvd and xyz_mm are in the
        frame's own coordinates; every other slot is the step without `handed`, bit for bit, and no launch is added.
        left_side = 0 is an ASSUMPTION (the detector's side targets are box_info[:, 1] of its training set; the 100DOH
        convention 0 = left is not stated by the reference, which never reads `sides`): check it on your checkpoint.  to_host
        records carry the sides behind the scores and ranks (read_hands_tail(..., handed=True)).
        track: the slots are tracked from step to step -- batch row i is one camera stream; a hand keeps its
        slot and its HandsOutput.track_id while its padded crop box overlaps the slot's last one with IoU >= track_iou, whatever
        its score rank; a slot whose hand is missing is held EMPTY (has_hand 0) for track_hold steps, then freed; new hands
        take the free slots, lowest first, in score order.  The engine owns one state per (N, K), shared by eager steps and
        captures of that shape (track_reset() empties it).  to_host records carry track_id and track_age last
        (read_hands_tail(..., tracked=True)).  Frames of at most 32767 x 32767 pixels.
        objects: the detector pass goes through FCOSEngine.detect_ext (one more launch) and the step also hands out what the
        contact heads say about every detection row: HandsOutput.contacts [N,cap] and .dxdymags [N,cap,3] -- with det_index,
        what ops.hand_objects takes (the live step's objects=True).  An engine whose detector has no ext heads: RuntimeError,
        before any launch."""
        if objects and not self.fcos.ext:
            raise RuntimeError("forward_hands(objects=True) needs a detector with the ext heads: build the FCOS engine with ext=True")
        return self._step(images, depth, ops.check_max_hands(max_hands), to_host, _record, _tail,
                          (int(left_side), _side) if handed else None,
                          ops.check_track_options(track_iou, track_hold) + (_track_out,) if track else None, bool(objects))

    def _track_state(self, n, hands):
        st = self._track_states.get((n, hands))
        if st is None:
            with torch.inference_mode(False):
                st = self._track_states[(n, hands)] = ops.track_state(n, hands, self.device)
        return st

    @ops.device_guarded
    def track_reset(self):
        """Empty every tracker of this engine (a memset on the current stream; also between replays of a captured step)."""
        for st in self._track_states.values():
            st.zero_()
        return self

    def _step(self, images, depth, hands, to_host, _record, _tail, handed=None, track=None, objects=False):
        """The body of forward_device (hands None: the top-1 crop, HandNetOutput) and forward_hands (hands = K; handed =
        (left_side, where the sides go or None): the handed step; track = (thr_milli, hold, (where the ids go, the ages) or
        None): the tracked step)."""
        want_c = 4 if self.a2j.rgbd else 1
        if depth.dim() != 4 or depth.shape[1] != want_c or depth.shape[0] != len(images):
            raise ValueError(f"depth_images must be [N,{want_c},H,W] matching images"
                             + (" (RGB + depth, ros_demo.py:268-270)" if self.a2j.rgbd else ""))
        noting = self.note_range or self.check_range
        if noting and self._range_block is None:
            self._range_block = torch.zeros((4,), device=self.device, dtype=torch.int32)
        n = len(images)
        rows = n if hands is None else n * hands
        record = None
        if hands is not None and (to_host or _record is not None):
            # (fetched first: the crop stage writes the scores and ranks straight into the record)
            record = _record if _record is not None else self._host_record_buffers(n, hands, handed is not None,
                                                                                   track is not None)
        # (the scope is this host thread's: another engine on another thread keeps its own switch and block)
        with ops.range_scope(self._range_block, on=noting):
            contacts = dxdymags = None
            if objects:      # (the K-hand step's option: the contact heads' rows ride along)
                det, cand, contacts, dxdymags = self.fcos.detect_ext(images, zero=False)
            else:
                det, cand = self.fcos.detect(images)
            if hands is None:
                crop_box, has_hand, crops = ops.crop_resize(det, self.num_classes - 1, depth.float().contiguous(), CROP, 4,
                                                            reorder_bgr=self.a2j.rgbd)
                box_rows, has_rows = crop_box, has_hand
            else:
                # (sides, ids and ages go where the caller wants them -- the live step's buffer -- else behind the scores and ranks
                # of this step's own record)
                score = det_index = mirror = None
                side = None if handed is None else handed[1]
                track_id, track_age = (None, None) if track is None or track[2] is None else track[2]
                if record is not None:
                    own_side, own_track = handed is not None and side is None, track is not None and track[2] is None
                    views = _hands_tail(record[1], rows, handed=own_side, tracked=own_track)
                    score, det_index = views[:2]
                    if own_side:
                        side = views[2]
                    if own_track:
                        track_id, track_age = views[-2:]
                tracking = {} if track is None else dict(track=self._track_state(n, hands), track_iou=track[0] / 1000.0,
                                                         track_hold=track[1], track_id=track_id, track_age=track_age)
                res = ops.crop_resize_hands(
                    det, self.num_classes - 1, depth.float().contiguous(), hands, CROP, 4, score=score, det_index=det_index,
                    reorder_bgr=self.a2j.rgbd, handed=handed is not None, left_side=0 if handed is None else handed[0], side=side,
                    **tracking)
                crop_box, has_hand, score, det_index, crops = res[:5]
                if handed is not None:
                    side, mirror = res[5].view(n, hands), res[6].view(n, hands)
                if track is not None:
                    track_id, track_age = res[-2].view(n, hands), res[-1].view(n, hands)
                box_rows, has_rows = crop_box.view(rows, 4), has_hand.view(rows)
            conv = self._convert_spec(box_rows, tuple(depth.shape[-2:]), n, hands)
            unconverted = hands is not None and mirror is not None and conv is None
            if unconverted:     # (the un-mirror is part of the converting aggregation: its image (u,v,d) is not handed out)
                conv = {"crop_box": box_rows, "paras": None, "crop": CROP}
            if hands is not None and mirror is not None:
                conv["mirror"] = mirror.view(rows)
            kp = self._a2j_sparse(crops, has_rows, conv) if self._use_compaction(rows) else None
            if kp is None:
                kp = self.a2j.forward_nhwc(crops, valid=has_rows, convert=conv)
            img_uvd = xyz = None
            if conv is not None:
                kp, img_uvd, xyz = kp
                if unconverted:
                    img_uvd = None
            if _tail is None:
                tail = None
            else:
                tail = _tail(kp, img_uvd, xyz, has_rows) if handed is None else _tail(kp, img_uvd, xyz, has_rows, mirror.view(rows))
            host_rec = None
            if to_host or _record is not None:
                host_rec, dev_rec = record if record is not None else (
                    _record if _record is not None else self._host_record_buffers(n))
                ops.pack_records(kp, box_rows, has_rows, rows + 1, dev_rec.shape[1], out=dev_rec[:rows + 1],
                                 extras=(img_uvd, xyz))   # (row `rows`: zeros)
                flags = ops.range_check_collect(self._range_block, out=dev_rec[rows, :16].view(torch.int32)) if noting else None
                if host_rec is not None:      # (None: the caller copies a larger buffer that holds the records -- the live step)
                    host_rec.copy_(dev_rec, non_blocking=True)
            else:
                flags = ops.range_check_collect(self._range_block) if noting else None
        self._note_hand_count(has_rows, rows)
        if self.check_range:
            bits = ops.range_bits(flags.cpu().tolist())
            if bits:
                raise ops.RangeError(range_message(bits))
        if hands is None:
            return HandNetOutput(kp, crops, crop_box, has_hand, det, cand, flags, img_uvd, xyz, tail, host_rec)
        per_slot = (n, hands) + tuple(kp.shape[1:])
        return HandsOutput(kp.view(per_slot), crops, crop_box, has_hand, score, det_index, det, cand, flags,
                           None if img_uvd is None else img_uvd.view(per_slot), None if xyz is None else xyz.view(per_slot),
                           host_rec, tail, side, mirror, contacts, dxdymags, track_id, track_age)

    # -------------------------------------------------------------------------------
    # sparse streams: A2J on the frames with a hand only
    # -------------------------------------------------------------------------------
    def _use_compaction(self, n: int) -> bool:
        if not self.compact_sparse or n < 8 or torch.cuda.is_current_stream_capturing():
            return False
        st = self._hand_stat
        if st is not None and st[0].query():          # the previous step's count has arrived: refresh the hint
            self._sparse_hint = int(st[1].item()) * 2 < st[2]
            self._hand_stat = None
        return self._sparse_hint

    def _note_hand_count(self, has_hand, n):
        """Asynchronous read-back of this step's hand count (hint for the next step; no sync)."""
        if not self.compact_sparse or n < 8 or torch.cuda.is_current_stream_capturing() or self._hand_stat is not None:
            return
        pinned = torch.empty((1,), dtype=torch.int64, pin_memory=True)
        pinned.copy_((has_hand != 0).sum(dtype=torch.int64).reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hand_stat = (ev, pinned, n)

    def _a2j_sparse(self, crops, has_hand, conv=None):
        """A2J on the frames with a hand only (one device -> host sync for the count); None = not sparse after all.
        conv: the step's conversion spec -> (crop uvd, image uvd, xyz or None), zero rows for the frames without a hand."""
        n = has_hand.shape[0]
        idx = torch.nonzero(has_hand, as_tuple=False).flatten()      # synchronises
        k = int(idx.numel())
        if k * 2 >= n:
            self._sparse_hint = False
            return None
        fields = 1 if conv is None else (3 if conv["paras"] is not None or conv.get("sample_paras") is not None else 2)
        outs = [torch.zeros((n, self.a2j.joints, 3), device=crops.device, dtype=torch.float32) for _ in range(fields)]
        if k:
            v = has_hand[idx].contiguous()
            sub = None if conv is None else dict(conv, crop_box=conv["crop_box"][idx].contiguous())
            for per_row in ("mirror", "sample_paras"):
                if sub is not None and sub.get(per_row) is not None:
                    sub[per_row] = sub[per_row][idx].contiguous()
            res = self.a2j.forward_nhwc(crops[idx].contiguous(), valid=v, convert=sub)
            for o, r in zip(outs, res if conv is not None else (res,)):
                o[idx] = r
            has_hand[idx] = v       # (the stem raises a flag to 2 for a crop with non-finite pixels: report it like the dense path)
        if conv is None:
            return outs[0]
        return outs[0], outs[1], (outs[2] if fields == 3 else None)

    # -------------------------------------------------------------------------------
    # hipGraph replay for a fixed batch shape (launch-bound at small batch)
    # -------------------------------------------------------------------------------
    def _new_record(self, n, hands=None, handed=False, tracked=False):
        """(pinned host, device) record buffers of a step over n frames (hands: forward_hands with that many slots per frame;
        handed: with the slots' sides; tracked: with their track ids and ages)."""
        rb = record_bytes(self._fields())
        rows = n + 1 if hands is None else hands_record_rows(n * hands, rb, handed, tracked)
        return (torch.zeros((rows, rb), dtype=torch.uint8, pin_memory=True),
                torch.zeros((rows, rb), dtype=torch.uint8, device=self.device))

    def _host_record_buffers(self, n, hands=None, handed=False, tracked=False):
        key = n if hands is None else ("hands", n, hands) + (("handed",) if handed else ()) + (("tracked",) if tracked else ())
        buf = self._host_records.get(key)
        if buf is None:
            with torch.inference_mode(False):   # ordinary tensors: written in place by later calls in any mode
                buf = self._host_records[key] = self._new_record(n, hands, handed, tracked)
        return buf

    @ops.device_guarded
    def graphed(self, images: torch.Tensor, depth: torch.Tensor, to_host: bool = False, limit: int | None = None):
        """Returns (run, static_images, static_depth, static_output): copy new inputs into the
        static tensors and call run() to replay the captured step.  to_host: the captured step ends with the record pack and
        the device -> host copy of forward_device(to_host=True) (static_output.host_record).  limit: at most that many
        captured steps are kept -- capturing one more evicts the least recently used (its static activation pool is freed)."""
        key = (tuple(images.shape), tuple(depth.shape), bool(to_host))
        return self._graphed(key, images, depth, to_host, limit, None)

    @ops.device_guarded
    def graphed_hands(self, images: torch.Tensor, depth: torch.Tensor, max_hands: int = 2, to_host: bool = False,
                      limit: int | None = None, handed: bool = False, left_side: int = 0, track: bool = False,
                      track_iou: float = 0.3, track_hold: int = 5):
        """graphed() for forward_hands(images, depth, max_hands, to_host, handed=, left_side=, track=, ...): (run,
        static_images, static_depth, static HandsOutput).  Its captures are keyed apart from graphed()'s (a handed step apart
        from a plain one, a tracked step apart from both) and share their eviction order (limit).  A tracked capture bakes in
        the engine's state of its (N, K) -- the one eager tracked steps of that shape use -- and capturing leaves that state as
        it found it."""
        k = ops.check_max_hands(max_hands)
        handed = (int(left_side), None) if handed else None
        track = ops.check_track_options(track_iou, track_hold) + (None,) if track else None
        return self._graphed(self._hands_key(images.shape, depth.shape, k, to_host, handed, track), images, depth, to_host, limit,
                             k, handed, track)

    @staticmethod
    def _hands_key(image_shape, depth_shape, max_hands, to_host, handed=None, track=None):
        key = ("hands", tuple(image_shape), tuple(depth_shape), int(max_hands), bool(to_host))
        key = key if handed is None else key + ("handed", handed[0])
        return key if track is None else key + ("tracked", track[0], track[1])

    def has_graph_hands(self, image_shape, depth_shape, max_hands, to_host: bool = False, handed: bool = False,
                        left_side: int = 0, track: bool = False, track_iou: float = 0.3, track_hold: int = 5) -> bool:
        return self._hands_key(image_shape, depth_shape, max_hands, to_host, (int(left_side), None) if handed else None,
                               ops.check_track_options(track_iou, track_hold) if track else None) in self._graphs

    def _track_untouched(self, n, hands):
        """Context manager around the capture of a tracked step over (n, hands): the capture's eager warm-up steps advance the
        tracker, so the state is put back as it was when the capture is done."""
        import contextlib

        @contextlib.contextmanager
        def keep():
            state = self._track_state(n, hands)
            saved = state.clone()
            try:
                yield state
            finally:
                state.copy_(saved)
        return keep()

    def _graphed(self, key, images, depth, to_host, limit, hands, handed=None, track=None):
        if key not in self._graphs:
            while limit is not None and len(self._graphs) >= max(1, limit):
                self._graphs.popitem(last=False)
            with torch.inference_mode(False), torch.no_grad():
                return self._capture(key, images, depth, to_host, hands, handed, track)
        self._graphs.move_to_end(key)
        g, s_img, s_dep, out = self._graphs[key]
        return g.replay, s_img, s_dep, out

    def has_graph(self, image_shape, depth_shape, to_host: bool = False) -> bool:
        return (tuple(image_shape), tuple(depth_shape), bool(to_host)) in self._graphs

    def graph_count(self) -> int:
        return len(self._graphs)

    def captured(self, image_shape, depth_shape, to_host: bool = False):
        """(graph, static images, static depth, static output) of a captured step for these shapes, or None; a hit counts as a
        use for the eviction order.  The caller fills the static inputs and calls graph.replay()."""
        key = (tuple(image_shape), tuple(depth_shape), bool(to_host))
        hit = self._graphs.get(key)
        if hit is not None:
            self._graphs.move_to_end(key)
        return hit

    def replay_frames(self, frames, depth, to_host: bool = False):
        """Steady state of the live caller (ros_demo.py:270: a list of equally sized frames per call): when a captured
        step for these shapes exists, stack the frames straight into its input buffer (one kernel instead of stack + copy),
        copy the depth map and replay.  Returns the step's static HandNetOutput, or None when nothing is captured for
        these shapes (or the frames differ in shape / dtype)."""
        first = frames[0]
        hit = self.captured((len(frames),) + tuple(first.shape), depth.shape, to_host)
        if hit is None or any(f.shape != first.shape for f in frames):
            return None
        g, s_img, s_dep, out = hit
        if len(frames) == 1:
            s_img[0].copy_(first)
        else:
            torch.stack(list(frames), out=s_img)
        s_dep.copy_(depth)
        g.replay()
        return out

    # -------------------------------------------------------------------------------
    # raw camera frames: the reference caller's host-side conversions as one kernel (ros_demo.py:227-231,266-269)
    # -------------------------------------------------------------------------------
    def _device_readable(self, t: torch.Tensor, used: list):
        """GPU tensors and pinned host tensors as they are; pageable host memory through a pinned staging buffer of the
        engine (one host memcpy; the ingest kernel then reads the pinned buffer over PCIe itself).  The ingest kernel reads the
        staging buffer ASYNCHRONOUSLY, so a buffer is only written again once the event recorded behind the ingest launch
        that read it has passed (_staged_done); two buffers per (shape, dtype) rotate, so that a pipelined caller -- call k + 1
        issued while step k still runs -- only ever waits for the ingest of call k - 1."""
        if t.is_cuda:
            return t.contiguous()
        if t.is_pinned() and t.is_contiguous():
            return t
        key = (tuple(t.shape), t.dtype)
        ring = self._raw_staging.get(key)
        if ring is None:
            with torch.inference_mode(False):
                ring = self._raw_staging[key] = {"slots": [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True), None]
                                                           for _ in range(2)], "next": 0}
        slot = ring["slots"][ring["next"]]
        ring["next"] ^= 1
        if slot[1] is not None:
            slot[1].synchronize()       # the ingest launch that last read this buffer has finished
            slot[1] = None
        slot[0].copy_(t)
        used.append(slot)
        return slot[0]

    @staticmethod
    def _staged_done(used: list):
        """Record, behind the ingest launch, the event that frees the staging buffers it reads."""
        for slot in used:
            ev = torch.cuda.Event()
            ev.record()
            slot[1] = ev

    @ops.device_guarded
    def forward_raw(self, bgr_u8, depth_raw, to_host: bool = False, use_graph: bool = False, limit: int | None = None):
        """bgr_u8 uint8 [N,H,W,3] (cv_bridge 'bgr8'), depth_raw [N,H,W] uint16 millimetres (16UC1) or float32 metres (32FC1);
        torch tensors on the GPU or on the host (pinned: read in place; pageable: staged once).  ONE ingest kernel writes the
        fp32 RGB batch and the metres depth map (RGB-D model: the 4-channel tensor) -- straight into the input buffers of the
        captured step when use_graph / a capture for these shapes exists -- then the step runs as forward_device does."""
        staged = []
        bgr, dep = self._device_readable(bgr_u8, staged), self._device_readable(depth_raw, staged)
        n, h, w, _ = bgr.shape
        dshape = (n, 4 if self.a2j.rgbd else 1, h, w)
        hit = self.captured((n, 3, h, w), dshape, to_host)
        if hit is None:
            rgb, d1, d4 = ops.ingest_raw(bgr, dep, device=self.device, want_rgbd=self.a2j.rgbd, want_depth=not self.a2j.rgbd)
            depth = d4 if self.a2j.rgbd else d1
            if not use_graph or torch.cuda.is_current_stream_capturing():
                self._staged_done(staged)
                return self.forward_device(rgb, depth, to_host=to_host)
            self.graphed(rgb, depth, to_host=to_host, limit=limit)
            hit = self.captured((n, 3, h, w), dshape, to_host)
        return self._ingest_replay(hit, bgr, dep, staged)

    def _ingest_replay(self, hit, bgr, dep, staged, flip_w=False):
        """Ingest into the static inputs of a captured step (this engine's, or a live step's around it) and replay it.  The
        staging event is recorded ONCE, behind the last ingest_raw of the call that reads the staging buffers.  flip_w: the
        live step's `left` mode, done by the ingest kernel."""
        g, s_img, s_dep, out = hit
        if self.a2j.rgbd:     # (the 4-channel tensor only: no separate depth map is written or allocated)
            ops.ingest_raw(bgr, dep, out_rgb=s_img, out_rgbd=s_dep, want_depth=False, flip_w=flip_w)
        else:
            ops.ingest_raw(bgr, dep, out_rgb=s_img, out_depth=s_dep, flip_w=flip_w)
        self._staged_done(staged)
        g.replay()
        return out

    def _capture(self, key, images, depth, to_host=False, hands=None, handed=None, track=None):
        # static buffers are ordinary (non-inference) tensors so that later copy_() works in any mode
        s_img, s_dep = torch.empty_like(images), torch.empty_like(depth)
        s_img.copy_(images)
        s_dep.copy_(depth)
        # the capture's own record buffers (addresses are baked into the graph)
        record = self._new_record(images.shape[0], hands, handed is not None, track is not None) if to_host else None

        def step():
            if hands is None:
                return self.forward_device(s_img, s_dep, _record=record)
            return self.forward_hands(s_img, s_dep, hands, _record=record, handed=handed is not None,
                                      left_side=0 if handed is None else handed[0], track=track is not None,
                                      track_iou=0.3 if track is None else track[0] / 1000.0,
                                      track_hold=5 if track is None else track[1])

        if track is not None:
            with self._track_untouched(images.shape[0], hands):
                g, out = ops.capture_step(step)
        else:
            g, out = ops.capture_step(step)
        self._graphs[key] = (g, s_img, s_dep, out)
        return g.replay, s_img, s_dep, out
