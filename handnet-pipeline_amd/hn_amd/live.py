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
import contextlib
import functools
import math
from dataclasses import dataclass, field

import numpy as np
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


POSE_LABEL = ops.LABEL_CROP                           # side of a pose_label image

LiveViews = collections.namedtuple("LiveViews", "records side lifted mesh overlay box_label pose_label")
# ... and of a tracked step: the same fields, then the two rows of the tracker
LiveTrackedViews = collections.namedtuple("LiveTrackedViews", LiveViews._fields + ("track_id", "track_age"))
# ... and of a smoothed step: those, then the two filtered signals
LiveSmoothedViews = collections.namedtuple("LiveSmoothedViews", LiveTrackedViews._fields + ("smooth_xyz", "smooth_mesh"))
SMOOTH_JOINTS = ops.SMOOTH_JOINTS


@functools.lru_cache(maxsize=None)
def _occluded_views(kind):
    """... and of an occluded step: the fields of its step without the option, then the silhouette and the coverage"""
    return collections.namedtuple(kind.__name__.replace("Views", "OccludedViews"), kind._fields + ("silhouette", "coverage"))


RIG_FIELDS = ops.RIG_FIELDS


@functools.lru_cache(maxsize=None)
def _rig_views(kind):
    """... and of a rig step: the fields of its step without the option, then the eight parts of the rig frame"""
    return collections.namedtuple(kind.__name__.replace("Views", "RigViews"), kind._fields + RIG_FIELDS)


CLOUD_FIELDS = ("cloud", "cloud_count", "cloud_resid")


@functools.lru_cache(maxsize=None)
def _cloud_views(kind):
    """... and of a cloud step: the fields of its step without the option, then the three parts of the hand clouds"""
    return collections.namedtuple(kind.__name__.replace("Views", "CloudViews"), kind._fields + CLOUD_FIELDS)


FIT_FIELDS = ("fit_mesh", "fit_xyz", "fit_rt", "fit_count", "fit_cost")


@functools.lru_cache(maxsize=None)
def _fit_views(kind):
    """... and of a fit step: the fields of its step without the option, then the five parts of the fitted meshes"""
    return collections.namedtuple(kind.__name__.replace("Views", "FitViews"), kind._fields + FIT_FIELDS)


@functools.lru_cache(maxsize=None)
def _fit_trace_views(kind):
    """... and of a fit step of two iterations or more: the fields of its fit step, then the trace"""
    return collections.namedtuple(kind.__name__.replace("Views", "TraceViews"), kind._fields + ("fit_trace",))


OBJECT_FIELDS = ops.OBJECT_FIELDS


@functools.lru_cache(maxsize=None)
def _objects_views(kind):
    """... and of an objects step: the fields of its step without the option, then the eight parts of the held objects"""
    return collections.namedtuple(kind.__name__.replace("Views", "ObjectsViews"), kind._fields + OBJECT_FIELDS)


# What a cloud or fit step keeps on the device beside its copy buffer: the raster's nearest Z fp32 [n,h,w]; the cloud launches'
# scratch, the fit launches' scratch and the iterated fit's work (each None in a step without them); a fit_draw step's geometry
# depth fp32 [n,h,w] and slot byte uint8 [n,h,w] (else None)
StepWork = collections.namedtuple("StepWork", "mesh_depth cloud_scratch fit_scratch fit_work geo_depth geo_who")


@dataclass(frozen=True)
class LiveLayout:
    """Byte layout of a live step's one copy buffer, in this order: the records (one-hand step: a wide record per frame + the
    range-word row; K-hand step: forward_hands' wide record unchanged -- a row per slot, the range-word row, the scores and
    detection ranks: hands_record_rows), `side` int32 [slots] (handed steps: the detector's side per slot), `track_id` and
    `track_age` int32 [slots] each (tracked steps), `lifted` int32 [slots] (K-hand steps), the mesh fp32 [slots,V,3], the overlay uint8 [frames,h,w,3], box_label uint8 [frames,h,w,3] and
    pose_label uint8 [slots,176,176,3] (each label image starts on a dword: the kernels store three dwords per four pixels),
    and -- smoothed steps -- `smooth_xyz` fp32 [slots,21,3] and `smooth_mesh` fp32 [slots,V,3], each on a dword, and -- occluded
    steps -- `silhouette` uint8 [frames,h,w] and `coverage` int32 [slots,2], each on a dword, and -- rig steps --
    `rig_xyz` fp32 [slots,21,3], `rig_mesh` fp32 [slots,V,3], `rig_hand` int32 [slots], `rig_count` int32 [1], `rig_views` and
    `rig_seed` int32 [slots], `fused_xyz` fp32 [slots,21,3] and `fused_mesh` fp32 [slots,V,3], each on a dword, and -- cloud steps
    (cloud = P, the rows per slot) -- `cloud` fp32 [slots,P,3] and `cloud_count` int32 [slots,2], each on a dword,
    and `cloud_resid` int64 [slots] on 8 bytes (their offsets cloud_at, cloud_count_at, cloud_resid_at are properties, not
    fields), and -- fit steps -- `fit_mesh` fp32 [slots,V,3], `fit_xyz` fp32 [slots,21,3], `fit_rt` fp32 [slots,12]
    and `fit_count` int32 [slots,2], each on a dword, and `fit_cost` int64 [slots] on 8 bytes, as the last parts (fit_mesh_at,
    fit_xyz_at, fit_rt_at, fit_count_at, fit_cost_at: properties too), and -- fit steps of I = 2..8 iterations, for
    which `fit` holds the integer I where a step of one iteration holds True -- `fit_trace` int64 [slots,I,3] on 8 bytes as the
    last part (fit_trace_at: a property), and -- objects steps (LiveObjectsLayout, the same class with `objects` on:
    a class attribute, not a field) -- `contact` and `object_index` int32 [slots], `object_box` fp32 [slots,4], `object_score` fp32
    [slots], `object_point` fp32 [slots,2], `object_xyz` fp32 [slots,3], `object_extent` fp32 [slots,6] and `object_count` int32
    [slots,2], each on a dword, behind every other part (contact_at, object_index_at, ...: properties).
    slots = frames for the one-hand step (hands None), frames * hands for the K-hand step.  A part the step does not have takes
    no bytes and its offset is None; every part in front of it stays where a step without the option has it."""
    frames: int
    hands: int                   # None: the one-hand step, else K
    vertices: int
    hw: tuple = None             # (h, w) of the frames; None: a step that draws nothing
    overlay: bool = False
    labels: bool = False
    handed: bool = False
    tracked: bool = False
    smoothed: bool = False
    occluded: bool = False       # (keyword: the overlay hidden behind nearer scene depth; needs overlay)
    fit: bool = False            # (keyword: every slot's mesh and joints fitted to the measured depth; needs occluded; an
    #                              integer 2..8: that many iterations, and the trace as the last part)
    cloud: int = 0               # (keyword: rows per slot of the hand clouds, 0: none; needs occluded)
    rig: bool = False            # (keyword: the slots in the rig frame, associated across frames and fused; a K-hand step's)
    record_rows: int = field(init=False)
    record_bytes: int = field(init=False)
    side_at: int = field(init=False)
    track_id_at: int = field(init=False)
    track_age_at: int = field(init=False)
    lifted_at: int = field(init=False)
    mesh_at: int = field(init=False)
    overlay_at: int = field(init=False)
    box_label_at: int = field(init=False)
    pose_label_at: int = field(init=False)
    smooth_xyz_at: int = field(init=False)
    smooth_mesh_at: int = field(init=False)
    silhouette_at: int = field(init=False)
    coverage_at: int = field(init=False)
    rig_xyz_at: int = field(init=False)
    rig_mesh_at: int = field(init=False)
    rig_hand_at: int = field(init=False)
    rig_count_at: int = field(init=False)
    rig_views_at: int = field(init=False)
    rig_seed_at: int = field(init=False)
    fused_xyz_at: int = field(init=False)
    fused_mesh_at: int = field(init=False)
    nbytes: int = field(init=False)
    objects = False              # (no field: LiveObjectsLayout switches the held objects' eight parts on)

    def __post_init__(self):
        if ((self.overlay or self.labels) and self.hw is None) or ((self.handed or self.tracked) and self.hands is None):
            raise ValueError("an overlay or label images need the frames' (h, w), and handed / tracked are a K-hand step's options")
        if self.smoothed and not self.tracked:
            raise ValueError("a smoothed step is a tracked step: the filters follow the track ids")
        if self.occluded and not self.overlay:
            raise ValueError("an occluded step is a step with an overlay: the silhouette is the overlay's by-product")
        if isinstance(self.cloud, bool) or not isinstance(self.cloud, (int, np.integer)) or self.cloud < 0:
            raise ValueError(f"cloud: the rows per slot, an integer >= 0 (got {self.cloud!r})")
        if self.cloud and not self.occluded:
            raise ValueError("a cloud step is an occluded step: the clouds are cut out with the silhouette")
        if self.fit and not self.occluded:
            raise ValueError("a fit step is an occluded step: the mesh is fitted to the depth pixels under its silhouette")
        if not isinstance(self.fit, bool) and (not isinstance(self.fit, (int, np.integer)) or not 2 <= self.fit <= ops.FIT_MAX_ITERS):
            raise ValueError(f"fit: False, True (one iteration) or the iterations as an integer 2..{ops.FIT_MAX_ITERS} "
                             f"(got {self.fit!r})")
        if self.objects and self.hands is None:
            raise ValueError("objects is a K-hand step's option: the slots' detection rows are what the objects are associated with")
        if self.rig:
            if self.hands is None:
                raise ValueError("rig is a K-hand step's option: the rig frame puts the slots of several frames together")
            ops.check_rig_slots(self.frames, self.hands)
        s, rb = self.slots, record_bytes(3)
        rows = self.frames + 1 if self.hands is None else hands_record_rows(s, rb)
        image = None if self.hw is None else (self.frames, *self.hw, 3)
        put = lambda name, value: object.__setattr__(self, name, value)
        end, spans = 0, {}
        for name, present, dtype, shape, align in (("records", True, torch.uint8, (rows, rb), 1),
                                                   ("side", self.handed, torch.int32, (s,), 1),
                                                   ("track_id", self.tracked, torch.int32, (s,), 1),
                                                   ("track_age", self.tracked, torch.int32, (s,), 1),
                                                   ("lifted", self.hands is not None, torch.int32, (s,), 1),
                                                   ("mesh", True, torch.float32, (s, self.vertices, 3), 1),
                                                   ("overlay", self.overlay, torch.uint8, image, 1),
                                                   ("box_label", self.labels, torch.uint8, image, 4),
                                                   ("pose_label", self.labels, torch.uint8, (s, POSE_LABEL, POSE_LABEL, 3), 4),
                                                   ("smooth_xyz", self.smoothed, torch.float32, (s, SMOOTH_JOINTS, 3), 4),
                                                   ("smooth_mesh", self.smoothed, torch.float32, (s, self.vertices, 3), 4),
                                                   ("silhouette", self.occluded, torch.uint8, image and image[:3], 4),
                                                   ("coverage", self.occluded, torch.int32, (s, 2), 4),
                                                   ("rig_xyz", self.rig, torch.float32, (s, SMOOTH_JOINTS, 3), 4),
                                                   ("rig_mesh", self.rig, torch.float32, (s, self.vertices, 3), 4),
                                                   ("rig_hand", self.rig, torch.int32, (s,), 4),
                                                   ("rig_count", self.rig, torch.int32, (1,), 4),
                                                   ("rig_views", self.rig, torch.int32, (s,), 4),
                                                   ("rig_seed", self.rig, torch.int32, (s,), 4),
                                                   ("fused_xyz", self.rig, torch.float32, (s, SMOOTH_JOINTS, 3), 4),
                                                   ("fused_mesh", self.rig, torch.float32, (s, self.vertices, 3), 4),
                                                   ("cloud", self.cloud, torch.float32, (s, self.cloud, 3), 4),
                                                   ("cloud_count", self.cloud, torch.int32, (s, 2), 4),
                                                   ("cloud_resid", self.cloud, torch.int64, (s,), 8),
                                                   ("fit_mesh", self.fit, torch.float32, (s, self.vertices, 3), 4),
                                                   ("fit_xyz", self.fit, torch.float32, (s, SMOOTH_JOINTS, 3), 4),
                                                   ("fit_rt", self.fit, torch.float32, (s, 12), 4),
                                                   ("fit_count", self.fit, torch.int32, (s, 2), 4),
                                                   ("fit_cost", self.fit, torch.int64, (s,), 8),
                                                   ("fit_trace", self.fit_iters > 1, torch.int64, (s, self.fit_iters, 3), 8),
                                                   ("contact", self.objects, torch.int32, (s,), 4),
                                                   ("object_index", self.objects, torch.int32, (s,), 4),
                                                   ("object_box", self.objects, torch.float32, (s, 4), 4),
                                                   ("object_score", self.objects, torch.float32, (s,), 4),
                                                   ("object_point", self.objects, torch.float32, (s, 2), 4),
                                                   ("object_xyz", self.objects, torch.float32, (s, 3), 4),
                                                   ("object_extent", self.objects, torch.float32, (s, 6), 4),
                                                   ("object_count", self.objects, torch.int32, (s, 2), 4)):
            start = None
            if present:
                start = (end + align - 1) // align * align
                end = start + math.prod(shape) * dtype.itemsize
                spans[name] = (start, end, dtype, shape)
            if name != "records" and name not in CLOUD_FIELDS + FIT_FIELDS + ("fit_trace",) + OBJECT_FIELDS:
                put(name + "_at", start)
        put("record_rows", rows)
        put("record_bytes", rb)
        put("nbytes", end)
        put("_spans", spans)         # (no field: what views() cuts, worked out once)

    @property
    def slots(self) -> int:
        return self.frames * (self.hands or 1)

    @property
    def fit_iters(self) -> int:
        """the iterations of a fit step (0: the step does not fit)"""
        return int(self.fit)

    def _part_at(self, name):
        span = self._spans.get(name)
        return None if span is None else span[0]

    cloud_at = property(lambda self: self._part_at("cloud"))
    cloud_count_at = property(lambda self: self._part_at("cloud_count"))
    cloud_resid_at = property(lambda self: self._part_at("cloud_resid"))
    fit_mesh_at = property(lambda self: self._part_at("fit_mesh"))
    fit_xyz_at = property(lambda self: self._part_at("fit_xyz"))
    fit_rt_at = property(lambda self: self._part_at("fit_rt"))
    fit_count_at = property(lambda self: self._part_at("fit_count"))
    fit_cost_at = property(lambda self: self._part_at("fit_cost"))
    fit_trace_at = property(lambda self: self._part_at("fit_trace"))
    contact_at = property(lambda self: self._part_at("contact"))
    object_index_at = property(lambda self: self._part_at("object_index"))
    object_box_at = property(lambda self: self._part_at("object_box"))
    object_score_at = property(lambda self: self._part_at("object_score"))
    object_point_at = property(lambda self: self._part_at("object_point"))
    object_xyz_at = property(lambda self: self._part_at("object_xyz"))
    object_extent_at = property(lambda self: self._part_at("object_extent"))
    object_count_at = property(lambda self: self._part_at("object_count"))

    def views(self, buf) -> LiveViews:
        """The parts of a step's flat uint8 buffer (the device buffer or its pinned copy), typed and shaped; None: not there."""
        cut = {name: buf[a:b].view(dtype).view(shape) for name, (a, b, dtype, shape) in self._spans.items()}
        kind = LiveSmoothedViews if self.smoothed else LiveTrackedViews if self.tracked else LiveViews
        if self.occluded:
            kind = _occluded_views(kind)
        if self.rig:
            kind = _rig_views(kind)
        if self.cloud:
            kind = _cloud_views(kind)
        if self.fit:
            kind = _fit_views(kind)
        if self.fit_iters > 1:
            kind = _fit_trace_views(kind)
        if self.objects:
            kind = _objects_views(kind)
        return kind(*(cut.get(name) for name in kind._fields))


@dataclass(frozen=True)
class LiveObjectsLayout(LiveLayout):
    """LiveLayout of a K-hand step with objects=True: the same fields and the same offsets for every part a step
    without the option has, and the held objects' eight parts behind them."""
    objects = True


@functools.lru_cache(maxsize=None)
def _read_type(step: str, base: tuple, overlay: bool, labels: bool, side: bool, tracked: bool = False, smoothed: bool = False,
               occluded: bool = False, rig: bool = False, cloud: bool = False):
    """The namedtuple a step's read() returns: the base fields, then overlay, box_label + pose_label, side, track_age +
    track_id, smooth_xyz + smooth_mesh, silhouette + coverage, the rig frame's eight and the clouds' three, each only when the step has it; an
    absent image (overlay / box_label / pose_label) reads as a None class attribute.  (One class per combination: call it with
    positional arguments only and without trailing defaults, the cache keys on them.)"""
    has = dict(overlay=overlay, box_label=labels, pose_label=labels, side=side, track_age=tracked, track_id=tracked,
               smooth_xyz=smoothed, smooth_mesh=smoothed, silhouette=occluded, coverage=occluded, **{f: rig for f in RIG_FIELDS},
               **{f: cloud for f in CLOUD_FIELDS})
    fields = base + tuple(f for f, on in has.items() if on)
    name = (step + "Overlay" * overlay + "Labels" * labels + "Sided" * side + "Tracked" * tracked + "Smoothed" * smoothed
            + "Occluded" * occluded + "Rig" * rig + "Cloud" * cloud + "Read")
    absent = {f: None for f, on in has.items() if not on and f in ("overlay", "box_label", "pose_label")}
    doc = f"{step}Output.read(): {' '.join(base)}" + "".join(f" + {f}" for f in fields[len(base):]) + "."
    return type(name, (collections.namedtuple(name, fields),), dict(absent, __slots__=(), __doc__=doc))


@functools.lru_cache(maxsize=None)
def _fit_read_type(kind):
    """The read type of a fit step: the fields of `kind` -- the read type of its step without the option --, then the fit's five."""
    name = kind.__name__[:-len("Read")] + "FitRead"
    absent = {f: None for f in ("overlay", "box_label", "pose_label") if f not in kind._fields}
    doc = kind.__doc__.rstrip(".") + "".join(f" + {f}" for f in FIT_FIELDS) + "."
    return type(name, (collections.namedtuple(name, kind._fields + FIT_FIELDS),), dict(absent, __slots__=(), __doc__=doc))


@functools.lru_cache(maxsize=None)
def _fit_trace_read_type(kind):
    """The read type of a fit step of two iterations or more: the fields of `kind` -- its fit step's read type --, then fit_trace."""
    name = kind.__name__[:-len("Read")] + "TraceRead"
    absent = {f: None for f in ("overlay", "box_label", "pose_label") if f not in kind._fields}
    doc = kind.__doc__.rstrip(".") + " + fit_trace."
    return type(name, (collections.namedtuple(name, kind._fields + ("fit_trace",)),), dict(absent, __slots__=(), __doc__=doc))


@functools.lru_cache(maxsize=None)
def _objects_read_type(kind):
    """The read type of an objects step: the fields of `kind` -- the read type of its step without the option --, then the eight."""
    name = kind.__name__[:-len("Read")] + "ObjectsRead"
    absent = {f: None for f in ("overlay", "box_label", "pose_label") if f not in kind._fields}
    doc = kind.__doc__.rstrip(".") + "".join(f" + {f}" for f in OBJECT_FIELDS) + "."
    return type(name, (collections.namedtuple(name, kind._fields + OBJECT_FIELDS),), dict(absent, __slots__=(), __doc__=doc))


def _read(step, base, values, layout, v, per_slot=lambda t: t):
    """read()'s result: `values` + fresh copies of the images and the sides the step has, as the step's read type."""
    if layout.overlay:
        values += (v.overlay.clone(),)
    if layout.labels:
        values += (v.box_label.clone(), per_slot(v.pose_label).clone())
    if layout.handed:
        values += (per_slot(v.side).clone(),)
    key = (layout.overlay, layout.labels, layout.handed)
    if layout.tracked:
        values += (per_slot(v.track_age).clone(), per_slot(v.track_id).clone())
        key += (True,)
        if layout.smoothed:
            values += (per_slot(v.smooth_xyz).clone(), per_slot(v.smooth_mesh).clone())
            key += (True,)
    if layout.occluded:
        values += (v.silhouette.clone(), per_slot(v.coverage).clone())
        key = key + (False,) * (5 - len(key)) + (True,)
    if layout.rig:      # (per slot [N,K,...]; per rig hand [N*K,...]; the count as a Python int)
        values += (per_slot(v.rig_xyz).clone(), per_slot(v.rig_mesh).clone(), per_slot(v.rig_hand).clone(), int(v.rig_count[0]),
                   v.rig_views.clone(), v.rig_seed.clone(), v.fused_xyz.clone(), v.fused_mesh.clone())
        key = key + (False,) * (6 - len(key)) + (True,)
    if layout.cloud:    # (per slot: [N,K,P,3], [N,K,2], [N,K]; the one-hand step: [N,P,3], [N,2], [N])
        values += (per_slot(v.cloud).clone(), per_slot(v.cloud_count).clone(), per_slot(v.cloud_resid).clone())
        key = key + (False,) * (7 - len(key)) + (True,)
    kind = _read_type(step, base, *key)
    if layout.fit:      # (per slot: [N,K,V,3], [N,K,21,3], [N,K,12], [N,K,2], [N,K]; the one-hand step without the K)
        values += tuple(per_slot(getattr(v, f)).clone() for f in FIT_FIELDS)
        kind = _fit_read_type(kind)
        if layout.fit_iters > 1:      # (per slot: [N,K,I,3]; the one-hand step: [N,I,3])
            values += (per_slot(v.fit_trace).clone(),)
            kind = _fit_trace_read_type(kind)
    if layout.objects:  # (per slot: [N,K], [N,K], [N,K,4], [N,K], [N,K,2], [N,K,3], [N,K,6], [N,K,2])
        values += tuple(per_slot(getattr(v, f)).clone() for f in OBJECT_FIELDS)
        kind = _objects_read_type(kind)
    return kind(*values)


_LIVE_FIELDS = ("keypoints", "has_hand", "crop_box", "words", "more", "mesh")      # the six a plain step always had
LiveRead, LiveOverlayRead, LiveLabelsRead, LiveOverlayLabelsRead = (
    _read_type("Live", _LIVE_FIELDS, overlay, labels, False) for labels in (False, True) for overlay in (False, True))


@dataclass
class LiveOutput:
    hand: HandNetOutput          # the step's detector / pose results (image_uvd and xyz_mm included), on the device
    pose2d: torch.Tensor         # [N,21,2] the lifter's standardised input
    mesh: torch.Tensor           # [N,V0,3] Pose2Mesh vertices (finest level of the graph hierarchy, coarsening order), or --
    #                              with perm_reverse -- [N,V,3] = out['mesh'] of ros_demo.py:337 (camera frame, original order)
    pose3d: torch.Tensor         # [N,21,3] PoseNet's lifted joints (millimetre scale of the lifter's training set)
    host: torch.Tensor           # pinned uint8 (`layout`): (N + 1) wide records, the mesh as fp32, the images -- ONE copy,
    #                              enqueued by the step
    n: int = 0
    raw_mesh: torch.Tensor = None   # [N,V0,3] the lifter's own output on the device (= mesh without perm_reverse)
    overlay: torch.Tensor = None    # [N,H,W,3] uint8 RGB on the device: the mesh drawn over the frame (engines with faces=)
    box_label: torch.Tensor = None  # [N,H,W,3] uint8 RGB on the device: the frame with the hand's crop box (engines with labels)
    pose_label: torch.Tensor = None  # [N,176,176,3] uint8 RGB on the device: the colour crop with the skeleton (zeros: no hand)
    layout: LiveLayout = None        # where everything lies in `host`
    silhouette: torch.Tensor = None  # occluded steps: [N,H,W] uint8 on the device (0 no mesh, 1 shown, 0x81 hidden)
    coverage: torch.Tensor = None    # occluded steps: [N,2] int32 on the device (pixels under the mesh, of those shown)
    cloud: torch.Tensor = None       # cloud steps, on the device: [N,P,3] fp32 the hand's measured depth points, metres
    cloud_count: torch.Tensor = None  # [N,2] int32 (matching pixels, rows written)
    cloud_resid: torch.Tensor = None  # [N] int64 the summed residual depth - mesh Z over all matching pixels, micrometres
    mesh_depth: torch.Tensor = None  # [N,H,W] fp32 the nearest mesh Z per pixel (0: no mesh); the engine's buffer, not in the copy
    fit_mesh: torch.Tensor = None    # fit steps, on the device: [N,V,3] fp32 the mesh fitted to the measured depth
    fit_xyz: torch.Tensor = None     # [N,21,3] fp32 the joints moved with it, camera millimetres
    fit_rt: torch.Tensor = None      # [N,12] fp32 R row-major, then t (metres): the motion about the root joint, camera frame
    fit_count: torch.Tensor = None   # [N,2] int32 (matching pixels, status: 0 fitted, 1 too few, 2 no solution, 3 beyond the caps)
    fit_cost: torch.Tensor = None    # [N] int64 the summed squared residual along the normals, 2^-30 m^2
    fit_trace: torch.Tensor = None   # fit steps of I >= 2 iterations: [N,I,3] int64 (matches, status, cost) of each

    def read(self):
        """After the stream is synchronised: (keypoints, has_hand, crop_box, range words, [image_uvd, xyz_mm], mesh) as fresh CPU
        tensors (LiveRead; `.overlay`, `.box_label`, `.pose_label` are None).  A step with faces= appends the overlay [N,H,W,3]
        uint8 (LiveOverlayRead); a step with labels appends box_label [N,H,W,3] and pose_label [N,176,176,3] (LiveLabelsRead,
        LiveOverlayLabelsRead); a step with occlude appends silhouette [N,H,W] uint8 and coverage [N,2] int32; a step with
        cloud appends cloud [N,P,3] fp32, cloud_count [N,2] int32 and cloud_resid [N] int64; a step with fit appends fit_mesh
        [N,V,3], fit_xyz [N,21,3], fit_rt [N,12] fp32, fit_count [N,2] int32 and fit_cost [N] int64 as the last fields, and --
        fit_iters >= 2 -- fit_trace [N,I,3] int64 behind them."""
        v = self.layout.views(self.host)
        kp, has, box, words, more = read_host_record(v.records, self.layout.frames, extras=True)
        return _read("Live", _LIVE_FIELDS, (kp, has, box, words, more, v.mesh.clone()), self.layout, v)


class _LiveStep:
    """The live step, for one hand per frame or K: the engines, the caller's conversion, the final-mesh permutation, the layout
    and the output buffers of a batch size, the step itself (forward_device), the camera feed (forward_raw) and the capture
    (graphed).  A subclass says which step of the hand engine runs (_hand_step), how the lifter's input is gated
    (_lifter_input), how the mesh is finished (_mesh) and what the step hands out (_output)."""
    hands = None                 # K of the K-hand step
    handed = False
    track = None                 # the tracked K-hand step: (track_iou, track_hold)
    smooth = None                # the smoothed K-hand step: (min_cutoff, beta, d_cutoff)
    rig = None                   # the rig K-hand step: its radius (metres); `extrinsics` is the device table [N,12]
    extrinsics = None
    cloud_frame = "camera"       # the frame of a cloud step's points ("rig": a K-hand step's with extrinsics)
    objects = None               # the objects K-hand step: (band, stride, min_points)

    def __init__(self, hand: HandNetEngine, lifter: Pose2MeshEngine, paras, clamp: bool = True, perm_reverse=None, faces=None,
                 labels: bool = False, left: bool = False, occlude: bool = False, occlude_margin: float = ops.OCCLUDE_MARGIN,
                 fit_iters: int = 1, fit_draw: bool = False, cloud: bool = False, cloud_points: int = ops.CLOUD_POINTS,
                 cloud_band: float = ops.CLOUD_BAND, cloud_stride: int = ops.CLOUD_STRIDE, fit: bool = False, fit_band: float = ops.FIT_BAND,
                 fit_stride: int = ops.FIT_STRIDE, fit_min_points: int = ops.FIT_MIN_POINTS, fit_damp: float = ops.FIT_DAMP,
                 fit_max_shift: float = ops.FIT_MAX_SHIFT, fit_max_angle: float = ops.FIT_MAX_ANGLE):
        if not _same_device(hand.device, lifter.device):
            raise ValueError(f"HandNet on {hand.device} but the lifter on {lifter.device}")
        self.hand, self.lifter, self.device = hand, lifter, hand.device
        hand.set_convert(paras=paras, clamp=clamp)
        self.perm, self.vertices = _final_mesh_perm(perm_reverse, lifter, self.device)
        # faces: the mesh's triangles (mesh_model.face) -- given, the step ends with the overlay (ops.mesh_render: the caller's
        # render(), ros_demo.py:86-116) and the image rides behind the mesh in the step's one copy
        # paras: one camera for every frame, or a camera per frame [N,4] -- then the engine keeps the rows in
        # device tables that its kernels read, so set_cameras() changes them under captured steps: this one, a row per frame,
        # for the raster; the hand engine's, a row per slot, for the conversion
        paras = ops.camera_paras(paras)
        self.faces, self.paras, self.cams = None, paras, None
        if isinstance(paras, np.ndarray):
            # (kept by this engine: its captured steps hold the tables' addresses, whatever the hand engine is told later)
            self._cameras = hand._convert["cams"]
            with ops.on_device(self.device):
                self.paras, self.cams = None, self._cameras.rows(1)
        if faces is not None:
            if self.perm is None:
                raise ValueError("faces= needs perm_reverse=: the overlay projects out['mesh'] (camera frame, the real mesh's "
                                 "vertex order); the lifter's raw output has no camera offset to project")
            with ops.on_device(self.device):
                self.faces = ops.mesh_faces(faces, self.vertices, self.device)
        # occlude: the overlay leaves out what lies behind the step's own depth map by more than the margin, and the step also
        # hands out which pixels belong to which hand (silhouette) and how much of each mesh the camera sees (coverage)
        self.occlude = None
        if occlude:
            if faces is None or self.perm is None:
                raise ValueError("occlude=True needs faces= (and therefore perm_reverse=): it is the overlay that is tested "
                                 "against the depth map")
            self.occlude = ops.check_occlude_margin(occlude_margin)
        # cloud: the step also cuts every hand's measured depth pixels out of its depth map (ops.hand_cloud: the pixels of the
        # hand's silhouette within cloud_band of the mesh, back-projected) -- (points, band, stride), or None
        self.cloud = None
        if cloud:
            if self.occlude is None:
                raise ValueError("cloud=True needs occlude=True (and therefore faces= and perm_reverse=): the clouds are cut out "
                                 "with the silhouette")
            self.cloud = ops.check_cloud(cloud_points, cloud_band, cloud_stride)
        # fit: the step also fits every hand's mesh and joints to the depth pixels under its silhouette (ops.mesh_fit: one
        # Gauss-Newton step of point-to-plane alignment) -- (band, stride, min_points, damp, max_shift, max_angle), or None
        self.fit = None
        if fit:
            if self.occlude is None:
                raise ValueError("fit=True needs occlude=True (and therefore faces= and perm_reverse=): the mesh is fitted to the "
                                 "depth pixels under its silhouette")
            self.fit = ops.check_fit(fit_band, fit_stride, fit_min_points, fit_damp, fit_max_shift, fit_max_angle)
        # fit_iters: that many Gauss-Newton steps, the moved mesh drawn again (ops.mesh_geometry) before every further one
        # (ops.mesh_fit_iters); fit_draw: overlay, silhouette, coverage, mesh depth and cloud from the FITTED mesh
        if not isinstance(fit_draw, (bool, np.bool_)):
            raise ValueError(f"fit_draw: True or False (got {fit_draw!r})")
        if not fit and (fit_draw or not (isinstance(fit_iters, (int, np.integer)) and not isinstance(fit_iters, bool)
                                         and fit_iters == 1)):
            raise ValueError("fit_iters / fit_draw need fit=True: they say how the fit runs and what is drawn from it")
        self.fit_iters, self.fit_draw = ops.check_fit_iters(fit_iters), bool(fit_draw)
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

    @property
    def _camera(self):
        """what the depth passes take as paras: the device table (row i for the k slots of frame i) of an engine built with a
        camera per frame, else the one camera's four values"""
        return self.paras if self.cams is None else self.cams

    def _raster_scratch(self, s):
        """the raster's scratch records of a step with s slots, allocated once"""
        scratch = self._render_scratch.get(s)
        if scratch is None:
            with torch.inference_mode(False):
                scratch = self._render_scratch[s] = torch.empty(
                    (ops.mesh_render_scratch_bytes(s, self.faces.shape[0]),), dtype=torch.uint8, device=self.device)
        return scratch

    def _draw(self, mesh, lifted, frames, k, out, depth=None, at=None, mesh_depth=None):
        paras, scratch = self._camera, self._raster_scratch(mesh.shape[0])
        if self.occlude is None:
            return ops.mesh_render(mesh, self.faces, paras, frames, lifted=lifted, k=k, out=out, scratch=scratch), None, None
        # (the depth map the step itself ran on: mirrored in a `left` step, channel 3 of an RGBD step's tensor)
        return ops.mesh_render(mesh, self.faces, paras, frames, lifted=lifted, k=k, out=out, scratch=scratch, depth_out=mesh_depth,
                               scene_depth=depth, margin=self.occlude, silhouette_out=at.silhouette, coverage_out=at.coverage)

    def _cloud(self, work, silhouette, depth, k, at):
        """The cloud step's last two launches: the clouds of the slots from the raster's nearest Z, the silhouette and the
        depth map, camera table and extrinsics table the step itself used, straight into the copy buffer."""
        points, band, stride = self.cloud
        return ops.hand_cloud(work.mesh_depth, silhouette, depth, self._camera, k, points=points, band=band, stride=stride,
                              extrinsics_table=self.extrinsics if self.cloud_frame == "rig" else None, out=at, scratch=work.cloud_scratch)

    def _fit(self, work, silhouette, depth, mesh, xyz_mm, k, at):
        """The fit step's last two launches: every slot's mesh and joints moved onto the depth pixels under its silhouette,
        from the raster's nearest Z, the silhouette, and the depth map, camera table, mesh and joints the step itself used,
        straight into the copy buffer."""
        band, stride, min_points, damp, max_shift, max_angle = self.fit
        mesh, xyz_mm = mesh.view(-1, self.vertices, 3), xyz_mm.view(-1, SMOOTH_JOINTS, 3)      # (a row per slot)
        return ops.mesh_fit(work.mesh_depth, silhouette, depth, self._camera, mesh, xyz_mm, k, band=band, stride=stride, min_points=min_points,
                            damp=damp, max_shift=max_shift, max_angle=max_angle, out=at, scratch=work.fit_scratch)

    def _fit_iters(self, work, best, who, depth, mesh, xyz_mm, drawn, k, at):
        """The iterated fit's launches (ops.mesh_fit_iters): fit_iters steps from the mesh depth `best` and the slot byte `who`
        that show `mesh`, the moved meshes drawn again into work buffers of their own before every further step; the results
        and the trace straight into the copy buffer."""
        band, stride, min_points, damp, max_shift, max_angle = self.fit
        mesh, xyz_mm = mesh.view(-1, self.vertices, 3), xyz_mm.view(-1, SMOOTH_JOINTS, 3)      # (a row per slot)
        return ops.mesh_fit_iters(best, who, depth, self._camera, mesh, xyz_mm, self.faces, k, iters=self.fit_iters, lifted=drawn, band=band,
                                  stride=stride, min_points=min_points, damp=damp, max_shift=max_shift, max_angle=max_angle, out=at,
                                  scratch=work.fit_scratch, work=work.fit_work)

    def _geometry(self, work, mesh, drawn, k):
        """A fit_draw step's first two launches, in place of the raster: the nearest Z and the slot byte of the unfitted mesh,
        into work buffers of their own -- what the fit reads."""
        return ops.mesh_geometry(mesh, self.faces, self._camera, tuple(work.geo_depth.shape[1:]), lifted=drawn, k=k,
                                 out_depth=work.geo_depth, out_who=work.geo_who, scratch=self._raster_scratch(mesh.shape[0]))

    def _check_frames(self, n):
        if self.cams is not None and n != self.cams.shape[0]:
            raise ValueError(f"a step over {n} frames, but the engine was built with {self.cams.shape[0]} cameras, one per frame")
        if self.extrinsics is not None and n != self.extrinsics.shape[0]:
            raise ValueError(f"a step over {n} frames, but the engine was built with {self.extrinsics.shape[0]} extrinsics, one "
                             "per frame")

    @ops.device_guarded
    def set_cameras(self, paras):
        """New intrinsics for an engine built with a camera per frame (paras [N,4]; same N): the values are copied into the
        engine's device tables on the current stream, and eager steps and every already captured step use them from the next
        step on -- the kernels read the tables, so nothing is recaptured.  An engine built with one camera raises ValueError:
        its four values are kernel arguments."""
        if self.cams is None:
            raise ValueError("set_cameras needs an engine built with a camera per frame: paras [N,4]")
        self._cameras.update(paras)      # (the raster's table, a row per frame, and the conversion's, a row per slot)
        return self

    @ops.device_guarded
    def set_extrinsics(self, extrinsics):
        """New camera -> rig extrinsics for an engine built with extrinsics= ([N,3,4] or [N,4,4]; same N, checked like the
        constructor's): the values are copied into the engine's device table on the current stream, and eager steps and every
        already captured step use them from the next step on -- the kernels read the table, so nothing is recaptured.  An engine
        built without extrinsics raises ValueError."""
        if self.extrinsics is None:
            raise ValueError("set_extrinsics needs an engine built with extrinsics=: one [R | t] per frame")
        self.extrinsics.copy_(torch.from_numpy(ops.rig_extrinsics(extrinsics, self.extrinsics.shape[0])))
        return self

    def _layout(self, n, hw=None) -> LiveLayout:
        """The buffer of a step over n frames (hw: of a step that draws, the frames' size)."""
        return (LiveLayout if self.objects is None else LiveObjectsLayout)(
                          n, self.hands, self.vertices, hw, hw is not None and self.faces is not None,
                          hw is not None and self.labels, self.handed, self.track is not None, self.smooth is not None,
                          occluded=self.occlude is not None,
                          fit=(True if self.fit_iters == 1 else self.fit_iters) if self.fit is not None and hw is not None else False,
                          cloud=self.cloud[0] if self.cloud and hw is not None else 0, rig=self.rig is not None)

    def _new_buffers(self, n, hw=None):
        """A fresh (layout, device buffer, pinned host buffer, work) of a step over n frames; work: a cloud or fit step's
        StepWork on the device -- not part of the copy --, else None."""
        layout = self._layout(n, hw)
        work = None
        if layout.cloud or layout.fit:
            scratch = lambda nbytes: torch.empty((nbytes,), dtype=torch.uint8, device=self.device)  # noqa: E731
            work = StepWork(torch.zeros((n, *hw), dtype=torch.float32, device=self.device),
                        scratch(ops.hand_cloud_scratch_bytes(n, self.hands or 1, hw[0])) if layout.cloud else None,
                        scratch(ops.mesh_fit_scratch_bytes(n, self.hands or 1, hw[0])) if layout.fit else None,
                        scratch(ops.mesh_fit_iters_scratch_bytes(n, self.hands or 1, hw[0], hw[1], self.vertices, self.faces.shape[0],
                                                                 SMOOTH_JOINTS, self.fit_iters)) if layout.fit_iters > 1 else None,
                        torch.zeros((n, *hw), dtype=torch.float32, device=self.device) if layout.fit and self.fit_draw else None,
                        torch.zeros((n, *hw), dtype=torch.uint8, device=self.device) if layout.fit and self.fit_draw else None)
        return (layout, torch.zeros((layout.nbytes,), dtype=torch.uint8, device=self.device),
                torch.zeros((layout.nbytes,), dtype=torch.uint8, pin_memory=True), work)

    def _out_buffers(self, n, hw=None):
        b = self._buffers.get((n, hw))
        if b is None:
            with torch.inference_mode(False):
                b = self._buffers[(n, hw)] = self._new_buffers(n, hw)
        return b

    @ops.device_guarded
    def forward_device(self, images, depth, _buffers=None, _mirror=None):
        """images [N,3,H,W] 0..1 (or a list), depth [N,1,H,W] metres on the GPU -> the step's output (no sync).
        (_mirror: a `left` capture's own mirrored-input buffers; False: the inputs are mirrored already.)"""
        n = len(images)
        self._check_frames(n)
        if self.left and _mirror is not False:
            images, depth = self._mirror_inputs(images, depth, _mirror)
        frames = self._frames(images)
        layout, dev, host, work = _buffers if _buffers is not None else self._out_buffers(n, self._hw(frames))
        at = layout.views(dev)

        def lift(_kp, image_uvd, xyz, has_hand, mirror=None):
            # (inside the step's range scope: the lifter's split producers note into the step's flag words, which the step's one
            # collect launch hands over -- an overflowing activation of the lifter raises like one of the pose network;
            # mirror: the handed step's per-slot flags)
            p2d = self._lifter_input(image_uvd, has_hand, at.lifted, mirror)
            return (p2d,) + self._mesh(p2d, xyz, has_hand, at, mirror)
        # the step packs its wide records and its range words straight into the buffer; ONE copy moves records, mesh and images
        out = self._hand_step(images, depth, at, lift)
        p2d, mesh, pose3d, raw = out.tail
        drawn, k = out.has_hand.view(-1) if self.hands is None else at.lifted, self.hands or 1
        overlay = box_label = pose_label = silhouette = coverage = None
        shown = at.smooth_mesh if layout.smoothed else mesh      # (a smoothed step draws, tests and fits what it smoothed)
        more, redraw = {}, bool(layout.fit and self.fit_draw)
        if redraw:      # (the geometry of the unfitted mesh, the fit, then everything drawn from the fitted mesh)
            best, who = self._geometry(work, shown, drawn, k)
            more.update(self._fit_parts(work, best, who, depth, shown, at.smooth_xyz if layout.smoothed else out.xyz_mm, drawn, k,
                                        at, layout))
            overlay, silhouette, coverage = self._draw(at.fit_mesh, drawn, frames, k, at.overlay, depth, at, work.mesh_depth)
        elif layout.overlay:
            overlay, silhouette, coverage = self._draw(shown, drawn, frames, k, at.overlay, depth, at, work and work.mesh_depth)
        if layout.labels:
            box_label, pose_label = ops.draw_labels(out.keypoints, out.crop_box, frames, drawn=drawn, k=k, clamp=self.clamp,
                                                    out_box=at.box_label, out_pose=at.pose_label)
        if coverage is not None:
            more.update(silhouette=silhouette, coverage=coverage)
        if layout.rig:      # (a smoothed step moves and fuses what it smoothed, the signals its overlay draws)
            more["rig"] = ops.rig_fuse(at.smooth_xyz if layout.smoothed else out.xyz_mm, at.smooth_mesh if layout.smoothed else mesh,
                                       out.has_hand, at.lifted, out.score, self.extrinsics, k, self.rig,
                                       side=out.side if self.handed else None, out=at)
        if layout.cloud:    # (against the mesh the overlay drew and the depth map it was tested against)
            cloud = self._cloud(work, silhouette, depth, k, at)
            more.update(cloud=cloud.cloud, cloud_count=cloud.count, cloud_resid=cloud.resid, mesh_depth=work.mesh_depth)
        if layout.fit and not redraw:      # (the mesh the overlay drew and the joints that go with it)
            more.update(self._fit_parts(work, work.mesh_depth, silhouette, depth, shown, at.smooth_xyz if layout.smoothed else out.xyz_mm,
                                        drawn, k, at, layout))
        if layout.objects:  # (against the depth map the step ran on -- mirrored in a `left` step -- and the unsmoothed root joint)
            band, stride, min_points = self.objects
            held = ops.hand_objects(out.detections, out.contacts, out.dxdymags, out.det_index.view(n, k), depth.float().contiguous(), out.xyz_mm,
                                    self._camera, k, band=band, stride=stride, min_points=min_points, silhouette=silhouette, out=at)
            if layout.labels:
                ops.draw_object_labels(out.detections, out.det_index.view(n, k), held.object_index, box_label)
            more.update({f: getattr(held, f) for f in OBJECT_FIELDS})
        host.copy_(dev, non_blocking=True)
        return self._output(out, at, layout, host, dict(pose2d=p2d, mesh=mesh, pose3d=pose3d, raw_mesh=raw, overlay=overlay,
                                                        box_label=box_label, pose_label=pose_label, **more))

    def _fit_parts(self, work, best, who, depth, mesh, xyz_mm, drawn, k, at, layout) -> dict:
        """The fit's launches -- one iteration: ops.mesh_fit, today's two; more: ops.mesh_fit_iters -- on the mesh depth `best` and
        the slot byte `who`, and what the step hands out of them."""
        if layout.fit_iters == 1:
            fit = self._fit(work._replace(mesh_depth=best), who, depth, mesh, xyz_mm, k, at)
            trace = {}
        else:
            fit = self._fit_iters(work, best, who, depth, mesh, xyz_mm, drawn, k, at)
            trace = dict(fit_trace=fit.trace)
        return dict(fit_mesh=fit.mesh, fit_xyz=fit.xyz, fit_rt=fit.rt, fit_count=fit.count, fit_cost=fit.cost, mesh_depth=work.mesh_depth,
                    **trace)

    def _key_options(self) -> tuple:
        """What a capture's key carries behind the shapes (the smoothed step: its filter's parameters; the occluded step: its
        margin -- kernel arguments)."""
        return ((() if self.occlude is None else ("occluded", self.occlude))
                + (() if self.cloud is None else ("cloud",) + self.cloud + (self.cloud_frame,))
                + (() if self.fit is None else ("fit",) + self.fit)
                + (() if self.fit_iters == 1 and not self.fit_draw else ("fit_iters", self.fit_iters, self.fit_draw))
                + (() if self.rig is None else ("rig", self.rig))
                + (() if self.objects is None else ("objects",) + self.objects))

    def _smooth_untouched(self, n):
        return contextlib.nullcontext()

    @ops.device_guarded
    def forward_raw(self, bgr_u8, depth_raw) -> LiveOutput:
        """The camera's buffers in, the mesh out: bgr_u8 uint8 [N,H,W,3] (cv_bridge 'bgr8'), depth_raw [N,H,W] uint16 millimetres
        (16UC1) or float32 metres (32FC1), on the GPU or on the host (pinned: read in place; pageable: staged) -- ONE ingest
        kernel writes the captured step's input buffers (ros_demo.py:227-231,266-269) and the live step replays (captured at
        the first call with these shapes).  Returns the capture's static LiveOutput (overwritten by the next call); no sync."""
        staged = []
        bgr, dep = self.hand._device_readable(bgr_u8, staged), self.hand._device_readable(depth_raw, staged)
        n, h, w, _ = bgr.shape
        self._check_frames(n)
        # (a `left` step: the ingest kernel mirrors while it converts, so this capture -- keyed apart from graphed()'s -- takes
        # its inputs as already mirrored and holds no mirror launch)
        key = ((n, 3, h, w), (n, 1, h, w)) + (("mirrored",) if self.left else ()) + self._key_options()
        if key not in self._graphs:
            rgb, d1, _ = ops.ingest_raw(bgr, dep, device=self.device, flip_w=self.left)
            self.graphed(rgb, d1, _mirrored=self.left)
        return self.hand._ingest_replay(self._graphs[key], bgr, dep, staged, flip_w=self.left)

    @ops.device_guarded
    def graphed(self, images: torch.Tensor, depth: torch.Tensor, _mirrored: bool = False):
        """(run, static images, static depth, static LiveOutput): copy new frames into the static inputs and call run().
        (A `left` step: the captured step mirrors the static inputs itself, one launch.)"""
        key = (tuple(images.shape), tuple(depth.shape)) + (("mirrored",) if _mirrored else ()) + self._key_options()
        hit = self._graphs.get(key)
        if hit is None:
            self._check_frames(images.shape[0])
            with torch.inference_mode(False), torch.no_grad():
                s_img, s_dep = torch.empty_like(images), torch.empty_like(depth)
                s_img.copy_(images)
                s_dep.copy_(depth)
                # the capture's own buffers, never the eager cache's (addresses are baked into the graph)
                bufs = self._new_buffers(images.shape[0], self._hw(self._frames(images)))
                if bufs[3] is not None:      # (a cloud or fit step's scratch: its address is baked into the graph and nothing the step
                    self._mirrored[("cloud work",) + key] = bufs[3]      # hands out refers to it -- owned like the mirrored inputs)
                flipped = None
                if self.left and not _mirrored:
                    # the capture's mirrored inputs: owned by the engine for as long as the capture lives (their addresses are
                    # baked into the graph, and nothing the step hands out refers to them)
                    flipped = self._mirrored[("capture",) + key] = (torch.empty_like(s_img), torch.empty_like(s_dep))
                step = lambda: self.forward_device(s_img, s_dep, _buffers=bufs, _mirror=False if _mirrored else flipped)
                if self.track is not None:      # (the warm-up steps of a capture must not advance the tracker, nor the filters)
                    with self.hand._track_untouched(images.shape[0], self.hands), self._smooth_untouched(images.shape[0]):
                        g, out = ops.capture_step(step)
                else:
                    g, out = ops.capture_step(step)
            hit = self._graphs[key] = (g, s_img, s_dep, out)
        g, s_img, s_dep, out = hit
        return g.replay, s_img, s_dep, out


class LiveHandEngine(_LiveStep):
    """paras = (fx, fy, cx, cy) of the depth camera (ros_demo.py:191-196), or a camera per frame [N,4] (frame i
    of every step is converted and drawn with row i, every other option unchanged; the step takes exactly N frames, and
    set_cameras() changes the values under captured steps); clamp: the caller's clamps before the
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
    ingest kernel (no launch added); fp32 feeds (forward_device / graphed) cost one launch.
    occlude (needs faces): a pixel of the mesh that lies more than occlude_margin metres behind the step's own
    depth map keeps the frame's pixel, and the step also hands out LiveOutput.silhouette / .coverage (read() likewise, as the
    last fields): silhouette [N,H,W] uint8 -- 0 no mesh, 1 mesh shown, 0x81 mesh hidden --, coverage [N,2] int32 -- pixels
    under the mesh, and of those the shown ones.  Holes of the depth map (0, NaN) hide nothing.  The default margin of 0.03 m
    is a starting value, NOT tuned on this model: a hand is 2-3 cm thick and the mesh's absolute Z hangs on the wrist key
    point's single depth reading.
    cloud (needs occlude): the step ends with two more launches (ops.hand_cloud) that cut the hand's measured
    depth pixels out of the step's own depth map -- the candidates (every cloud_stride-th row and column) under the mesh's
    silhouette, hidden or not, whose depth D is finite and > 0 and lies within cloud_band metres of the mesh Z drawn there --
    and back-project them: ((c + 0.5 - cx) D / fx, (r + 0.5 - cy) D / fy, D), metres in the frame of xyz_mm (x right, y down,
    z forward), the pixel centre at +0.5.  LiveOutput.cloud [N,P,3] holds the first P = cloud_points matches in row-major
    order (zero rows behind them), .cloud_count [N,2] (matches, rows written), .cloud_resid [N] int64 the summed D - mesh Z over
    all matches in micrometres, read() likewise as the last fields, in the step's one copy; .mesh_depth [N,H,W] is the nearest
    mesh Z per pixel on the device.  cloud_points = 4096, cloud_band = 0.03 m and cloud_stride = 2 are starting values, NOT
    tuned on this model.
    fit (needs occlude): the step ends with two more launches (ops.mesh_fit) that fit the hand's mesh to its
    measured depth -- ONE Gauss-Newton step of projective point-to-plane alignment over the candidates (every fit_stride-th
    row and column) under the mesh's silhouette whose depth is valid and within fit_band metres of the mesh Z drawn there,
    damped by fit_damp per match -- and move the mesh and the joints by the rigid motion found: LiveOutput.fit_mesh [N,V,3],
    .fit_xyz [N,21,3] (camera millimetres), .fit_rt [N,12] (R row-major, then t in metres: x' = R (x - c0) + c0 + t about the
    root joint c0, camera frame), .fit_count [N,2] (matches, status: 0 fitted; 1 fewer than fit_min_points matches; 2 no
    solution; 3 a step beyond fit_max_shift metres or fit_max_angle radians -- then R = I, t = 0 and fit_mesh / fit_xyz are
    byte copies) and .fit_cost [N] int64 (the summed squared residual, 2^-30 m^2), read() likewise as the last fields, in the
    step's one copy.  The overlay, the silhouette and the cloud are NOT redrawn from the fitted mesh (fit_draw=True does that).
    fit_iters = I (1..8) runs I such steps, the moved mesh drawn again before every further one by a raster pass
    that keeps only the nearest Z and the slot (ops.mesh_fit_iters: 4 (I - 1) + 1 more launches): fit_mesh / fit_xyz are the
    state after the last step, fit_rt the composed motion about the original root joint, fit_count / fit_cost those of the
    first step, and -- I >= 2 -- .fit_trace [N,I,3] int64 holds (matches, status, cost) of every step, behind fit_cost in
    read().  fit_draw=True draws the overlay, the silhouette, the coverage and mesh_depth, and cuts the cloud, from fit_mesh:
    the geometry pass of the unfitted mesh runs in place of the first raster, then the fit, then the step's occluded raster
    of fit_mesh; the fit_* fields are the same bytes with it on or off.  Either one without fit=True: ValueError.  fit_band = 0.03 m,
    fit_stride = 2, fit_min_points = 200, fit_damp = 1e-3, fit_max_shift = 0.05 m and fit_max_angle = 0.35 rad are starting
    values, NOT tuned on this model."""

    def _hand_step(self, images, depth, at, lift):
        return self.hand.forward_device(images, depth, _record=(None, at.records), _tail=lift)

    def _lifter_input(self, image_uvd, has_hand, _lifted, _mirror):
        return ops.joints2d_standardize(image_uvd, valid=has_hand)

    def _mesh(self, p2d, xyz, has_hand, at, _mirror):
        if self.perm is None:
            mesh, pose3d = self.lifter.forward(p2d, mesh_out=at.mesh)               # the last layer writes into the copy buffer
            return mesh, pose3d, mesh
        raw, pose3d = self.lifter.forward(p2d)
        return ops.mesh_finish(raw, self.perm, xyz, valid=has_hand, out=at.mesh), pose3d, raw

    def _output(self, out, at, layout, host, parts) -> LiveOutput:
        return LiveOutput(hand=out, host=host, n=layout.frames, layout=layout, **parts)


_HANDS_FIELDS = ("keypoints", "has_hand", "crop_box", "score", "det_index", "image_uvd", "xyz_mm", "lifted", "mesh", "words")
LiveHandsRead, LiveHandsOverlayRead, LiveHandsLabelsRead, LiveHandsOverlayLabelsRead = (       # (plain: the ten it always had)
    _read_type("LiveHands", _HANDS_FIELDS, overlay, labels, False) for labels in (False, True) for overlay in (False, True))
# ... and of a handed step: the same fields + `side` [N,K] int32 (the detector's side of the slot's detection, -1: empty slot)


@dataclass
class LiveHandsOutput:
    hands: HandsOutput           # the step's forward_hands results (image_uvd and xyz_mm included), on the device
    pose2d: torch.Tensor         # [N*K,21,2] the lifter's input; zero rows where not lifted
    lifted: torch.Tensor         # [N,K] int32: 1 where the slot's hand went through the lifter (the caller's skip rule)
    mesh: torch.Tensor           # [N,K,V,3] as LiveOutput.mesh, per slot; zero rows where not lifted
    pose3d: torch.Tensor         # [N*K,21,3] PoseNet's lifted joints (every row: rows not lifted are the lifter on zeros)
    host: torch.Tensor           # pinned uint8 (`layout`): records, side, lifted, mesh, images -- ONE copy, enqueued by the step
    n: int = 0
    k: int = 0
    raw_mesh: torch.Tensor = None   # [N*K,V0,3] the lifter's own output on the device
    overlay: torch.Tensor = None    # [N,H,W,3] uint8 RGB on the device: all lifted meshes of a frame drawn over it (faces=)
    box_label: torch.Tensor = None  # [N,H,W,3] uint8 RGB on the device: the frame with the crop box of every lifted slot (labels)
    pose_label: torch.Tensor = None  # [N*K,176,176,3] uint8 RGB on the device: per slot, the colour crop with the skeleton
    side: torch.Tensor = None        # handed steps: [N,K] int32 on the device, the detector's side per slot (-1: empty slot)
    mirror: torch.Tensor = None      # handed steps: [N,K] int32 on the device, 1 where the slot ran mirrored (a left hand)
    layout: LiveLayout = None        # where everything lies in `host`
    track_id: torch.Tensor = None    # tracked steps: [N,K] int32 on the device, the slot's track id (held slots included; 0: free)
    track_age: torch.Tensor = None   # tracked steps: [N,K] int32 on the device, the steps on which the slot's track was seen again
    silhouette: torch.Tensor = None  # occluded steps: [N,H,W] uint8 on the device (0 no mesh, k + 1 slot k shown, 0x80 | (k + 1) hidden)
    coverage: torch.Tensor = None    # occluded steps: [N,K,2] int32 on the device (pixels where the slot's mesh is nearest, of those shown)
    rig_xyz: torch.Tensor = None     # rig steps, on the device: [N,K,21,3] the joints in the rig frame, metres
    rig_mesh: torch.Tensor = None    # [N,K,V,3] the mesh in the rig frame, metres (zero rows: not lifted)
    rig_hand: torch.Tensor = None    # [N,K] int32 the slot's rig hand (-1: none)
    rig_count: torch.Tensor = None   # [1] int32 the number of rig hands
    rig_views: torch.Tensor = None   # [N*K] int32 members per rig hand (0 beyond the count)
    rig_seed: torch.Tensor = None    # [N*K] int32 the rig hand's seed slot i * K + k (-1 beyond the count): the way to its track_id
    fused_xyz: torch.Tensor = None   # [N*K,21,3] per rig hand: its members' joints, weighted by their scores
    fused_mesh: torch.Tensor = None  # [N*K,V,3] per rig hand: its members' meshes, weighted by their scores
    cloud: torch.Tensor = None       # cloud steps, on the device: [N,K,P,3] fp32 each slot's measured depth points, metres
    cloud_count: torch.Tensor = None  # [N,K,2] int32 (matching pixels, rows written)
    cloud_resid: torch.Tensor = None  # [N,K] int64 the summed residual depth - mesh Z over all matching pixels, micrometres
    mesh_depth: torch.Tensor = None  # [N,H,W] fp32 the nearest mesh Z per pixel (0: no mesh); the engine's buffer, not in the copy
    fit_mesh: torch.Tensor = None    # fit steps, on the device: [N,K,V,3] fp32 the mesh fitted to the measured depth
    fit_xyz: torch.Tensor = None     # [N,K,21,3] fp32 the joints moved with it, camera millimetres
    fit_rt: torch.Tensor = None      # [N,K,12] fp32 R row-major, then t (metres): the motion about the root joint, camera frame
    fit_count: torch.Tensor = None   # [N,K,2] int32 (matching pixels, status: 0 fitted, 1 too few, 2 no solution, 3 beyond the caps)
    fit_cost: torch.Tensor = None    # [N,K] int64 the summed squared residual along the normals, 2^-30 m^2
    fit_trace: torch.Tensor = None   # fit steps of I >= 2 iterations: [N,K,I,3] int64 (matches, status, cost) of each
    contact: torch.Tensor = None     # objects steps, on the device: [N,K] int32 the slot's contact state (-1: empty slot)
    object_index: torch.Tensor = None  # [N,K] int32 the held object's row in hands.detections, or -1
    object_box: torch.Tensor = None    # [N,K,4] fp32 its box (zeros: no object)
    object_score: torch.Tensor = None  # [N,K] fp32 its score
    object_point: torch.Tensor = None  # [N,K,2] fp32 the point the hand's offset vector names (zeros: empty slot)
    object_xyz: torch.Tensor = None    # [N,K,3] fp32 the centroid of the object's depth pixels, camera frame, metres (zeros unless status 0)
    object_extent: torch.Tensor = None  # [N,K,6] fp32 (min x y z, max x y z) of those pixels (zeros: no match)
    object_count: torch.Tensor = None  # [N,K,2] int32 (matches, status: 0 ok, 1 no object, 2 too few matches, -1 empty slot)
    smooth_xyz: torch.Tensor = None  # smoothed steps: [N,K,21,3] on the device, xyz_mm filtered over time (zeros: has_hand != 1)
    smooth_mesh: torch.Tensor = None  # smoothed steps: [N,K,V,3] on the device, `mesh` filtered over time (zeros: not lifted)

    def read(self) -> LiveHandsRead:
        """After the stream is synchronised: the step's results per frame and slot as fresh CPU tensors (LiveHandsRead;
        lifted as bool, words = the step's range words; a step with faces=: LiveHandsOverlayRead, + overlay [N,H,W,3] uint8; a
        step with labels: + box_label [N,H,W,3], pose_label [N,K,176,176,3] -- LiveHandsLabelsRead, LiveHandsOverlayLabelsRead;
        a handed step: the same with `side` [N,K] int32 behind them; a tracked step: track_age and then track_id [N,K] int32
        as the last fields; a smoothed step: behind those, smooth_xyz [N,K,21,3] and smooth_mesh [N,K,V,3]; an occluded step:
        behind everything else, silhouette [N,H,W] uint8 and coverage [N,K,2] int32; a rig step: behind those, rig_xyz
        [N,K,21,3], rig_mesh [N,K,V,3], rig_hand [N,K] int32, rig_count (a Python int), rig_views and rig_seed [N*K] int32,
        fused_xyz [N*K,21,3] and fused_mesh [N*K,V,3]; a cloud step: behind those, cloud [N,K,P,3] fp32, cloud_count [N,K,2]
        int32 and cloud_resid [N,K] int64; a fit step: behind those, fit_mesh [N,K,V,3], fit_xyz [N,K,21,3], fit_rt [N,K,12]
        fp32, fit_count [N,K,2] int32 and fit_cost [N,K] int64, and -- fit_iters >= 2 -- fit_trace [N,K,I,3] int64; an objects
        step: behind those, contact and object_index [N,K] int32, object_box [N,K,4], object_score [N,K], object_point [N,K,2],
        object_xyz [N,K,3] and object_extent [N,K,6] fp32 and object_count [N,K,2] int32 -- a read type whose name ends in
        ObjectsRead)."""
        v, s = self.layout.views(self.host), self.layout.slots
        per = lambda t: t.reshape((self.layout.frames, self.layout.hands) + tuple(t.shape[1:]))
        kp, has, box, words, (img, xyz) = read_host_record(v.records, s, extras=True)
        score, index = read_hands_tail(v.records, s)
        values = (per(kp), per(has), per(box), per(score), per(index), per(img), per(xyz), per(v.lifted) != 0, per(v.mesh).clone(),
                  words)
        return _read("LiveHands", _HANDS_FIELDS, values, self.layout, v, per)


class LiveHandsEngine(_LiveStep):
    """LiveHandEngine for up to max_hands hands per frame: HandNet's forward_hands step (slot k of frame i = frame i's k-th
    hand detection) -> clamp + convert in the aggregation's epilogue -> the lifter's input WITH the caller's skip rule per
    slot (ros_demo.py:288-300: a hand whose 2D box process_bbox refuses is not lifted; hn_lifter_input_gated_f32) ->
    Pose2Mesh on all N*K rows (dense: rejected rows are zeros, so the step stays capturable and its activations finite) ->
    the final mesh (perm_reverse) -> ONE device -> host copy of records + lifted + mesh (LiveLayout).  Eager steps may run A2J
    on the filled slots only (HandNetEngine.forward_hands); the lifter always runs on all N*K rows."""

    def __init__(self, hand: HandNetEngine, lifter: Pose2MeshEngine, paras, max_hands: int = 2, clamp: bool = True,
                 perm_reverse=None, faces=None, labels: bool = False, left: bool = False, handed: bool = False,
                 left_side: int = 0, track: bool = False, track_iou: float = 0.3, track_hold: int = 5, occlude: bool = False,
                 occlude_margin: float = ops.OCCLUDE_MARGIN, objects: bool = False, object_band: float = ops.OBJECT_BAND,
                 object_stride: int = ops.OBJECT_STRIDE, object_min_points: int = ops.OBJECT_MIN_POINTS, extrinsics=None,
                 rig_radius: float = ops.RIG_RADIUS,
                 fit_iters: int = 1, fit_draw: bool = False, cloud: bool = False, cloud_points: int = ops.CLOUD_POINTS, cloud_band: float = ops.CLOUD_BAND,
                 cloud_stride: int = ops.CLOUD_STRIDE, cloud_frame: str = "camera", fit: bool = False,
                 fit_band: float = ops.FIT_BAND, fit_stride: int = ops.FIT_STRIDE, fit_min_points: int = ops.FIT_MIN_POINTS,
                 fit_damp: float = ops.FIT_DAMP, fit_max_shift: float = ops.FIT_MAX_SHIFT,
                 fit_max_angle: float = ops.FIT_MAX_ANGLE, smooth: bool = False, smooth_min_cutoff: float = 1.0, smooth_beta: float = 0.007, smooth_d_cutoff: float = 1.0,
                 smooth_rate: float = 30.0):
        """paras: as LiveHandEngine's -- with a camera per frame [N,4], all K slots of frame i use row i.
        faces: mesh_model.face ([F,3]; needs perm_reverse) -- given, the step ends with the overlay: every lifted mesh of a
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
        left and handed together: ValueError (a mirrored frame swaps the sides).
        track: the slots are tracked from step to step (HandNetEngine.forward_hands(track=True)): batch row i is
        one camera stream, a hand keeps its slot and its id (LiveHandsOutput.track_id, read().track_id) whatever its score
        rank, and a slot whose hand is missing is held for track_hold steps -- has_hand 0, so not lifted, a zero mesh, nothing
        drawn and a zero pose_label, the path of every empty slot.  max_hands = 1 is the sticky top-1.  The state lives in the
        hand engine, one per (N, K), shared by forward_device, graphed and forward_raw; track_reset() empties it.
        smooth (needs track and perm_reverse): a One Euro filter over time on every coordinate of the slots'
        xyz_mm and final mesh, inside the launch that finishes the mesh -- LiveHandsOutput.smooth_xyz / .smooth_mesh,
        read().smooth_xyz / .smooth_mesh behind track_id; mesh, records and label images stay unfiltered, the overlay (faces=)
        is drawn from smooth_mesh.  A slot's filter restarts when the slot was empty or held, or its track id changed.
        smooth_min_cutoff / smooth_d_cutoff in Hz, smooth_beta per mm/s (the vertices, in metres, use 1000 * smooth_beta),
        smooth_rate = steps per second (dt = 1 / rate; smooth_dt(seconds) sets another dt, also between replays).  The
        defaults are the paper's starting values and have NOT been tuned on this model.  This engine owns one filter state and
        one dt word per (N, K), shared by forward_device, graphed and forward_raw; smooth_reset() -- and track_reset() --
        empties the state.
        occlude (needs faces): as LiveHandEngine's, for all K slots of a frame against the frame's one depth map
        -- silhouette [N,H,W] uint8: 0 no mesh, k + 1 where slot k's mesh is the nearest and shown, 0x80 | (k + 1) where it is
        hidden; coverage [N,K,2] int32: per slot, the pixels where its mesh is the nearest mesh and those of them that are
        shown ((0, 0): not lifted).  A `left` step tests against the mirrored depth map, a `handed` step against the frame's
        own, a smoothed step tests the smoothed mesh it draws.  occlude_margin (metres, default 0.03) is a starting value, NOT
        tuned on this model.
        extrinsics (needs paras and perm_reverse): the rig of a multi-camera step -- one camera -> rig transform
        [R | t] per frame, [N,3,4] or [N,4,4] (p_rig = R p_cam + t, t in metres; checked on the host: finite, last row
        (0, 0, 0, 1), R orthonormal within 1e-4 with det > 0), N * max_hands <= 256.  The step then takes exactly N frames and
        ends with three more launches (ops.rig_fuse) whose results ride in the same copy: every slot's joints and mesh in the
        rig frame (metres, no OpenGL flip: rig_xyz, rig_mesh), the lifted slots of DIFFERENT frames whose centres lie within
        rig_radius metres of each other put into one rig hand (rig_hand, rig_count, rig_views, rig_seed; greedy, at most one
        slot per frame, with handed=True only slots of one side), and per rig hand the members' score-weighted mean (fused_xyz,
        fused_mesh) -- LiveHandsOutput and read() likewise, behind every other field.  A smoothed step moves and fuses
        smooth_xyz / smooth_mesh.  rig_radius = 0.08 m is a starting value, NOT tuned on this model.  left=True: ValueError (a
        mirrored frame is not the camera's frame).  set_extrinsics(new) rewrites the device table under captured steps.
        cloud (needs occlude): the step ends with two more launches (ops.hand_cloud) that cut every slot's
        measured depth pixels out of the step's own depth map -- the candidates (every cloud_stride-th row and column) whose
        silhouette byte names the slot, hidden or not, whose depth D is finite and > 0 and lies within cloud_band metres of
        the mesh Z drawn there -- and back-project them with the frame's camera: ((c + 0.5 - cx) D / fx, (r + 0.5 - cy) D / fy,
        D), metres in the frame of xyz_mm (x right, y down, z forward), the pixel centre at +0.5.  LiveHandsOutput.cloud
        [N,K,P,3] holds each slot's first P = cloud_points matches in row-major order (zero rows behind them), .cloud_count
        [N,K,2] (matches, rows written), .cloud_resid [N,K] int64 the summed D - mesh Z over all matches in micrometres (how
        far the mesh sits from the surface the camera sees), read() likewise behind every other field, in the step's one copy;
        .mesh_depth [N,H,W] is the nearest mesh Z per pixel on the device.  cloud_frame="rig" (needs extrinsics=) hands the
        points out in the rig frame.  A `left` step cuts the mirrored depth map, a smoothed step works against the smoothed
        mesh it draws.  cloud_points = 4096, cloud_band = 0.03 m and cloud_stride = 2 are starting values, NOT tuned on this
        model.
        fit (needs occlude): as LiveHandEngine's, per slot against the frame's one depth map and with the frame's
        camera: LiveHandsOutput.fit_mesh [N,K,V,3], .fit_xyz [N,K,21,3], .fit_rt [N,K,12], .fit_count [N,K,2] (matches, status)
        and .fit_cost [N,K] int64, read() likewise behind every other field, in the step's one copy.  Only pixels whose own and
        whose four neighbours' silhouette bytes name the slot enter, so a slot's border with another hand does not.  A `left`
        step fits to the mirrored depth map, a smoothed step moves the smoothed mesh and joints it draws; the rig outputs, the
        overlay and the cloud stay what they are.  fit_iters / fit_draw: as LiveHandEngine's, .fit_trace
        [N,K,I,3]; every slot that is lifted is drawn again before a further iteration, fitted or not, because it may cover
        another slot's pixels; labels, rig outputs and the smoothing state are not touched.  fit_band = 0.03 m, fit_stride = 2, fit_min_points = 200, fit_damp = 1e-3,
        fit_max_shift = 0.05 m and fit_max_angle = 0.35 rad are starting values, NOT tuned on this model.
        objects (needs paras and a detector with the ext heads): the step also says what every hand holds.  The
        detector pass goes through detect_ext (one more launch) and the step ends with three more launches (ops.hand_objects)
        whose results ride in the same copy, behind every other field: LiveHandsOutput.contact [N,K] int32 (the slot's contact
        state; -1: empty slot), .object_index [N,K] int32 (the held object's row in hands.detections, -1: none), .object_box
        [N,K,4], .object_score [N,K] and .object_point [N,K,2] (the point the hand's offset vector names) -- the association
        of the reference's evaluation (voc_eval.py:687-699) on the detections as they are, without its file round trip --,
        .object_xyz [N,K,3] and .object_extent [N,K,6] (the centroid and the min / max corner, camera frame, metres, of the
        candidates -- every object_stride-th row and column -- inside the object's box whose depth is finite and > 0, lies
        within object_band metres of the depth of the slot's root joint and -- occlude=True -- is under no hand's mesh) and
        .object_count [N,K,2] (matches, status: 0 ok, 1 no object, 2 fewer than object_min_points matches, -1 empty slot);
        read() likewise, a read type whose name ends in ObjectsRead.  labels=True: box_label also carries the object's
        rectangle and the line from the hand box's centre to the object's, in (0, 0, 255) (one more launch); pose_label is
        untouched.  A `left` step works in the mirrored frame; handed, track, smooth, fit, cloud and extrinsics change nothing
        here: the root joint is the unsmoothed xyz_mm's and the object stays in the camera frame.  That a contact state > 0
        means "in contact" (3 / 4: a portable / stationary object) is 100DOH's numbering, which the reference's live code never
        reads: check it against your checkpoint.  object_band = 0.15 m, object_stride = 2 and object_min_points = 50 are
        starting values, NOT tuned on any model."""
        self.hands = self.max_hands = ops.check_max_hands(max_hands)
        if left and handed:
            raise ValueError("left=True mirrors the whole frame and handed=True mirrors the left-hand slots: give one of them")
        self.handed, self.left_side = bool(handed), int(left_side)
        self.track = (float(track_iou), track_hold) if track else None
        if track:
            ops.check_track_options(track_iou, track_hold)
        if smooth:
            if not track:
                raise ValueError("smooth=True needs track=True: the filters follow the slots' track ids")
            if perm_reverse is None:
                raise ValueError("smooth=True needs perm_reverse=: the filter runs in the launch that finishes the mesh")
            mc, beta, dc, rate = ops.check_smooth_options(smooth_min_cutoff, smooth_beta, smooth_d_cutoff, smooth_rate)
            self.smooth, self._dt, self._smooth_states = (mc, beta, dc), 1.0 / rate, {}
        table = None
        if extrinsics is not None:
            if paras is None or perm_reverse is None:
                raise ValueError("extrinsics= needs paras= and perm_reverse=: the rig frame moves xyz_mm and the final mesh "
                                 "(out['mesh']), and a step without them has neither")
            if left:
                raise ValueError("extrinsics= with left=True: a mirrored frame is not the camera's frame (handed=True mirrors per "
                                 "slot and keeps the frame's own coordinates)")
            table = ops.rig_extrinsics(extrinsics)
            ops.check_rig_slots(table.shape[0], self.hands)
            self.rig = ops.check_rig_radius(rig_radius)
        if cloud_frame not in ("camera", "rig"):
            raise ValueError(f'cloud_frame: "camera" or "rig" (got {cloud_frame!r})')
        if cloud_frame == "rig" and extrinsics is None:
            raise ValueError('cloud_frame="rig" needs extrinsics=: the camera -> rig transforms the points go through')
        self.cloud_frame = cloud_frame
        if objects:
            if paras is None:
                raise ValueError("objects=True needs paras=: the object's depth pixels are back-projected with the camera, around "
                                 "the depth of xyz_mm's root joint")
            if not hand.fcos.ext:
                raise ValueError("objects=True needs a detector with the ext heads (contact state and offset vector): build the "
                                 "FCOS engine with ext=True")
            self.objects = ops.check_objects(object_band, object_stride, object_min_points)
        super().__init__(hand, lifter, paras, clamp, perm_reverse, faces, labels, left, occlude, occlude_margin, fit_iters,
                         fit_draw, cloud, cloud_points, cloud_band, cloud_stride, fit, fit_band, fit_stride, fit_min_points, fit_damp,
                         fit_max_shift, fit_max_angle)
        if table is not None:
            if self.cams is not None and self.cams.shape[0] != table.shape[0]:
                raise ValueError(f"{table.shape[0]} extrinsics for a step built with {self.cams.shape[0]} cameras: one [R | t] per "
                                 "frame")
            with ops.on_device(self.device), torch.inference_mode(False):
                self.extrinsics = torch.from_numpy(table).to(self.device)

    def _hand_step(self, images, depth, at, lift):
        # (the per-slot records, range words, scores and ranks go straight into the buffer, the handed step's sides behind them)
        more = {} if self.track is None else dict(track=True, track_iou=self.track[0], track_hold=self.track[1],
                                                  _track_out=(at.track_id, at.track_age))      # (at: LiveTrackedViews)
        return self.hand.forward_hands(images, depth, self.hands, _record=(None, at.records), _tail=lift, handed=self.handed,
                                       left_side=self.left_side, _side=at.side, objects=self.objects is not None, **more)

    def track_reset(self):
        """Empty the hand engine's trackers (HandNetEngine.track_reset; also between replays of a captured step) and, on a
        smoothed engine, the filters."""
        self.hand.track_reset()
        return self.smooth_reset() if self.smooth is not None else self

    def _need_smooth(self):
        if self.smooth is None:
            raise ValueError("this engine does not smooth: build it with smooth=True")

    def _smooth_state(self, n):
        """(filter state, dt word) of the step over n frames: made empty, with the engine's dt, on first use."""
        st = self._smooth_states.get(n)
        if st is None:
            with torch.inference_mode(False):
                st = self._smooth_states[n] = (ops.smooth_state(n * self.hands, SMOOTH_JOINTS, self.vertices, self.device),
                                               torch.full((1,), self._dt, dtype=torch.float32, device=self.device))
        return st

    @ops.device_guarded
    def smooth_reset(self):
        """Empty every filter of this engine: each slot's next value passes unfiltered (a memset on the current stream; also
        between replays of a captured step)."""
        self._need_smooth()
        for state, _dt in self._smooth_states.values():
            state.zero_()
        return self

    @ops.device_guarded
    def smooth_dt(self, seconds):
        """The time between two steps from now on, 0 < seconds < inf (checked here, on the host; the kernel reads the word
        from device memory): filled on the current stream, so a captured step takes it at its next replay."""
        self._need_smooth()
        dt = float(seconds)
        if not (0.0 < dt < math.inf) or not (0.0 < float(np.float32(dt)) < math.inf):
            raise ValueError(f"smooth_dt: 0 < seconds < inf as fp32 (got {seconds!r})")
        self._dt = dt
        for _state, word in self._smooth_states.values():
            word.fill_(dt)
        return self

    def _key_options(self) -> tuple:
        return (() if self.smooth is None else ("smoothed",) + self.smooth) + super()._key_options()

    def _smooth_untouched(self, n):
        """Context manager around the capture of a smoothed step over n frames: the warm-up steps run the filters, so the
        state is put back as it was when the capture is done (HandNetEngine._track_untouched)."""
        if self.smooth is None:
            return contextlib.nullcontext()

        @contextlib.contextmanager
        def keep():
            state = self._smooth_state(n)[0]
            saved = state.clone()
            try:
                yield state
            finally:
                state.copy_(saved)
        return keep()

    def _lifter_input(self, image_uvd, has_hand, lifted, mirror):
        return ops.lifter_input_gated(image_uvd, valid=has_hand, lifted=lifted, mirror=mirror)[0]

    def _mesh(self, p2d, xyz, has_hand, at, mirror):
        raw, pose3d = self.lifter.forward(p2d)
        if self.smooth is not None:      # (ONE launch in place of mesh_finish's: the mesh, and both signals filtered)
            state, dt = self._smooth_state(at.lifted.numel() // self.hands)
            mesh = ops.mesh_finish_smooth(raw, self.perm, xyz, at.lifted, has_hand, at.track_id, dt, state, *self.smooth,
                                          mirror=mirror, out=at.mesh, smooth_xyz=at.smooth_xyz, smooth_mesh=at.smooth_mesh)[0]
        elif mirror is not None:      # (also without perm_reverse: the raw vertices, x negated where mirrored)
            mesh = ops.mesh_finish(raw, self.perm, xyz if self.perm is not None else None, valid=at.lifted, out=at.mesh,
                                   mirror=mirror)
        elif self.perm is None:
            mesh = torch.mul(raw, at.lifted.view(-1, 1, 1), out=at.mesh)       # (x * 1 is x: rows not lifted -> zeros)
        else:
            mesh = ops.mesh_finish(raw, self.perm, xyz, valid=at.lifted, out=at.mesh)
        return mesh, pose3d, raw

    def _output(self, out, at, layout, host, parts) -> LiveHandsOutput:
        n, k = layout.frames, layout.hands
        parts["mesh"] = parts["mesh"].view(n, k, self.vertices, 3)
        if "coverage" in parts:
            parts["coverage"] = parts["coverage"].view(n, k, 2)
        parts.update(parts.pop("rig", ops.RigFused(*(None,) * 8))._asdict())
        if "cloud" in parts:
            parts.update(cloud=parts["cloud"].view(n, k, -1, 3), cloud_count=parts["cloud_count"].view(n, k, 2),
                         cloud_resid=parts["cloud_resid"].view(n, k))
        if "fit_mesh" in parts:
            parts.update(fit_mesh=parts["fit_mesh"].view(n, k, self.vertices, 3), fit_xyz=parts["fit_xyz"].view(n, k, SMOOTH_JOINTS, 3),
                         fit_rt=parts["fit_rt"].view(n, k, 12), fit_count=parts["fit_count"].view(n, k, 2),
                         fit_cost=parts["fit_cost"].view(n, k))
        if "fit_trace" in parts:
            parts["fit_trace"] = parts["fit_trace"].view(n, k, -1, 3)
        if "contact" in parts:
            parts.update({f: parts[f].view((n, k) + tuple(parts[f].shape[1:])) for f in OBJECT_FIELDS})
        return LiveHandsOutput(hands=out, lifted=at.lifted.view(n, k), host=host, n=n, k=k, side=out.side, mirror=out.mirror,
                               layout=layout, track_id=out.track_id, track_age=out.track_age,
                               smooth_xyz=None if self.smooth is None else at.smooth_xyz.view(n, k, SMOOTH_JOINTS, 3),
                               smooth_mesh=None if self.smooth is None else at.smooth_mesh.view(n, k, self.vertices, 3), **parts)


class CropMeshRead(collections.namedtuple("CropMeshRead", "keypoints image_uvd xyz_mm mesh words")):
    """CropMeshOutput.read(): the five items it always returned -- same length, unpacking and equality as that tuple -- and
    `.overlay`: uint8 [K,H,W,3] RGB of a step with faces= and frames, else None."""
    overlay = None

    def __new__(cls, *values, overlay=None):
        self = super().__new__(cls, *values)
        self.overlay = overlay
        return self


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
    overlay: torch.Tensor = None        # [K,H,W,3] uint8 RGB on the device: sample i's mesh over its own image with its own
    #                                     intrinsics (engines with faces=, steps with frames; a2j_mesh.py's demo_mesh_{idx}.png)
    host_overlay: torch.Tensor = None   # its pinned copy, a second copy enqueued behind `host`'s

    def read(self) -> CropMeshRead:
        """After the stream is synchronised: (keypoints, image_uvd, xyz_mm, mesh, range words) as fresh CPU tensors; `.overlay`
        of the result: the images [K,H,W,3] uint8 of a step that drew them, else None."""
        k, j3 = self.k, self.keypoints.shape[1] * 3
        h = self.host
        parts = [h[i * k * j3:(i + 1) * k * j3].reshape(k, -1, 3).clone() for i in range(3)]
        mesh = h[3 * k * j3:-4].reshape(k, -1, 3).clone()
        return CropMeshRead(parts[0], parts[1], parts[2], mesh, h[-4:].view(torch.int32).tolist(),
                            overlay=None if self.host_overlay is None else self.host_overlay.clone())


class CropMeshEngine:
    """The stand-alone mesh demo's loop body (a2j_mesh.py:58-80) as one step on the device: dataset crops -> A2J -> np.clip to
    [0, 176] + convert_joints twice (image uv; camera xyz with the sample's intrinsics -- the dataset's float32 box, fractional
    corners: a2jdataset.py:293) in the aggregation's epilogue -> the lifter's input (predict_mesh, ros_demo.py:148-157) ->
    Pose2Mesh -> the caller's last lines (vertex order, camera offset by the first joint, y / z negated: a2j_mesh.py:77-80) ->
    ONE device -> host copy.  The reference goes to the CPU after A2J, converts in numpy and uploads the normalised joints.
    faces: mesh_model.face ([F,3]; needs perm_reverse) -- given, a step that is handed the samples' full images (frames) ends
    with the loop's last call, render(out, paras, h, w, full_image, face) (a2j_mesh.py): sample i's mesh drawn over frames[i]
    with ITS intrinsics paras[i] (ops.mesh_render with a camera per frame, one slot per frame) ->
    CropMeshOutput.overlay, read().overlay."""

    def __init__(self, a2j, lifter: Pose2MeshEngine, clamp: bool = True, perm_reverse=None, faces=None):
        if not _same_device(a2j.device, lifter.device):
            raise ValueError(f"A2J on {a2j.device} but the lifter on {lifter.device}")
        self.a2j, self.lifter, self.device, self.clamp = a2j, lifter, a2j.device, bool(clamp)
        self.perm, self.vertices = _final_mesh_perm(perm_reverse, lifter, self.device)
        self.faces = None
        if faces is not None:
            if self.perm is None:
                raise ValueError("faces= needs perm_reverse=: the overlay projects out['mesh'] (camera frame, the real mesh's "
                                 "vertex order); the lifter's raw output has no camera offset to project")
            with ops.on_device(self.device):
                self.faces = ops.mesh_faces(faces, self.vertices, self.device)
        self._block = None
        self._graphs = {}
        self._hosts = {}
        self._overlays = {}
        self._render_scratch = {}

    def _new_overlay(self, frames):
        """(device, pinned) overlay buffers of a step over these frames: uint8 [K,H,W,3]"""
        k, (h, w) = frames.shape[0], frames.shape[1:3] if frames.dtype == torch.uint8 else frames.shape[2:]
        return (torch.empty((k, h, w, 3), dtype=torch.uint8, device=self.device),
                torch.zeros((k, h, w, 3), dtype=torch.uint8, pin_memory=True))

    def _check_frames(self, frames, k):
        if frames is None:
            return
        if self.faces is None:
            raise ValueError("frames are what an engine with faces= draws over: build the engine with faces=")
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[0] != k:
            raise ValueError(f"frames: one full image per sample, fp32 [{k},3,H,W] or uint8 [{k},H,W,3]")

    @ops.device_guarded
    def forward_device(self, crops, box_f32, paras, frames=None, _host=None, _overlay=None) -> CropMeshOutput:
        """crops [K,1,176,176] (or [K,4,..] for the RGB-D network), box_f32 [K,4] float32, paras [K,4] float32, on the GPU.
        frames (an engine with faces=): the samples' full images, fp32 [K,3,H,W] in 0..1 or uint8 [K,H,W,3] 'bgr8', on the GPU
        -- the step then ends with the two raster launches and hands out `overlay`."""
        k = crops.shape[0]
        self._check_frames(frames, k)
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
        overlay = host_overlay = None
        if frames is not None:
            frames = frames.contiguous()
            key = (tuple(frames.shape), frames.dtype)
            if _overlay is None:
                _overlay = self._overlays.get(key)
                if _overlay is None:
                    with torch.inference_mode(False):
                        _overlay = self._overlays[key] = self._new_overlay(frames)
            scratch = self._render_scratch.get(k)
            if scratch is None:
                with torch.inference_mode(False):
                    scratch = self._render_scratch[k] = torch.empty(
                        (ops.mesh_render_scratch_bytes(k, self.faces.shape[0]),), dtype=torch.uint8, device=self.device)
            # (the samples' intrinsics are the table: one slot per frame, sample i reads row i)
            overlay = ops.mesh_render(mesh, self.faces, paras, frames, k=1, out=_overlay[0], scratch=scratch)
            host_overlay = _overlay[1]
            host_overlay.copy_(overlay, non_blocking=True)
        return CropMeshOutput(kp, img, xyz, p2d, mesh, pose3d, raw, _host, k, overlay, host_overlay)

    def _new_host(self, k):
        """The pinned buffer of a step over k crops, as forward_device's torch.cat fills it: three [k,J,3] fields (keypoints,
        image_uvd, xyz_mm), the mesh [k,V,3], 4 range words."""
        return torch.zeros((3 * k * self.a2j.joints * 3 + k * self.vertices * 3 + 4,), dtype=torch.float32, pin_memory=True)

    @ops.device_guarded
    def graphed(self, crops, box_f32, paras, frames=None):
        """(run, static crops, static boxes, static intrinsics, static CropMeshOutput): copy a new batch into the static inputs and
        call run() -- every launch of the step and its copy replay from one hipGraph.  With frames (an engine with faces=) the
        captured step draws, and the static frames are a fourth static input: (run, static crops, static boxes, static
        intrinsics, static frames, static CropMeshOutput).  The raster reads the static intrinsics from the device, so new
        values copied into them move the next replay's meshes AND images."""
        self._check_frames(frames, crops.shape[0])
        key = (tuple(crops.shape),) + (() if frames is None else (tuple(frames.shape), frames.dtype))
        hit = self._graphs.get(key)
        if hit is None:
            with torch.inference_mode(False), torch.no_grad():
                inputs = (crops, box_f32, paras) + (() if frames is None else (frames.contiguous(),))
                s = [torch.empty_like(t) for t in inputs]
                for a, b in zip(s, inputs):
                    a.copy_(b)
                host = self._new_host(crops.shape[0])
                overlay = None if frames is None else self._new_overlay(s[3])
                g, out = ops.capture_step(lambda: self.forward_device(*s, _host=host, _overlay=overlay))
            hit = self._graphs[key] = (g, *s, out)
        return (hit[0].replay,) + tuple(hit[1:])
