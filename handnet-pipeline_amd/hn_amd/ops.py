"""Torch-facing wrappers over the C ABI: allocate outputs with torch, launch on the
current HIP stream.  PyTorch is only the allocator / stream provider here.

Every function requires CUDA(HIP) tensors and raises if the extension is unavailable;
there is deliberately no CPU or eager fallback.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, ConvGroup, FcosLevels, check, ptr


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """Raw handle of the current HIP stream.  torch.cuda.current_stream() builds a Stream object through four
    Python layers (40 % of the host time of an eager batch-1 step); the C accessors behind it are used directly."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _check_device(t: torch.Tensor, name="tensor"):
    """Launches go to the CURRENT device's stream: a tensor of another GPU would be a memory fault (or silently
    run on the wrong device under peer access).  The engines enter `on_device(self.device)`; direct callers of
    these wrappers must make the tensor's device current (torch.cuda.device / set_device)."""
    if _cur_device is not None and t.device.index != _cur_device():
        raise RuntimeError(f"{name} lives on cuda:{t.device.index} but the current device is cuda:{_cur_device()}; "
                           "wrap the call in `with torch.cuda.device(tensor.device):`")


class on_device:
    """`with on_device(dev):` -- make `dev` current for the block (no-op, and no torch.cuda.device object, when
    it already is: the hot path stays free of the context-manager cost)."""

    __slots__ = ("idx", "ctx")

    def __init__(self, dev):
        self.idx = torch.device(dev).index
        self.ctx = None

    def __enter__(self):
        if self.idx is not None and (_cur_device is None or _cur_device() != self.idx):
            self.ctx = torch.cuda.device(self.idx)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
            self.ctx = None
        return False


def device_guarded(fn):
    """Method decorator: run with `self.device` as the current device."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        with on_device(self.device):
            return fn(self, *a, **k)
    return wrapper


def _req(t: torch.Tensor, dtype=torch.float32, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (no CPU fallback in handnet-pipeline_amd)")
    _check_device(t, name)
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def conv_out_size(h, w, r, s, stride, pad, dil):
    return ((h + 2 * pad - dil * (r - 1) - 1) // stride + 1,
            (w + 2 * pad - dil * (s - 1) - 1) // stride + 1)


def is_split(t) -> bool:
    """S32 split activation tensor: fp16 [N,H,W,C/32,2,32] (hi[32] | lo[32] per 32-channel block)."""
    return t is not None and t.dtype == torch.float16 and t.dim() == 6 and t.shape[4] == 2 and t.shape[5] == 32


def channels(t) -> int:
    return t.shape[3] * 32 if is_split(t) else t.shape[3]


def _pixel_stride(t: torch.Tensor, name: str) -> int:
    """Accept a dense NHWC tensor (fp32 or S32) or a channel slice of one (x[..., c0:c1] /
    xs[:, :, :, b0:b1]).  Returns the pixel stride in elements (floats or halfs)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (no CPU fallback in handnet-pipeline_amd)")
    _check_device(t, name)
    n, h, w = t.shape[:3]
    ps = t.stride(2)
    if is_split(t):
        inner_ok = t.stride(5) == 1 and t.stride(4) == 32 and t.stride(3) == 64 and ps >= 64 * t.shape[3]
    elif t.dtype == torch.float32 and t.dim() == 4:
        inner_ok = t.stride(3) == 1 and ps >= t.shape[3]
    else:
        raise TypeError(f"{name}: expected fp32 [N,H,W,C] or fp16 S32 [N,H,W,C/32,2,32], got {t.dtype} {tuple(t.shape)}")
    if not inner_ok or t.stride(1) != w * ps or t.stride(0) != h * w * ps:
        raise ValueError(f"{name} must be NHWC-dense or a channel slice of an NHWC-dense tensor")
    return ps


_DESC_TEMPLATES = {}
# Launch plans of conv2d_nhwc / conv2d_nhwc_multi: a call whose tensors have the shapes / strides / flags of an earlier call
# reuses that call's validated struct (the checks cost more host time than the launch at batch 1).
_PLANS = {}


def _plan_get(*parts):
    """-> (key, plan or None).  The key is the front end's own parts (its struct type first) and the development switches
    that every plan depends on."""
    key = (SPLITK, SPLITK_EAGER, F16_TERMS, parts)
    return key, _PLANS.get(key)


def _plan_put(key, struct, out_specs, use_ws):
    """plan = (the stamped struct, what the outputs are, does the launch take the split-K workspace?)"""
    _PLANS[key] = (type(struct).from_buffer_copy(struct), out_specs, bool(use_ws))


def make_conv_desc(n, h, w, cin, cout, r, s, stride=1, pad=0, dil=1, relu_cols=0, res_mode=0,
                   res_h=0, res_w=0, in_affine=0, tile=0, in_pix_stride=0, out_pix_stride=0) -> ConvDesc:
    """A fresh (mutable) descriptor.  The 25-keyword ctypes constructor costs ~5 us, more than the launch it
    describes at batch 1, so descriptors are stamped from cached templates."""
    key = (n, h, w, cin, cout, r, s, stride, pad, dil, relu_cols, res_mode, res_h, res_w, in_affine, tile,
           in_pix_stride, out_pix_stride)
    tpl = _DESC_TEMPLATES.get(key)
    if tpl is None:
        oh, ow = conv_out_size(h, w, r, s, stride, pad, dil)
        tpl = _DESC_TEMPLATES[key] = ConvDesc(
            n=n, h=h, w=w, cin=cin, cout=cout, r=r, s=s, stride=stride, pad=pad, dil=dil, oh=oh, ow=ow,
            relu_cols=relu_cols, res_mode=res_mode, res_h=res_h, res_w=res_w, in_affine=in_affine, tile=tile,
            out_split=0, res_split=0, res_pix_stride=0, in_pix_stride=in_pix_stride, out_pix_stride=out_pix_stride,
            in_affine_stride=0, splitk=0)
    return ConvDesc.from_buffer_copy(tpl)


# ---- the argument checks and descriptor stamps that the convolution front ends share ----
def _table_stride(scale, shift, n, c, stride=None, names="scale / shift", width="C"):
    """The (scale, shift) tables of a per-(image, channel) affine, possibly column slices of wider tables -> their row
    stride (which must be `stride` where the caller's other tables fixed it)."""
    if stride is None:
        stride = scale.stride(0)
    for t in (scale, shift):
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (n, c) or t.stride(1) != 1 or t.stride(0) != stride:
            raise ValueError(f"{names} must be fp32 GPU [N, {width}] tables with equal row stride")
    return stride


def _s32_levels(xs, cin, what="levels"):
    """The S32 maps of one launch -> (batch size, pixel stride), the same for all of them."""
    n, xstride = xs[0].shape[0], _pixel_stride(xs[0], "x")
    for x in xs:
        if not is_split(x) or x.shape[0] != n or channels(x) != cin or _pixel_stride(x, "x") != xstride:
            raise ValueError(f"{what} must be S32 tensors of one batch size, channel count and pixel stride")
    return n, xstride


def _f32_levels(ts, c):
    """The fp32 maps of one launch (channel slices of wider tensors are fine) -> (batch size, pixel stride)."""
    n, xstride = ts[0].shape[0], _pixel_stride(ts[0], "x")
    for t in ts:
        if t.dtype != torch.float32 or is_split(t) or t.shape[0] != n or t.shape[3] != c or _pixel_stride(t, "x") != xstride:
            raise ValueError("levels must be fp32 NHWC tensors of one batch size, channel count and pixel stride")
    return n, xstride


def _rows(xs) -> int:
    """Pixels of all the maps together: the GEMM rows of a level launch."""
    return sum(x.shape[0] * x.shape[1] * x.shape[2] for x in xs)


def _alloc_out(n, oh, ow, cout, split, device):
    """A fresh dense output: S32 when split, else fp32."""
    if split:
        if cout % 32:
            raise ValueError("out_split needs Cout % 32 == 0")
        return torch.empty((n, oh, ow, cout // 32, 2, 32), device=device, dtype=torch.float16)
    return torch.empty((n, oh, ow, cout), device=device, dtype=torch.float32)


def _relu_cols(cout, relu, relu_cols):
    """Output columns that get the ReLU: relu_cols where given, else all of them or none."""
    return (cout if relu else 0) if relu_cols is None else relu_cols


def _stamp_out(d, out, cout, f16=True, splitk=None):
    """Into the descriptor: the format and pixel stride of `out`, the term count, and (splitk = is it allowed? None: leave the
    field alone) the split-K rule -> out's pixel stride."""
    ys = _pixel_stride(out, "out")
    d.out_split = 1 if is_split(out) else 0
    d.out_pix_stride = 0 if ys == (2 * cout if d.out_split else cout) else ys
    d.terms = 1 if (f16 and F16_TERMS == 1) else 0
    if splitk is not None:
        d.splitk = (1 if SPLITK_EAGER else 0) if splitk else -1
    return ys


def _stamp_residual(d, residual):
    """Into an f16x3 descriptor: the format and pixel stride of the residual."""
    d.res_split = 1 if is_split(residual) else 0
    d.res_pix_stride = _pixel_stride(residual, "residual")


def to_split(x, scale=None, shift=None, relu=False, out=None):
    """fp32 [N,H,W,C] -> S32 [N,H,W,C/32,2,32]; optional per-(image, channel) affine (+ReLU) first
    (GroupNorm-apply of the FCOS towers)."""
    lib = _lib.load()
    xs = _pixel_stride(x, "x")
    if is_split(x):
        raise TypeError("x is already split")
    n, h, w, c = x.shape
    if c % 32:
        raise ValueError("the S32 format needs C % 32 == 0")
    if out is None:
        out = torch.empty((n, h, w, c // 32, 2, 32), device=x.device, dtype=torch.float16)
    ys = _pixel_stride(out, "out")
    a_stride = 0 if scale is None else _table_stride(scale, shift, n, c)
    check(lib.hn_affine_split_f32(ptr(x), ptr(scale), ptr(shift), 1 if relu else 0, n, h * w, c, xs, a_stride,
                                  ptr(out), ys, _stream()), "hn_affine_split_f32")
    return out


def from_split(xs16, out=None):
    """S32 -> fp32 [N,H,W,C] (exact)."""
    lib = _lib.load()
    ps = _pixel_stride(xs16, "x")
    if not is_split(xs16):
        raise TypeError("x is not an S32 tensor")
    n, h, w, nb = xs16.shape[:4]
    if out is None:
        out = torch.empty((n, h, w, nb * 32), device=xs16.device, dtype=torch.float32)
    check(lib.hn_unsplit_f32(ptr(xs16), n, h * w, nb * 32, ps, ptr(out), _pixel_stride(out, "out"), _stream()),
          "hn_unsplit_f32")
    return out


# bench.py's roofline leg: when set to a list, every conv launch is bracketed by HIP events
# on the launch stream and ((precision, tile id), algorithmic MACs, timer, shape) is appended.
CONV_PROFILE = None
# which stage of the hot path the engines are in (bench.py's roofline.stages): "resnet34_body", "fpn", "towers",
# "head_outputs", "a2j_trunk", "a2j_heads"; recorded with every profiled conv launch
PROFILE_STAGE = None
TILE_NAMES = {1: "128x128", 2: "128x64", 3: "64x64", 4: "128x32", 6: "64x128", 7: "32x64", 8: "256x64", 12: "64x64k2"}   # (5, 9-11: retired sweep forms)
TILE_RS = 0x100  # profile records: tile id | TILE_RS when the launch ran the row-shared-A instantiation of that tile
TILE_HALO = 0x200  # ... | TILE_HALO when it was routed to the halo-patch kernel (conv3x3_halo_kernel)
TILE_MULTI = 0x400  # ... | TILE_MULTI for a heterogeneous launch (conv_igemm_f16x3_multi_kernel): several convolutions, one record
TILE_STREAM = 0x800  # ... | TILE_STREAM when it was routed to the streaming 1x1 kernel (conv1x1_stream_kernel)


def tile_name(tile) -> str:
    """'128x128' / '128x128+rs' (the row-shared-A kernels are separate instantiations, i.e. separate profiler rows)."""
    if isinstance(tile, int) and tile & TILE_HALO:
        return "halo16x16"
    if isinstance(tile, int) and tile & TILE_STREAM:
        return "stream1x1"
    base = TILE_NAMES.get(tile & 0xFF, str(tile & 0xFF)) if isinstance(tile, int) else str(tile)
    return base + ("+rs" if isinstance(tile, int) and tile & TILE_RS else "") + \
        ("+multi" if isinstance(tile, int) and tile & TILE_MULTI else "")


def _profile_start():
    """Before a conv launch: a started HipTimer when CONV_PROFILE is a list, else None (and nothing is created)."""
    if CONV_PROFILE is None:
        return None
    timer = HipTimer()
    timer.start()
    return timer


def _profile_stop(timer, describe):
    """After the launch, where _profile_start gave a timer: close the bracket and append the record.  describe() -> ((precision,
    tile or form), algorithmic MACs, shape tuple); it runs after the closing event is on the stream, so the library queries it
    makes stay outside the bracket."""
    timer.stop()
    kind, macs, shape = describe()
    CONV_PROFILE.append((kind, macs, timer, shape, PROFILE_STAGE))


# Term count of the f16x3 kernels for the launches issued from now on: 3 = the split-precision product (default),
# 1 = hi*hi only (the engines' precision="f16x1" throughput mode, reported beside the headline by bench.py).
F16_TERMS = 3


class f16_terms:
    """`with ops.f16_terms(1):` -- launches inside the block carry hn_conv_desc.terms = 1."""

    def __init__(self, terms):
        self.terms = terms

    def __enter__(self):
        global F16_TERMS
        self._old, F16_TERMS = F16_TERMS, self.terms

    def __exit__(self, *a):
        global F16_TERMS
        F16_TERMS = self._old


def clear_plan_caches():
    """Drop the cached conv descriptors / launch plans (they are keyed by weight addresses: engines call this when
    they are rebuilt, so that a recycled address can never meet a stale plan and the caches stay bounded)."""
    _PLANS.clear()
    _DESC_TEMPLATES.clear()


# split-K workspace: one fp32 buffer per (device, stream) -- a convolution only uses it between its own two
# launches, and launches on one stream are ordered
CONV_WORKSPACE_BYTES = 32 << 20
SPLITK = True  # development switch (forms.apply_env: HN_SPLITK=0)
# split short k loops too (desc.splitk = 1).  It used to pay only under graph replay; since the host path got
# cheaper (raw stream handle, cached descriptors) it also wins in eager mode (batch 1: 294 -> 301 frames/s)
SPLITK_EAGER = True


class launch_cost_hidden:
    """Context for code whose launches will be replayed from a hipGraph: forces the aggressive split-K setting
    (the default since the host path became cheap; HN_SPLITK_EAGER=0 restores the conservative eager rule)."""

    def __enter__(self):
        global SPLITK_EAGER
        self._old, SPLITK_EAGER = SPLITK_EAGER, True

    def __exit__(self, *a):
        global SPLITK_EAGER
        SPLITK_EAGER = self._old


def warm_up_on_side_stream(step, steps: int = 2):
    """First half of capture_step: `step()` run eagerly on a side stream, then the streams joined."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with launch_cost_hidden(), torch.cuda.stream(side):
        for _ in range(steps):  # warm-up (allocator, lazy module load) outside capture
            step()
    torch.cuda.current_stream().wait_stream(side)


def capture(step):
    """Second half of capture_step: `step()` captured into a hipGraph -> (graph, what step returned)."""
    g = torch.cuda.CUDAGraph()
    # thread_local: GPU work another thread of the host process issues meanwhile (a ROS node's other callbacks)
    # does not invalidate the capture
    with launch_cost_hidden(), torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = step()
    return g, out


def capture_step(step):
    """The engines' one capture recipe -> (graph, out).  `step` takes no argument and reads static tensors its caller
    has filled; the caller also holds torch.inference_mode(False) / torch.no_grad() where it allocates them."""
    warm_up_on_side_stream(step)
    return capture(step)


_WORKSPACES = {}


def _conv_workspace(device):
    key = (device.index, _stream())
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = torch.empty((CONV_WORKSPACE_BYTES // 4,), device=device, dtype=torch.float32)
    return ws


def conv2d_nhwc(x, w, bias=None, *, stride=1, pad=0, dil=1, relu=False, relu_cols=None,
                residual=None, res_upsample=False, in_scale=None, in_shift=None, out=None, tile=0,
                algo_cin=None, w16=None, out_split=False, gn_partial=None, splitk=True, force_splits=None):
    """Convolution with fused epilogue.  x: fp32 [N,H,W,Cin] or S32 split; w [Cout,R,S,Cin] fp32.

    w16 given  -> f16x3 kernel (split-fp16 operands on the f16 MFMA, fp32-grade results); an fp32
                  x (and a GroupNorm-on-load affine in_scale/in_shift) is first converted with
                  one hn_affine_split_f32 pass.  Otherwise the exact f32-MFMA kernel runs.
    out_split  -> y is written in the S32 format (Cout % 32 == 0), ready for the next f16x3 conv.
    residual   -> fp32 or S32 tensor added before the ReLU; res_upsample = nearest-neighbour
                  read of a coarser map (FPN top-down path).
    algo_cin   -> input channels the reference's conv really has when Cin is zero-padded
                  (FLOP accounting only).
    splitk     -> (f16x3) allow split-K for small grids (deterministic two-launch scheme, needs the workspace).
    gn_partial -> (f16x3, fp32 output, no residual / ReLU) fp32 scratch of gn_rows32_scratch_floats(rows, Cout)
                  floats: the epilogue also writes GroupNorm partial sums for groupnorm_finalize_rows32()."""
    lib = _lib.load()
    plan_key = None
    if (out is None and in_scale is None and w16 is not None and gn_partial is None and CONV_PROFILE is None
            and x.dtype == torch.float16 and x.is_cuda):
        _check_device(x, "x")
        dev = x.device
        plan_key, plan = _plan_get(
            ConvDesc, dev.index, x.shape, x.stride(), w.data_ptr(), tuple(w.shape), w16.data_ptr(),
            None if bias is None else bias.data_ptr(), stride, pad, dil, relu, relu_cols, tile, out_split, res_upsample, splitk,
            None if residual is None else (residual.shape, residual.stride(), residual.dtype))
        if plan is not None:
            tpl, (out_shape, out_dtype), use_ws = plan
            d = ConvDesc.from_buffer_copy(tpl)
            out = torch.empty(out_shape, device=dev, dtype=out_dtype)
            ws = _conv_workspace(dev) if use_ws else None
            check(lib.hn_conv2d_nhwc_f16x3_ws(C.byref(d), ptr(x), ptr(w16), ptr(bias), ptr(residual), ptr(out),
                                              ptr(ws), ws.numel() * 4 if use_ws else 0, _stream()),
                  "hn_conv2d_nhwc_f16x3_ws")
            return out
    _req(w, name="w")
    cout, r, s, cin = w.shape
    use16 = w16 is not None
    if use16:
        if is_split(x):
            if in_scale is not None:
                raise ValueError("apply the affine with to_split() before an S32-input convolution")
        else:
            x = to_split(x, in_scale, in_shift, relu=in_scale is not None)
            in_scale = in_shift = None
    elif is_split(x):
        raise TypeError("the f32 kernel needs an fp32 input (use from_split)")
    xs = _pixel_stride(x, "x")
    n, h, wd = x.shape[:3]
    if channels(x) != cin:
        raise ValueError(f"weight Cin {cin} != input channels {channels(x)}")
    rc = _relu_cols(cout, relu, relu_cols)
    res_mode, rh, rw = 0, 0, 0
    if residual is not None:
        if channels(residual) != cout or residual.shape[0] != n:
            raise ValueError("residual shape mismatch")
        if is_split(residual) and not use16:
            raise TypeError("the f32 kernel takes fp32 residuals only")
        if res_upsample:
            res_mode, rh, rw = 2, residual.shape[1], residual.shape[2]
        else:
            res_mode = 1
    dense_in = xs == (2 * cin if is_split(x) else cin)
    d = make_conv_desc(n, h, wd, cin, cout, r, s, stride, pad, dil, rc, res_mode, rh, rw,
                       1 if in_scale is not None else 0, tile, in_pix_stride=0 if dense_in else xs)
    if out is None:
        out = _alloc_out(n, d.oh, d.ow, cout, out_split, x.device)
    if tuple(out.shape[:3]) != (n, d.oh, d.ow) or channels(out) != cout:
        raise ValueError("out has the wrong shape")
    # split-K is a matter of the plain f16x3 launch only (None: the field keeps the template's 0)
    splitk = bool(splitk and SPLITK) if use16 and gn_partial is None else None
    _stamp_out(d, out, cout, use16, splitk)
    if residual is not None:
        if res_mode == 1 and tuple(residual.shape[:3]) != (n, d.oh, d.ow):
            raise ValueError("residual shape mismatch")
        if use16:
            _stamp_residual(d, residual)
        elif _pixel_stride(residual, "residual") != cout:
            raise ValueError("the f32 kernel needs a dense residual")
    if bias is not None:
        _req(bias, name="bias")
    if in_scale is not None:
        a_stride = _table_stride(in_scale, in_shift, n, cin, names="in_scale / in_shift", width="Cin")
        d.in_affine_stride = 0 if a_stride == cin else a_stride
    timer = _profile_start()
    if use16:
        if (not w16.is_cuda or w16.dtype != torch.float16 or not w16.is_contiguous()
                or w16.numel() != 2 * w.numel()):
            raise ValueError("w16 must be the contiguous fp16 GPU tensor produced by weights.split_f16x3(w)")
        if gn_partial is not None:
            if residual is not None or rc or d.out_split:
                raise ValueError("gn_partial needs an fp32 output without residual / ReLU")
            need = lib.hn_groupnorm_rows32_scratch_floats(n * d.oh * d.ow, cout)
            if not gn_partial.is_cuda or gn_partial.dtype != torch.float32 or gn_partial.numel() < need:
                raise ValueError(f"gn_partial must be an fp32 GPU buffer of >= {need} floats")
            check(lib.hn_conv2d_nhwc_f16x3_gn(C.byref(d), ptr(x), ptr(w16), ptr(bias), ptr(out), ptr(gn_partial),
                                              _stream()), "hn_conv2d_nhwc_f16x3_gn")
        else:
            if force_splits is not None:      # sweeps only: exactly this many splits (1 = none)
                d.splitk = int(force_splits) if force_splits >= 2 else -1
                plan_key = None
            ws = _conv_workspace(x.device) if splitk else None
            if plan_key is not None and (bias is None or bias.is_contiguous()):
                _plan_put(plan_key, d, (tuple(out.shape), out.dtype), splitk)
            check(lib.hn_conv2d_nhwc_f16x3_ws(C.byref(d), ptr(x), ptr(w16), ptr(bias), ptr(residual), ptr(out),
                                              ptr(ws), ws.numel() * 4 if splitk else 0, _stream()),
                  "hn_conv2d_nhwc_f16x3_ws")
    else:
        if gn_partial is not None:
            raise ValueError("gn_partial is an f16x3-kernel feature")
        check(lib.hn_conv2d_nhwc_f32(C.byref(d), ptr(x), ptr(w), ptr(bias), ptr(residual), ptr(in_scale),
                                     ptr(in_shift), ptr(out), _stream()), "hn_conv2d_nhwc_f32")
    if timer is not None:
        def describe():
            if use16:
                flags = TILE_HALO if lib.hn_conv2d_f16x3_uses_halo(C.byref(d), 1 if residual is not None else 0) else \
                    (TILE_STREAM if lib.hn_conv2d_f16x3_uses_stream(C.byref(d)) else
                     TILE_RS if lib.hn_conv2d_f16x3_uses_rs(C.byref(d)) else 0)
                kind = ("f16x3", lib.hn_conv2d_f16x3_pick_tile(C.byref(d)) | flags)
            else:
                kind = ("f32", lib.hn_conv2d_pick_tile(C.byref(d)))
            return kind, n * d.oh * d.ow * cout * r * s * (algo_cin or cin), (n, h, wd, cin, cout, r, stride, dil)
        _profile_stop(timer, describe)
    return out


def conv2d_nhwc_multi(items, fused=None):
    """INDEPENDENT f16x3 convolutions of different shapes as one launch (hn_conv2d_nhwc_f16x3_multi; at most
    _lib.CONV_MULTI_MAX members).  items: [(x S32, ConvW-like cw, opts)], opts = dict(relu=False, relu_cols=None,
    residual=None, out_split=True); every member computes exactly what conv2d_nhwc(x, cw.w, cw.bias, stride=cw.stride,
    pad=cw.pad, dil=cw.dil, w16=cw.w16, **opts) would (bit-identical: same kernel body, same split-K plan) -- the library
    falls back to that, member after member, when the members' tile forms differ.  Returns the outputs.
    fused: optional one-element list that receives whether the members ran as one launch (tests)."""
    lib = _lib.load()
    k = len(items)
    if k == 0 or k > _lib.CONV_MULTI_MAX:
        raise ValueError(f"need 1..{_lib.CONV_MULTI_MAX} members")
    splitk = SPLITK
    # Plan (like conv2d_nhwc's): the validated descriptor table of an earlier call with the same shapes / strides / weights
    # is stamped out again; only the activation pointers change.
    key = [_lib.ConvMulti]
    for x, cw, opts in items:
        res = opts.get("residual")
        key.append((x.device.index, x.shape, x.stride(), x.dtype, cw.w16.data_ptr() if cw.w16 is not None else None,
                    None if cw.bias is None else cw.bias.data_ptr(), cw.stride, cw.pad, cw.dil, opts.get("relu", False),
                    opts.get("relu_cols"), opts.get("out_split", True),
                    None if res is None else (res.shape, res.stride(), res.dtype)))
    key, plan = _plan_get(*key)
    if plan is not None and CONV_PROFILE is None and fused is None:
        tpl, out_specs, use_ws = plan
        mm = _lib.ConvMulti.from_buffer_copy(tpl)
        outs = []
        for i, ((x, _cw, opts), (shape, dtype)) in enumerate(zip(items, out_specs)):
            _check_device(x, "x")
            y = torch.empty(shape, device=x.device, dtype=dtype)
            mm.x16[i], mm.residual[i], mm.y[i] = x.data_ptr(), ptr(opts.get("residual")), y.data_ptr()
            outs.append(y)
        ws = _conv_workspace(items[0][0].device) if use_ws else None
        check(lib.hn_conv2d_nhwc_f16x3_multi(C.byref(mm), ptr(ws), ws.numel() * 4 if use_ws else 0, _stream()),
              "hn_conv2d_nhwc_f16x3_multi")
        return outs
    mm = _lib.ConvMulti()
    mm.count = k
    outs = []
    macs, shapes = 0, []
    for i, (x, cw, opts) in enumerate(items):
        if not is_split(x) or cw.w16 is None:
            raise TypeError("multi launches take S32 inputs and split filter banks")
        if not x.is_cuda:
            raise RuntimeError("x must live on the GPU (no CPU fallback in handnet-pipeline_amd)")
        _check_device(x, "x")
        relu, relu_cols = opts.get("relu", False), opts.get("relu_cols")
        residual, out_split = opts.get("residual"), opts.get("out_split", True)
        cout, r, s_, cin = cw.w.shape
        n, h, wd = x.shape[:3]
        if channels(x) != cin:
            raise ValueError(f"member {i}: weight Cin {cin} != input channels {channels(x)}")
        xs = _pixel_stride(x, "x")
        d = make_conv_desc(n, h, wd, cin, cout, r, s_, cw.stride, cw.pad, cw.dil, _relu_cols(cout, relu, relu_cols),
                           1 if residual is not None else 0, 0, 0, 0, 0, in_pix_stride=0 if xs == 2 * cin else xs)
        y = _alloc_out(n, d.oh, d.ow, cout, out_split, x.device)
        _stamp_out(d, y, cout, splitk=bool(splitk))
        if residual is not None:
            if tuple(residual.shape[:3]) != (n, d.oh, d.ow) or channels(residual) != cout:
                raise ValueError(f"member {i}: residual shape mismatch")
            _stamp_residual(d, residual)
        if cw.bias is not None:
            _req(cw.bias, name="bias")
        mm.desc[i] = d
        mm.x16[i], mm.w16[i], mm.bias[i] = ptr(x), ptr(cw.w16), ptr(cw.bias)
        mm.residual[i], mm.y[i] = ptr(residual), ptr(y)
        outs.append(y)
        macs += n * d.oh * d.ow * cout * r * s_ * cin
        shapes.append((n, h, wd, cin, cout, r, cw.stride, cw.dil))
    ws = _conv_workspace(items[0][0].device) if splitk else None
    if fused is not None:
        fused.append(bool(lib.hn_conv2d_f16x3_multi_fuses(C.byref(mm), ws.numel() * 4 if splitk else 0)))
    timer = _profile_start()
    check(lib.hn_conv2d_nhwc_f16x3_multi(C.byref(mm), ptr(ws), ws.numel() * 4 if splitk else 0, _stream()),
          "hn_conv2d_nhwc_f16x3_multi")
    if timer is not None:
        def describe():     # one record: the largest member's tile and shape, the MACs of all
            big = max(range(k), key=lambda i: shapes[i][0] * shapes[i][1] * shapes[i][2] * shapes[i][3] * shapes[i][4] * shapes[i][5] ** 2)
            return ("f16x3", lib.hn_conv2d_f16x3_pick_tile(C.byref(mm.desc[big])) | TILE_MULTI), macs, shapes[big]
        _profile_stop(timer, describe)
    else:
        _plan_put(key, mm, [(tuple(y.shape), y.dtype) for y in outs], splitk)
    return outs


def conv2d_nhwc_grouped(xs, ws, *, pad=0, relu=False, relu_cols=None, out_split=False, tile=0, gn_partials=None,
                        outs=None, out_channel_offsets=None, gn=None, gn_units=0, carry=None, carry_query=False):
    """Independent stride-1 f16x3 convolutions with identical channels / filter / batch as ONE launch
    (gridDim.z = member); the members may differ in spatial size (the FPN levels of one layer).
      xs            S32 inputs (same N, channels and pixel stride); ws: ConvW-like objects (.w [Cout,R,S,Cin], .bias,
                    .w16), all of one shape
      outs          optional preallocated outputs (one per member, or the same tensor several times); member i writes
                    channels [out_channel_offsets[i], +Cout) of outs[i] -- stacking members in one wide tensor keeps
                    e.g. the cls / reg towers of a level together.  Default: fresh dense outputs.
      gn_partials   one GroupNorm-sum buffer per member (each Cout/8 units wide), or
      gn, gn_units  [(buffer, unit offset)] per member into slabs that are gn_units units wide (stacked members).
      carry         (xs, affines, outs, relu) as to_split_levels takes them: the launch also runs that apply pass, every
                    workgroup a slice of it once its output tile is stored (hn_conv2d_nhwc_f16x3_grouped_carry) -- on a
                    tensor this convolution neither reads nor writes; only where grouped_carry_applies() says so.
      carry_query   plan only: returns True / False, would this launch carry? (launches nothing)
    Returns the list of outputs.  A single plain member falls through to conv2d_nhwc."""
    k = len(xs)
    if k != len(ws) or k == 0 or k > _lib.CONV_MAX_GROUP:
        raise ValueError(f"need 1..{_lib.CONV_MAX_GROUP} inputs and as many weight sets")
    if k == 1 and outs is None and gn is None and carry is None and not carry_query:
        return [conv2d_nhwc(xs[0], ws[0].w, ws[0].bias, pad=pad, relu=relu, relu_cols=relu_cols, w16=ws[0].w16,
                            out_split=out_split, tile=tile, gn_partial=None if gn_partials is None else gn_partials[0])]
    lib = _lib.load()
    cout, r, s, cin = ws[0].w.shape
    x0 = xs[0]
    n, xstride = _s32_levels(xs, cin, "grouped inputs")
    for cw in ws:
        if tuple(cw.w.shape) != (cout, r, s, cin) or cw.w16 is None or (cw.bias is None) != (ws[0].bias is None):
            raise ValueError("grouped weights must share one shape (and all or none have a bias)")
    rc = _relu_cols(cout, relu, relu_cols)
    h0, w0 = x0.shape[1:3]
    d = make_conv_desc(n, h0, w0, cin, cout, r, s, 1, pad, 1, rc, 0, 0, 0, 0, tile,
                       in_pix_stride=0 if xstride == 2 * cin else xstride)
    if gn_partials is not None:
        if gn is not None or len(gn_partials) != k:
            raise ValueError("give gn_partials (one per member) or gn, not both")
        gn, gn_units = [(g, 0) for g in gn_partials], 0
    if gn is not None and (rc or out_split):
        raise ValueError("GroupNorm sums need fp32 outputs without ReLU")
    sizes = [conv_out_size(x.shape[1], x.shape[2], r, s, 1, pad, 1) for x in xs]
    if outs is None:
        outs = [_alloc_out(n, oh, ow, cout, out_split, x0.device) for oh, ow in sizes]
    offs = [0] * k if out_channel_offsets is None else list(out_channel_offsets)
    ystride = _stamp_out(d, outs[0], cout, splitk=False)
    grp = ConvGroup()
    grp.count = k
    grp.gn_units = int(gn_units)
    units = gn_units if gn_units else cout // 8
    for i, (x, cw, y, (oh, ow)) in enumerate(zip(xs, ws, outs, sizes)):
        if (tuple(y.shape[:3]) != (n, oh, ow) or is_split(y) != bool(d.out_split) or _pixel_stride(y, "out") != ystride
                or offs[i] % 32 or offs[i] + cout > channels(y)):
            raise ValueError("grouped outputs must match their member's size and share type / pixel stride")
        elt = 2 if d.out_split else 4
        grp.x16[i], grp.w16[i], grp.bias[i] = ptr(x), ptr(cw.w16), ptr(cw.bias)
        grp.y[i] = y.data_ptr() + elt * (2 * offs[i] if d.out_split else offs[i])
        grp.h[i], grp.w[i] = x.shape[1], x.shape[2]
        grp.gn_partial[i] = None
        if gn is not None:
            buf, uoff = gn[i]
            need = lib.hn_groupnorm_rows32_scratch_floats(n * oh * ow, units * 8)
            if buf.numel() < need or buf.dtype != torch.float32 or not buf.is_cuda or uoff * 8 + cout > units * 8:
                raise ValueError(f"member {i}: GroupNorm slab must be an fp32 GPU buffer of >= {need} floats")
            grp.gn_partial[i] = buf.data_ptr() + 16 * uoff
    if carry_query:
        return bool(lib.hn_conv2d_f16x3_grouped_carry_applies(C.byref(d), C.byref(grp)))
    timer = _profile_start()
    if carry is not None:
        cxs, caff, couts, crelu = carry
        lv, cn, cc, cxstride, ca_stride, cystride, _ = _split_levels_arg(cxs, caff, couts)
        check(lib.hn_conv2d_nhwc_f16x3_grouped_carry(C.byref(d), C.byref(grp), C.byref(lv), 1 if crelu else 0, cn, cc, cxstride,
                                                     ca_stride, cystride, _stream()), "hn_conv2d_nhwc_f16x3_grouped_carry")
    else:
        check(lib.hn_conv2d_nhwc_f16x3_grouped(C.byref(d), C.byref(grp), _stream()), "hn_conv2d_nhwc_f16x3_grouped")
    if timer is not None:
        def describe():
            rows = sum(n * oh * ow for oh, ow in sizes)
            tot = make_conv_desc(1, rows, 1, cin, cout, 1, 1)          # what the tile heuristic saw: all rows together
            picked = lib.hn_conv2d_f16x3_pick_tile(C.byref(tot))
            q = ConvDesc.from_buffer_copy(d)                           # geometry of the launch, picked tile, narrowest member
            q.tile, q.w = picked, min(ow for _, ow in sizes)
            return (("f16x3", picked | (TILE_RS if lib.hn_conv2d_f16x3_uses_rs(C.byref(q)) else 0)), rows * cout * r * s * cin,
                    (1, rows, 1, cin, cout, r, 1, 1))
        _profile_stop(timer, describe)
    return outs


def conv3x3_thin_levels(xs, cw, relu_cols=0):
    """3x3 / pad 1 convolution with <= 16 output channels on several maps at once (the FCOS head outputs on all FPN levels,
    hn_conv3x3_thin_f16x3_levels): xs = S32 inputs [N,h_l,w_l,Cin/32,2,32] (channel slices allowed), cw = ConvW-like with
    .w [Cout,3,3,Cin], .w16, .bias -> list of fp32 [N,h_l,w_l,Cout].  Cout <= 5: the P-form kernel (equal to
    conv2d_nhwc_grouped(xs, [cw]*L, pad=1) to fp32 rounding); else the tap kernel (bit-identical to it)."""
    lib = _lib.load()
    cout, r, s, cin = cw.w.shape
    if (r, s) != (3, 3) or cout > 16 or cw.w16 is None or len(xs) > _lib.HN_FCOS_MAX_LEVELS:
        raise ValueError("conv3x3_thin_levels needs a 3x3 filter bank with <= 16 output channels and a split bank")
    n, xstride = _s32_levels(xs, cin)
    lv = _thin_levels_of(xs, inputs=True)
    outs = _thin_outs(lv, xs, cout)
    timer = _profile_start()
    check(lib.hn_conv3x3_thin_f16x3_levels(C.byref(lv), n, cin, cout, ptr(cw.w16), ptr(cw.bias), int(relu_cols),
                                           0 if xstride == 2 * cin else xstride, _stream()), "hn_conv3x3_thin_f16x3_levels")
    if timer is not None:
        def describe():
            rows = _rows(xs)
            form = "thin-P" if lib.hn_conv3x3_thin_uses_flat(C.byref(lv), n, cin, cout) else "thin16x16"
            return ("f16x3", form), rows * cout * 9 * cin, (1, rows, 1, cin, cout, 3, 1, 1)
        _profile_stop(timer, describe)
    return outs


def conv3x3_thin_levels_group(members):
    """Up to three conv3x3_thin_levels calls as ONE launch where they run the tap kernel (hn_conv3x3_thin_f16x3_levels_group; the
    FCOS head outputs of a single frame: 89 workgroups each, latency-bound): members = [(xs, cw, relu_cols), ...] with one batch
    size, channel count and pixel stride -> [outs of member 0, outs of member 1, ...], bit-identical to the separate calls (which
    is what runs where a member takes the P form)."""
    lib = _lib.load()
    if not 1 <= len(members) <= 3:
        raise ValueError("1..3 members")
    cin = members[0][1].w.shape[3]
    n, xstride = _s32_levels([x for xs, _, _ in members for x in xs], cin)
    arr = (_lib.ThinMember * len(members))()
    results = []
    for m, (xs, cw, relu_cols) in enumerate(members):
        cout, r, s_, c = cw.w.shape
        if (r, s_) != (3, 3) or cout > 16 or cw.w16 is None or len(xs) > _lib.HN_FCOS_MAX_LEVELS or c != cin:
            raise ValueError("members need 3x3 filter banks with <= 16 output channels, a split bank and one input channel count")
        mm = arr[m]
        mm.lv = _thin_levels_of(xs, inputs=True)
        results.append(_thin_outs(mm.lv, xs, cout))
        mm.cout, mm.relu_cols, mm.w16, mm.bias = cout, int(relu_cols), ptr(cw.w16), ptr(cw.bias)
    timer = _profile_start()
    check(lib.hn_conv3x3_thin_f16x3_levels_group(arr, len(members), n, cin, 0 if xstride == 2 * cin else xstride, _stream()),
          "hn_conv3x3_thin_f16x3_levels_group")
    if timer is not None:
        def describe():     # the shape: member 0's pixels by the output channels of all members
            flat = any(lib.hn_conv3x3_thin_uses_flat(C.byref(arr[m].lv), n, cin, arr[m].cout) for m in range(len(members)))
            macs = sum(_rows(xs) * cw.w.shape[0] for xs, cw, _ in members) * 9 * cin
            couts = sum(cw.w.shape[0] for _, cw, _ in members)
            return ("f16x3", "thin-P" if flat else f"thin16x16x{len(members)}"), macs, (1, _rows(members[0][0]), 1, cin, couts, 3, 1, 1)
        _profile_stop(timer, describe)
    return results


def _thin_levels_of(ts, inputs=False):
    """hn_thin_levels with the sizes of the maps ts (and, for a launch on S32 maps, their addresses as its inputs)."""
    lv = _lib.ThinLevels()
    lv.count = len(ts)
    for i, t in enumerate(ts):
        lv.h[i], lv.w[i] = t.shape[1], t.shape[2]
        if inputs:
            lv.x16[i] = t.data_ptr()
    return lv


def _thin_outs(lv, ts, cout):
    """Fresh fp32 [N,h_l,w_l,Cout] outputs of a thin launch on the maps ts, their addresses stamped into lv."""
    outs = [torch.empty((t.shape[0], t.shape[1], t.shape[2], cout), device=t.device, dtype=torch.float32) for t in ts]
    for i, y in enumerate(outs):
        lv.y[i] = y.data_ptr()
    return outs


def thin_affine_applies(ts, cw) -> bool:
    """Would conv3x3_thin_affine_levels take these raw tower outputs ts (fp32 [N,h_l,w_l,C]) with filter bank cw?"""
    cout, _, _, cin = cw.w.shape
    lv = _thin_levels_of(ts)
    return len(ts) <= _lib.HN_FCOS_MAX_LEVELS and bool(_lib.load().hn_conv3x3_thin_affine_applies(C.byref(lv), ts[0].shape[0], cin, cout))


def conv3x3_thin_affine_levels(ts, affines, ch0, cw, relu_cols=0):
    """The head-output convolution on the RAW outputs of the last tower layer with that layer's GroupNorm apply pass fused
    in (hn_conv3x3_thin_affine_f16x3_levels): ts[l] fp32 [N,h_l,w_l,C] raw conv outputs, affines[l] = (scale, shift) fp32
    [N,C] from groupnorm_finalize_rows32_levels, ch0 = first channel of this head's cw.cin channels inside C.  Equals
    conv3x3_thin_levels(to_split_levels(ts, affines)[..., ch0 // 32 : (ch0 + cin) // 32], cw) bit for bit, without the pass."""
    lib = _lib.load()
    cout, r, s, cin = cw.w.shape
    c = ts[0].shape[3]
    if (r, s) != (3, 3) or cw.w16 is None or ch0 % 32 or ch0 + cin > c:
        raise ValueError("conv3x3_thin_affine_levels needs a split 3x3 filter bank and a 32-aligned channel range")
    n, xstride = _f32_levels(ts, c)
    a_stride = affines[0][0].stride(0)
    lv, aff = _thin_levels_of(ts), _lib.ThinAffine()
    aff.in_pix_stride, aff.affine_stride = xstride, a_stride
    for i, (t, (scale, shift)) in enumerate(zip(ts, affines)):
        _table_stride(scale, shift, n, c, a_stride)
        aff.x[i], aff.scale[i], aff.shift[i] = t.data_ptr() + 4 * ch0, scale.data_ptr() + 4 * ch0, shift.data_ptr() + 4 * ch0
    outs = _thin_outs(lv, ts, cout)
    timer = _profile_start()
    check(lib.hn_conv3x3_thin_affine_f16x3_levels(C.byref(lv), C.byref(aff), n, cin, cout, ptr(cw.w16), ptr(cw.bias),
                                                  int(relu_cols), _stream()), "hn_conv3x3_thin_affine_f16x3_levels")
    if timer is not None:
        def describe():
            rows = _rows(ts)
            return ("f16x3", "thin-P+gn"), rows * cout * 9 * cin, (1, rows, 1, cin, cout, 3, 1, 1)
        _profile_stop(timer, describe)
    return outs


def conv3x3_thin_backward_levels(a16s, members, *, want_dx=True, dx_out=None, dx_channel_offset=0):
    """The backward of conv3x3_thin_levels for the one or two filter banks that read one map (hn_conv3x3_thin_backward_f32;
    DESIGN.md section 9t): a16s = the S32 inputs the forward read [N,h_l,w_l,Cin/32,2,32] (channel slices allowed), members =
    [(cw, relu_cols, ys, gs), ...] with cw.w [Cout,3,3,Cin] fp32 (Cout <= 16, at most 16 columns together), ys = the forward's
    own outputs and gs = the upstream gradients, fp32 [N,h_l,w_l,Cout] per level -> ([(dW [Cout,3,3,Cin], db [Cout]), ...],
    dA levels or None).  The ReLU mask is torch's on the stored result: a gradient passes where column >= relu_cols or y > 0.
    dW and db are ONE sum over all levels and images.  dA (want_dx) is fp32 [N,h_l,w_l,Cin], the gradient at float(hi) +
    float(lo), summed over the members; dx_out = per-level fp32 tensors [N,h_l,w_l,C >= dx_channel_offset + Cin] to write
    channels dx_channel_offset .. + Cin of instead (the other channels are left alone).  Two launches, every element written
    once, the same bytes on every run; every refusal happens before a launch."""
    lib = _lib.load()
    if not 1 <= len(members) <= 2:
        raise ValueError("conv3x3_thin_backward_levels: one or two members on a map")
    if not 1 <= len(a16s) <= _lib.HN_FCOS_MAX_LEVELS:
        raise ValueError(f"conv3x3_thin_backward_levels: 1..{_lib.HN_FCOS_MAX_LEVELS} levels")
    cin = members[0][0].w.shape[3]
    n, xstride = _s32_levels(a16s, cin)
    dev, nl = a16s[0].device, len(a16s)
    lv = _thin_levels_of(a16s, inputs=True)
    couts, relus = (C.c_int32 * len(members))(), (C.c_int32 * len(members))()
    wp, dwp, dbp = ((C.c_void_p * len(members))() for _ in range(3))
    yp, gp = ((C.c_void_p * (len(members) * nl))() for _ in range(2))
    results = []
    for m, (cw, relu_cols, ys, gs) in enumerate(members):
        cout, r, s_, c = cw.w.shape
        if (r, s_) != (3, 3) or cout > 16 or c != cin or not 0 <= int(relu_cols) <= cout:
            raise ValueError("members need fp32 3x3 filter banks with <= 16 output channels, one input channel count and "
                             "0 <= relu_cols <= Cout")
        _req(cw.w, name="w")
        if len(ys) != nl or len(gs) != nl:
            raise ValueError("members need one output and one gradient per level")
        for ts, arr in ((ys, yp), (gs, gp)):
            if _f32_levels(ts, cout) != (n, cout):
                raise ValueError("outputs and gradients must be dense fp32 [N,h,w,Cout] tensors of the inputs' batch size")
            for l, (t, a) in enumerate(zip(ts, a16s)):
                if tuple(t.shape[1:3]) != tuple(a.shape[1:3]) or t.device != dev:
                    raise ValueError("outputs and gradients must have the inputs' map sizes and device")
                arr[m * nl + l] = t.data_ptr()
        dw = torch.empty((cout, 3, 3, cin), device=dev, dtype=torch.float32)
        db = torch.empty((cout,), device=dev, dtype=torch.float32)
        couts[m], relus[m], wp[m], dwp[m], dbp[m] = cout, int(relu_cols), cw.w.data_ptr(), dw.data_ptr(), db.data_ptr()
        results.append((dw, db))
    das, dxs = 0, None
    if want_dx:
        if dx_out is None:
            if dx_channel_offset:
                raise ValueError("dx_channel_offset needs dx_out")
            dxs = [torch.empty(tuple(a.shape[:3]) + (cin,), device=dev, dtype=torch.float32) for a in a16s]
        else:
            dxs = list(dx_out)
            if len(dxs) != nl or any(tuple(t.shape[:3]) != tuple(a.shape[:3]) or t.device != dev for t, a in zip(dxs, a16s)):
                raise ValueError("dx_out must hold one tensor per level with the inputs' [N,h,w] on their device")
            width = dxs[0].shape[3]
            if _f32_levels([_req(t, name="dx_out") for t in dxs], width) != (n, width) \
                    or not 0 <= int(dx_channel_offset) <= width - cin:
                raise ValueError("dx_out must be dense fp32 [N,h,w,C] tensors with dx_channel_offset + Cin <= C")
        das = dxs[0].shape[3]
        for l, t in enumerate(dxs):
            lv.y[l] = t.data_ptr()
    nbytes = lib.hn_conv3x3_thin_backward_ws_bytes(C.byref(lv), n, cin, len(members), couts)
    if nbytes < 0:
        check(1, "hn_conv3x3_thin_backward_ws_bytes")
    ws = _conv_workspace(dev)
    if nbytes > 4 * ws.numel():
        ws = torch.empty(((nbytes + 3) // 4,), device=dev, dtype=torch.float32)
    timer = _profile_start()
    check(lib.hn_conv3x3_thin_backward_f32(C.byref(lv), n, cin, 0 if xstride == 2 * cin else xstride, len(members), couts, relus,
                                           wp, yp, gp, dwp, dbp, das, int(dx_channel_offset) if want_dx else 0, ptr(ws), 4 * ws.numel(), _stream()),
          "hn_conv3x3_thin_backward_f32")
    if timer is not None:
        def describe():
            rows, cols = _rows(a16s), sum(int(c) for c in couts)
            return ("f32", "thin-bwd"), rows * cols * 9 * cin * (2 if want_dx else 1), (1, rows, 1, cin, cols, 3, 1, 1)
        _profile_stop(timer, describe)
    return results, dxs


# ---- the backward of a tower layer: conv3x3 -> GroupNorm -> ReLU (include/handnet_hip_train.h) ----
_BIG_WORKSPACES = {}


def _backward_workspace(device, nbytes):
    """The convolution workspace where the partial sums fit it, else one grown buffer per (device, stream): the weight
    gradient's partials are (K ranges) x |dW| floats, beyond the split-K workspace for a 256 -> 256 layer."""
    ws = _conv_workspace(device)
    if nbytes <= 4 * ws.numel():
        return ws
    key = (device.index, _stream())
    big = _BIG_WORKSPACES.get(key)
    if big is None or 4 * big.numel() < nbytes:
        big = _BIG_WORKSPACES[key] = torch.empty(((nbytes + 3) // 4,), device=device, dtype=torch.float32)
    return big


def _level_count(ts, what):
    if not 1 <= len(ts) <= _lib.HN_FCOS_MAX_LEVELS:
        raise ValueError(f"{what}: 1..{_lib.HN_FCOS_MAX_LEVELS} levels")


def _gn_levels_arg(ys, groups, what):
    """The raw fp32 outputs of one layer over the levels -> (hn_gn_bwd_levels with sizes and y stamped, n, c, y stride)."""
    _level_count(ys, what)
    c = ys[0].shape[3] if ys[0].dim() == 4 else -1
    n, ystride = _f32_levels(ys, c)
    if c % 8 or c > 512 or groups <= 0 or c % groups or (c // groups) % 8:
        raise ValueError(f"{what}: C must be a multiple of 8, at most 512, and C / groups a multiple of 8 (C {c}, groups {groups})")
    lv = _lib.GnBwdLevels()
    lv.count = len(ys)
    for i, y in enumerate(ys):
        lv.h[i], lv.w[i], lv.y[i] = y.shape[1], y.shape[2], y.data_ptr()
    return lv, n, c, ystride


def _gn_ws(lv, n, c, groups, device):
    nbytes = _lib.load().hn_groupnorm_relu_backward_ws_bytes(C.byref(lv), n, c, groups)
    if nbytes < 0:
        check(1, "hn_groupnorm_relu_backward_ws_bytes")
    return _backward_workspace(device, nbytes)


def groupnorm_stats_levels(ys, groups, eps=1e-5):
    """mean and rstd of GroupNorm per (level, image, group) from the raw outputs ys[l] fp32 [N,h_l,w_l,C] (channel slices are
    fine) -> [(mean [N,G], rstd [N,G])] per level: mean = sum y / M, rstd = 1 / sqrt(sum y^2 / M - mean^2 + eps), fp32 partial
    sums per 64-pixel chunk in a fixed order, combined in fp64 (hn_groupnorm_stats_levels_f32).  What the forward's finalize
    computes before it folds the two into its scale / shift tables."""
    lib = _lib.load()
    lv, n, c, ystride = _gn_levels_arg(ys, groups, "groupnorm_stats_levels")
    dev = ys[0].device
    tables = torch.empty((len(ys), 2, n, groups), device=dev, dtype=torch.float32)
    for i in range(len(ys)):
        lv.mean[i], lv.rstd[i] = tables[i, 0].data_ptr(), tables[i, 1].data_ptr()
    ws = _gn_ws(lv, n, c, groups, dev)
    check(lib.hn_groupnorm_stats_levels_f32(C.byref(lv), n, c, groups, ystride, float(eps), ptr(ws), 4 * ws.numel(), _stream()),
          "hn_groupnorm_stats_levels_f32")
    return [(tables[i, 0], tables[i, 1]) for i in range(len(ys))]


def groupnorm_relu_backward_levels(ys, gs, affines, stats, gamma, groups, dy_out=None):
    """The backward of relu(GroupNorm(y)) over the levels of one tower layer (hn_groupnorm_relu_backward_f32; DESIGN.md section
    9u): ys[l] = the raw convolution outputs, gs[l] = the gradients at the ReLU'd result, fp32 [N,h_l,w_l,C] (channel slices are
    fine); affines[l] = the forward's (scale, shift) [N,C] tables; stats[l] = (mean, rstd) [N,G] of groupnorm_stats_levels; gamma
    [C] -> (dys per level, d_gamma [C], d_beta [C]).  The mask is the sign of fma(y, scale, shift), the forward's own expression.
    d_gamma and d_beta are ONE sum over levels and images.  dy_out: per-level fp32 tensors (or channel slices) to write instead
    of fresh ones.  Three launches, every element written once, the same bytes on every run; refusals come before a launch."""
    lib = _lib.load()
    what = "groupnorm_relu_backward_levels"
    lv, n, c, ystride = _gn_levels_arg(ys, groups, what)
    dev, nl = ys[0].device, len(ys)
    if len(gs) != nl or len(affines) != nl or len(stats) != nl or (dy_out is not None and len(dy_out) != nl):
        raise ValueError(f"{what}: one gradient, one (scale, shift) pair and one (mean, rstd) pair per level")
    _, gstride = _f32_levels(gs, c)
    dys = [torch.empty(tuple(y.shape), device=dev, dtype=torch.float32) for y in ys] if dy_out is None else list(dy_out)
    _, dstride = _f32_levels(dys, c)
    _req(gamma, name="gamma")
    if tuple(gamma.shape) != (c,):
        raise ValueError(f"{what}: gamma must hold C values")
    tstride = affines[0][0].stride(0)
    for i, (y, g, dy, (scale, shift), (mean, rstd)) in enumerate(zip(ys, gs, dys, affines, stats)):
        if tuple(g.shape) != tuple(y.shape) or tuple(dy.shape) != tuple(y.shape) or g.device != dev or dy.device != dev:
            raise ValueError(f"{what}: gradients must have the outputs' shapes and device")
        _table_stride(scale, shift, n, c, tstride)
        for t in (mean, rstd):
            if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (n, groups) or not t.is_contiguous():
                raise ValueError(f"{what}: mean / rstd must be dense fp32 GPU [N, groups] tables")
        lv.g[i], lv.dy[i], lv.scale[i], lv.shift[i] = g.data_ptr(), dy.data_ptr(), scale.data_ptr(), shift.data_ptr()
        lv.mean[i], lv.rstd[i] = mean.data_ptr(), rstd.data_ptr()
    d_gamma = torch.empty((c,), device=dev, dtype=torch.float32)
    d_beta = torch.empty((c,), device=dev, dtype=torch.float32)
    ws = _gn_ws(lv, n, c, groups, dev)
    timer = _profile_start()
    check(lib.hn_groupnorm_relu_backward_f32(C.byref(lv), n, c, groups, ystride, gstride, dstride, tstride, ptr(gamma),
                                             ptr(d_gamma), ptr(d_beta), ptr(ws), 4 * ws.numel(), _stream()),
          "hn_groupnorm_relu_backward_f32")
    if timer is not None:
        def describe():
            rows = _rows(ys)
            return ("f32", "gn-bwd"), 0, (1, rows, 1, c, c, 1, 1, 1)
        _profile_stop(timer, describe)
    return dys, d_gamma, d_beta


def conv3x3_wgrad_levels(a16s, dys):
    """Weight and bias gradient of a 3x3 / stride 1 / pad 1 convolution on the f32-input MFMA (hn_conv3x3_wgrad_f32; DESIGN.md
    section 9u): a16s[l] = the S32 inputs the forward read [N,h_l,w_l,Cin/32,2,32], dys[l] = the gradients at its outputs, fp32
    [N,h_l,w_l,Cout]; both may be channel slices; Cin and Cout multiples of 32, at most 512 -> (dW [Cout,3,3,Cin], db [Cout]),
    ONE sum over levels and images.  A dW element is one fmaf chain over the pixels of a K range, then the ranges in order; two
    launches, every element written once, the same bytes on every run."""
    lib = _lib.load()
    _level_count(a16s, "conv3x3_wgrad_levels")
    if len(dys) != len(a16s):
        raise ValueError("conv3x3_wgrad_levels: one gradient per level")
    cin, cout = channels(a16s[0]), dys[0].shape[3] if dys[0].dim() == 4 else -1
    n, astride = _s32_levels(a16s, cin)
    if _f32_levels(dys, cout)[0] != n:
        raise ValueError("conv3x3_wgrad_levels: gradients must have the inputs' batch size")
    dystride = _pixel_stride(dys[0], "dy")
    if cout % 32 or not 0 < cout <= 512 or not 0 < cin <= 512:
        raise ValueError(f"conv3x3_wgrad_levels: Cin and Cout must be multiples of 32, at most 512 (Cin {cin}, Cout {cout})")
    dev = a16s[0].device
    lv = _lib.WgradLevels()
    lv.count = len(a16s)
    for i, (a, dy) in enumerate(zip(a16s, dys)):
        if tuple(dy.shape[1:3]) != tuple(a.shape[1:3]) or dy.device != dev:
            raise ValueError("conv3x3_wgrad_levels: gradients must have the inputs' map sizes and device")
        lv.h[i], lv.w[i], lv.a16[i], lv.dy[i] = a.shape[1], a.shape[2], a.data_ptr(), dy.data_ptr()
    nbytes = lib.hn_conv3x3_wgrad_ws_bytes(C.byref(lv), n, cin, cout)
    if nbytes < 0:
        check(1, "hn_conv3x3_wgrad_ws_bytes")
    ws = _backward_workspace(dev, nbytes)
    dw = torch.empty((cout, 3, 3, cin), device=dev, dtype=torch.float32)
    db = torch.empty((cout,), device=dev, dtype=torch.float32)
    timer = _profile_start()
    check(lib.hn_conv3x3_wgrad_f32(C.byref(lv), n, cin, cout, astride, dystride, ptr(dw), ptr(db), ptr(ws), 4 * ws.numel(),
                                   _stream()), "hn_conv3x3_wgrad_f32")
    if timer is not None:
        def describe():
            rows = _rows(a16s)
            return ("f32", "wgrad"), rows * cout * 9 * cin, (1, rows, 1, cin, cout, 3, 1, 1)
        _profile_stop(timer, describe)
    return dw, db


def conv3x3_dgrad_levels(dys, bank, outs=None, out_channel_offset=0, residuals=None):
    """Input gradient of a 3x3 / stride 1 / pad 1 convolution: the FORWARD convolution of dys[l] (fp32 [N,h_l,w_l,Cout],
    channel slices are fine) with bank = weights.dgrad_bank(w) [Cin,3,3,Cout] on the exact f32-MFMA kernel, one launch per
    level -> fp32 [N,h_l,w_l,Cin] per level, or written into channels out_channel_offset .. + Cin of outs[l].  An element is one
    fmaf chain over its 9 Cout terms.  residuals: per level None or a dense fp32 [N,h_l,w_l,Cin] tensor that the epilogue adds
    after the chain (one more rounding; the FPN's top-down term)."""
    _level_count(dys, "conv3x3_dgrad_levels")
    cin = bank.shape[0]
    if outs is None:
        if out_channel_offset:
            raise ValueError("out_channel_offset needs outs")
        outs = [None] * len(dys)
    elif len(outs) != len(dys):
        raise ValueError("conv3x3_dgrad_levels: one output per level")
    if residuals is None:
        residuals = [None] * len(dys)
    elif len(residuals) != len(dys):
        raise ValueError("conv3x3_dgrad_levels: one residual (or None) per level")
    res = []
    for dy, out, residual in zip(dys, outs, residuals):
        view = None if out is None else out[..., out_channel_offset:out_channel_offset + cin]
        res.append(conv2d_nhwc(dy, bank, None, pad=1, out=view, residual=residual))
    return res


# ---- the backward of the FPN: lateral weight gradient, adjoint of the top-down read (include/handnet_hip_train_fpn.h; 9v) ----
def conv1x1_wgrad(a16, dy):
    """Weight and bias gradient of a 1x1 / stride 1 convolution on the f32-input MFMA (hn_conv1x1_wgrad_f32; DESIGN.md section
    9v): a16 = the S32 input the forward read [N,h,w,Cin/32,2,32], dy = the gradient at its output, fp32 [N,h,w,Cout]; both may
    be channel slices; Cin and Cout multiples of 32, at most 512 -> (dW [Cout,Cin], db [Cout]), ONE sum over images and pixels.
    A dW element is one fmaf chain over the pixels of a K range, then the ranges in order; two launches, every element written
    once, the same bytes on every run."""
    lib = _lib.load()
    if not is_split(a16) or dy.dim() != 4 or dy.dtype != torch.float32:
        raise TypeError("conv1x1_wgrad: a16 must be an S32 tensor [N,h,w,Cin/32,2,32] and dy fp32 [N,h,w,Cout]")
    cin, cout = channels(a16), dy.shape[3]
    if cout % 32 or not 0 < cout <= 512 or not 0 < cin <= 512:
        raise ValueError(f"conv1x1_wgrad: Cin and Cout must be multiples of 32, at most 512 (Cin {cin}, Cout {cout})")
    dev = a16.device
    if tuple(dy.shape[:3]) != tuple(a16.shape[:3]) or dy.device != dev:
        raise ValueError("conv1x1_wgrad: the gradient must have the input's batch size, map size and device")
    rows = _rows([a16])
    if rows == 0:
        raise ValueError("conv1x1_wgrad: empty map")
    n, astride = _s32_levels([a16], cin, "conv1x1_wgrad: a16")
    dystride = _f32_levels([dy], cout)[1]
    nbytes = lib.hn_conv1x1_wgrad_ws_bytes(rows, cin, cout)
    if nbytes < 0:
        check(1, "hn_conv1x1_wgrad_ws_bytes")
    ws = _backward_workspace(dev, nbytes)
    dw = torch.empty((cout, cin), device=dev, dtype=torch.float32)
    db = torch.empty((cout,), device=dev, dtype=torch.float32)
    timer = _profile_start()
    check(lib.hn_conv1x1_wgrad_f32(ptr(a16), ptr(dy), rows, cin, cout, astride, dystride, ptr(dw), ptr(db), ptr(ws), 4 * ws.numel(),
                                   _stream()), "hn_conv1x1_wgrad_f32")
    if timer is not None:
        def describe():
            return ("f32", "wgrad1x1"), rows * cout * cin, (1, rows, 1, cin, cout, 1, 1, 1)
        _profile_stop(timer, describe)
    return dw, db


def upsample_nearest_backward(g, size, out=None):
    """Adjoint of the convolution epilogues' nearest-neighbour read of a coarser map (hn_upsample_nearest_backward_f32; DESIGN.md
    section 9v): g = the gradient at the fine map, fp32 [N,OH,OW,C] (a channel slice is fine), size = (rh, rw) of the coarse map,
    rh <= OH, rw <= OW, C % 4 == 0 -> fp32 [N,rh,rw,C]: out[n,s,t] = the sum of g[n,o,p] over floor(o rh / OH) = s and
    floor(p rw / OW) = t, one fp32 chain in (row, column) order.  out: an fp32 tensor (or channel slice) to write instead of a
    fresh one.  One launch, every element written once."""
    lib = _lib.load()
    if g.dim() != 4 or g.dtype != torch.float32:
        raise TypeError("upsample_nearest_backward: g must be fp32 [N,OH,OW,C]")
    n, c = g.shape[0], g.shape[3]
    rh, rw = (int(v) for v in size)
    if c <= 0 or c % 4:
        raise ValueError(f"upsample_nearest_backward: C must be a multiple of 4 (got {c})")
    if not (0 < rh <= g.shape[1] and 0 < rw <= g.shape[2]):
        raise ValueError(f"upsample_nearest_backward: the coarse map {rh} x {rw} must be non-empty and no larger than the fine "
                         f"map {g.shape[1]} x {g.shape[2]}")
    if n == 0:
        raise ValueError("upsample_nearest_backward: empty batch")
    if out is not None and (out.dim() != 4 or tuple(out.shape) != (n, rh, rw, c) or out.device != g.device):
        raise ValueError("upsample_nearest_backward: out must be fp32 [N,rh,rw,C] on the gradient's device")
    gstride = _f32_levels([g], c)[1]
    if out is None:
        out = torch.empty((n, rh, rw, c), device=g.device, dtype=torch.float32)
    ostride = _f32_levels([out], c)[1]
    timer = _profile_start()
    check(lib.hn_upsample_nearest_backward_f32(ptr(g), n, g.shape[1], g.shape[2], rh, rw, c, gstride, ostride, ptr(out), _stream()),
          "hn_upsample_nearest_backward_f32")
    if timer is not None:
        def describe():
            return ("f32", "upsample-bwd"), 0, (1, _rows([g]), 1, c, c, 1, 1, 1)
        _profile_stop(timer, describe)
    return out


def thin_uses_flat(xs, cw) -> bool:
    """Would conv3x3_thin_levels(xs, cw) run the P-form kernel (True) or the tap kernel (False)?"""
    cout, _, _, cin = cw.w.shape
    return bool(_lib.load().hn_conv3x3_thin_uses_flat(C.byref(_thin_levels_of(xs)), xs[0].shape[0], cin, cout))


def maxpool3x3s2_nhwc(x, out=None):
    lib = _lib.load()
    if is_split(x):
        if not x.is_contiguous():
            raise ValueError("x must be contiguous")
        n, h, w, nb = x.shape[:4]
        oh, ow = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        if out is None:
            out = torch.empty((n, oh, ow, nb, 2, 32), device=x.device, dtype=torch.float16)
        check(lib.hn_maxpool3x3s2_s32(ptr(x), ptr(out), n, h, w, nb * 32, oh, ow, _stream()), "hn_maxpool3x3s2_s32")
        return out
    _req(x, name="x")
    n, h, w, c = x.shape
    oh, ow = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    if out is None:
        out = torch.empty((n, oh, ow, c), device=x.device, dtype=torch.float32)
    check(lib.hn_maxpool3x3s2_nhwc_f32(ptr(x), ptr(out), n, h, w, c, oh, ow, _stream()), "hn_maxpool3x3s2_nhwc_f32")
    return out


def groupnorm_affine(x, gamma, beta, groups=32, eps=1e-5, scratch=None, scale=None, shift=None):
    """x [N,H,W,C] -> (scale [N,C], shift [N,C]) such that GN(x) = x*scale + shift."""
    lib = _lib.load()
    _req(x, name="x"); _req(gamma, name="gamma"); _req(beta, name="beta")
    n, h, w, c = x.shape
    need = lib.hn_groupnorm_scratch_floats(n, h * w, c, groups)
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty((need,), device=x.device, dtype=torch.float32)
    if scale is None:
        scale = torch.empty((n, c), device=x.device, dtype=torch.float32)
    if shift is None:
        shift = torch.empty((n, c), device=x.device, dtype=torch.float32)
    check(lib.hn_groupnorm_affine_f32(ptr(x), ptr(gamma), ptr(beta), n, h * w, c, groups, eps, ptr(scratch),
                                      ptr(scale), ptr(shift), _stream()), "hn_groupnorm_affine_f32")
    return scale, shift


def gn_rows32_scratch_floats(rows, c):
    return _lib.load().hn_groupnorm_rows32_scratch_floats(int(rows), int(c))


def groupnorm_finalize_rows32(partial, gamma, beta, n, hw, groups=32, eps=1e-5, scale=None, shift=None):
    """Partial sums written by conv2d_nhwc(..., gn_partial=partial) -> (scale [N,C], shift [N,C])."""
    lib = _lib.load()
    _req(partial, name="partial"); _req(gamma, name="gamma"); _req(beta, name="beta")
    c = gamma.numel()
    if partial.numel() < lib.hn_groupnorm_rows32_scratch_floats(n * hw, c):
        raise ValueError("partial buffer too small")
    if scale is None:
        scale = torch.empty((n, c), device=partial.device, dtype=torch.float32)
    if shift is None:
        shift = torch.empty((n, c), device=partial.device, dtype=torch.float32)
    check(lib.hn_groupnorm_finalize_rows32(ptr(partial), ptr(gamma), ptr(beta), n, hw, c, groups, eps, ptr(scale),
                                           ptr(shift), _stream()), "hn_groupnorm_finalize_rows32")
    return scale, shift


def groupnorm_finalize_rows32_levels(partials, gamma, beta, n, hws, groups=32, eps=1e-5):
    """groupnorm_finalize_rows32 for all FPN levels of one tower layer in ONE launch -> [(scale, shift)] per level."""
    lib = _lib.load()
    _req(gamma, name="gamma"); _req(beta, name="beta")
    c = gamma.numel()
    lv = _lib.GnLevels()
    lv.count = len(partials)
    tables = torch.empty((len(partials), 2, n, c), device=gamma.device, dtype=torch.float32)
    for i, (part, hw) in enumerate(zip(partials, hws)):
        _req(part, name="partial")
        if part.numel() < lib.hn_groupnorm_rows32_scratch_floats(n * hw, c):
            raise ValueError("partial buffer too small")
        lv.hw[i], lv.partial[i] = hw, part.data_ptr()
        lv.scale[i], lv.shift[i] = tables[i, 0].data_ptr(), tables[i, 1].data_ptr()
    check(lib.hn_groupnorm_finalize_rows32_levels(C.byref(lv), ptr(gamma), ptr(beta), n, c, groups, eps, _stream()),
          "hn_groupnorm_finalize_rows32_levels")
    return [(tables[i, 0], tables[i, 1]) for i in range(len(partials))]


def _split_levels_arg(xs, affines, outs=None):
    """The levels of one apply pass as the library takes them -> (hn_split_levels, n, c, x stride, table stride, out stride, outs).
    xs: fp32 [N,h_l,w_l,C] (channel slices of wider tensors are fine); affines: [(scale, shift)] [N,C] tables; outs: S32
    [N,h_l,w_l,C/32,2,32] destinations (block slices of wider tensors are fine), default fresh dense ones."""
    c = xs[0].shape[3]
    a_stride = affines[0][0].stride(0)
    if len(xs) > _lib.HN_FCOS_MAX_LEVELS or len(affines) != len(xs) or (outs is not None and len(outs) != len(xs)):
        raise ValueError(f"need 1..{_lib.HN_FCOS_MAX_LEVELS} levels with one (scale, shift) pair (and one output) each")
    n, xstride = _f32_levels(xs, c)
    lv = _lib.SplitLevels()
    lv.count = len(xs)
    made = []
    ystride = None
    for i, (x, (scale, shift)) in enumerate(zip(xs, affines)):
        _table_stride(scale, shift, n, c, a_stride)
        if outs is None:
            out = _alloc_out(n, x.shape[1], x.shape[2], c, True, x.device)
        else:
            out = outs[i]
            if not is_split(out) or tuple(out.shape) != (n, x.shape[1], x.shape[2], c // 32, 2, 32) or out.device != x.device:
                raise ValueError("outputs must be S32 tensors [N,h,w,C/32,2,32] of their level's size")
        ys = _pixel_stride(out, "out")
        if ystride is not None and ys != ystride:
            raise ValueError("outputs must share one pixel stride")
        ystride = ys
        lv.hw[i] = x.shape[1] * x.shape[2]
        lv.x[i], lv.scale[i], lv.shift[i], lv.y16[i] = x.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr()
        made.append(out)
    return lv, n, c, xstride, a_stride, ystride, made


def to_split_levels(xs, affines, relu=True, outs=None):
    """to_split(x, scale, shift, relu) for the FPN levels of one tower layer in ONE launch (per-level launches when a
    level is too large for the caches, decided by the library).  xs: fp32 [N,h_l,w_l,C]; affines: [(scale, shift)];
    outs: optional preallocated S32 destinations (e.g. one tower's blocks of the stacked operand)."""
    lib = _lib.load()
    lv, n, c, xstride, a_stride, ystride, outs = _split_levels_arg(xs, affines, outs)
    check(lib.hn_affine_split_f32_levels(C.byref(lv), 1 if relu else 0, n, c, xstride, a_stride, ystride, _stream()),
          "hn_affine_split_f32_levels")
    return outs


def split_levels_stream(n, hws, c) -> bool:
    """Is the apply pass of these levels an HBM stream (a level beyond the caches: the library runs per-level launches with
    streaming stores)?  The threshold at which FCOSEngine.heads_grouped lets the tower convolutions carry the pass."""
    arr = (C.c_int32 * len(hws))(*[int(v) for v in hws])
    return bool(_lib.load().hn_affine_split_f32_levels_streams(arr, len(hws), int(n), int(c)))


def _device_readable(t: torch.Tensor, name: str):
    """A raw input buffer of ingest_raw: device memory of the current GPU, or PINNED host memory (the kernel reads it over
    PCIe itself).  Pageable host memory is not readable by the device: the caller stages it (HandNet.forward_raw does)."""
    if t.is_cuda:
        _check_device(t, name)
    elif not t.is_pinned():
        raise RuntimeError(f"{name}: host memory must be pinned (tensor.pin_memory()) to be read by the ingest kernel")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def ingest_raw(bgr_u8, depth=None, device=None, out_rgb=None, out_depth=None, out_rgbd=None, want_rgbd=False, want_depth=True,
               flip_w=False):
    """The reference caller's host-side conversions as ONE kernel (hn_ingest_u8bgr_u16mm; ros_demo.py:227-231,266-269):
    bgr_u8 uint8 [N,H,W,3] (cv_bridge 'bgr8' frames), depth [N,H,W] uint16 / int16 millimetres (16UC1) or float32 metres
    (32FC1), each on the GPU or in PINNED host memory -> (rgb fp32 [N,3,H,W] in 0..1, depth fp32 [N,1,H,W] metres or None,
    rgbd fp32 [N,4,H,W] or None) on the GPU; bit-identical to `astype(float32) / 255.0` and `/ 1000.0`.
    want_depth=False (with an RGB-D output): the separate depth map is neither allocated nor written.
    flip_w: the caller's `left` mode (cv2.flip(., 1) of frame and depth, ros_demo.py:259-262) in the same launch
    (hn_ingest_u8bgr_u16mm_flip): every output is the one of the arrays flipped along the width axis, bit for bit."""
    if bgr_u8.dtype != torch.uint8 or bgr_u8.dim() != 4 or bgr_u8.shape[3] != 3:
        raise TypeError(f"bgr_u8: expected uint8 [N,H,W,3], got {bgr_u8.dtype} {tuple(bgr_u8.shape)}")
    _device_readable(bgr_u8, "bgr_u8")
    n, h, w, _ = bgr_u8.shape
    kind = 0
    if depth is not None:
        if depth.dtype in (torch.uint16, torch.int16):
            kind = 1        # (int16: the same bits; 16UC1 is unsigned and the kernel reads it so)
        elif depth.dtype == torch.float32:
            kind = 2
        else:
            raise TypeError(f"depth: expected uint16 / int16 millimetres or float32 metres, got {depth.dtype}")
        if tuple(depth.shape) not in ((n, h, w), (n, 1, h, w)):
            raise ValueError(f"depth: expected [N,H,W] matching the frames, got {tuple(depth.shape)}")
        _device_readable(depth, "depth")
    if device is None:
        device = bgr_u8.device if bgr_u8.is_cuda else torch.device("cuda", _cur_device() if _cur_device else 0)
    if out_rgb is None:
        out_rgb = torch.empty((n, 3, h, w), device=device, dtype=torch.float32)
    if want_rgbd and out_rgbd is None:
        if not kind:
            raise ValueError("the RGB-D tensor needs a depth input")
        out_rgbd = torch.empty((n, 4, h, w), device=device, dtype=torch.float32)
    if kind and out_depth is None and (want_depth or out_rgbd is None):
        out_depth = torch.empty((n, 1, h, w), device=device, dtype=torch.float32)
    for t, nm in ((out_rgb, "out_rgb"), (out_depth, "out_depth"), (out_rgbd, "out_rgbd")):
        if t is not None:
            _req(t, name=nm)
    args = (bgr_u8.data_ptr(), depth.data_ptr() if kind else None, kind, ptr(out_rgb),
            ptr(out_depth) if (kind and out_depth is not None) else None, ptr(out_rgbd), n, h, w)
    if flip_w:
        check(_lib.load().hn_ingest_u8bgr_u16mm_flip(*args, 1, _stream()), "hn_ingest_u8bgr_u16mm_flip")
    else:
        check(_lib.load().hn_ingest_u8bgr_u16mm(*args, _stream()), "hn_ingest_u8bgr_u16mm")
    return out_rgb, (out_depth if kind else None), out_rgbd


def flip_w(x, other=None, out=None, out_other=None):
    """x [..., W] fp32 mirrored along its last axis (x.flip(-1), bit for bit) in ONE launch (hn_flip_w_f32) -- and `other`
    (same W) with it in the same launch: the frames and the depth map of a `left` live step fed with fp32 tensors.  Returns
    out, or (out, out_other) when `other` is given.  Not in place."""
    _req(x, name="x")
    w = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    _req(out, name="out")
    if out.shape != x.shape or out.data_ptr() == x.data_ptr():
        raise ValueError("out must have x's shape and its own memory")
    rows_b = 0
    if other is not None:
        _req(other, name="other")
        if other.shape[-1] != w:
            raise ValueError("other must have x's width")
        if out_other is None:
            out_other = torch.empty_like(other)
        _req(out_other, name="out_other")
        if out_other.shape != other.shape or out_other.data_ptr() == other.data_ptr():
            raise ValueError("out_other must have other's shape and its own memory")
        rows_b = other.numel() // w
    if x.numel():
        check(_lib.load().hn_flip_w_f32(ptr(x), ptr(out), x.numel() // w, ptr(other) if rows_b else None,
                                        ptr(out_other) if rows_b else None, rows_b, w, _stream()), "hn_flip_w_f32")
    return out if other is None else (out, out_other)


def fcos_preprocess(images, oh, ow, ph, pw, mean, std, out=None):
    """images [N,3,H,W] fp32 (0..1) -> [N,ph,pw,4] normalized / resized / padded NHWC."""
    lib = _lib.load()
    _req(images, name="images")
    n, c, h, w = images.shape
    if c != 3:
        raise ValueError("images must be [N,3,H,W]")
    if out is None:
        out = torch.empty((n, ph, pw, 4), device=images.device, dtype=torch.float32)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    check(lib.hn_fcos_preprocess_f32(ptr(images), ptr(out), n, h, w, oh, ow, ph, pw, m, s, _stream()),
          "hn_fcos_preprocess_f32")
    return out


def fcos_preprocess_split(images, oh, ow, ph, pw, mean, std, border=3, out=None):
    """images [N,3,H,W] fp32 (0..1) -> stem image: fp16 [2 (hi, lo), N, ph+2b, pw+2b, 4], zero border b."""
    lib = _lib.load()
    _req(images, name="images")
    n, c, h, w = images.shape
    if c != 3:
        raise ValueError("images must be [N,3,H,W]")
    if out is None:
        out = torch.empty((2, n, ph + 2 * border, pw + 2 * border, 4), device=images.device, dtype=torch.float16)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    check(lib.hn_fcos_preprocess_split(ptr(images), ptr(out), n, h, w, oh, ow, ph, pw, border, m, s, _stream()),
          "hn_fcos_preprocess_split")
    return out


def fcos_preprocess_list(images, geom, ph, pw, mean, std, split=True, border=3):
    """Differently sized images (torchvision batch_images): images = list of fp32 GPU [3,h_i,w_i] tensors,
    geom = [(h_i, w_i, oh_i, ow_i)] -> the common canvas (stem image when split, else fp32 [N,ph,pw,4])."""
    lib = _lib.load()
    n = len(images)
    if n == 0 or len(geom) != n:
        raise ValueError("need one geometry row per image")
    keep = []
    for i, (img, (h, w, oh, ow)) in enumerate(zip(images, geom)):
        img = _req(img.float().contiguous(), name=f"images[{i}]")
        if tuple(img.shape) != (3, h, w) or oh > ph or ow > pw or min(h, w, oh, ow) <= 0:
            raise ValueError(f"images[{i}]: shape {tuple(img.shape)} does not match its geometry {(h, w, oh, ow)} "
                             f"or exceeds the canvas {(ph, pw)}")
        keep.append(img)
    dev = keep[0].device
    ptrs = torch.tensor([t.data_ptr() for t in keep], dtype=torch.int64).to(dev)
    gtab = torch.tensor([list(g) for g in geom], dtype=torch.int32).to(dev)
    if split:
        out = torch.empty((2, n, ph + 2 * border, pw + 2 * border, 4), device=dev, dtype=torch.float16)
    else:
        out = torch.empty((n, ph, pw, 4), device=dev, dtype=torch.float32)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    check(lib.hn_fcos_preprocess_list(ptr(ptrs), ptr(gtab), ptr(out), 1 if split else 0, n, ph, pw, border, m, s,
                                      _stream()), "hn_fcos_preprocess_list")
    # the kernel reads `keep` / the tables asynchronously: tie their lifetime to the output
    out._hn_sources = (keep, ptrs, gtab)
    return out


def _stem_sizes(x16, w16, cout, r, stride):
    """Stem image and packed filter bank of a stem launch -> (N, image height, image width, border, conv output height, width)."""
    pad = r // 2
    if x16.dim() != 5 or x16.shape[0] != 2 or x16.shape[4] != 4 or x16.dtype != torch.float16 or not x16.is_cuda \
            or not x16.is_contiguous():
        raise ValueError("x16 must be the contiguous fp16 GPU stem image [2, N, H+2p, W+2p, 4]")
    n, hb, wb = x16.shape[1:4]
    if tuple(w16.shape) != (cout, r, 2, 32) or w16.dtype != torch.float16 or not w16.is_cuda or not w16.is_contiguous():
        raise ValueError("w16 must be the fp16 GPU tensor [cout, r, 2, 32] from weights.pack_stem_split")
    return n, hb - 2 * pad, wb - 2 * pad, pad, (hb - r) // stride + 1, (wb - r) // stride + 1


def conv_stem_split(x16, w16, bias, cout, r=7, stride=2, relu=True, out_split=True, algo_cin=3, out=None):
    """Stem conv on the f16x3 kernel.  x16: stem image from fcos_preprocess_split (border = r // 2);
    w16: weights.pack_stem_split(...).w16.  -> [N, oh, ow, cout] fp32 or S32."""
    lib = _lib.load()
    n, ph, pw, pad, oh, ow = _stem_sizes(x16, w16, cout, r, stride)
    if out is None:
        out = _alloc_out(n, oh, ow, cout, out_split, x16.device)
    timer = _profile_start()
    check(lib.hn_conv_stem_f16x3(ptr(x16), n, ph, pw, pad, r, stride, cout, ptr(w16), ptr(bias), 1 if relu else 0,
                                 ptr(out), 1 if is_split(out) else 0, _stream()), "hn_conv_stem_f16x3")
    if timer is not None:
        tile = 4 if cout <= 32 else (2 if cout <= 64 else 1)  # HN_TILE_128x32 / 128x64 / 128x128
        _profile_stop(timer, lambda: (("f16x3", tile), n * oh * ow * cout * r * r * algo_cin, (n, ph, pw, 4, cout, r, stride, 1)))
    return out


def conv_stem_pool_split(x16, w16, bias, cout=64, r=7, stride=2, algo_cin=3, out=None):
    """Stem conv + ReLU + 3x3/2 max pooling in ONE kernel (hn_conv_stem_pool_f16x3): stem image -> pooled S32 map
    [N, (oh+1)//2, (ow+1)//2, cout/32, 2, 32].  from_split of it is bit-identical to from_split of conv_stem_split(...) followed
    by maxpool3x3s2_nhwc; the planes are identical too, except where a pooling window holds two fp32 values either side of an
    fp16 rounding midpoint whose (hi, lo) pairs recombine to the same sum: this kernel splits the maximum, the unfused pooling
    copies the first such pair (tests/test_stem_gpu.py, equal-sum pairs)."""
    lib = _lib.load()
    n, ph, pw, pad, oh, ow = _stem_sizes(x16, w16, cout, r, stride)
    _check_device(x16, "x16")
    if out is None:
        out = _alloc_out(n, (oh + 2 - 3) // 2 + 1, (ow + 2 - 3) // 2 + 1, cout, True, x16.device)
    timer = _profile_start()
    check(lib.hn_conv_stem_pool_f16x3_terms(ptr(x16), n, ph, pw, pad, r, stride, cout, ptr(w16), ptr(bias), ptr(out),
                                            1 if F16_TERMS == 1 else 3, _stream()), "hn_conv_stem_pool_f16x3_terms")
    if timer is not None:
        # algorithmic work = the stem convolution as the reference executes it (the patch halo is overhead, not work)
        _profile_stop(timer, lambda: (("f16x3", 8), n * oh * ow * cout * r * r * algo_cin, (n, ph, pw, 4, cout, r, stride, 1)))
    return out


@dataclass
class Candidates:
    boxes: torch.Tensor
    scores: torch.Tensor
    labels: torch.Tensor
    sides: torch.Tensor
    level: torch.Tensor
    count: torch.Tensor
    point: torch.Tensor = None  # anchor-point index of each candidate (row of the [P, ...] head tensors)


@dataclass
class Detections:
    boxes: torch.Tensor
    scores: torch.Tensor
    labels: torch.Tensor
    sides: torch.Tensor
    level: torch.Tensor
    keep: torch.Tensor
    count: torch.Tensor


def _zero_fields(n, cap, device, widths, zero=True):
    """One zero-filled allocation carved into [n, cap(, w)] fields + an [n] counter (a torch.zeros per field was 14
    fill launches per detector pass: 65 us of the 2.8 ms batch-1 step, profiles/r03_b1_timeline.txt).  Every field is
    4 bytes wide; int fields are int32 views of the fp32 buffer."""
    words = sum(widths) * n * cap + n
    flat = (torch.zeros if zero else torch.empty)((words,), device=device, dtype=torch.float32)
    out, off = [], 0
    for w in widths:
        t = flat[off:off + n * cap * w]
        out.append(t.view(n, cap, w) if w > 1 else t.view(n, cap))
        off += n * cap * w
    out.append(flat[off:off + n])
    return out


def alloc_candidates(n, cap, device) -> Candidates:
    # internal to the detector (rows beyond count[i] are never read; hn_fcos_candidates* writes every count): no fill launch
    b, s, l, sd, lv, pt, cnt = _zero_fields(n, cap, device, [4, 1, 1, 1, 1, 1], zero=False)
    i32 = torch.int32
    return Candidates(b, s, l.view(i32), sd.view(i32), lv.view(i32), cnt.view(i32), pt.view(i32))


def alloc_detections(n, cap, device, zero=True) -> Detections:
    """zero=False: no fill launch -- rows at or beyond count[i] are then undefined (hn_fcos_nms writes every count and the
    rows below it; the engines, which only ever read those, allocate this way: one launch fewer per detector pass)."""
    b, s, l, sd, lv, kp, cnt = _zero_fields(n, cap, device, [4, 1, 1, 1, 1, 1], zero=zero)
    i32 = torch.int32
    return Detections(b, s, l.view(i32), sd.view(i32), lv.view(i32), kp.view(i32), cnt.view(i32))


CANDIDATES_CHUNKED = True   # development switch (forms.apply_env): hn_fcos_candidates_ws vs one workgroup per image


def fcos_candidates(cls_lr, reg_ctr, strides, num_classes, score_thresh=0.7, out: Candidates | None = None):
    """cls_lr[l] [N,h,w,C+2], reg_ctr[l] [N,h,w,5] per level -> ordered candidates (hn_fcos_candidates_ws: the points of
    an image spread over 1024-point workgroups; identical output to the one-workgroup form)."""
    lib = _lib.load()
    lv = FcosLevels()
    lv.num_levels = len(cls_lr)
    n = cls_lr[0].shape[0]
    cap = 0
    for i, (a, b, st) in enumerate(zip(cls_lr, reg_ctr, strides)):
        _req(a, name="cls_lr"); _req(b, name="reg_ctr")
        if a.shape[3] != num_classes + 2 or b.shape[3] != 5 or a.shape[:3] != b.shape[:3]:
            raise ValueError("bad head tensor shapes")
        lv.h[i], lv.w[i], lv.stride[i] = a.shape[1], a.shape[2], int(st)
        lv.cls_lr[i], lv.reg_ctr[i] = a.data_ptr(), b.data_ptr()
        cap += a.shape[1] * a.shape[2]
    if out is None:
        out = alloc_candidates(n, cap, cls_lr[0].device)
    points, cap = cap, out.scores.shape[1]
    if CANDIDATES_CHUNKED:
        nbytes = lib.hn_fcos_candidates_ws_bytes(n, points)
        ws = torch.empty((nbytes // 4,), device=cls_lr[0].device, dtype=torch.int32)
        check(lib.hn_fcos_candidates_ws(C.byref(lv), n, num_classes, score_thresh, ptr(out.boxes), ptr(out.scores),
                                        ptr(out.labels), ptr(out.sides), ptr(out.level),
                                        ptr(out.point) if out.point is not None else None, ptr(out.count), cap,
                                        ptr(ws), nbytes, _stream()), "hn_fcos_candidates_ws")
        return out
    check(lib.hn_fcos_candidates(C.byref(lv), n, num_classes, score_thresh, ptr(out.boxes), ptr(out.scores),
                                 ptr(out.labels), ptr(out.sides), ptr(out.level),
                                 ptr(out.point) if out.point is not None else None, ptr(out.count), cap, _stream()),
          "hn_fcos_candidates")
    return out


def fcos_ext_gather(ext, det: "Detections", cand: Candidates, *, out=None):
    """ext[l] [N,h,w,8] raw (relu(dxdy)[3], contact[5]) per level -> (contacts [N,cap] int32,
    dxdymags [N,cap,3] fp32) for the kept detections (fcos.py:299-320,605-607,631-647).  out: the caller's (contacts, dxdymags)
    to write into -- no allocation and no zero fill here, so rows at and beyond count[i] keep what they held (a captured step
    passes its own buffers); without it both are allocated and zero-filled, as ever."""
    lib = _lib.load()
    if cand.point is None:
        raise ValueError("candidates were produced without anchor-point indices")
    lv = FcosLevels()
    lv.num_levels = len(ext)
    arr = (C.c_void_p * len(ext))()
    for i, e in enumerate(ext):
        _req(e, name="ext")
        if e.shape[3] != 8:
            raise ValueError("ext tensors must be [N,h,w,8]")
        lv.h[i], lv.w[i], lv.stride[i] = e.shape[1], e.shape[2], 1
        arr[i] = e.data_ptr()
    n, cap = det.scores.shape
    if sum(e.shape[1] * e.shape[2] for e in ext) != cand.scores.shape[1] or cand.scores.shape[1] != cap:
        raise ValueError("ext levels do not match the candidate capacity")
    if out is None:
        contacts = torch.zeros((n, cap), device=det.scores.device, dtype=torch.int32)
        dxdymags = torch.zeros((n, cap, 3), device=det.scores.device, dtype=torch.float32)
    else:
        contacts, dxdymags = out
        _req(contacts, torch.int32, "out contacts"); _req(dxdymags, name="out dxdymags")
        if tuple(contacts.shape) != (n, cap) or tuple(dxdymags.shape) != (n, cap, 3) or contacts.device != det.scores.device \
                or dxdymags.device != det.scores.device:
            raise ValueError(f"out: (contacts int32 [{n},{cap}], dxdymags fp32 [{n},{cap},3]) on {det.scores.device}, got "
                             f"{tuple(contacts.shape)} on {contacts.device} and {tuple(dxdymags.shape)} on {dxdymags.device}")
    check(lib.hn_fcos_ext_gather(C.byref(lv), arr, ptr(det.keep), ptr(cand.point), ptr(det.count), n, cap,
                                 ptr(contacts), ptr(dxdymags), _stream()), "hn_fcos_ext_gather")
    return contacts, dxdymags


FCOS_MAX_GT = 64            # HN_FCOS_MAX_GT: ground-truth rows per image
FCOS_LOSS_KEYS = ("classification", "bbox_regression", "bbox_ctrness", "hand_lr", "hand_contact_state", "hand_dxdy")


@dataclass
class FcosTargets:
    """The criterion's ground truth as padded device tables (pack_fcos_targets)."""
    boxes: torch.Tensor     # [N, G, 4] fp32, scaled to the canvas
    labels: torch.Tensor    # [N, G] int32
    info: torch.Tensor      # [N, G, 5] fp32 = (contactstate, handside, mag, dx, dy)
    count: torch.Tensor     # [N] int32


@dataclass
class FcosLoss:
    terms: torch.Tensor     # [N, 6] fp32: per-image sums before any factor or division, FCOS_LOSS_KEYS order
    fg: torch.Tensor        # [N] int32: foreground points
    losses: torch.Tensor    # [6] fp32: the dict values of the batch
    matched: torch.Tensor = None   # [N, P] int32: each point's ground-truth row or -1 (want_matched)


def fcos_target_ratios(original_sizes, new_sizes):
    """per image (ratio_h, ratio_w) = float32(new) / float32(original), the float32 division of torchvision's resize_boxes
    (FCOSEngine.detect divides the other way round for the detections)"""
    f = np.float32
    return [(f(nh) / f(oh), f(nw) / f(ow)) for (oh, ow), (nh, nw) in zip(original_sizes, new_sizes)]


def pack_fcos_targets(targets, ratios, G=None, *, num_classes=None, ext=False, device=None) -> FcosTargets:
    """The reference's list of target dicts ('boxes' [M,4] in image pixels, 'labels' [M], 'box_info' [M,5]) -> FcosTargets.
    ratios: one (ratio_h, ratio_w) pair for every image or one pair per image (fcos_target_ratios); the boxes are scaled in
    float32 on the host, box * ratio per axis, as torchvision's transform scales them.  Refused here, before anything reaches
    the device: a box that is degenerate after scaling (the reference drops the box and keeps its label, which misaligns the
    two), a label outside [0, num_classes) (when num_classes is given), more than FCOS_MAX_GT boxes in an image, and, with ext,
    an image without boxes (the reference raises KeyError('hand_contact_state') there, fcos.py:75)."""
    f = np.float32
    n = len(targets)
    if n == 0:
        raise ValueError("pack_fcos_targets: no images")
    if len(ratios) == 2 and not isinstance(ratios[0], (tuple, list, np.ndarray)):
        ratios = [ratios] * n
    if len(ratios) != n:
        raise ValueError("pack_fcos_targets: one (ratio_h, ratio_w) pair per image")
    host = lambda t, dt: (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dt)
    rows = []
    for i, (t, (rh, rw)) in enumerate(zip(targets, ratios)):
        boxes, labels = host(t["boxes"], f).reshape(-1, 4), host(t["labels"], np.int64).reshape(-1)
        info = host(t["box_info"], f).reshape(-1, 5) if "box_info" in t else np.zeros((len(labels), 5), f)
        if not (len(boxes) == len(labels) == len(info)):
            raise ValueError(f"image {i}: boxes, labels and box_info differ in length")
        if len(labels) > FCOS_MAX_GT:
            raise ValueError(f"image {i}: {len(labels)} boxes, more than {FCOS_MAX_GT}")
        if ext and len(labels) == 0:
            raise KeyError("hand_contact_state")
        boxes = (boxes * np.array([rw, rh, rw, rh], f)[None, :]).astype(f)
        if len(boxes) and ((boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])).any():
            raise ValueError(f"image {i}: a degenerate box (x1 <= x0 or y1 <= y0 after scaling)")
        if num_classes is not None and len(labels) and (labels.min() < 0 or labels.max() >= num_classes):
            raise ValueError(f"image {i}: a label outside [0, {num_classes})")
        rows.append((boxes, labels.astype(np.int32), info))
    most = max(len(r[1]) for r in rows)
    G = max(1, most) if G is None else int(G)
    if G < max(1, most) or G > FCOS_MAX_GT:
        raise ValueError(f"G = {G} outside {max(1, most)}..{FCOS_MAX_GT}")
    tb, tl, ti, tc = np.zeros((n, G, 4), f), np.zeros((n, G), np.int32), np.zeros((n, G, 5), f), np.zeros((n,), np.int32)
    for i, (b, l, info) in enumerate(rows):
        k = len(l)
        tb[i, :k], tl[i, :k], ti[i, :k], tc[i] = b, l, info, k
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    up = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
    return FcosTargets(up(tb), up(tl), up(ti), up(tc))


def alloc_fcos_loss(n, points, device, want_matched=False) -> FcosLoss:
    return FcosLoss(torch.empty((n, 6), device=device, dtype=torch.float32), torch.empty((n,), device=device, dtype=torch.int32),
                    torch.empty((6,), device=device, dtype=torch.float32),
                    torch.empty((n, points), device=device, dtype=torch.int32) if want_matched else None)


def _fcos_loss_args(cls_lr, reg_ctr, strides, num_classes, targets, ext, want_matched, out):
    """The argument checks fcos_loss and fcos_loss_grad share -> (level table, ext pointer array or None, n, points, G, out,
    workspace, its bytes); every refusal happens here, before a launch."""
    lib = _lib.load()
    nl = len(cls_lr)
    if nl == 0 or len(reg_ctr) != nl or len(strides) != nl or (ext is not None and len(ext) != nl):
        raise ValueError("fcos_loss: cls_lr, reg_ctr, strides and ext must have one entry per level")
    if not 1 <= int(num_classes) <= 8:
        raise ValueError(f"fcos_loss: num_classes = {num_classes} outside 1..8")
    lv = FcosLevels()
    lv.num_levels = nl
    n = cls_lr[0].shape[0]
    points = 0
    arr = (C.c_void_p * nl)() if ext is not None else None
    for i, (a, b, st) in enumerate(zip(cls_lr, reg_ctr, strides)):
        _req(a, name="cls_lr"); _req(b, name="reg_ctr")
        if a.dim() != 4 or a.shape[0] != n or a.shape[3] != num_classes + 2 or b.shape[3] != 5 or a.shape[:3] != b.shape[:3]:
            raise ValueError("bad head tensor shapes")
        if ext is not None:
            if tuple(_req(ext[i], name="ext").shape) != tuple(a.shape[:3]) + (8,):
                raise ValueError("ext tensors must be [N,h,w,8] on the levels of cls_lr")
            arr[i] = ext[i].data_ptr()
        lv.h[i], lv.w[i], lv.stride[i] = a.shape[1], a.shape[2], int(st)
        lv.cls_lr[i], lv.reg_ctr[i] = a.data_ptr(), b.data_ptr()
        points += a.shape[1] * a.shape[2]
    _req(targets.boxes, name="targets.boxes"); _req(targets.info, name="targets.info")
    _req(targets.labels, torch.int32, "targets.labels"); _req(targets.count, torch.int32, "targets.count")
    g = targets.boxes.shape[1] if targets.boxes.dim() == 3 else 0
    if not 1 <= g <= FCOS_MAX_GT:
        raise ValueError(f"fcos_loss: G = {g} outside 1..{FCOS_MAX_GT}")
    if (tuple(targets.boxes.shape) != (n, g, 4) or tuple(targets.labels.shape) != (n, g) or tuple(targets.info.shape) != (n, g, 5)
            or tuple(targets.count.shape) != (n,)):
        raise ValueError("fcos_loss: targets must be boxes [N,G,4], labels [N,G], info [N,G,5], count [N]")
    dev = cls_lr[0].device
    if out is None:
        out = alloc_fcos_loss(n, points, dev, want_matched)
    else:
        _req(out.terms, name="out.terms"); _req(out.fg, torch.int32, "out.fg"); _req(out.losses, name="out.losses")
        if tuple(out.terms.shape) != (n, 6) or tuple(out.fg.shape) != (n,) or tuple(out.losses.shape) != (6,):
            raise ValueError("out must be terms [N,6], fg [N], losses [6]")
        if want_matched and (out.matched is None or tuple(_req(out.matched, torch.int32, "out.matched").shape) != (n, points)):
            raise ValueError("out.matched must be int32 [N,P]")
    nbytes = lib.hn_fcos_loss_ws_bytes(n, points)
    ws = torch.empty((nbytes // 8,), device=dev, dtype=torch.float64)
    return lv, arr, n, points, g, out, ws, nbytes


def _fcos_loss_call(entry, name, num_classes, n, points, g, launch):
    """the profile bracket fcos_loss and fcos_loss_grad share: stage "fcos_loss", one record under `name`"""
    global PROFILE_STAGE
    prev, PROFILE_STAGE = PROFILE_STAGE, "fcos_loss"
    try:
        timer = _profile_start()
        check(launch(), entry)
        if timer is not None:
            _profile_stop(timer, lambda: (("f32", name), 0, (n, points, int(num_classes), g)))
    finally:
        PROFILE_STAGE = prev


def fcos_loss(cls_lr, reg_ctr, strides, num_classes, targets: FcosTargets, ext=None, radius=1.5, want_matched=False,
              out: FcosLoss | None = None) -> FcosLoss:
    """The FCOS criterion's forward on the detector's head tensors (hn_fcos_loss_f32; fcos_utils/fcos.py:44-178,523-570,
    DESIGN.md section 9p): cls_lr[l] [N,h,w,C+2], reg_ctr[l] [N,h,w,5] and, for the ext terms, ext[l] [N,h,w,8] per level;
    targets as pack_fcos_targets builds them (boxes already on the canvas's scale) -> FcosLoss, everything on the device and
    nothing waited for.  Two launches with a fixed summation order: the same bytes on every run, and row i of a batch is the
    row of image i alone.  Every refusal happens before a launch.  The backward at the heads is fcos_loss_grad."""
    lib = _lib.load()
    lv, arr, n, points, g, out, ws, nbytes = _fcos_loss_args(cls_lr, reg_ctr, strides, num_classes, targets, ext, want_matched, out)
    _fcos_loss_call("hn_fcos_loss_f32", "fcos_loss", num_classes, n, points, g, lambda: lib.hn_fcos_loss_f32(
        C.byref(lv), arr, n, int(num_classes), ptr(targets.boxes), ptr(targets.labels), ptr(targets.info), ptr(targets.count), g,
        float(radius), ptr(out.terms), ptr(out.fg), ptr(out.losses), ptr(out.matched) if want_matched else None, ptr(ws), nbytes,
        _stream()))
    return out


def fcos_loss_grad(cls_lr, reg_ctr, strides, num_classes, targets: FcosTargets, ext=None, radius=1.5, upstream=None,
                   want_forward=False, out=None):
    """The FCOS criterion's backward at the detector heads (hn_fcos_loss_grad_f32): fcos_loss's arguments
    and refusals -> per-level lists (d_cls_lr, d_reg_ctr, d_ext or None), the gradient of sum_k upstream[k] * losses[k] at the
    tensors as they are handed in (the regressions and the ext (mag, dx, dy) are a ReLU's outputs: the gradient is at those
    outputs).  upstream: six fp32 weights ON THE DEVICE in FCOS_LOSS_KEYS order (None: ones; without ext [4:] is ignored); the
    kernel reads them, so the call sits inside a captured step.  The matching and the divisor max(1, sum fg) are constants.
    The forward's two launches, then one more; every element is written once, the same bytes on every run.  want_forward: also
    return the FcosLoss, the bytes fcos_loss gives.  out: (d_cls_lr, d_reg_ctr, d_ext or None) lists to write into."""
    lib = _lib.load()
    lv, arr, n, points, g, res, ws, nbytes = _fcos_loss_args(cls_lr, reg_ctr, strides, num_classes, targets, ext, False, None)
    dev = cls_lr[0].device
    if upstream is not None and (tuple(_req(upstream, name="upstream").shape) != (6,) or upstream.device != dev):
        raise ValueError("fcos_loss_grad: upstream must be fp32 [6] on the heads' device")
    heads = (cls_lr, reg_ctr, ext)
    if out is None:
        out = tuple(None if h is None else [torch.empty_like(t) for t in h] for h in heads)
    else:
        if len(out) != 3 or (out[2] is None) != (ext is None):
            raise ValueError("fcos_loss_grad: out must be (d_cls_lr, d_reg_ctr, d_ext or None)")
        for h, o in zip(heads, out):
            if h is not None and (len(o) != len(h) or any(_req(t, name="out").shape != s.shape or t.device != dev for t, s in zip(o, h))):
                raise ValueError("fcos_loss_grad: out must hold tensors of the heads' shapes on their device")
    nl = len(cls_lr)
    arrays = [None if o is None else (C.c_void_p * nl)(*[t.data_ptr() for t in o]) for o in out]
    _fcos_loss_call("hn_fcos_loss_grad_f32", "fcos_loss_grad", num_classes, n, points, g, lambda: lib.hn_fcos_loss_grad_f32(
        C.byref(lv), arr, n, int(num_classes), ptr(targets.boxes), ptr(targets.labels), ptr(targets.info), ptr(targets.count), g,
        float(radius), ptr(res.terms), ptr(res.fg), ptr(res.losses), None, ptr(ws), nbytes, ptr(upstream), arrays[0], arrays[1],
        arrays[2], _stream()))
    grads = (out[0], out[1], out[2])
    return grads + (res,) if want_forward else grads


def fcos_nms(cand: Candidates, iou_thresh, ratio_h, ratio_w, scratch=None, out: Detections | None = None,
             ratios=None):
    """ratios: optional fp32 GPU [N,2] = (ratio_h, ratio_w) per image (batches of differently sized images);
    otherwise the scalar pair applies to every image."""
    lib = _lib.load()
    n, cap = cand.scores.shape
    _check_device(cand.scores, "candidates")
    need = lib.hn_fcos_nms_scratch_bytes(n, cap)
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty((need,), device=cand.scores.device, dtype=torch.uint8)
    if out is None:
        out = alloc_detections(n, cap, cand.scores.device)
    if ratios is not None:
        _req(ratios, name="ratios")
        if tuple(ratios.shape) != (n, 2):
            raise ValueError("ratios must be [N,2]")
        check(lib.hn_fcos_nms_ratios(ptr(cand.boxes), ptr(cand.scores), ptr(cand.labels), ptr(cand.sides),
                                     ptr(cand.level), ptr(cand.count), n, cap, float(iou_thresh), ptr(ratios),
                                     ptr(scratch), ptr(out.boxes), ptr(out.scores), ptr(out.labels), ptr(out.sides),
                                     ptr(out.level), ptr(out.keep), ptr(out.count), _stream()), "hn_fcos_nms_ratios")
        return out
    check(lib.hn_fcos_nms(ptr(cand.boxes), ptr(cand.scores), ptr(cand.labels), ptr(cand.sides), ptr(cand.level),
                          ptr(cand.count), n, cap, float(iou_thresh), float(ratio_h), float(ratio_w), ptr(scratch),
                          ptr(out.boxes), ptr(out.scores), ptr(out.labels), ptr(out.sides), ptr(out.level),
                          ptr(out.keep), ptr(out.count), _stream()), "hn_fcos_nms")
    return out


def nms(boxes, scores, iou_thresh):
    """torchvision.ops.nms semantics: indices of kept boxes, descending score."""
    lib = _lib.load()
    _req(boxes, name="boxes"); _req(scores, name="scores")
    k = boxes.shape[0]
    if k == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    scratch = torch.empty((lib.hn_fcos_nms_scratch_bytes(1, k),), device=boxes.device, dtype=torch.uint8)
    keep = torch.empty((k,), device=boxes.device, dtype=torch.int32)
    cnt = torch.zeros((1,), device=boxes.device, dtype=torch.int32)
    check(lib.hn_nms(ptr(boxes), ptr(scores), k, float(iou_thresh), ptr(scratch), ptr(keep), ptr(cnt), _stream()),
          "hn_nms")
    return keep[: int(cnt.item())].to(torch.int64)


def crop_resize(det: Detections, hand_label, depth, out_size=176, cpad=4, crop_box=None, has_hand=None, crops=None,
                reorder_bgr=False):
    """depth [N,C,H,W] (C = 1 depth, or 4 RGB-D) -> (crop_box [N,4] int64, has_hand [N] int32,
    crops [N,out,out,cpad] NHWC).  reorder_bgr applies the RGBD channel permutation [2,1,0,3]."""
    lib = _lib.load()
    _req(depth, name="depth")
    n, c, h, w = depth.shape
    if c not in (1, 4):
        raise ValueError("depth must be [N,1,H,W] or [N,4,H,W]")
    cap = det.scores.shape[1]
    dev = depth.device
    if crop_box is None:
        crop_box = torch.empty((n, 4), device=dev, dtype=torch.int64)
    if has_hand is None:
        has_hand = torch.empty((n,), device=dev, dtype=torch.int32)
    if crops is None:
        crops = torch.empty((n, out_size, out_size, cpad), device=dev, dtype=torch.float32)
    check(lib.hn_crop_resize(ptr(det.boxes), ptr(det.labels), ptr(det.count), cap, int(hand_label), ptr(depth), n, c,
                             1 if reorder_bgr else 0, h, w, out_size, cpad, ptr(crop_box), ptr(has_hand), ptr(crops),
                             _stream()), "hn_crop_resize")
    return crop_box, has_hand, crops


MAX_HANDS = 16


def check_max_hands(max_hands) -> int:
    """max_hands as an int in 1..MAX_HANDS (the bound of the crop batch: N * K crops of 176 x 176), else ValueError."""
    try:
        k = int(max_hands)
    except (TypeError, ValueError):
        k = None
    if k is None or k != max_hands or not 1 <= k <= MAX_HANDS:
        raise ValueError(f"max_hands must be an integer in 1..{MAX_HANDS} (got {max_hands!r})")
    return k


TRACK_WORDS = 12           # int32 words of a row of the tracker's state (48 bytes)
TRACK_MAX_SIDE = 32767     # frames the tracked step takes: the rule's products then fit in int64


def check_track_options(track_iou, track_hold):
    """(thr_milli, hold) of the tracked step's C entry: int(round(1000 * track_iou)) in 1..1000 and track_hold as an int in
    0..1000000, else ValueError."""
    thr_milli = int(round(1000 * float(track_iou)))
    if not 1 <= thr_milli <= 1000:
        raise ValueError(f"track_iou must round to 0.001..1 (got {track_iou!r})")
    try:
        hold = int(track_hold)
    except (TypeError, ValueError):
        hold = None
    if hold is None or hold != track_hold or not 0 <= hold <= 1000000:
        raise ValueError(f"track_hold must be an integer in 0..1000000 (got {track_hold!r})")
    return thr_milli, hold


def track_state(n, k, device):
    """The empty tracker of n frames with k slots each: zeroed int32 [n, 1 + k, 12] (reset: state.zero_())."""
    return torch.zeros((int(n), 1 + check_max_hands(k), TRACK_WORDS), device=device, dtype=torch.int32)


def _slot_out(t, name, shape, dtype, device, wrong_size):
    """An output of the crop stage: a fresh tensor of `shape` when t is None, else t after _req and -- unless wrong_size is
    None -- the size check (as many elements as `shape`, else ValueError(wrong_size))."""
    if t is None:
        return torch.empty(shape, device=device, dtype=dtype)
    _req(t, dtype, name)
    if wrong_size is not None and t.numel() != math.prod(shape):
        raise ValueError(wrong_size)
    return t


def crop_resize_hands(det: Detections, hand_label, depth, max_hands, out_size=176, cpad=4, crop_box=None, has_hand=None,
                      score=None, det_index=None, crops=None, reorder_bgr=False, handed=False, left_side=0, side=None,
                      mirror=None, track=None, track_iou=0.3, track_hold=5, track_id=None, track_age=None):
    """crop_resize for the first max_hands hand detections of each frame: slot k of frame i is the k-th detection with label
    hand_label in frame i's score-ordered list, padded and cut as crop_resize cuts the first.  -> (crop_box [N,K,4] int64,
    has_hand [N,K] int32, score [N,K] fp32, det_index [N,K] int32 (-1: empty slot), crops [N*K,out,out,cpad] NHWC).
    An empty slot (no such detection, or an empty padded slice) has zeros everywhere and still uses up its rank.
    handed: the slots' handedness in the same two launches (hn_crop_resize_hands_sided) -- two more results, side [N,K] int32
    (det.sides of the slot's detection, -1 for an empty slot) and mirror [N,K] int32 (1 for a filled slot whose side is
    left_side); the crop of a mirror slot is the plain crop flipped along its width, everything else is unchanged.
    track: a state tensor of track_state(N, K) -- the slots are TRACKED from call to call (hn_crop_resize_hands_tracked, DESIGN.md
    9e: a hand keeps its slot and its id while its padded box overlaps the slot's last one with IoU >= track_iou; a slot whose
    hand is missing is held, empty, for track_hold steps), the state is updated in place, and two more results end the tuple:
    track_id, track_age [N,K] int32.  Frames of at most 32767 x 32767 pixels."""
    k = check_max_hands(max_hands)
    if track is not None:       # (the options and the frame-size limit first: refused before anything touches a device)
        thr_milli, hold = check_track_options(track_iou, track_hold)
        if max(depth.shape[-2:]) > TRACK_MAX_SIDE:
            raise ValueError(f"tracked hands: frames of at most {TRACK_MAX_SIDE} x {TRACK_MAX_SIDE} pixels "
                             f"(got {depth.shape[-2]} x {depth.shape[-1]})")
    _req(depth, name="depth")
    n, c, h, w = depth.shape
    if c not in (1, 4):
        raise ValueError("depth must be [N,1,H,W] or [N,4,H,W]")
    cap = det.scores.shape[1]
    dev = depth.device
    i32 = torch.int32
    crop_box = _slot_out(crop_box, "crop_box", (n, k, 4), torch.int64, dev, "crop_box must hold four values per slot")
    has_hand = _slot_out(has_hand, "has_hand", (n, k), i32, dev, "has_hand must hold one value per slot")
    score = _slot_out(score, "score", (n, k), torch.float32, dev, "score must hold one value per slot")
    det_index = _slot_out(det_index, "det_index", (n, k), i32, dev, "det_index must hold one value per slot")
    # (the crops' size follows out_size and cpad, which the C entry judges)
    crops = _slot_out(crops, "crops", (n * k, out_size, out_size, cpad), torch.float32, dev, None)
    if handed:
        side = _slot_out(side, "side", (n, k), i32, dev, "side and mirror must hold one value per slot")
        mirror = _slot_out(mirror, "mirror", (n, k), i32, dev, "side and mirror must hold one value per slot")
        _req(det.sides, i32, "det.sides")
    if track is not None:
        _req(track, i32, "track")
        if track.numel() != n * (1 + k) * TRACK_WORDS:
            raise ValueError(f"track must be track_state({n}, {k}): int32 [{n},{1 + k},{TRACK_WORDS}]")
        track_id = _slot_out(track_id, "track_id", (n, k), i32, dev, "track_id and track_age must hold one value per slot")
        track_age = _slot_out(track_age, "track_age", (n, k), i32, dev, "track_id and track_age must hold one value per slot")
    dets = (ptr(det.boxes), ptr(det.scores), ptr(det.labels))
    stage = (k, ptr(depth), n, c, 1 if reorder_bgr else 0, h, w, out_size, cpad, ptr(crop_box), ptr(has_hand), ptr(score),
             ptr(det_index))
    sides = (ptr(det.sides), ptr(side), ptr(mirror)) if handed else (None, None, None)
    if track is not None:
        name = "hn_crop_resize_hands_tracked"
        args = dets + (sides[0], ptr(det.count), cap, int(hand_label), int(left_side)) + stage + sides[1:] + (
            ptr(crops), ptr(track), thr_milli, hold, ptr(track_id), ptr(track_age))
    elif handed:
        name = "hn_crop_resize_hands_sided"
        args = dets + (sides[0], ptr(det.count), cap, int(hand_label), int(left_side)) + stage + sides[1:] + (ptr(crops),)
    else:
        name = "hn_crop_resize_hands"
        args = dets + (ptr(det.count), cap, int(hand_label)) + stage + (ptr(crops),)
    check(getattr(_lib.load(), name)(*args, _stream()), name)
    return ((crop_box, has_hand, score, det_index, crops) + ((side, mirror) if handed else ())
            + ((track_id, track_age) if track is not None else ()))


def stem_image_nhwc4(x, border=3, out=None, valid=None):
    """fp32 [N,H,W,4] -> stem image fp16 [2 (hi, lo), N, H+2b, W+2b, 4] with a zero border (input of conv_stem_*_split).
    valid [N] int32 (optional): images with valid == 1 that hold a non-finite pixel get valid = 2 (a2j_aggregate then writes
    NaN rows for them, as the reference's network does)."""
    _req(x, name="x")
    n, h, w, c = x.shape
    if c != 4:
        raise ValueError("x must be [N,H,W,4]")
    if out is None:
        out = torch.empty((2, n, h + 2 * border, w + 2 * border, 4), device=x.device, dtype=torch.float16)
    if valid is not None:
        _req(valid, torch.int32, "valid")
    check(_lib.load().hn_stem_image_nhwc4_valid(ptr(x), n, h, w, border, ptr(out), ptr(valid) if valid is not None else None,
                                                _stream()), "hn_stem_image_nhwc4_valid")
    return out


def pack_depth_nhwc(depth, cpad=4, out=None):
    """depth [N,1,H,W] -> [N,H,W,cpad] with depth in channel 0."""
    lib = _lib.load()
    _req(depth, name="depth")
    n, c, h, w = depth.shape
    if c != 1:
        raise ValueError("depth must be [N,1,H,W]")
    if out is None:
        out = torch.empty((n, h, w, cpad), device=depth.device, dtype=torch.float32)
    check(lib.hn_pack_depth_nhwc(ptr(depth), ptr(out), n, h * w, cpad, _stream()), "hn_pack_depth_nhwc")
    return out


def _convert_arg(convert, k, joints, device):
    """The `convert` dict of a2j_aggregate / a2j_loss as the library takes it -> (crop_box or None, crop side, paras array or
    None, ConvertOpts or None, image_uvd, xyz_mm or None); the two outputs are fresh where the dict brings none."""
    # the evaluation caller's operands (a2j/a2j.py:339-346): the dataset's fp32 boxes / per-sample intrinsics on the device
    sbox, sparas = convert.get("sample_box"), convert.get("sample_paras")
    box = convert.get("crop_box")
    if (box is None) == (sbox is None):
        raise ValueError("convert needs crop_box (int64, the detector's) or sample_box (fp32, the dataset's), one of them")
    for t, dt, nm in ((box, torch.int64, "crop_box"), (sbox, torch.float32, "sample_box"), (sparas, torch.float32, "sample_paras")):
        if t is not None and tuple(_req(t, dt, nm).shape) != (k, 4):
            raise ValueError(f"{nm} must be [K,4]")
    paras = convert.get("paras")
    if paras is not None and sparas is not None:
        raise ValueError("convert: paras (one camera) or sample_paras (one per sample), not both")
    img, xyz = convert.get("image_uvd"), convert.get("xyz_mm")
    if img is None:
        img = torch.empty((k, joints, 3), device=device, dtype=torch.float32)
    if xyz is None and (paras is not None or sparas is not None):
        xyz = torch.empty((k, joints, 3), device=device, dtype=torch.float32)
    pp = (C.c_float * 4)(*[float(v) for v in paras]) if paras is not None else None
    opts = None
    cb = convert.get("clamp_box")
    if convert.get("clamp_keypoints") or cb or sbox is not None or sparas is not None:
        opts = _lib.ConvertOpts(1 if convert.get("clamp_keypoints") else 0, int(cb[0]) if cb else 0, int(cb[1]) if cb else 0, 0,
                                ptr(sbox), ptr(sparas))
    return box, float(convert.get("crop", 176)), pp, opts, img, xyz


def _a2j_heads(cls, reg, dep, joints, gt=None, valid=None):
    """The argument checks a2j_aggregate, a2j_loss and a2j_loss_grad share: cls/dep [K,fh,fw,16*J], reg [K,fh,fw,16*J*2], gt
    [K,J,3] (where the caller takes one), valid [K] int32 or None, all contiguous fp32 / int32 on the device -> (k, fh, fw)."""
    _req(cls, name="cls"); _req(reg, name="reg"); _req(dep, name="dep")
    if gt is not None:
        _req(gt, name="gt")
    if cls.dim() != 4 or reg.dim() != 4:
        raise ValueError("bad head shapes")
    k, fh, fw, aj = cls.shape
    if joints < 1 or aj != 16 * joints or reg.shape[3] != 2 * aj or dep.shape != cls.shape or reg.shape[:3] != cls.shape[:3]:
        raise ValueError("bad head shapes")
    if gt is not None and tuple(gt.shape) != (k, joints, 3):
        raise ValueError("gt must be [K,J,3]")
    if valid is not None and _req(valid, torch.int32, "valid").numel() != k:
        raise ValueError("valid must hold one flag per crop")
    return k, fh, fw


def a2j_aggregate(cls, reg, dep, joints=21, stride=16, valid=None, out=None, convert=None):
    """cls/dep [K,fh,fw,16*J], reg [K,fh,fw,16*J*2] -> [K,J,3].
    convert: optional dict -- convert_joints + uvd2xyz in the SAME launch (hn_a2j_aggregate_convert_f32):
      crop_box [K,4] int64 (the boxes the crops were cut with), paras = (fx, fy, cx, cy) or None, crop = 176,
      clamp_keypoints / clamp_box = (H, W): the live caller's clamps (ros_demo.py:279-283),
      image_uvd / xyz_mm: preallocated outputs (optional),
      mirror [K] int32: rows whose crop was cut mirrored (crop_resize_hands(handed=True)) -- u = crop - u before anything
      else sees the value (hn_a2j_aggregate_convert_mirror_f32).
    Then returns (crop_uvd, image_uvd [K,J,3], xyz_mm [K,J,3] or None), bit-identical to convert_joints() on crop_uvd."""
    lib = _lib.load()
    k, fh, fw = _a2j_heads(cls, reg, dep, joints, valid=valid)
    if out is None:
        out = torch.empty((k, joints, 3), device=cls.device, dtype=torch.float32)
    if k == 0:
        return out
    if convert is not None:
        box, crop, pp, opts, img, xyz = _convert_arg(convert, k, joints, cls.device)
        mirror = convert.get("mirror")
        if mirror is not None:
            if _req(mirror, torch.int32, "mirror").numel() != k:
                raise ValueError("mirror must hold one flag per crop")
            check(lib.hn_a2j_aggregate_convert_mirror_f32(ptr(cls), ptr(reg), ptr(dep), ptr(valid), ptr(mirror), k, fh, fw, joints,
                                                          stride, ptr(box), crop, crop, pp,
                                                          C.byref(opts) if opts is not None else None, ptr(out), ptr(img),
                                                          ptr(xyz), _stream()), "hn_a2j_aggregate_convert_mirror_f32")
            return out, img, xyz
        check(lib.hn_a2j_aggregate_convert_f32(ptr(cls), ptr(reg), ptr(dep), ptr(valid), k, fh, fw, joints, stride, ptr(box),
                                               crop, crop, pp, C.byref(opts) if opts is not None else None, ptr(out), ptr(img),
                                               ptr(xyz), _stream()), "hn_a2j_aggregate_convert_f32")
        return out, img, xyz
    check(lib.hn_a2j_aggregate_f32(ptr(cls), ptr(reg), ptr(dep), ptr(valid), k, fh, fw, joints, stride, ptr(out),
                                   _stream()), "hn_a2j_aggregate_f32")
    return out


def a2j_loss(cls, reg, dep, gt, joints=21, stride=16, spatial_factor=0.5, reg_loss_factor=3.0, valid=None, convert=None, out=None):
    """The aggregation with the A2J criterion in its sweep (hn_a2j_aggregate_loss_f32; a2j/anchor.py:99-153, DESIGN.md section
    9o): heads as a2j_aggregate takes them, gt [K,J,3] fp32 in crop (coord0, coord1, depth)
      -> (uvd [K,J,3] -- or, with convert, a2j_aggregate's triple (crop_uvd, image_uvd, xyz_mm or None) --,
          terms [K,J,8] = (La_h, La_w, Lr_h, Lr_w, d, squared uvd differences x 3),
          sample [K,2] = (anchor_loss, regression_loss) per sample,
          batch [5] = (classification, the criterion's regression mean, regression * reg_loss_factor, total, rmse)),
    all on the device.  uvd and the converted outputs are a2j_aggregate's on the same heads bit for bit.
    valid: rows with 0 are left out of the batch values, rows with 2 make them NaN.  convert: a2j_aggregate's dict without
    mirror.  out: a preallocated uvd."""
    lib = _lib.load()
    k, fh, fw = _a2j_heads(cls, reg, dep, joints, gt, valid)
    dev = cls.device
    if out is None:
        out = torch.empty((k, joints, 3), device=dev, dtype=torch.float32)
    elif tuple(_req(out, name="out").shape) != (k, joints, 3):
        raise ValueError("out must be [K,J,3]")
    terms = torch.empty((k, joints, 8), device=dev, dtype=torch.float32)
    sample = torch.empty((k, 2), device=dev, dtype=torch.float32)
    # (no crop at all: nothing is launched, and the batch values are the mean of nothing)
    batch = torch.empty((5,), device=dev, dtype=torch.float32) if k else torch.full((5,), float("nan"), device=dev)
    box = img = xyz = pp = opts = None
    crop = 0.0
    if convert is not None:
        if convert.get("mirror") is not None:
            raise ValueError("a2j_loss: convert takes no mirror flags")
        box, crop, pp, opts, img, xyz = _convert_arg(convert, k, joints, dev)
    res = out if convert is None else (out, img, xyz)
    if k == 0:
        return res, terms, sample, batch
    check(lib.hn_a2j_aggregate_loss_f32(ptr(cls), ptr(reg), ptr(dep), ptr(valid), ptr(gt), k, fh, fw, joints, stride,
                                        float(spatial_factor), float(reg_loss_factor), ptr(box), crop, crop, pp,
                                        C.byref(opts) if opts is not None else None, ptr(out), ptr(img), ptr(xyz), ptr(terms),
                                        ptr(sample), ptr(batch), _stream()), "hn_a2j_aggregate_loss_f32")
    return res, terms, sample, batch


def a2j_loss_grad(cls, reg, dep, gt, joints=21, stride=16, spatial_factor=0.5, reg_loss_factor=3.0, valid=None, upstream=None,
                  want_forward=False):
    """The A2J criterion's backward at the three heads in one launch (hn_a2j_loss_grad_f32): heads, gt
    and valid as a2j_loss takes them -> (d_cls, d_reg, d_dep), the gradients of
    wa * classification + wr * regression (a2j_loss's batch [0] and [2]) in the layouts of the heads, on the device.
    upstream: fp32 [2] on the device = (wa, wr), or None for (1, 1), the gradient of total_loss; it is read by the kernel, so
    nothing here synchronises.  Rows with valid == 0 get zero gradients and are not counted in the batch mean, rows with
    valid == 2 get NaN.  want_forward: also return a2j_loss's uvd [K,J,3] and terms [K,J,8] of the same heads, bit for bit."""
    lib = _lib.load()
    k, fh, fw = _a2j_heads(cls, reg, dep, joints, gt, valid)
    if upstream is not None and _req(upstream, name="upstream").numel() != 2:
        raise ValueError("upstream must hold (wa, wr)")
    d_cls, d_reg, d_dep = torch.empty_like(cls), torch.empty_like(reg), torch.empty_like(dep)
    uvd = terms = None
    if want_forward:
        uvd = torch.empty((k, joints, 3), device=cls.device, dtype=torch.float32)
        terms = torch.empty((k, joints, 8), device=cls.device, dtype=torch.float32)
    if k:
        check(lib.hn_a2j_loss_grad_f32(ptr(cls), ptr(reg), ptr(dep), ptr(valid), ptr(gt), k, fh, fw, joints, stride,
                                       float(spatial_factor), float(reg_loss_factor), ptr(upstream), ptr(d_cls), ptr(d_reg),
                                       ptr(d_dep), ptr(uvd), ptr(terms), _stream()), "hn_a2j_loss_grad_f32")
    return (d_cls, d_reg, d_dep, uvd, terms) if want_forward else (d_cls, d_reg, d_dep)


def joints2d_standardize(image_uvd, valid=None, out=None):
    """image (u,v,d) joints [N,J,3] -> the lifter's input [N,J,2]: per frame and axis (x - mean) / std over the joints
    (hn_joints2d_standardize_f32 = the live caller's bbox / affine / normalisation chain, ros_demo.py:148-157, which reduces
    to exactly this when there is no rotation); rows with valid != 1 are zeros."""
    _req(image_uvd, name="image_uvd")
    n, j, _ = image_uvd.shape
    if out is None:
        out = torch.empty((n, j, 2), device=image_uvd.device, dtype=torch.float32)
    if valid is not None:
        _req(valid, torch.int32, "valid")
    check(_lib.load().hn_joints2d_standardize_f32(ptr(image_uvd), ptr(valid), n, j, ptr(out), _stream()),
          "hn_joints2d_standardize_f32")
    return out


def lifter_input_gated(image_uvd, valid=None, out=None, lifted=None, mirror=None):
    """joints2d_standardize with the live caller's skip rule (ros_demo.py:288-300): image (u,v,d) [N,J,3] -> (the lifter's
    input [N,J,2], lifted [N] int32).  A row is lifted (1, and joints2d_standardize's row bit for bit) iff valid is None or 1
    there, its (u,v) are finite and process_bbox(get_bbox(uv)) is not None (coord_utils.py:21-49, fp32 as numpy evaluates
    it); every other row is zeros with lifted 0 -- so a degenerate hand never reaches the lifter as inf / NaN.
    mirror [N] int32: a lifted row with mirror != 0 has column 0 negated (hn_lifter_input_gated_mirror_f32) -- the
    standardisation of the joints mirrored in x; the gate sees the plain joints."""
    _req(image_uvd, name="image_uvd")
    n, j, _ = image_uvd.shape
    if out is None:
        out = torch.empty((n, j, 2), device=image_uvd.device, dtype=torch.float32)
    if lifted is None:
        lifted = torch.empty((n,), device=image_uvd.device, dtype=torch.int32)
    _req(out, name="out"); _req(lifted, torch.int32, "lifted")
    if tuple(out.shape) != (n, j, 2) or lifted.numel() != n:
        raise ValueError("out must be [N,J,2] and lifted [N]")
    if valid is not None:
        _req(valid, torch.int32, "valid")
        if valid.numel() != n:
            raise ValueError("valid must hold one flag per row")
    if mirror is not None:
        if _req(mirror, torch.int32, "mirror").numel() != n:
            raise ValueError("mirror must hold one flag per row")
        check(_lib.load().hn_lifter_input_gated_mirror_f32(ptr(image_uvd), ptr(valid), ptr(mirror), n, j, ptr(out), ptr(lifted),
                                                           _stream()), "hn_lifter_input_gated_mirror_f32")
        return out, lifted
    check(_lib.load().hn_lifter_input_gated_f32(ptr(image_uvd), ptr(valid), n, j, ptr(out), ptr(lifted), _stream()),
          "hn_lifter_input_gated_f32")
    return out, lifted


def convert_joints(kp, crop_box, valid=None, paras=None, crop=176, out=None):
    """kp [N,J,3] crop-(u,v,d), crop_box [N,4] int64 -> image (u,v,d), or camera xyz in mm when
    paras = (fx, fy, cx, cy) is given (convert_joints + uvd2xyz of the reference, on the device)."""
    lib = _lib.load()
    _req(kp, name="kp")
    _req(crop_box, torch.int64, "crop_box")
    n, j, _ = kp.shape
    if out is None:
        out = torch.empty_like(kp)
    if valid is not None:
        _req(valid, torch.int32, "valid")
    pp = None
    if paras is not None:
        pp = (C.c_float * 4)(*[float(v) for v in paras])
    check(lib.hn_convert_joints_f32(ptr(kp), ptr(crop_box), ptr(valid), n, j, float(crop), float(crop), pp, ptr(out),
                                    _stream()), "hn_convert_joints_f32")
    return out


def convert_joints_samples(kp, box_f32, sample_paras=None, valid=None, crop=176, want_image=True):
    """The evaluation caller's conversion (A2JModelLightning.test_step, a2j/a2j.py:339-346): kp [N,J,3] crop-(u,v,d), box_f32
    [N,4] fp32 = the dataset's boxes (fractional corners), sample_paras [N,4] fp32 = each sample's (fx, fy, cx, cy), all on the
    device -> (image (u,v,d) or None, camera xyz in mm or None); fp32 in the reference's order (bit-identical to numpy)."""
    _req(kp, name="kp")
    n, j, _ = kp.shape
    if tuple(_req(box_f32, torch.float32, "box_f32").shape) != (n, 4):
        raise ValueError("box_f32 must be [N,4]")
    if sample_paras is not None and tuple(_req(sample_paras, torch.float32, "sample_paras").shape) != (n, 4):
        raise ValueError("sample_paras must be [N,4]")
    if valid is not None:
        _req(valid, torch.int32, "valid")
    if not want_image and sample_paras is None:
        raise ValueError("nothing to compute: no image (u,v,d) wanted and no intrinsics given")
    img = torch.empty_like(kp) if want_image else None
    xyz = torch.empty_like(kp) if sample_paras is not None else None
    check(_lib.load().hn_convert_joints_samples_f32(ptr(kp), ptr(box_f32), ptr(sample_paras), ptr(valid), n, j, float(crop),
                                                    float(crop), ptr(img), ptr(xyz), _stream()), "hn_convert_joints_samples_f32")
    return img, xyz


HPE_MAX_JOINTS = 64        # one lane per joint
HPE_MAX_STEPS = 1024       # thresholds of a PCK curve
HPE_WAVES_PER_GROUP = 4    # samples per workgroup of hn_hpe_accumulate_f32 (csrc/hpe_metrics.hip kWaves)

HPEState = collections.namedtuple("HPEState", "hist sum n flat")
# hist int64 [3,J,T+1], sum int64 [3,J], n int64 [2]: views of `flat`, ONE int64 buffer (a single copy moves the whole state)
HPEBatch = collections.namedtuple("HPEBatch", "state dist aligned")


def hpe_state(joints, steps, device) -> HPEState:
    """A zeroed state of the evaluator's tables for `joints` joints and `steps` thresholds."""
    joints, steps = int(joints), int(steps)
    if not 1 <= joints <= HPE_MAX_JOINTS or not 1 <= steps <= HPE_MAX_STEPS:
        raise ValueError(f"joints 1..{HPE_MAX_JOINTS} and thresholds 1..{HPE_MAX_STEPS}, got {joints} and {steps}")
    a, b = 3 * joints * (steps + 1), 3 * joints
    flat = torch.zeros((a + b + 2,), device=device, dtype=torch.int64)
    return HPEState(flat[:a].view(3, joints, steps + 1), flat[a:a + b].view(3, joints), flat[a + b:], flat)


def hpe_accumulate(pred, gt, thresholds, state=None, valid=None, want_dist=False, want_aligned=False) -> HPEBatch:
    """One batch into the evaluator's tables (hn_hpe_accumulate_f32: one launch, no synchronisation; tests/hpe_ref.py is the rule
    and every output equals it bit for bit).  pred, gt fp32 [S,J,3] camera millimetres, J <= 64; thresholds fp64 [T] non-decreasing,
    T <= 1024; valid int32 [S] (0: the sample is skipped) or None, all on one device.  state: an HPEState to add to (hpe_state), or
    None for a new zeroed one.  Returns HPEBatch(state, dist fp64 [S,3,J] or None, aligned fp64 [S,J,3] or None): the absolute,
    root-relative and Procrustes-aligned distances and align_w_scale(gt, pred); rows of skipped samples are NaN."""
    _req(pred, name="pred"); _req(gt, name="gt"); _req(thresholds, torch.float64, "thresholds")
    if pred.dim() != 3 or pred.shape[2] != 3 or tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"pred and gt must be fp32 [S,J,3] of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    s, j, _ = pred.shape
    if not 1 <= j <= HPE_MAX_JOINTS:
        raise ValueError(f"{j} joints: 1..{HPE_MAX_JOINTS} (one lane per joint)")
    if thresholds.dim() != 1 or not 1 <= thresholds.shape[0] <= HPE_MAX_STEPS:
        raise ValueError(f"thresholds must be fp64 [T], T in 1..{HPE_MAX_STEPS}, got {tuple(thresholds.shape)}")
    t = thresholds.shape[0]
    if valid is not None and _req(valid, torch.int32, "valid").numel() != s:
        raise ValueError(f"valid must hold one value per sample ({s}), got {valid.numel()}")
    if state is None:
        state = hpe_state(j, t, pred.device)
    else:
        for name, part, shape in (("hist", state.hist, (3, j, t + 1)), ("sum", state.sum, (3, j)), ("n", state.n, (2,))):
            if tuple(_req(part, torch.int64, f"state.{name}").shape) != shape:
                raise ValueError(f"state.{name}: expected int64 {list(shape)}, got {tuple(part.shape)}")
    for name, other in (("gt", gt), ("thresholds", thresholds), ("valid", valid), ("state", state.hist)):
        if other is not None and other.device != pred.device:
            raise ValueError(f"{name} lives on {other.device}, pred on {pred.device}")
    dist = torch.empty((s, 3, j), device=pred.device, dtype=torch.float64) if want_dist else None
    aligned = torch.empty((s, j, 3), device=pred.device, dtype=torch.float64) if want_aligned else None
    check(_lib.load().hn_hpe_accumulate_f32(ptr(pred), ptr(gt), ptr(valid), s, j, ptr(thresholds), t, ptr(state.hist), ptr(state.sum),
                                            ptr(state.n), ptr(dist), ptr(aligned), _stream()), "hn_hpe_accumulate_f32")
    return HPEBatch(state, dist, aligned)


def procrustes_align(gt, pred):
    """align_w_scale (freihand/eval.py:72-95) for a batch on the device: gt, pred fp32 [S,J,3] -> fp64 [S,J,3], the prediction
    moved, turned (reflections allowed, as scipy's orthogonal_procrustes leaves them) and scaled onto the ground truth; rows of
    samples with a non-finite value or one of 2^20 and beyond are NaN.  The rule's own kernel (hpe_accumulate's `aligned`)."""
    _req(pred, name="pred")
    return hpe_accumulate(pred, gt, torch.zeros((1,), device=pred.device, dtype=torch.float64), want_aligned=True).aligned


DET_AP_MAX_GT = 64                 # ground-truth boxes per image and class: one lane each (csrc/det_ap.hip)
DET_AP_MAX_RECORDS = 1 << 27       # images * max_dets of one record table: 512 MiB of int32, and the state holds two
DET_AP_SCORE_BITS, DET_AP_TP_SHIFT, DET_AP_FP_SHIFT, DET_AP_VALID = 10, 10, 15, 1 << 20

DetAPTable = collections.namedtuple("DetAPTable", "hand_off hand_box hand_meta hand_obj obj_off obj_box obj_diff num_images "
                                                  "npos_hand npos_obj")
DetAPState = collections.namedtuple("DetAPState", "hand obj fed overflow flat")
# hand, obj int32 [I,max_dets], fed int32 [I], overflow int32 [1]: views of `flat`, ONE int32 buffer


def det_ap_table(hand_off, hand_box, hand_meta, hand_obj, obj_off, obj_box, obj_diff, device) -> DetAPTable:
    """The annotation cache, flattened, on the device (uploaded once).  Host arrays: hand_off int [I+1]
    into hand_box int [H,4], hand_meta int [H,4] (difficult, handstate, leftright, objectbbox present), hand_obj float64 [H,4];
    obj_off int [I+1] into obj_box int [O,4], obj_diff int [O].  Refused: offsets that do not partition their rows, more than
    64 boxes of a class in one image."""
    hand_off, obj_off = (np.asarray(x, np.int64).reshape(-1) for x in (hand_off, obj_off))
    hand_box, hand_meta, obj_box = (np.asarray(x, np.int64).reshape(-1, 4) for x in (hand_box, hand_meta, obj_box))
    hand_obj, obj_diff = np.asarray(hand_obj, np.float64).reshape(-1, 4), np.asarray(obj_diff, np.int64).reshape(-1)
    num_images = hand_off.shape[0] - 1
    if num_images < 1 or obj_off.shape[0] != num_images + 1:
        raise ValueError(f"hand_off and obj_off must hold images + 1 >= 2 offsets, got {hand_off.shape[0]} and {obj_off.shape[0]}")
    for name, off, rows in (("hand", hand_off, hand_box.shape[0]), ("obj", obj_off, obj_box.shape[0])):
        per = np.diff(off)
        if off[0] != 0 or off[-1] != rows or (per < 0).any():
            raise ValueError(f"{name}_off must rise from 0 to the {rows} rows of {name}_box")
        if (per > DET_AP_MAX_GT).any():
            raise ValueError(f"image {int(np.argmax(per))} has {int(per.max())} {name} boxes: at most {DET_AP_MAX_GT} (one lane each)")
    if hand_meta.shape[0] != hand_box.shape[0] or hand_obj.shape[0] != hand_box.shape[0] or obj_diff.shape[0] != obj_box.shape[0]:
        raise ValueError("hand_meta, hand_obj and obj_diff must hold one row per box")
    if max(np.abs(hand_box).max(initial=0), np.abs(obj_box).max(initial=0), np.abs(hand_meta).max(initial=0)) >= 1 << 24:
        raise ValueError("box coordinates and hand fields must be integers below 2^24")
    dev = torch.device(device)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x.astype(dt))).to(dev)
    return DetAPTable(up(hand_off, np.int32), up(hand_box, np.int32), up(hand_meta, np.int32), up(hand_obj, np.float64),
                      up(obj_off, np.int32), up(obj_box, np.int32), up(obj_diff, np.int32), num_images,
                      int((hand_meta[:, 0] == 0).sum()), int((obj_diff == 0).sum()))


def det_ap_state(num_images, max_dets, device) -> DetAPState:
    """A zeroed state of the detector evaluation: one record word per (image, rank) and class, the per-image feed counts and the
    overflow counter.  num_images * max_dets is bounded by DET_AP_MAX_RECORDS (2^27 words: 512 MiB per table)."""
    num_images, max_dets = int(num_images), int(max_dets)
    if num_images < 1 or max_dets < 1 or num_images * max_dets > DET_AP_MAX_RECORDS:
        raise ValueError(f"num_images >= 1, max_dets >= 1 and num_images * max_dets <= {DET_AP_MAX_RECORDS}, got {num_images} and {max_dets}")
    a = num_images * max_dets
    flat = torch.zeros((2 * a + num_images + 1,), device=device, dtype=torch.int32)
    return DetAPState(flat[:a].view(num_images, max_dets), flat[a:2 * a].view(num_images, max_dets), flat[2 * a:2 * a + num_images],
                      flat[2 * a + num_images:], flat)


def det_ap_accumulate(det, contacts, dxdymags, image_ids, table: DetAPTable, state: DetAPState | None = None, max_dets=100,
                      hand_label=2, object_label=1, score_min=0.1, ovthresh=0.5) -> DetAPState:
    """One batch of detections into the evaluation's record tables (hn_det_ap_accumulate_f32: one launch, no synchronisation;
    tests/ap_ref.py is the rule and the state equals it byte for byte).  det: the detector's `Detections` (boxes fp32 [N,cap,4],
    scores fp32 [N,cap], labels / sides int32 [N,cap], count int32 [N]); contacts int32 [N,cap], dxdymags fp32 [N,cap,3] (ext
    heads); image_ids int32 [N]: the row of `table` each image is matched against -- an id outside it writes nothing and counts
    into `overflow`, on the device.  state: a DetAPState to write into (det_ap_state), or None for a new one of `max_dets`."""
    _req(det.boxes, name="det.boxes"); _req(det.scores, name="det.scores")
    if det.scores.dim() != 2 or tuple(det.boxes.shape) != tuple(det.scores.shape) + (4,):
        raise ValueError(f"det.scores must be fp32 [N,cap] and det.boxes [N,cap,4], got {tuple(det.scores.shape)} and {tuple(det.boxes.shape)}")
    n, cap = det.scores.shape
    for name, t, shape in (("det.labels", det.labels, (n, cap)), ("det.sides", det.sides, (n, cap)), ("det.count", det.count, (n,)),
                           ("contacts", contacts, (n, cap)), ("image_ids", image_ids, (n,))):
        if tuple(_req(t, torch.int32, name).shape) != shape:
            raise ValueError(f"{name}: expected int32 {list(shape)}, got {tuple(t.shape)}")
    if tuple(_req(dxdymags, name="dxdymags").shape) != (n, cap, 3):
        raise ValueError(f"dxdymags: expected fp32 {[n, cap, 3]}, got {tuple(dxdymags.shape)}")
    if not isinstance(table, DetAPTable):
        raise TypeError("table must come from det_ap_table")
    if int(hand_label) == int(object_label):
        raise ValueError(f"hand_label and object_label are both {hand_label}")
    if not 0.0 <= float(score_min) < 1.0 or math.isnan(float(ovthresh)):
        raise ValueError(f"score_min in [0, 1) and a threshold that is a number, got {score_min} and {ovthresh}")
    if n * cap > 1 << 28:
        raise ValueError(f"{n} x {cap} detections: at most 2^28 a batch")
    images = table.num_images
    if state is None:
        state = det_ap_state(images, max_dets, det.scores.device)
    else:
        if state.hand.dim() != 2 or state.hand.shape[0] != images:
            raise ValueError(f"state.hand: expected int32 [{images}, max_dets], got {tuple(state.hand.shape)}")
        m = state.hand.shape[1]
        for name, part, shape in (("hand", state.hand, (images, m)), ("obj", state.obj, (images, m)), ("fed", state.fed, (images,)),
                                  ("overflow", state.overflow, (1,))):
            if tuple(_req(part, torch.int32, f"state.{name}").shape) != shape:
                raise ValueError(f"state.{name}: expected int32 {list(shape)}, got {tuple(part.shape)}")
    for name, other in (("det.boxes", det.boxes), ("det.labels", det.labels), ("det.sides", det.sides), ("det.count", det.count),
                        ("contacts", contacts), ("dxdymags", dxdymags), ("image_ids", image_ids), ("table", table.hand_off),
                        ("state", state.hand)):
        if other.device != det.scores.device:
            raise ValueError(f"{name} lives on {other.device}, det.scores on {det.scores.device}")
    check(_lib.load().hn_det_ap_accumulate_f32(
        ptr(det.boxes), ptr(det.scores), ptr(det.labels), ptr(det.sides), ptr(det.count), ptr(contacts), ptr(dxdymags), ptr(image_ids),
        n, cap, ptr(table.hand_off), ptr(table.hand_box), ptr(table.hand_meta), ptr(table.hand_obj), table.hand_box.shape[0],
        ptr(table.obj_off), ptr(table.obj_box), ptr(table.obj_diff), table.obj_box.shape[0], images, int(hand_label),
        int(object_label), float(score_min), float(ovthresh), ptr(state.hand), ptr(state.obj), ptr(state.fed), ptr(state.overflow),
        state.hand.shape[1], _stream()), "hn_det_ap_accumulate_f32")
    return state


def pack_records(kp, crop_box, has_hand, rows, rec_bytes, out=None, extras=()):
    """One step's per-frame results -> [rows, rec_bytes] uint8 records (rows >= frames: shard padding is zero rows).
    extras: up to two more [N,J,3] fp32 fields behind the keypoints (image uvd, camera xyz: the wide record)."""
    _req(kp, name="keypoints"); _req(crop_box, torch.int64, "crop_box"); _req(has_hand, torch.int32, "has_hand")
    n, j = kp.shape[0], kp.shape[1]
    if out is None:
        out = torch.empty((rows, rec_bytes), device=kp.device, dtype=torch.uint8)
    extras = [e for e in extras if e is not None]
    if extras:
        for e in extras:
            _req(e, name="extra")
            if e.shape != kp.shape:
                raise ValueError("extra fields must have the keypoints' shape")
        e0, e1 = extras[0], (extras[1] if len(extras) > 1 else None)
        check(_lib.load().hn_pack_records_ex(ptr(kp), ptr(crop_box), ptr(has_hand), n, rows, j, rec_bytes, ptr(e0), ptr(e1),
                                             ptr(out), _stream()), "hn_pack_records_ex")
        return out
    check(_lib.load().hn_pack_records(ptr(kp), ptr(crop_box), ptr(has_hand), n, rows, j, rec_bytes, ptr(out), _stream()),
          "hn_pack_records")
    return out


def unpack_records(rec, joints):
    """[rows, rec_bytes] uint8 records -> (keypoints [rows,J,3], crop_box [rows,4] int64, has_hand [rows] int32,
    valid [rows] int32)."""
    _req(rec, torch.uint8, "records")
    rows, rec_bytes = rec.shape
    dev = rec.device
    kp = torch.empty((rows, joints, 3), device=dev, dtype=torch.float32)
    box = torch.empty((rows, 4), device=dev, dtype=torch.int64)
    has = torch.empty((rows,), device=dev, dtype=torch.int32)
    valid = torch.empty((rows,), device=dev, dtype=torch.int32)
    check(_lib.load().hn_unpack_records(ptr(rec), rows, joints, rec_bytes, ptr(kp), ptr(box), ptr(has), ptr(valid), _stream()),
          "hn_unpack_records")
    return kp, box, has, valid


def nonfinite_count(x, flag=None):
    """Adds the number of non-finite values of x (fp32 GPU) to flag[0] (int32 GPU; fresh zero by default); no sync."""
    _req(x, name="x")
    if flag is None:
        flag = torch.zeros((1,), device=x.device, dtype=torch.int32)
    check(_lib.load().hn_nonfinite_count_f32(ptr(x), x.numel(), ptr(flag), _stream()), "hn_nonfinite_count_f32")
    return flag


def tickets_nonzero() -> int:
    """Split-K ticket counters of the current device that are not zero (hn_debug_tickets_nonzero; synchronises).  0 after any
    sequence of completed launches: the counters are zero at rest."""
    c = C.c_int64(0)
    check(_lib.load().hn_debug_tickets_nonzero(C.byref(c)), "hn_debug_tickets_nonzero")
    return int(c.value)


def set_form(name: str, on=True):
    """Kernel-form switch of the library (hn_set_form; names in include/handnet_hip.h): an older form of a kernel as a
    bit-identity reference or for A/B timing.  Process-wide; the product never sets one (hn_amd/forms.py)."""
    check(_lib.load().hn_set_form(name.encode(), 1 if on else 0), "hn_set_form")


def range_check_enable(on=True):
    """f16x3 range contract (see include/handnet_hip.h): split producers launched from now on flag values that
    cannot be represented as fp16 hi + lo (|v| > 65504 or non-finite)."""
    check(_lib.load().hn_range_check_enable(1 if on else 0), "hn_range_check_enable")


def range_check_bits(reset=True) -> int:
    """OR of the _lib.RANGE_* bits a split producer has set in the LIBRARY's flag block since the last reset (synchronises)."""
    flag = C.c_int32(0)
    check(_lib.load().hn_range_check_fetch(C.byref(flag), 1 if reset else 0, _stream()), "hn_range_check_fetch")
    return int(flag.value)


def range_check_fetch(reset=True) -> bool:
    """True if a split producer met an out-of-range / non-finite value since the last reset (synchronises)."""
    return range_check_bits(reset) != 0


def range_check_bind(block=None):
    """Split producers launched from now on note into `block` (4 zeroed int32 on the GPU) instead of the library's own
    flag words; None unbinds.  Host-side state, read at launch time."""
    check(_lib.load().hn_range_check_bind(ptr(block) if block is not None else None), "hn_range_check_bind")


@contextlib.contextmanager
def range_scope(block=None, on=True):
    """The f16x3 range contract for the launches of ONE step of ONE engine: inside the scope the split producers this HOST
    THREAD launches note into `block` (4 zeroed int32 on the GPU; on=False: nowhere); on exit the thread's previous switch and
    block are back (hn_range_scope_begin / _end: per-thread state in the library, so engines on other threads of the process
    are never redirected or switched off)."""
    lib = _lib.load()
    check(lib.hn_range_scope_begin(ptr(block) if (block is not None and on) else None, 1 if on else 0), "hn_range_scope_begin")
    try:
        yield
    finally:
        check(lib.hn_range_scope_end(), "hn_range_scope_end")


def range_check_collect(block=None, out=None):
    """One tiny launch: the flag words of `block` (None: the library's) -> out [4] int32 (activation, input out of range,
    input non-finite, 0), and cleared.  No synchronisation."""
    if out is None:
        dev = block.device if block is not None else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((4,), device=dev, dtype=torch.int32)
    check(_lib.load().hn_range_check_collect(ptr(block) if block is not None else None, ptr(out), _stream()),
          "hn_range_check_collect")
    return out


def range_bits(words) -> int:
    """host list of the four collected words -> OR of the _lib.RANGE_* bits"""
    return ((_lib.RANGE_ACTIVATION if words[0] else 0) | (_lib.RANGE_INPUT if words[1] else 0)
            | (_lib.RANGE_INPUT_NONFINITE if words[2] else 0))


class RangeError(RuntimeError):
    """A value left the dynamic range the f16x3 split format supports."""


def clock_sample(micros, out=None, stream=None):
    """Enqueue the one-wave shader-clock sampler (MHz -> out[0], fp32 GPU) on `stream` (default: current)."""
    if out is None:
        out = torch.zeros((1,), device=torch.device("cuda", _cur_device() if _cur_device else 0), dtype=torch.float32)
    st = _stream() if stream is None else stream.cuda_stream
    check(_lib.load().hn_clock_sample(int(micros), ptr(out), st), "hn_clock_sample")
    return out


class HipTimer:
    """HIP-event pair recorded on the current stream through the C ABI (bench.py)."""

    def __init__(self):
        lib = _lib.load()
        self._a, self._b = C.c_void_p(), C.c_void_p()
        check(lib.hn_event_create(C.byref(self._a)), "hn_event_create")
        check(lib.hn_event_create(C.byref(self._b)), "hn_event_create")

    def start(self):
        check(_lib.load().hn_event_record(self._a, _stream()), "hn_event_record")

    def stop(self):
        check(_lib.load().hn_event_record(self._b, _stream()), "hn_event_record")

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        check(_lib.load().hn_event_elapsed_ms(self._a, self._b, C.byref(ms)), "hn_event_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        try:
            lib = _lib.load()
            lib.hn_event_destroy(self._a)
            lib.hn_event_destroy(self._b)
        except Exception:
            pass


# ---------------------------------------------------------------------------------------
# Pose2Mesh lifter: Chebyshev graph convolution helpers (csrc/graph_ops.hip)
# ---------------------------------------------------------------------------------------
@dataclass
class CsrGraph:
    indptr: torch.Tensor   # int32 [V+1]
    indices: torch.Tensor  # int32 [nnz], ascending per row
    values: torch.Tensor   # fp32 [nnz]
    v: int


def csr_graph(L, device) -> CsrGraph:
    """scipy sparse matrix (or anything with .tocsr()) / torch sparse tensor -> device CSR."""
    if torch.is_tensor(L):
        c = L.coalesce() if L.layout == torch.sparse_coo else L.to_sparse_coo().coalesce()
        import scipy.sparse as sp
        idx = c.indices().cpu().numpy()
        L = sp.csr_matrix((c.values().cpu().numpy(), (idx[0], idx[1])), shape=tuple(c.shape))
    m = L.tocsr().astype(np.float32)
    m.sort_indices()
    if m.shape[0] != m.shape[1]:
        raise ValueError("graph Laplacian must be square")
    return CsrGraph(torch.from_numpy(m.indptr.astype(np.int32)).to(device), torch.from_numpy(m.indices.astype(np.int32)).to(device),
                    torch.from_numpy(m.data.astype(np.float32)).to(device), m.shape[0])


def cheby2_graph(L, device) -> CsrGraph:
    """2 L L - I as a device CSR (the second-order Chebyshev polynomial of the graph convolution, formed in fp64 on the host)."""
    import scipy.sparse as sp
    m = L.tocsr().astype(np.float64)
    q = (2.0 * (m @ m) - sp.identity(m.shape[0], dtype=np.float64, format="csr")).tocsr()
    q.sum_duplicates()
    return csr_graph(q, device)


def _csr_struct(g: CsrGraph):
    return _lib.GraphCsr(g.indptr.data_ptr(), g.indices.data_ptr(), g.values.data_ptr(), g.v)


def graph_conv_cheby3(g: CsrGraph, g2: CsrGraph, x, cw, relu=True, xin=None, up=1, out_split=False, out=None):
    """One Chebyshev graph convolution (K = 3) as ONE launch (hn_graph_conv_cheby3_f16x3): x fp32 [B,V,Fin] ->
    act(Linear([x0 | L x0 | (2 L L - I) x0]) + bias) (+ feature-axis interpolation of xin [B,V,Fi], rows repeated `up` times);
    cw: ConvW-like with .w [Fout,1,1,K], .w16, .bias over K = pad32(3 Fin) k-major channels.  -> fp32 [B,V*up,Fout] or, with
    out_split, the S32 operand [B,V*up,1,Fout/32,2,32]."""
    _req(x, name="x")
    b, v, fin = x.shape
    fout, _, _, k = cw.w.shape
    if v != g.v or g2.v != g.v or k != (3 * fin + 31) // 32 * 32:
        raise ValueError("graph / filter bank do not match the input")
    if xin is not None:
        _req(xin, name="xin")
        if tuple(xin.shape[:2]) != (b, v):
            raise ValueError("xin must be [B,V,Fi]")
    if out is not None:
        y = _req(out, torch.float16 if out_split else torch.float32, "out")
        if y.numel() != b * v * up * fout * (2 if out_split else 1):
            raise ValueError("out has the wrong size")
    elif out_split:
        y = torch.empty((b, v * up, 1, fout // 32, 2, 32), device=x.device, dtype=torch.float16)
    else:
        y = torch.empty((b, v * up, fout), device=x.device, dtype=torch.float32)
    wf = getattr(cw, "w_frag", None)       # (the filter bank in MFMA fragment order, ops.fragment_order(cw.w16): optional)
    check(_lib.load().hn_graph_conv_cheby3_f16x3(C.byref(_csr_struct(g)), C.byref(_csr_struct(g2)), ptr(x), b, fin,
                                                 ptr(wf if wf is not None else cw.w16), 1 if wf is not None else 0,
                                                 ptr(cw.bias), fout, 1 if relu else 0, ptr(xin), xin.shape[2] if xin is not None else 0,
                                                 up, ptr(y), 1 if out_split else 0, _stream()), "hn_graph_conv_cheby3_f16x3")
    return y


def fragment_order(w16):
    """Split filter bank [Fout, K/32, 2, 32] fp16 -> the same values in MFMA fragment order [ceil(Fout/16), K/32, 2, 64, 8]
    (hn_graph_conv_cheby3_f16x3 with w_frag = 1): element i of lane l = column 16 nt + (l & 15), channel 32 kt + 8 (l >> 4) + i,
    zero rows behind Fout."""
    fout, kt, _, _ = w16.shape
    nt = (fout + 15) // 16
    w = torch.zeros((nt * 16, kt, 2, 32), dtype=w16.dtype, device=w16.device)
    w[:fout] = w16
    # [nt, col 16, kt, pl, chunk 4, i 8] -> [nt, kt, pl, chunk, col, i]: lane = chunk * 16 + col
    return w.view(nt, 16, kt, 2, 4, 8).permute(0, 2, 3, 4, 1, 5).contiguous().view(nt, kt, 2, 64, 8)


def linear_rows(x, cw, scale=None, shift=None, residual=None, relu=False, n_out=None):
    """x fp32 [M <= 4, Kx] -> fp32 [M, N]: act(W pre(x) + bias (+ residual)) as a matrix-vector product (hn_linear_rows_f16x3);
    cw: ConvW-like 1x1 bank (.w [N,1,1,K], .w16, .bias), K >= Kx zero padded; scale / shift [Kx]: pre-activation affine + ReLU."""
    _req(x, name="x")
    m, kx = x.shape
    n, _, _, k = cw.w.shape
    y = torch.empty((m, n), device=x.device, dtype=torch.float32)
    for t, nm in ((scale, "scale"), (shift, "shift"), (residual, "residual")):
        if t is not None:
            _req(t, name=nm)
    check(_lib.load().hn_linear_rows_f16x3(ptr(x), m, x.stride(0), kx, ptr(scale), ptr(shift), ptr(cw.w16), k, n, ptr(cw.bias),
                                           ptr(residual), residual.stride(0) if residual is not None else 0, 1 if relu else 0,
                                           ptr(y), n, _stream()), "hn_linear_rows_f16x3")
    return y


def mesh_finish(mesh, perm, xyz_mm, valid=None, out=None, mirror=None):
    """mesh [N,V0,3], perm int64 [V] (graph_perm_reverse[:V]), xyz_mm [N,J,3] -> [N,V,3] = ((mesh[:, perm] * 1000 + xyz_mm[:, 0])
    / 1000) * (1, -1, -1): out['mesh'] of ros_demo.py:162,332-337, bit-identical to the numpy float32 arithmetic.
    mirror [N] int32 (hn_mesh_finish_mirror_f32): rows with mirror != 0 are meshes of mirrored hands -- the x of their raw
    vertices is negated before the arithmetic; then perm and xyz_mm may both be None: the raw vertices, x negated where
    mirrored, zero rows where valid != 1."""
    _req(mesh, name="mesh")
    n, v0, _ = mesh.shape
    if mirror is not None and perm is None and xyz_mm is None:
        v, joints = v0, 1
    else:
        _req(perm, torch.int64, "perm"); _req(xyz_mm, name="xyz_mm")
        v, joints = perm.shape[0], xyz_mm.shape[1]
    if out is None:
        out = torch.empty((n, v, 3), device=mesh.device, dtype=torch.float32)
    if valid is not None:
        _req(valid, torch.int32, "valid")
    if mirror is not None:
        if _req(mirror, torch.int32, "mirror").numel() != n:
            raise ValueError("mirror must hold one flag per row")
        check(_lib.load().hn_mesh_finish_mirror_f32(ptr(mesh), ptr(perm), ptr(xyz_mm), ptr(valid), ptr(mirror), n, v0, v, joints,
                                                    ptr(out), _stream()), "hn_mesh_finish_mirror_f32")
        return out
    check(_lib.load().hn_mesh_finish_f32(ptr(mesh), ptr(perm), ptr(xyz_mm), ptr(valid), n, v0, v, xyz_mm.shape[1], ptr(out), _stream()),
          "hn_mesh_finish_f32")
    return out


SMOOTH_WORDS = 4           # int32 words of a record of the filter's state: {xh, dxh as fp32 bits, track id, 0}
SMOOTH_JOINTS = 21         # joints of a slot in the live step's filter state


def check_smooth_options(min_cutoff=1.0, beta=0.007, d_cutoff=1.0, rate=30.0):
    """(min_cutoff, beta, d_cutoff, rate) of the smoothed step as floats: min_cutoff, d_cutoff (Hz) and rate (steps per second,
    dt = 1 / rate) finite and > 0, beta (stated for speeds in mm/s) finite and >= 0 -- also after the rounding to fp32 that the
    kernel's arguments get, and so is the vertices' beta, float32(1000 * beta) --, else ValueError."""
    def number(name, value, low_ok):
        try:
            f = float(value)
        except (TypeError, ValueError):
            f = math.nan
        with np.errstate(over="ignore"):
            g = float(np.float32(f))
        if not (math.isfinite(f) and math.isfinite(g) and (g >= 0 if low_ok else g > 0)):
            raise ValueError(f"{name} must be finite and {'>= 0' if low_ok else '> 0'} as fp32 (got {value!r})")
        return f
    mc, b, dc = number("smooth_min_cutoff", min_cutoff, False), number("smooth_beta", beta, True), number("smooth_d_cutoff", d_cutoff, False)
    number("smooth_beta * 1000", b * 1000.0, True)
    r = number("smooth_rate", rate, False)
    number("1 / smooth_rate", 1.0 / r, False)
    return mc, b, dc, r


def smooth_state(slots, joints, v, device):
    """The empty filter of `slots` hand slots with `joints` joints and v vertices each: zeroed int32 [slots, joints + v, 3, 4]
    (one 16-byte record per coordinate, a slot's joints first, then its vertices; reset: state.zero_())."""
    slots, joints, v = int(slots), int(joints), int(v)
    if slots <= 0 or joints <= 0 or v <= 0:
        raise ValueError(f"smooth_state: slots, joints and v must be positive (got {slots}, {joints}, {v})")
    return torch.zeros((slots, joints + v, 3, SMOOTH_WORDS), device=device, dtype=torch.int32)


def mesh_finish_smooth(mesh, perm, xyz_mm, lifted, has_hand, track_id, dt, state, min_cutoff=1.0, beta=0.007, d_cutoff=1.0,
                       mirror=None, out=None, smooth_xyz=None, smooth_mesh=None):
    """mesh_finish(mesh, perm, xyz_mm, valid=lifted, mirror=mirror) and, in the same launch (hn_mesh_finish_smooth_f32), a One
    Euro filter over time on every coordinate of that final mesh (gate: lifted == 1) and of xyz_mm (gate: has_hand == 1)
    -> (mesh [N,V,3], smooth_xyz [N,J,3], smooth_mesh [N,V,3]).  lifted, has_hand, track_id: int32 [N]; dt: ONE fp32 word on
    the device (seconds since the last step); state: smooth_state(N, J, V), updated in place.  A row's filter restarts when
    its gate was off or its track id changed; beta is stated for mm/s, the vertices (metres) use float32(1000 * beta)."""
    mc, b, dc, _ = check_smooth_options(min_cutoff, beta, d_cutoff)
    _req(mesh, name="mesh"); _req(perm, torch.int64, "perm"); _req(xyz_mm, name="xyz_mm")
    n, v0, _ = mesh.shape
    v, joints = perm.shape[0], xyz_mm.shape[1]
    if xyz_mm.shape[0] != n:
        raise ValueError("xyz_mm must hold one row per mesh")
    for name, t in (("lifted", lifted), ("has_hand", has_hand), ("track_id", track_id)) + ((("mirror", mirror),) if mirror is not None else ()):
        if _req(t, torch.int32, name).numel() != n:
            raise ValueError(f"{name} must hold one int32 per row")
    if _req(dt, name="dt").numel() != 1:
        raise ValueError("dt must be one fp32 word on the device")
    if _req(state, torch.int32, "state").numel() != n * (joints + v) * 3 * SMOOTH_WORDS:
        raise ValueError(f"state must be smooth_state({n}, {joints}, {v}): int32 [{n},{joints + v},3,{SMOOTH_WORDS}]")
    if out is None:
        out = torch.empty((n, v, 3), device=mesh.device, dtype=torch.float32)
    if smooth_xyz is None:
        smooth_xyz = torch.empty((n, joints, 3), device=mesh.device, dtype=torch.float32)
    if smooth_mesh is None:
        smooth_mesh = torch.empty((n, v, 3), device=mesh.device, dtype=torch.float32)
    _req(out, name="out"); _req(smooth_xyz, name="smooth_xyz"); _req(smooth_mesh, name="smooth_mesh")
    if out.numel() != n * v * 3 or smooth_mesh.numel() != n * v * 3 or smooth_xyz.numel() != n * joints * 3:
        raise ValueError("out / smooth_mesh must hold [N,V,3] and smooth_xyz [N,J,3] values")
    check(_lib.load().hn_mesh_finish_smooth_f32(ptr(mesh), ptr(perm), ptr(xyz_mm), ptr(lifted), ptr(has_hand), ptr(mirror),
                                                ptr(track_id), ptr(dt), ptr(state), n, v0, v, joints, mc, b,
                                                float(np.float32(b * 1000.0)), dc, ptr(out), ptr(smooth_xyz), ptr(smooth_mesh),
                                                _stream()), "hn_mesh_finish_smooth_f32")
    return out, smooth_xyz, smooth_mesh


def camera_paras(paras):
    """The caller's intrinsics as the engines keep them: one camera (fx, fy, cx, cy) -> a tuple of four floats, as ever; a
    camera per frame -- a nested sequence, an ndarray or a tensor [N,4] -- -> a float32 ndarray [N,4] (the rounding to fp32 that
    the one camera's values get when they are passed to a kernel).  None stays None."""
    if paras is None:
        return None
    if torch.is_tensor(paras):
        paras = paras.detach().cpu().numpy()
    if np.ndim(paras) < 2:
        return tuple(float(v) for v in paras)
    table = np.ascontiguousarray(np.asarray(paras, dtype=np.float64).astype(np.float32))
    if table.ndim != 2 or table.shape[1] != 4 or table.shape[0] == 0:
        raise ValueError(f"paras: one camera (fx, fy, cx, cy) or a camera per frame [N,4], got shape {tuple(table.shape)}")
    return table


def mesh_faces(faces, vertices, device):
    """The caller's face list (mesh_model.face: numpy / tensor / list, [F,3] vertex indices) checked ON THE HOST against the
    vertex count and uploaded once: int32 [F,3] on `device`, what mesh_render and the live engines draw with."""
    f = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0 or f.dtype.kind not in "iu":
        raise ValueError(f"faces: expected a non-empty integer [F,3] list, got {f.dtype} {tuple(f.shape)}")
    if int(f.min()) < 0 or int(f.max()) >= vertices:
        raise ValueError(f"faces use vertex {int(f.min())}..{int(f.max())} of a mesh with {vertices} vertices")
    return torch.from_numpy(np.ascontiguousarray(f.astype(np.int32))).to(device)


def mesh_render_scratch_bytes(slots, faces):
    return int(_lib.load().hn_mesh_render_scratch_bytes(slots, faces))


OCCLUDE_MARGIN = 0.03      # metres; a starting value, NOT tuned on this model


def check_occlude_margin(margin) -> float:
    """occlude_margin as a float that is finite in fp32 (it is a kernel argument)."""
    m = float(margin)
    if not math.isfinite(m) or abs(m) > float(np.finfo(np.float32).max):
        raise ValueError(f"occlude_margin: a finite number of metres (got {margin!r})")
    return m


# What the depth passes' wrappers (mesh_render, hand_cloud, mesh_fit, mesh_geometry, mesh_fit_iters) share.  `anchor` names the
# tensor whose device the others must be on, in the words of the caller's message ("the mesh", "the silhouette").

def _on_device(name, t, device, anchor):
    if t.device != device:
        raise ValueError(f"{name} on {t.device} but {anchor} on {device}")


def _slot_meshes(mesh):
    """mesh fp32 [S,V,3] or [N,K,V,3] -> (mesh [S,V,3], S, V)"""
    _req(mesh, name="mesh")
    if mesh.dim() == 4:
        mesh = mesh.view(-1, mesh.shape[2], 3)
    if mesh.dim() != 3 or mesh.shape[2] != 3:
        raise ValueError(f"mesh: expected [S,V,3], got {tuple(mesh.shape)}")
    return mesh, mesh.shape[0], mesh.shape[1]


def _faces_arg(faces, device, nonempty=False):
    """faces [F,3]: an int32 GPU tensor, or a host list, which the C entry checks index by index and this call uploads ->
    (the GPU tensor, a pointer to the host list or None, F)"""
    host = None
    if not (torch.is_tensor(faces) and faces.is_cuda):
        host = np.ascontiguousarray(np.asarray(faces.cpu() if torch.is_tensor(faces) else faces).astype(np.int32))
        if host.ndim != 2 or host.shape[1] != 3:
            raise ValueError(f"faces: expected [F,3], got {tuple(host.shape)}")
        faces = torch.from_numpy(host).to(device)
    _req(faces, torch.int32, "faces")
    if faces.dim() != 2 or faces.shape[1] != 3 or (nonempty and faces.shape[0] < 1):
        raise ValueError(f"faces: expected {'a non-empty ' if nonempty else ''}[F,3], got {tuple(faces.shape)}")
    # (data_as: the pointer keeps the host array alive until the caller has made its call)
    return faces, (host.ctypes.data_as(C.c_void_p) if host is not None else None), int(faces.shape[0])


def _lifted_arg(lifted, s):
    if lifted is not None:
        _req(lifted, torch.int32, "lifted")
        if lifted.numel() != s:
            raise ValueError(f"lifted: expected {s} flags, got {lifted.numel()}")
    return lifted


def _camera_arg(paras, n, device, anchor):
    """paras -> (the one camera's four values for a by-value argument, None), or -- a camera per frame: a device table fp32
    [N,4] -- (None, the table's address)"""
    if torch.is_tensor(paras) and paras.dim() != 1:
        if paras.dtype != torch.float32 or tuple(paras.shape) != (n, 4):
            raise ValueError(f"paras: a camera per frame is fp32 [{n},4] (fx, fy, cx, cy), got {paras.dtype} {tuple(paras.shape)}")
        _on_device("paras", paras, device, anchor)
        return None, ptr(_req(paras, torch.float32, "paras"))
    return (C.c_float * 4)(*[float(x) for x in paras]), None


def _scene_depth_arg(scene_depth, n, h, w, device, anchor):
    """The camera's depth map, fp32 [N,1,H,W], [N,H,W] or RGBD [N,4,H,W] (channel 3 is read in place) -> (the address of frame
    0's depth, the frame stride in elements)"""
    _req(scene_depth, name="scene_depth")
    _on_device("scene_depth", scene_depth, device, anchor)
    shape = tuple(scene_depth.shape)
    if shape not in ((n, 1, h, w), (n, h, w), (n, 4, h, w)):
        raise ValueError(f"scene_depth: expected fp32 [{n},1,{h},{w}], [{n},{h},{w}] or RGBD [{n},4,{h},{w}], got {shape}")
    rgbd = len(shape) == 4 and shape[1] == 4
    return scene_depth.data_ptr() + (3 * h * w * 4 if rgbd else 0), (4 if rgbd else 1) * h * w


def _depth_maps(mesh_depth, silhouette, k):
    """What the occluded raster leaves, silhouette uint8 [N,H,W] and mesh_depth fp32 of as many values -> (N, H, W, int k)"""
    if silhouette.dim() != 3:
        raise ValueError(f"silhouette: expected uint8 [N,H,W], got {tuple(silhouette.shape)}")
    n, h, w = (int(v) for v in silhouette.shape)
    if mesh_depth.numel() != n * h * w:
        raise ValueError(f"mesh_depth: expected fp32 [{n},{h},{w}], got {tuple(mesh_depth.shape)}")
    k = int(k)
    if not 1 <= k <= 16:
        raise ValueError(f"the silhouette's byte holds at most 16 slots per frame (k = {k})")
    return n, h, w, k


def _fit_meshes(mesh, xyz_mm, s):
    """mesh fp32 [s,V,3] and xyz_mm fp32 [s,J,3] -> (V, J)"""
    if mesh.dim() != 3 or mesh.shape[0] != s or mesh.shape[2] != 3 or mesh.shape[1] < 1:
        raise ValueError(f"mesh: expected fp32 [{s},V,3], got {tuple(mesh.shape)}")
    if xyz_mm.dim() != 3 or xyz_mm.shape[0] != s or xyz_mm.shape[2] != 3 or xyz_mm.shape[1] < 1:
        raise ValueError(f"xyz_mm: expected fp32 [{s},J,3], got {tuple(xyz_mm.shape)}")
    return int(mesh.shape[1]), int(xyz_mm.shape[1])


def _out_parts(out, specs, device):
    """specs: (name, dtype, shape) per output -> the tensors, allocated, or `out`'s attributes of those names, viewed in shape"""
    parts = []
    for name, dtype, shp in specs:
        t = torch.empty(shp, device=device, dtype=dtype) if out is None else getattr(out, name)
        if _req(t, dtype, name).numel() != math.prod(shp):
            raise ValueError(f"{name}: expected {dtype} {list(shp)}, got {tuple(t.shape)}")
        parts.append(t.view(shp))
    return parts


def _scratch_arg(scratch, device, size, *dims, name="scratch"):
    """the caller's byte buffer, or one of size(*dims) bytes"""
    if scratch is None:
        scratch = torch.empty((size(*dims),), device=device, dtype=torch.uint8)
    return _req(scratch, torch.uint8, name)


def _check_count(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= 2 ** 31 - 1:
        raise ValueError(f"{name}: an integer >= 1 (got {value!r})")


def _check_band(name, b, given, limit):
    """b, `given` as a float (NaN: not a number): finite and in (0, limit] metres, also as the fp32 kernel argument it becomes"""
    with np.errstate(over="ignore"):
        g = float(np.float32(b))
    if not (math.isfinite(b) and 0.0 < g <= limit and b <= limit):
        raise ValueError(f"{name}: a finite number of metres in (0, {limit:g}] as fp32 (got {given!r})")


def mesh_render(mesh, faces, paras, frame, lifted=None, k=1, out=None, depth_out=None, scratch=None, *, scene_depth=None,
                margin=OCCLUDE_MARGIN, silhouette_out=None, coverage_out=None):
    """The meshes drawn over their frames (hn_mesh_render_u8; render() of ros_demo.py:86-116 without a graphics pipeline):
    mesh fp32 [S,V,3] or [N,K,V,3] as mesh_finish writes it, S = N * k slots; faces [F,3]: an int32 GPU tensor (mesh_faces) or
    a host list (checked index by index and uploaded by THIS call: a caller that renders repeatedly uploads once with mesh_faces
    and passes the tensor, as the live engines do); paras (fx, fy, cx, cy), or -- a camera per frame, hn_mesh_render_cams_u8 /
    _cams_occluded_u8, DESIGN.md section 9h -- an fp32 tensor [N,4] on the mesh's device, row i for the k slots of frame i
    (ValueError for another shape, dtype or device); frame fp32 [N,3,H,W] in 0..1 or uint8 [N,H,W,3]
    'bgr8', on the GPU; lifted int32 [S] (0: the slot is not drawn).  Returns the overlay uint8 [N,H,W,3] RGB (`out`);
    depth_out fp32 [N,H,W], when given, receives the drawn Z (0 where nothing was drawn).
    scene_depth (hn_mesh_render_occluded_u8): the camera's depth map in metres, fp32 [N,1,H,W], [N,H,W]
    or an [N,4,H,W] RGBD tensor (channel 3 is read in place), on the mesh's device and of the frames' size.  A covered pixel
    whose depth value D is finite and > 0 and whose nearest mesh Z > D + margin (fp32, strict) is hidden: it keeps the frame's
    pixel.  The call then returns (overlay, silhouette uint8 [N,H,W]: 0 no mesh, slot + 1 shown, 0x80 | (slot + 1) hidden --
    slot within the frame, k <= 16 --, coverage int32 [S,2]: per slot, the pixels where its mesh is the nearest and those of
    them that are shown), written into silhouette_out / coverage_out when given; depth_out holds the nearest mesh Z on every
    covered pixel, hidden or not.  Without scene_depth the call is the plain one and the three other keywords must stay unset."""
    mesh, s, v = _slot_meshes(mesh)
    faces, fh, f = _faces_arg(faces, mesh.device)
    if frame.dtype == torch.uint8:
        _req(frame, torch.uint8, "frame")
        fmt, (n, h, w) = _lib.FRAME_U8_BGR_HWC, frame.shape[:3]
        ok = frame.dim() == 4 and frame.shape[3] == 3
    else:
        _req(frame, name="frame")
        fmt, n, (h, w) = _lib.FRAME_F32_CHW, frame.shape[0], frame.shape[2:]
        ok = frame.dim() == 4 and frame.shape[1] == 3
    if not ok:
        raise ValueError(f"frame: expected fp32 [N,3,H,W] or uint8 [N,H,W,3], got {frame.dtype} {tuple(frame.shape)}")
    if k < 1 or n * k != s:
        raise ValueError(f"{s} mesh slots for {n} frames with k = {k} slots per frame")
    _lifted_arg(lifted, s)
    if out is None:
        out = torch.empty((n, h, w, 3), device=mesh.device, dtype=torch.uint8)
    _req(out, torch.uint8, "out")
    if out.numel() != n * h * w * 3:
        raise ValueError(f"out: expected uint8 [{n},{h},{w},3], got {tuple(out.shape)}")
    if depth_out is not None:
        _req(depth_out, name="depth_out")
        if depth_out.numel() != n * h * w:
            raise ValueError(f"depth_out: expected fp32 [{n},{h},{w}], got {tuple(depth_out.shape)}")
    scratch = _scratch_arg(scratch, mesh.device, mesh_render_scratch_bytes, s, f)
    # a camera per frame: a device table [N,4] (hn_mesh_render_cams_*); else the one camera's four values, passed by value
    host4, cams = _camera_arg(paras, n, mesh.device, "the mesh")
    p4 = host4 if cams is None else cams
    plain, occluded = ("hn_mesh_render_cams_u8", "hn_mesh_render_cams_occluded_u8") if cams else (
        "hn_mesh_render_u8", "hn_mesh_render_occluded_u8")
    if scene_depth is None:
        if silhouette_out is not None or coverage_out is not None:
            raise ValueError("silhouette_out / coverage_out belong to the occluded call: give scene_depth")
        check(getattr(_lib.load(), plain)(ptr(mesh), ptr(faces), fh, ptr(lifted), s, v, f, k, p4, ptr(frame), fmt, h, w,
                                          ptr(scratch), scratch.numel(), ptr(out), ptr(depth_out), _stream()), plain)
        return out.view(n, h, w, 3)
    margin = check_occlude_margin(margin)
    depth_ptr, depth_stride = _scene_depth_arg(scene_depth, n, h, w, mesh.device, "the mesh")
    if k > 16:
        raise ValueError(f"the silhouette's byte holds at most 16 slots per frame (k = {k})")
    if silhouette_out is None:
        silhouette_out = torch.empty((n, h, w), device=mesh.device, dtype=torch.uint8)
    _req(silhouette_out, torch.uint8, "silhouette_out")
    if silhouette_out.numel() != n * h * w:
        raise ValueError(f"silhouette_out: expected uint8 [{n},{h},{w}], got {tuple(silhouette_out.shape)}")
    if coverage_out is None:
        coverage_out = torch.empty((s, 2), device=mesh.device, dtype=torch.int32)
    _req(coverage_out, torch.int32, "coverage_out")
    if coverage_out.numel() != s * 2:
        raise ValueError(f"coverage_out: expected int32 [{s},2], got {tuple(coverage_out.shape)}")
    check(getattr(_lib.load(), occluded)(ptr(mesh), ptr(faces), fh, ptr(lifted), s, v, f, k, p4, ptr(frame), fmt, h, w,
                                         depth_ptr, depth_stride, margin, ptr(scratch), scratch.numel(),
                                         ptr(out), ptr(depth_out), ptr(silhouette_out), ptr(coverage_out), _stream()), occluded)
    return out.view(n, h, w, 3), silhouette_out.view(n, h, w), coverage_out.view(s, 2)


RIG_RADIUS = 0.08          # metres; a starting value, NOT tuned on this model
RIG_MAX_SLOTS = 256        # frames * hands of a rig step: the association runs in one 256-thread workgroup
RIG_ORTHO_TOL = 1e-4       # max |R^T R - I| of a caller's rotation (an fp32-rounded rotation sits near 1e-7)

RIG_FIELDS = ("rig_xyz", "rig_mesh", "rig_hand", "rig_count", "rig_views", "rig_seed", "fused_xyz", "fused_mesh")
RigFused = collections.namedtuple("RigFused", RIG_FIELDS)


def rig_extrinsics(ext, frames=None):
    """The caller's camera -> rig extrinsics, checked ON THE HOST and rounded to fp32 once (as camera_paras rounds the
    intrinsics): one [R | t] per frame, [N,3,4] or [N,4,4] with the last row (0, 0, 0, 1) -- a nested sequence, an ndarray or a
    tensor; p_rig = R p_cam + t, t in metres -- -> a float32 ndarray [N,12], the rows of [R | t], what the device table holds.
    ValueError: another shape (or N != frames), a value that is not finite as fp32, another last row, a rotation with
    max |R^T R - I| > 1e-4 or det R <= 0 (a scaled or reflected frame)."""
    if torch.is_tensor(ext):
        ext = ext.detach().cpu().numpy()
    try:
        e = np.asarray(ext, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise ValueError(f"extrinsics: one [R | t] per frame, [N,3,4] or [N,4,4] ({err})") from None
    if e.ndim != 3 or e.shape[0] == 0 or tuple(e.shape[1:]) not in ((3, 4), (4, 4)) or (frames is not None and e.shape[0] != frames):
        raise ValueError(f"extrinsics: one [R | t] per frame, [N,3,4] or [N,4,4]"
                         + (f" with N = {frames}" if frames is not None else "") + f", got shape {tuple(e.shape)}")
    with np.errstate(over="ignore"):
        rows = e[:, :3, :].astype(np.float32)
    if not (np.isfinite(e).all() and np.isfinite(rows).all()):
        raise ValueError("extrinsics: every value must be finite as fp32")
    if e.shape[1] == 4 and not np.array_equal(e[:, 3, :], np.tile([0.0, 0.0, 0.0, 1.0], (e.shape[0], 1))):
        raise ValueError("extrinsics: the last row of a [4,4] transform must be (0, 0, 0, 1)")
    r = rows[:, :, :3].astype(np.float64)
    off = np.abs(np.swapaxes(r, 1, 2) @ r - np.eye(3)).max(axis=(1, 2))
    det = np.linalg.det(r)
    for i in range(e.shape[0]):
        if not off[i] <= RIG_ORTHO_TOL or not det[i] > 0:
            raise ValueError(f"extrinsics: row {i} is no rotation (max |R^T R - I| = {off[i]:.3g}, det R = {det[i]:.3g}): a rigid "
                             "camera -> rig transform has an orthonormal R with det +1")
    return np.ascontiguousarray(rows.reshape(e.shape[0], 12))


def check_rig_radius(radius) -> float:
    """rig_radius as a float that is finite and > 0, also as the fp32 kernel argument it becomes, else ValueError."""
    try:
        r = float(radius)
    except (TypeError, ValueError):
        r = math.nan
    with np.errstate(over="ignore"):
        g = float(np.float32(r))
    if not (math.isfinite(r) and math.isfinite(g) and g > 0):
        raise ValueError(f"rig_radius: a finite number of metres > 0 as fp32 (got {radius!r})")
    return r


def check_rig_slots(frames, hands) -> int:
    """frames * hands of a rig step, at most 256 (the association's one workgroup), else ValueError."""
    slots = int(frames) * int(hands)
    if int(frames) < 1 or int(hands) < 1 or slots > RIG_MAX_SLOTS:
        raise ValueError(f"a rig step holds at most {RIG_MAX_SLOTS} slots: {frames} frames x {hands} hands = {slots}")
    return slots


def rig_fuse(xyz_mm, mesh, has_hand, lifted, score, extrinsics_table, k, radius=RIG_RADIUS, side=None, out=None) -> RigFused:
    """The hands of N cameras x k slots in ONE frame, one entry per physical hand (hn_rig_fuse_f32: three launches; DESIGN.md
    section 9i, tests/rig_ref.py is the rule and the outputs equal it bit for bit).  xyz_mm fp32 [S,J,3] or [N,k,J,3] (camera
    frame, millimetres), mesh fp32 [S,V,3] or [N,k,V,3] (the final mesh, out['mesh']), has_hand / lifted int32 [S], score fp32
    [S], S = N * k <= 256; extrinsics_table fp32 [N,12] on the same device (rig_extrinsics(...) uploaded); side int32 [S]: only
    slots of one side are put together (None: no gate).  Returns RigFused: rig_xyz [N,k,J,3], rig_mesh [N,k,V,3], rig_hand
    [N,k] int32, rig_count [1] int32, rig_views / rig_seed [S] int32, fused_xyz [S,J,3], fused_mesh [S,V,3] -- allocated, or
    `out`'s attributes of these names (the live step's buffer views), every one fully written."""
    _req(xyz_mm, name="xyz_mm"); _req(mesh, name="mesh"); _req(extrinsics_table, name="extrinsics_table")
    if xyz_mm.dim() == 4:
        xyz_mm = xyz_mm.view(-1, xyz_mm.shape[2], 3)
    if mesh.dim() == 4:
        mesh = mesh.view(-1, mesh.shape[2], 3)
    if xyz_mm.dim() != 3 or mesh.dim() != 3 or xyz_mm.shape[2] != 3 or mesh.shape[2] != 3 or xyz_mm.shape[0] != mesh.shape[0]:
        raise ValueError(f"xyz_mm [S,J,3] and mesh [S,V,3] of the same S slots, got {tuple(xyz_mm.shape)} and {tuple(mesh.shape)}")
    s, joints, _ = xyz_mm.shape
    v, k = mesh.shape[1], int(k)
    if k < 1 or s % k or s == 0 or joints == 0 or v == 0:
        raise ValueError(f"{s} slots with k = {k} slots per frame, {joints} joints, {v} vertices")
    n = s // k
    check_rig_slots(n, k)
    if extrinsics_table.dim() != 2 or tuple(extrinsics_table.shape) != (n, 12):
        raise ValueError(f"extrinsics_table: fp32 [{n},12], a row per frame, got {tuple(extrinsics_table.shape)}")
    radius = check_rig_radius(radius)
    for name, t, dtype in (("has_hand", has_hand, torch.int32), ("lifted", lifted, torch.int32), ("score", score, torch.float32)) + (
            (("side", side, torch.int32),) if side is not None else ()):
        if _req(t, dtype, name).numel() != s:
            raise ValueError(f"{name} must hold one value per slot ({s}), got {t.numel()}")
    shapes = dict(rig_xyz=(n, k, joints, 3), rig_mesh=(n, k, v, 3), rig_hand=(n, k), rig_count=(1,), rig_views=(s,), rig_seed=(s,),
                  fused_xyz=(s, joints, 3), fused_mesh=(s, v, 3))
    parts = []
    for name in RIG_FIELDS:
        dtype = torch.float32 if name.endswith(("xyz", "mesh")) else torch.int32
        t = torch.empty(shapes[name], device=mesh.device, dtype=dtype) if out is None else getattr(out, name)
        if _req(t, dtype, name).numel() != math.prod(shapes[name]):
            raise ValueError(f"{name}: expected {dtype} {list(shapes[name])}, got {tuple(t.shape)}")
        parts.append(t.view(shapes[name]))
    check(_lib.load().hn_rig_fuse_f32(ptr(xyz_mm), ptr(mesh), ptr(has_hand), ptr(lifted), ptr(score), ptr(side),
                                      ptr(extrinsics_table), n, k, joints, v, radius, *(ptr(t) for t in parts), _stream()),
          "hn_rig_fuse_f32")
    return RigFused(*parts)


CLOUD_POINTS = 4096        # rows per slot of a hand cloud; a starting value, NOT tuned on this model
CLOUD_BAND = 0.03          # metres between the measured depth and the mesh Z; a starting value, NOT tuned on this model
CLOUD_STRIDE = 2           # every second row and column is a candidate; a starting value, NOT tuned on this model
CLOUD_MAX_BAND = 100.0     # metres: the residual in micrometres then fits an int32

HandCloud = collections.namedtuple("HandCloud", "cloud count resid")


def check_cloud(points=CLOUD_POINTS, band=CLOUD_BAND, stride=CLOUD_STRIDE):
    """A hand cloud's three parameters as (int points >= 1, float band, int stride >= 1), the band finite and in (0, 100] metres
    also as the fp32 kernel argument it becomes; else ValueError.  The defaults (4096 rows, 0.03 m, every second row and column)
    are starting values, NOT tuned on this model."""
    _check_count("cloud_points", points)
    _check_count("cloud_stride", stride)
    try:
        b = float(band)
    except (TypeError, ValueError):
        b = math.nan
    _check_band("cloud_band", b, band, CLOUD_MAX_BAND)
    return int(points), b, int(stride)


def hand_cloud_scratch_bytes(frames, k, h):
    return int(_lib.load().hn_hand_cloud_scratch_bytes(frames, k, h))


def hand_cloud(mesh_depth, silhouette, scene_depth, paras, k, *, points=CLOUD_POINTS, band=CLOUD_BAND, stride=CLOUD_STRIDE,
               extrinsics_table=None, out=None, scratch=None) -> HandCloud:
    """Each hand's measured depth pixels as a compact 3-D point cloud (hn_hand_cloud_f32: two launches, csrc/hand_cloud.hip;
    DESIGN.md section 9j, tests/cloud_ref.py is the rule and the outputs equal it bit for bit).  mesh_depth fp32 [N,H,W] and
    silhouette uint8 [N,H,W] are what the occluded mesh_render leaves (depth_out, the silhouette); scene_depth is the depth map
    it was given: fp32 [N,1,H,W], [N,H,W] or an RGB-D [N,4,H,W] (channel 3 is read in place); paras (fx, fy, cx, cy) on the
    host, or an fp32 tensor [N,4] on the device, a camera per frame, as mesh_render takes it; k slots per frame (1..16).
    A pixel (r, c) with r % stride == 0 and c % stride == 0 matches slot j of frame i when (silhouette & 0x7F) == j + 1 (hidden
    or not), its depth D is finite and > 0 and |D - mesh_depth| <= band metres; its point is ((c + 0.5 - cx) D / fx,
    (r + 0.5 - cy) D / fy, D): metres in the camera frame of xyz_mm (x right, y down, z forward), the pixel centre at +0.5 as
    the raster samples it -- or, with extrinsics_table (fp32 [N,12] on the device, rig_extrinsics(...) uploaded), that point in
    the rig frame.  Returns HandCloud: cloud fp32 [N*k,points,3] -- slot s = i * k + j: its first min(total, points) matches in
    row-major order, zero rows behind them --, count int32 [N*k,2] = (total matches, rows written), resid int64 [N*k] = the sum
    of rint((D - mesh_depth) * 1e6) over ALL matches, micrometres: how far the mesh sits from the surface the camera sees.
    Allocated, or `out`'s attributes cloud / cloud_count / cloud_resid (the live step's buffer views), every one fully written.
    points = 4096, band = 0.03 m and stride = 2 are starting values, NOT tuned on this model."""
    points, band, stride = check_cloud(points, band, stride)
    _req(mesh_depth, name="mesh_depth"); _req(silhouette, torch.uint8, "silhouette"); _req(scene_depth, name="scene_depth")
    n, h, w, k = _depth_maps(mesh_depth, silhouette, k)
    _on_device("mesh_depth", mesh_depth, silhouette.device, "the silhouette")
    depth_ptr, depth_stride = _scene_depth_arg(scene_depth, n, h, w, silhouette.device, "the silhouette")
    host4, table = _camera_arg(paras, n, silhouette.device, "the silhouette")
    if extrinsics_table is not None:
        _req(extrinsics_table, name="extrinsics_table")
        if tuple(extrinsics_table.shape) != (n, 12) or extrinsics_table.device != silhouette.device:
            raise ValueError(f"extrinsics_table: fp32 [{n},12] on {silhouette.device}, a row per frame, got "
                             f"{tuple(extrinsics_table.shape)} on {extrinsics_table.device}")
    s = n * k
    parts = _out_parts(out, (("cloud", torch.float32, (s, points, 3)), ("cloud_count", torch.int32, (s, 2)),
                             ("cloud_resid", torch.int64, (s,))), silhouette.device)
    scratch = _scratch_arg(scratch, silhouette.device, hand_cloud_scratch_bytes, n, k, h)
    check(_lib.load().hn_hand_cloud_f32(ptr(mesh_depth), ptr(silhouette), depth_ptr, depth_stride, host4, table,
                                        ptr(extrinsics_table), n, k, h, w, points, stride, band, ptr(scratch), scratch.numel(),
                                        *(ptr(t) for t in parts), _stream()), "hn_hand_cloud_f32")
    return HandCloud(*parts)


FIT_BAND = 0.03            # metres between the measured depth and the mesh Z; a starting value, NOT tuned on this model
FIT_STRIDE = 2             # every second row and column is a candidate; a starting value, NOT tuned on this model
FIT_MIN_POINTS = 200       # fewer matches: the slot is left as it is; a starting value, NOT tuned on this model
FIT_DAMP = 1e-3            # Levenberg damping per match; a starting value, NOT tuned on this model
FIT_MAX_SHIFT = 0.05       # metres: a larger step is refused; a starting value, NOT tuned on this model
FIT_MAX_ANGLE = 0.35       # radians: a larger step is refused; a starting value, NOT tuned on this model
FIT_MAX_BAND = 100.0       # metres

MeshFit = collections.namedtuple("MeshFit", "mesh xyz rt count cost")


def check_fit(band=FIT_BAND, stride=FIT_STRIDE, min_points=FIT_MIN_POINTS, damp=FIT_DAMP, max_shift=FIT_MAX_SHIFT,
              max_angle=FIT_MAX_ANGLE):
    """A mesh fit's six parameters as (float band, int stride >= 1, int min_points >= 1, float damp >= 0, float max_shift > 0,
    float max_angle in (0, pi)), the band finite and in (0, 100] metres also as the fp32 kernel argument it becomes; else
    ValueError.  The defaults (0.03 m, every second row and column, 200 matches, 1e-3, 0.05 m, 0.35 rad) are starting values,
    NOT tuned on this model."""
    _check_count("fit_stride", stride)
    _check_count("fit_min_points", min_points)

    def number(value):
        try:
            return math.nan if isinstance(value, bool) else float(value)
        except (TypeError, ValueError):
            return math.nan
    b, lam, shift, angle = number(band), number(damp), number(max_shift), number(max_angle)
    _check_band("fit_band", b, band, FIT_MAX_BAND)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"fit_damp: a finite number >= 0 (got {damp!r})")
    if not (math.isfinite(shift) and shift > 0.0 and math.isfinite(shift * shift) and shift * shift > 0.0):
        raise ValueError(f"fit_max_shift: a finite number of metres > 0 whose square is finite and > 0 (got {max_shift!r})")
    if not (math.isfinite(angle) and 0.0 < angle < math.pi and 0.0 < math.tan(angle / 2.0) ** 2 < math.inf):
        raise ValueError(f"fit_max_angle: radians in (0, pi) (got {max_angle!r})")
    return b, int(stride), int(min_points), lam, shift, angle


def fit_caps(max_shift, max_angle):
    """the two caps as the doubles the kernel takes: max_shift^2 and tan^2(max_angle / 2)"""
    half = math.tan(max_angle / 2.0)
    return max_shift * max_shift, half * half


def _fit_specs(s, v, joints):
    """a fit's outputs as _out_parts takes them"""
    return (("fit_mesh", torch.float32, (s, v, 3)), ("fit_xyz", torch.float32, (s, joints, 3)), ("fit_rt", torch.float32, (s, 12)),
            ("fit_count", torch.int32, (s, 2)), ("fit_cost", torch.int64, (s,)))


def mesh_fit_scratch_bytes(frames, k, h):
    return int(_lib.load().hn_mesh_fit_scratch_bytes(frames, k, h))


def mesh_fit(mesh_depth, silhouette, scene_depth, paras, mesh, xyz_mm, k, *, band=FIT_BAND, stride=FIT_STRIDE,
             min_points=FIT_MIN_POINTS, damp=FIT_DAMP, max_shift=FIT_MAX_SHIFT, max_angle=FIT_MAX_ANGLE, out=None,
             scratch=None) -> MeshFit:
    """Each hand's mesh fitted to its measured depth: one Gauss-Newton step of projective point-to-plane alignment per hand
    slot (hn_mesh_fit_f32: two launches, csrc/mesh_fit.hip; DESIGN.md section 9k, tests/fit_ref.py is the rule and the outputs
    equal it bit for bit).  mesh_depth fp32 [N,H,W], silhouette uint8 [N,H,W], scene_depth and paras: as hand_cloud takes
    them; mesh fp32 [N*k,V,3]: the meshes the raster drew (metres, (x, -y, -z) of the camera point); xyz_mm fp32 [N*k,J,3]:
    camera millimetres, joint 0 the root the motion turns about; k slots per frame (1..16).
    A pixel (r, c) off the frame's border with r % stride == 0 and c % stride == 0 matches slot j of frame i when
    (silhouette & 0x7F) == j + 1 there and at its four neighbours, mesh_depth > 0 at all five, its depth D is finite and > 0,
    |D - mesh_depth| <= band metres, its normal (from mesh_depth) is not seen at a grazing angle and its lever and residual
    are bounded.  The damped (damp per match) normal equations are summed as integers and solved in fp64.  Returns MeshFit:
    mesh fp32 [N*k,V,3] and xyz fp32 [N*k,J,3] -- moved by x' = R (x - c0) + c0 + t, c0 the root joint --, rt fp32 [N*k,12] = R
    row-major, then t (metres, camera frame), count int32 [N*k,2] = (matches, status: 0 fitted, 1 fewer than min_points
    matches, 2 no solution, 3 beyond max_shift metres or max_angle radians; != 0: R = I, t = 0, mesh and xyz are byte copies),
    cost int64 [N*k] = the summed squared residual in 2^-30 m^2 (RMS = sqrt(cost / 2^30 / matches)).
    Allocated, or `out`'s attributes fit_mesh / fit_xyz / fit_rt / fit_count / fit_cost (the live step's buffer views), every
    one fully written.  band = 0.03 m, stride = 2, min_points = 200, damp = 1e-3, max_shift = 0.05 m and max_angle = 0.35 rad
    are starting values, NOT tuned on this model."""
    band, stride, min_points, damp, max_shift, max_angle = check_fit(band, stride, min_points, damp, max_shift, max_angle)
    _req(mesh_depth, name="mesh_depth"); _req(silhouette, torch.uint8, "silhouette"); _req(scene_depth, name="scene_depth")
    _req(mesh, name="mesh"); _req(xyz_mm, name="xyz_mm")
    n, h, w, k = _depth_maps(mesh_depth, silhouette, k)
    s = n * k
    v, joints = _fit_meshes(mesh, xyz_mm, s)
    for name, t in (("mesh_depth", mesh_depth), ("mesh", mesh), ("xyz_mm", xyz_mm)):
        _on_device(name, t, silhouette.device, "the silhouette")
    depth_ptr, depth_stride = _scene_depth_arg(scene_depth, n, h, w, silhouette.device, "the silhouette")
    host4, table = _camera_arg(paras, n, silhouette.device, "the silhouette")
    parts = _out_parts(out, _fit_specs(s, v, joints), silhouette.device)
    scratch = _scratch_arg(scratch, silhouette.device, mesh_fit_scratch_bytes, n, k, h)
    shift2, tan2 = fit_caps(max_shift, max_angle)
    check(_lib.load().hn_mesh_fit_f32(ptr(mesh_depth), ptr(silhouette), depth_ptr, depth_stride, host4, table,
                                      ptr(mesh), ptr(xyz_mm), n, k, h, w, v, joints, stride, band, min_points, damp, shift2, tan2,
                                      ptr(scratch), scratch.numel(), *(ptr(t) for t in parts), _stream()), "hn_mesh_fit_f32")
    return MeshFit(*parts)


def mesh_geometry(mesh, faces, paras, hw, lifted=None, k=1, *, out_depth=None, out_who=None, scratch=None):
    """The geometry pass of mesh_render's raster (hn_mesh_geometry_f32: two launches, csrc/mesh_raster.hip; DESIGN.md section 9l,
    tests/refit_ref.py::geometry is the rule and the outputs equal it bit for bit): the nearest mesh Z and its slot per pixel,
    and nothing else -- no frame is read and no image stored.  mesh, faces, paras, lifted, k (1..16), scratch: as mesh_render
    takes them; hw = (h, w) of the frames.  Returns (depth fp32 [N,H,W]: the nearest Z, 0 where nothing was drawn; who uint8
    [N,H,W]: 0, or the nearest slot within the frame + 1) -- the occluded mesh_render's depth_out and silhouette & 0x7F, bit for
    bit --, allocated or out_depth / out_who, both fully written."""
    mesh, s, v = _slot_meshes(mesh)
    faces, fh, f = _faces_arg(faces, mesh.device)
    h, w = (int(x) for x in hw)
    k = int(k)
    if not 1 <= k <= 16:
        raise ValueError(f"the slot byte holds at most 16 slots per frame (k = {k})")
    if s % k or s == 0:
        raise ValueError(f"{s} mesh slots with k = {k} slots per frame")
    n = s // k
    _lifted_arg(lifted, s)
    if out_depth is None:
        out_depth = torch.empty((n, h, w), device=mesh.device, dtype=torch.float32)
    if out_who is None:
        out_who = torch.empty((n, h, w), device=mesh.device, dtype=torch.uint8)
    _req(out_depth, name="out_depth"); _req(out_who, torch.uint8, "out_who")
    if out_depth.numel() != n * h * w or out_who.numel() != n * h * w:
        raise ValueError(f"out_depth fp32 and out_who uint8 [{n},{h},{w}], got {tuple(out_depth.shape)} and {tuple(out_who.shape)}")
    scratch = _scratch_arg(scratch, mesh.device, mesh_render_scratch_bytes, s, f)
    host4, table = _camera_arg(paras, n, mesh.device, "the mesh")
    check(_lib.load().hn_mesh_geometry_f32(ptr(mesh), ptr(faces), fh, ptr(lifted), s, v, f, k, host4, table, h, w, ptr(scratch),
                                           scratch.numel(), ptr(out_depth), ptr(out_who), _stream()), "hn_mesh_geometry_f32")
    return out_depth.view(n, h, w), out_who.view(n, h, w)


FIT_MAX_ITERS = 8          # iterations of the iterated fit

MeshFitIters = collections.namedtuple("MeshFitIters", "mesh xyz rt count cost trace")


def check_fit_iters(iters) -> int:
    """fit_iters as an int in 1..8, else ValueError."""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= int(iters) <= FIT_MAX_ITERS:
        raise ValueError(f"fit_iters: an integer in 1..{FIT_MAX_ITERS} (got {iters!r})")
    return int(iters)


def mesh_fit_iters_scratch_bytes(frames, k, h, w, vertices, faces, joints, iters):
    return int(_lib.load().hn_mesh_fit_iters_scratch_bytes(frames, k, h, w, vertices, faces, joints, iters))


def mesh_fit_iters(mesh_depth, silhouette, scene_depth, paras, mesh, xyz_mm, faces, k, *, iters, lifted=None, band=FIT_BAND,
                   stride=FIT_STRIDE, min_points=FIT_MIN_POINTS, damp=FIT_DAMP, max_shift=FIT_MAX_SHIFT, max_angle=FIT_MAX_ANGLE,
                   out=None, scratch=None, work=None) -> MeshFitIters:
    """mesh_fit iterated (hn_mesh_fit_iters_f32: 2 + 4 (iters - 1) + 1 launches, csrc/mesh_refit.hip; DESIGN.md section 9l,
    tests/refit_ref.py::mesh_fit_iters is the rule and the outputs equal it bit for bit): `iters` (1..8) Gauss-Newton steps.
    Iteration 1 is mesh_fit on the given mesh_depth / silhouette; before every further one the current meshes are drawn again
    (mesh_geometry with `faces` -- a GPU int32 tensor or a host list -- and `lifted`: a slot with lifted == 0 is not drawn) and
    the step turns about the current root joint, with the same parameters and caps.  A slot whose iteration ends with a status
    other than 0 keeps its bytes for that iteration and is tried again in the next; there is no early stop.  Every other
    argument: as mesh_fit takes it.  Returns MeshFitIters: mesh and xyz after the last iteration, rt fp32 [N*k,12] the composed
    motion about the ORIGINAL root joint (the identity when no iteration fitted), count and cost those of iteration 1 (what
    mesh_fit hands out), trace int64 [N*k,iters,3] = (matches, status, cost) of every iteration -- the cost of iteration t is the
    residual after t - 1 motions.  Allocated, or `out`'s attributes fit_mesh / fit_xyz / fit_rt / fit_count / fit_cost /
    fit_trace, every one fully written."""
    iters = check_fit_iters(iters)
    band, stride, min_points, damp, max_shift, max_angle = check_fit(band, stride, min_points, damp, max_shift, max_angle)
    _req(mesh_depth, name="mesh_depth"); _req(silhouette, torch.uint8, "silhouette"); _req(scene_depth, name="scene_depth")
    _req(mesh, name="mesh"); _req(xyz_mm, name="xyz_mm")
    n, h, w, k = _depth_maps(mesh_depth, silhouette, k)
    s = n * k
    v, joints = _fit_meshes(mesh, xyz_mm, s)
    faces, fh, f = _faces_arg(faces, mesh.device, nonempty=True)
    _lifted_arg(lifted, s)
    for name, t in (("mesh_depth", mesh_depth), ("mesh", mesh), ("xyz_mm", xyz_mm), ("faces", faces)):
        _on_device(name, t, silhouette.device, "the silhouette")
    depth_ptr, depth_stride = _scene_depth_arg(scene_depth, n, h, w, silhouette.device, "the silhouette")
    host4, table = _camera_arg(paras, n, silhouette.device, "the silhouette")
    parts = _out_parts(out, _fit_specs(s, v, joints) + (("fit_trace", torch.int64, (s, iters, 3)),), silhouette.device)
    scratch = _scratch_arg(scratch, silhouette.device, mesh_fit_scratch_bytes, n, k, h)
    work = _scratch_arg(work, silhouette.device, mesh_fit_iters_scratch_bytes, n, k, h, w, v, f, joints, iters, name="work")
    shift2, tan2 = fit_caps(max_shift, max_angle)
    check(_lib.load().hn_mesh_fit_iters_f32(ptr(mesh_depth), ptr(silhouette), depth_ptr, depth_stride, host4, table,
                                            ptr(mesh), ptr(xyz_mm), ptr(faces), fh, ptr(lifted), n, k, h, w, v, f, joints, iters,
                                            stride, band, min_points, damp, shift2, tan2, ptr(scratch), scratch.numel(), ptr(work),
                                            work.numel(), *(ptr(t) for t in parts), _stream()), "hn_mesh_fit_iters_f32")
    return MeshFitIters(*parts)


OBJECT_BAND = 0.15         # metres around the depth of the hand's root joint; a starting value, NOT tuned on any model
OBJECT_STRIDE = 2          # every second row and column is a candidate; a starting value, NOT tuned on any model
OBJECT_MIN_POINTS = 50     # fewer matches: no centroid is handed out; a starting value, NOT tuned on any model
OBJECT_MAX_BAND = 100.0    # metres
OBJECT_FIELDS = ("contact", "object_index", "object_box", "object_score", "object_point", "object_xyz", "object_extent", "object_count")


@dataclass
class HandObjects:
    """ops.hand_objects: per hand slot s = i * k + j"""
    contact: torch.Tensor        # [S] int32: the slot's contact state (100DOH: 0 none, 1 self, 2 other person, 3 portable, 4 stationary; -1: empty slot)
    object_index: torch.Tensor   # [S] int32: the held object's detection row, or -1
    object_box: torch.Tensor     # [S,4] fp32: its box (zeros: no object)
    object_score: torch.Tensor   # [S] fp32: its score (0: no object)
    object_point: torch.Tensor   # [S,2] fp32: the point the hand's offset vector names (zeros: empty slot)
    object_xyz: torch.Tensor     # [S,3] fp32: the centroid of the object's depth pixels, camera frame, metres (zeros unless status 0)
    object_extent: torch.Tensor  # [S,6] fp32: (min x y z, max x y z) of those pixels (zeros: no match)
    object_count: torch.Tensor   # [S,2] int32: (matches, status: 0 ok, 1 no object, 2 fewer than min_points matches, -1 empty slot)


def check_objects(band=OBJECT_BAND, stride=OBJECT_STRIDE, min_points=OBJECT_MIN_POINTS):
    """The held objects' three parameters as (float band, int stride >= 1, int min_points >= 1), the band finite and in (0, 100]
    metres also as the fp32 kernel argument it becomes; else ValueError.  The defaults (0.15 m, every second row and column, 50
    matches) are starting values, NOT tuned on any model."""
    _check_count("object_stride", stride)
    _check_count("object_min_points", min_points)
    try:
        b = math.nan if isinstance(band, bool) else float(band)
    except (TypeError, ValueError):
        b = math.nan
    _check_band("object_band", b, band, OBJECT_MAX_BAND)
    return b, int(stride), int(min_points)


def hand_objects_scratch_bytes(frames, k, h):
    return int(_lib.load().hn_hand_objects_scratch_bytes(frames, k, h))


def hand_objects(det: Detections, contacts, dxdymags, det_index, depth, xyz_mm, paras, k, *, object_label=1, band=OBJECT_BAND,
                 stride=OBJECT_STRIDE, min_points=OBJECT_MIN_POINTS, silhouette=None, scratch=None, out=None) -> HandObjects:
    """The object each hand holds (hn_hand_objects_f32: three launches, csrc/hand_object.hip; DESIGN.md section 9q,
    tests/object_ref.py is the rule and the outputs equal it bit for bit).  det: the detector's Detections of N frames (boxes
    [N,cap,4], scores, labels, count); contacts int32 [N,cap] and dxdymags fp32 [N,cap,3]: what fcos_ext_gather /
    FCOSEngine.detect_ext leave; det_index int32 [N,k]: each slot's detection row (-1: empty slot), as forward_hands hands it
    out; depth: the camera's depth map, fp32 [N,1,H,W], [N,H,W] or an RGB-D [N,4,H,W] (channel 3 is read in place); xyz_mm fp32
    [N*k,J,3] or [N,k,J,3]: camera millimetres, joint 0 the root; paras (fx, fy, cx, cy) on the host, or an fp32 tensor [N,4] on
    the device, a camera per frame; k slots per frame (1..16).
    A slot whose contact state is > 0 is given, among the frame's rows of `object_label` (1: the targetobject of num_classes =
    3), the one whose centre lies nearest to hand centre + (magnitude * 10000) * (x, y) -- the association of the reference's
    evaluation (voc_eval.py:687-699) on the detections AS THEY ARE: its %.1f / %.3f file round trip and its + 1 are left out on
    purpose; ties go to the earlier rank.  The candidates (every stride-th row and column) whose centre (c + 0.5, r + 0.5) lies
    in that box, whose depth D is finite and > 0, whose silhouette byte -- silhouette uint8 [N,H,W], the occluded raster's, or
    None -- names no hand ((byte & 0x7F) == 0) and |D - z of the slot's root joint| <= band metres are back-projected as
    hand_cloud does and reduced to a centroid (integer sums of micrometres) and an extent.  Returns HandObjects, a row per
    slot; allocated, or `out`'s attributes of the same names (the live step's buffer views), every one fully written.
    That contact states > 0 mean "in contact" (3 / 4: a portable / stationary object) is 100DOH's numbering, which the
    reference's live code never reads: check it against the checkpoint in use.  band = 0.15 m, stride = 2 and min_points = 50
    are starting values, NOT tuned on any model."""
    band, stride, min_points = check_objects(band, stride, min_points)
    for name, t, dtype in (("det.boxes", det.boxes, torch.float32), ("det.scores", det.scores, torch.float32),
                           ("det.labels", det.labels, torch.int32), ("det.count", det.count, torch.int32),
                           ("contacts", contacts, torch.int32), ("dxdymags", dxdymags, torch.float32),
                           ("det_index", det_index, torch.int32), ("xyz_mm", xyz_mm, torch.float32)):
        _req(t, dtype, name)
    dev = det.scores.device
    if det.scores.dim() != 2:
        raise ValueError(f"det.scores: expected [N,cap], got {tuple(det.scores.shape)}")
    n, cap = (int(v) for v in det.scores.shape)
    k = int(k)
    if not 1 <= k <= 16:
        raise ValueError(f"k = {k} slots per frame (1..16)")
    for name, t, shape in (("det.boxes", det.boxes, (n, cap, 4)), ("det.labels", det.labels, (n, cap)), ("det.count", det.count, (n,)),
                           ("contacts", contacts, (n, cap)), ("dxdymags", dxdymags, (n, cap, 3)), ("det_index", det_index, (n, k))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected {list(shape)}, got {tuple(t.shape)}")
        _on_device(name, t, dev, "the detections")
    s = n * k
    if xyz_mm.dim() < 3 or xyz_mm.shape[-1] != 3 or xyz_mm.numel() != s * xyz_mm.shape[-2] * 3 or xyz_mm.shape[-2] < 1:
        raise ValueError(f"xyz_mm: expected fp32 [{s},J,3] or [{n},{k},J,3], got {tuple(xyz_mm.shape)}")
    _on_device("xyz_mm", xyz_mm, dev, "the detections")
    joints = int(xyz_mm.shape[-2])
    if not torch.is_tensor(depth) or depth.dim() < 3:
        raise ValueError("depth: expected fp32 [N,1,H,W], [N,H,W] or RGBD [N,4,H,W]")
    h, w = (int(v) for v in depth.shape[-2:])
    depth_ptr, depth_stride = _scene_depth_arg(depth, n, h, w, dev, "the detections")
    if silhouette is not None:
        _req(silhouette, torch.uint8, "silhouette")
        if tuple(silhouette.shape) != (n, h, w):
            raise ValueError(f"silhouette: expected uint8 [{n},{h},{w}], got {tuple(silhouette.shape)}")
        _on_device("silhouette", silhouette, dev, "the detections")
    host4, table = _camera_arg(paras, n, dev, "the detections")
    parts = _out_parts(out, (("contact", torch.int32, (s,)), ("object_index", torch.int32, (s,)), ("object_box", torch.float32, (s, 4)),
                             ("object_score", torch.float32, (s,)), ("object_point", torch.float32, (s, 2)),
                             ("object_xyz", torch.float32, (s, 3)), ("object_extent", torch.float32, (s, 6)),
                             ("object_count", torch.int32, (s, 2))), dev)
    scratch = _scratch_arg(scratch, dev, hand_objects_scratch_bytes, n, k, h)
    check(_lib.load().hn_hand_objects_f32(ptr(det.boxes), ptr(det.scores), ptr(det.labels), ptr(det.count), ptr(contacts), ptr(dxdymags),
                                          ptr(det_index), cap, int(object_label), depth_ptr, depth_stride, ptr(silhouette), ptr(xyz_mm),
                                          joints, host4, table, n, k, h, w, stride, band, min_points, ptr(scratch), scratch.numel(),
                                          *(ptr(t) for t in parts), _stream()), "hn_hand_objects_f32")
    return HandObjects(*parts)


def draw_object_labels(det: Detections, det_index, object_index, box_label):
    """The held objects on the box label image, IN PLACE (hn_draw_object_labels_u8: one launch, csrc/hand_object.hip;
    tests/object_ref.py draw_object_labels is the rule): box_label uint8 [N,H,W,3] as draw_labels leaves it; for every slot with
    object_index >= 0 (int32 [N,k] or [N*k], as hand_objects hands it out) the object's rectangle and the line from the hand
    box's centre (det.boxes of det_index) to the object box's centre, both in (0, 0, 255); corners and centres are rounded to
    the nearest integer and saturated at 2^20, as the crop boxes are.  Every other pixel keeps its bytes.  Returns box_label."""
    _req(det.boxes, name="det.boxes"); _req(det_index, torch.int32, "det_index"); _req(object_index, torch.int32, "object_index")
    _req(box_label, torch.uint8, "box_label")
    if det.boxes.dim() != 3 or det.boxes.shape[2] != 4 or box_label.dim() != 4 or box_label.shape[3] != 3 \
            or box_label.shape[0] != det.boxes.shape[0]:
        raise ValueError(f"det.boxes [N,cap,4] and box_label uint8 [N,H,W,3], got {tuple(det.boxes.shape)} and {tuple(box_label.shape)}")
    n, cap = (int(v) for v in det.boxes.shape[:2])
    h, w = (int(v) for v in box_label.shape[1:3])
    if det_index.numel() % n or det_index.numel() != object_index.numel() or not 1 <= det_index.numel() // n <= 16:
        raise ValueError(f"det_index / object_index: int32 [{n},k] each, k 1..16, got {tuple(det_index.shape)} and {tuple(object_index.shape)}")
    for name, t in (("det_index", det_index), ("object_index", object_index), ("box_label", box_label)):
        _on_device(name, t, det.boxes.device, "the detections")
    check(_lib.load().hn_draw_object_labels_u8(ptr(det.boxes), ptr(det_index), ptr(object_index), cap, n, det_index.numel() // n, h, w,
                                               ptr(box_label), _stream()), "hn_draw_object_labels_u8")
    return box_label


LABEL_CROP = 176      # side of a pose_label image


def draw_labels(keypoints, crop_box, frame, drawn=None, k=1, clamp=True, out_box=None, out_pose=None, box=True, pose=True):
    """The live loop's box and pose images (hn_draw_labels_u8; ros_demo.py:310-326 without OpenCV): keypoints fp32 [S,21,3] (or
    [N,K,21,3]) crop-space (u,v,d), crop_box int64 [S,4] (x1,y1,x2,y2), S = N * k slots; frame fp32 [N,3,H,W] in 0..1 or uint8
    [N,H,W,3] 'bgr8', on the GPU; drawn int32 [S] (a slot is drawn when its flag is 1; None: every slot); clamp: the caller's
    clamps first (box to the frame as written at ros_demo.py:280-281, keypoints to [0,176]).  Returns (box_label uint8
    [N,H,W,3] RGB: the frame with the drawn slots' crop rectangles; pose_label uint8 [S,176,176,3] RGB: each drawn slot's colour
    crop resized to 176 x 176 with its skeleton, zeros for the others); box=False / pose=False leaves that image out (None)."""
    _req(keypoints, name="keypoints"); _req(crop_box, torch.int64, "crop_box")
    keypoints, crop_box = keypoints.view(-1, 21, 3), crop_box.view(-1, 4)
    s = keypoints.shape[0]
    if crop_box.shape[0] != s:
        raise ValueError(f"{s} keypoint rows but {crop_box.shape[0]} crop boxes")
    if frame.dtype == torch.uint8:
        _req(frame, torch.uint8, "frame")
        fmt, (n, h, w) = _lib.FRAME_U8_BGR_HWC, frame.shape[:3]
        ok = frame.dim() == 4 and frame.shape[3] == 3
    else:
        _req(frame, name="frame")
        fmt, n, (h, w) = _lib.FRAME_F32_CHW, frame.shape[0], frame.shape[2:]
        ok = frame.dim() == 4 and frame.shape[1] == 3
    if not ok:
        raise ValueError(f"frame: expected fp32 [N,3,H,W] or uint8 [N,H,W,3], got {frame.dtype} {tuple(frame.shape)}")
    if k < 1 or n * k != s:
        raise ValueError(f"{s} slots for {n} frames with k = {k} slots per frame")
    if drawn is not None:
        _req(drawn, torch.int32, "drawn")
        if drawn.numel() != s:
            raise ValueError(f"drawn: expected {s} flags, got {drawn.numel()}")
    if not (box or pose):
        raise ValueError("neither image asked for")
    if box and out_box is None:
        out_box = torch.empty((n, h, w, 3), device=keypoints.device, dtype=torch.uint8)
    if pose and out_pose is None:
        out_pose = torch.empty((s, LABEL_CROP, LABEL_CROP, 3), device=keypoints.device, dtype=torch.uint8)
    for t, want, nm in ((out_box if box else None, n * h * w * 3, "out_box"),
                        (out_pose if pose else None, s * LABEL_CROP * LABEL_CROP * 3, "out_pose")):
        if t is not None:
            _req(t, torch.uint8, nm)
            if t.numel() != want:
                raise ValueError(f"{nm}: expected {want} bytes, got {tuple(t.shape)}")
    check(_lib.load().hn_draw_labels_u8(ptr(keypoints), ptr(crop_box), ptr(drawn), s, k, ptr(frame), fmt, h, w, 1 if clamp else 0,
                                        ptr(out_box) if box else None, ptr(out_pose) if pose else None, _stream()),
          "hn_draw_labels_u8")
    return (out_box.view(n, h, w, 3) if box else None,
            out_pose.view(s, LABEL_CROP, LABEL_CROP, 3) if pose else None)


def pad_split_rows(x, cpad):
    """fp32 [rows, f] -> S32 [rows,1,1,cpad/32,2,32], channels f.. zero (hn_pad_split_rows_f32)."""
    _req(x, name="x")
    rows, f = x.shape
    out = torch.empty((rows, 1, 1, cpad // 32, 2, 32), device=x.device, dtype=torch.float16)
    check(_lib.load().hn_pad_split_rows_f32(ptr(x), rows, f, cpad, ptr(out), _stream()), "hn_pad_split_rows_f32")
    return out


def lifter_combine(pose2d, pose3d, fpad=8):
    """pose2d [B,J,2], pose3d [B,J,3] (a view of padded [B,S >= 3J] rows is fine) fp32 -> [B,J,fpad] = [pose2d | pose3d / 1000 | 0]
    (pose2mesh_net.py:20)."""
    _req(pose2d, name="pose2d")
    b, j, _ = pose2d.shape
    if (not pose3d.is_cuda or pose3d.dtype != torch.float32 or tuple(pose3d.shape) != (b, j, 3) or pose3d.stride(2) != 1
            or pose3d.stride(1) != 3 or pose3d.stride(0) < 3 * j):
        raise ValueError("pose3d must be fp32 GPU [B,J,3] with dense joints (rows may be padded)")
    out = torch.empty((b, j, fpad), device=pose2d.device, dtype=torch.float32)
    check(_lib.load().hn_lifter_combine_f32(ptr(pose2d), ptr(pose3d), b, j, pose3d.stride(0), fpad, ptr(out), _stream()),
          "hn_lifter_combine_f32")
    return out


def spmm_csr(g: CsrGraph, x):
    """x fp32 [B,V,F] -> L x."""
    _req(x, name="x")
    b, v, f = x.shape
    if v != g.v:
        raise ValueError("vertex count mismatch")
    y = torch.empty_like(x)
    check(_lib.load().hn_spmm_csr_f32(ptr(g.indptr), ptr(g.indices), ptr(g.values), v, ptr(x), ptr(y), b, f, _stream()),
          "hn_spmm_csr_f32")
    return y


def cheby3_basis_split(g: CsrGraph, x0, x1):
    """x0, x1 = L x0 (fp32 [B,V,F]) -> S32 operand [B,V,1,Cpad/32,2,32] holding [x0 | x1 | 2 L x1 - x0 | 0]."""
    _req(x0, name="x0"); _req(x1, name="x1")
    b, v, f = x0.shape
    cpad = (3 * f + 31) // 32 * 32
    out = torch.empty((b, v, 1, cpad // 32, 2, 32), device=x0.device, dtype=torch.float16)
    check(_lib.load().hn_cheby3_basis_split(ptr(g.indptr), ptr(g.indices), ptr(g.values), v, ptr(x0), ptr(x1), ptr(out),
                                            b, f, cpad, _stream()), "hn_cheby3_basis_split")
    return out


def feat_interp_add(xin, y, up=1):
    """y [B,V,Fo] + linear interpolation of xin [B,V,Fi] along the feature axis, rows repeated `up` times."""
    _req(xin, name="xin"); _req(y, name="y")
    b, v, fo = y.shape
    if tuple(xin.shape[:2]) != (b, v):
        raise ValueError("shape mismatch")
    out = torch.empty((b, v * up, fo), device=y.device, dtype=torch.float32)
    check(_lib.load().hn_feat_interp_add_f32(ptr(xin), ptr(y), ptr(out), b * v, xin.shape[2], fo, up, _stream()),
          "hn_feat_interp_add_f32")
    return out
