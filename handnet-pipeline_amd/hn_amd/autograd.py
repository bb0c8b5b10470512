"""The head-output convolution as a differentiable torch module on the HIP kernels: ThinConv3x3Levels runs
ops.conv3x3_thin_levels forward and one ops.conv3x3_thin_backward_levels call backward, so that a torch-built detector's output
layers get their weight, bias and input gradients from the device kernels."""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .weights import ConvW, split_f16x3


class _ThinConv(torch.autograd.Function):
    """(weight [Cout,Cin,3,3], bias [Cout], the level tensors) -> the level outputs; relu_cols and the packed bank cw (the
    module's cache of weight in the kernels' layout, bias a view of the parameter) ride along undifferentiated"""

    @staticmethod
    def forward(ctx, relu_cols, cw, weight, bias, *xs):
        a16 = [ops.to_split(x.detach()) for x in xs]
        ys = ops.conv3x3_thin_levels(a16, cw, relu_cols)
        ctx.save_for_backward(cw.w, *a16, *ys)
        ctx.relu_cols, ctx.levels = relu_cols, len(xs)
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        w, *rest = ctx.saved_tensors
        a16, ys = rest[:ctx.levels], rest[ctx.levels:]
        # a level that took no part in the differentiated scalar weighs zero
        gs = [torch.zeros_like(y) if g is None else g.to(torch.float32).contiguous() for g, y in zip(gs, ys)]
        want_dx = any(ctx.needs_input_grad[4:])
        [(d_w, d_b)], d_a = ops.conv3x3_thin_backward_levels(list(a16), [(ConvW(w, None), ctx.relu_cols, list(ys), gs)], want_dx=want_dx)
        d_x = tuple(d_a[l] if ctx.needs_input_grad[4 + l] else None for l in range(ctx.levels)) if want_dx else (None,) * ctx.levels
        return (None, None, d_w.permute(0, 3, 1, 2), d_b) + d_x


class ThinConv3x3Levels(torch.nn.Module):
    """A 3x3 / pad 1 convolution with at most 16 output channels and ONE weight shared over up to five maps -- the FCOS head
    output layers (fcos_utils/fcos.py:247-264: cls_logits, bbox_reg, ...) -- for a torch-built detector on this card.

        conv = ThinConv3x3Levels(256, 5, relu_cols=4)          # e.g. bbox_reg + bbox_ctrness stacked, ReLU on the regressions
        outs = conv([p3, p4, p5])                               # fp32 [N,h_l,w_l,Cin] each -> fp32 [N,h_l,w_l,Cout] each
        loss(outs).backward()                                   # .grad of weight, bias and every level input

    weight [Cout,Cin,3,3] and bias [Cout] are in the reference's (torch.nn.Conv2d's) layout.  The inputs are contiguous fp32
    tensors on the device, Cin a multiple of 32; anything else raises ValueError.  A torch conv2d output in channels_last
    memory format, viewed with permute(0, 2, 3, 1), is this layout.  The forward splits every input into fp16 hi + lo
    (ops.to_split) and runs ops.conv3x3_thin_levels; the backward is once-differentiable and makes one
    ops.conv3x3_thin_backward_levels call (the ReLU's mask is torch's, on the stored output).  The input gradient is the
    gradient with respect to the split value hi + lo; the split is the identity to 2^-22 relative, so it is passed through as
    the gradient at the input.  Values beyond the fp16 range (inputs or weights) are outside the split format: the weights are
    split and checked (ValueError; one device-to-host wait) when they have changed since the last forward -- the packed bank
    is cached on the parameter's version counter, so forwards between two optimizer steps pack nothing and wait for nothing."""

    def __init__(self, cin, cout, relu_cols=0):
        super().__init__()
        if cin % 32 or not 1 <= cout <= 16 or not 0 <= relu_cols <= cout:
            raise ValueError("ThinConv3x3Levels: need cin % 32 == 0, 1 <= cout <= 16 and 0 <= relu_cols <= cout")
        self.cin, self.cout, self.relu_cols = int(cin), int(cout), int(relu_cols)
        self.weight = torch.nn.Parameter(torch.empty((cout, cin, 3, 3)))
        self.bias = torch.nn.Parameter(torch.zeros((cout,)))
        torch.nn.init.normal_(self.weight, std=1.0 / math.sqrt(9 * cin))
        self._packed = (None, None)   # (what the bank was packed from, the ConvW)

    def _bank(self):
        """weight in the kernels' layout [Cout,3,3,Cin] + its split bank, repacked when the parameter was written (an optimizer
        step, copy_, load_state_dict: the version counter) or replaced (.to / .cuda: another tensor)"""
        # (an inference tensor keeps no version counter: such a parameter is packed on every forward)
        version = None if self.weight.is_inference() else self.weight._version
        key = (version, self.weight.data_ptr(), self.weight.device, self.bias.data_ptr())
        if version is None or self._packed[0] != key:
            w = self.weight.detach().permute(0, 2, 3, 1).contiguous()
            # (bias: a view of the parameter, always current; the saved w is a copy of its own, never written again)
            self._packed = (key, ConvW(w, self.bias.detach(), 1, 1, 1, split_f16x3(w)))
        return self._packed[1]

    def forward(self, xs):
        if not isinstance(xs, (list, tuple)) or not 1 <= len(xs) <= ops._lib.HN_FCOS_MAX_LEVELS:
            raise ValueError(f"ThinConv3x3Levels: expected a list of 1..{ops._lib.HN_FCOS_MAX_LEVELS} level tensors")
        dev = self.weight.device
        for t in xs:
            if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("ThinConv3x3Levels: the levels must be contiguous fp32 tensors on the module's device "
                                 f"([N,h,w,{self.cin}]; a channels_last conv output viewed with permute(0, 2, 3, 1))")
            if t.dim() != 4 or t.shape[3] != self.cin or t.shape[0] != xs[0].shape[0]:
                raise ValueError(f"ThinConv3x3Levels: expected [N,h,w,{self.cin}] levels of one batch size")
        with ops.on_device(dev):
            return list(_ThinConv.apply(self.relu_cols, self._bank(), self.weight, self.bias, *xs))
