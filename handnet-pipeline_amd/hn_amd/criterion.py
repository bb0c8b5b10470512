"""The A2J criterion as a differentiable torch module on the HIP kernels: forward is ops.a2j_loss, the
backward one ops.a2j_loss_grad launch that hands autograd the gradients at the three heads."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import ops


class _A2JLoss(torch.autograd.Function):
    """(cls, reg, dep) -> (classification, regression, total_loss, uvd); gt, valid and the settings ride along undifferentiated"""

    @staticmethod
    def forward(ctx, cls, reg, dep, gt, valid, joints, stride, spatial_factor, reg_loss_factor):
        uvd, _terms, _sample, batch = ops.a2j_loss(cls, reg, dep, gt, joints=joints, stride=stride, spatial_factor=spatial_factor,
                                                   reg_loss_factor=reg_loss_factor, valid=valid)
        ctx.save_for_backward(cls, reg, dep, gt)
        ctx.valid, ctx.settings = valid, (joints, stride, spatial_factor, reg_loss_factor)
        ctx.mark_non_differentiable(uvd)
        return batch[0:1], batch[2:3], batch[3:4], uvd

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_reg, g_total, _g_uvd):
        cls, reg, dep, gt = ctx.saved_tensors
        joints, stride, spatial_factor, reg_loss_factor = ctx.settings
        # (wa, wr) on the device: total_loss = classification + regression, so its gradient joins both (no host read)
        upstream = torch.cat([g_cls + g_total, g_reg + g_total]).to(torch.float32).contiguous()
        d_cls, d_reg, d_dep = ops.a2j_loss_grad(cls, reg, dep, gt, joints=joints, stride=stride, spatial_factor=spatial_factor,
                                                reg_loss_factor=reg_loss_factor, valid=ctx.valid, upstream=upstream)
        return d_cls, d_reg, d_dep, None, None, None, None, None, None


class A2JCriterion(torch.nn.Module):
    """The A2J criterion (a2j/anchor.py:99-153 with A2JModel's reg_loss_factor, a2j/a2j.py:224,233-238) with a backward, for a
    torch-built network on this card.  No parameters.

        crit = A2JCriterion(joints=21, stride=16, spatial_factor=0.5, reg_loss_factor=3.0)
        losses, uvd = crit(cls, reg, dep, gt)          # losses = {"classification", "regression", "total_loss"}, fp32 [1]
        losses["total_loss"].backward()                # cls.grad, reg.grad, dep.grad

    cls, dep [K,fh,fw,16*J] and reg [K,fh,fw,32*J] are contiguous fp32 tensors on the device in the layout of ops.a2j_loss
    (channel = anchor * J + joint, reg with (h, w) innermost); anything else raises ValueError.  A torch conv2d output in
    channels_last memory format, viewed with permute(0, 2, 3, 1), is exactly this layout: [K,C,fh,fw] channels_last is
    [K,fh,fw,C] in memory, and the permuted view is contiguous.  gt [K,J,3] fp32 crop (coord0, coord1, depth); valid [K] int32
    as ops.a2j_loss takes it.  The three losses are the bytes of ops.a2j_loss's batch values [0], [2], [3]; uvd is its
    keypoints.  The backward is once-differentiable and makes one ops.a2j_loss_grad launch with the upstream weights
    (g_classification + g_total, g_regression + g_total) formed on the device; gt and valid get no gradient."""

    def __init__(self, joints=21, stride=16, spatial_factor=0.5, reg_loss_factor=3.0):
        super().__init__()
        self.joints, self.stride = int(joints), int(stride)
        self.spatial_factor, self.reg_loss_factor = float(spatial_factor), float(reg_loss_factor)

    def forward(self, cls, reg, dep, gt, valid=None):
        for name, t in (("cls", cls), ("reg", reg), ("dep", dep), ("gt", gt)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"A2JCriterion: {name} must be a contiguous fp32 tensor on the device "
                                 "(heads [K,fh,fw,16*J] / [K,fh,fw,32*J]; a channels_last conv output viewed with permute(0, 2, 3, 1))")
        if cls.dim() != 4 or cls.shape[3] != 16 * self.joints or tuple(reg.shape) != (*cls.shape[:3], 32 * self.joints) \
                or dep.shape != cls.shape or tuple(gt.shape) != (cls.shape[0], self.joints, 3):
            raise ValueError(f"A2JCriterion: expected cls, dep [K,fh,fw,{16 * self.joints}], reg [K,fh,fw,{32 * self.joints}], "
                             f"gt [K,{self.joints},3]")
        c, r, total, uvd = _A2JLoss.apply(cls, reg, dep, gt.detach(), valid, self.joints, self.stride, self.spatial_factor,
                                          self.reg_loss_factor)
        return {"classification": c, "regression": r, "total_loss": total}, uvd
