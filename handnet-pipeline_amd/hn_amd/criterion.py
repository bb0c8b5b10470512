"""The two criteria as differentiable torch modules on the HIP kernels.  A2JCriterion: forward is
ops.a2j_loss, the backward one ops.a2j_loss_grad launch that hands autograd the gradients at the three heads.  FCOSCriterion
(section 9s): forward is ops.fcos_loss, the backward one ops.fcos_loss_grad call for the detector's per-level heads."""
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


class _FCOSLoss(torch.autograd.Function):
    """(the 2L or 3L level tensors) -> (the six dict values [6], fg); targets and the settings ride along undifferentiated"""

    @staticmethod
    def forward(ctx, targets, strides, num_classes, radius, levels, ext, *heads):
        cls_lr, reg_ctr = list(heads[:levels]), list(heads[levels:2 * levels])
        ex = list(heads[2 * levels:]) if ext else None
        res = ops.fcos_loss(cls_lr, reg_ctr, strides, num_classes, targets, ext=ex, radius=radius)
        ctx.save_for_backward(*heads)
        ctx.settings = (targets, strides, num_classes, radius, levels, ext)
        ctx.mark_non_differentiable(res.fg)
        return res.losses, res.fg

    @staticmethod
    @once_differentiable
    def backward(ctx, g_losses, _g_fg):
        targets, strides, num_classes, radius, levels, ext = ctx.settings
        heads = ctx.saved_tensors
        # the [6] upstream on the device (no host read); a missing gradient is zero
        upstream = (torch.zeros((6,), device=heads[0].device) if g_losses is None else g_losses).to(torch.float32).contiguous()
        grads = ops.fcos_loss_grad(list(heads[:levels]), list(heads[levels:2 * levels]), strides, num_classes, targets,
                                   ext=list(heads[2 * levels:]) if ext else None, radius=radius, upstream=upstream)
        return (None,) * 6 + tuple(t for g in grads if g is not None for t in g)


class FCOSCriterion(torch.nn.Module):
    """The FCOS criterion (fcos_utils/fcos.py:523-570 the matching, :44-178 the six terms) with a backward, for a torch-built
    detector on this card.  No parameters.

        crit = FCOSCriterion(num_classes=3, strides=(8, 16, 32, 64, 128), ext=True)
        losses, fg = crit(cls_lr, reg_ctr, targets, ext=ext_levels)     # losses: the reference's dict, 0-d fp32 on the device
        sum(losses.values()).backward()                                  # .grad of every level tensor

    cls_lr[l] [N,h,w,C+2] (class logits, then the two side logits), reg_ctr[l] [N,h,w,5] (the four ReLU'd regressions, then the
    centre-ness logit) and, with ext, ext[l] [N,h,w,8] (the ReLU'd (mag, dx, dy), then the five contact logits) are contiguous
    fp32 tensors on the device, one per level, the layout of ops.fcos_loss; anything else raises ValueError.  A torch conv2d
    output in channels_last memory format, viewed with permute(0, 2, 3, 1), is this layout.  targets: an ops.FcosTargets
    (ops.pack_fcos_targets), boxes on the canvas's scale.  The dict's values are the bytes of ops.fcos_loss's losses, in the
    reference's key order (four keys without ext); fg int32 [N] gets no gradient.  The matching and the divisor max(1, sum fg)
    are constants.  The backward is once-differentiable and makes one ops.fcos_loss_grad call with the [6] upstream formed on
    the device from the incoming gradients (a value that took no part in the differentiated scalar weighs zero)."""

    def __init__(self, num_classes, strides, ext=False, radius=1.5):
        super().__init__()
        self.num_classes, self.strides = int(num_classes), tuple(int(s) for s in strides)
        self.ext, self.radius = bool(ext), float(radius)

    def forward(self, cls_lr, reg_ctr, targets, ext=None):
        levels = len(self.strides)
        if (ext is not None) != self.ext:
            raise ValueError(f"FCOSCriterion(ext={self.ext}): ext levels must be given exactly when ext is set")
        groups = (("cls_lr", cls_lr, self.num_classes + 2), ("reg_ctr", reg_ctr, 5)) + ((("ext", ext, 8),) if self.ext else ())
        for name, ts, cols in groups:
            if not isinstance(ts, (list, tuple)) or len(ts) != levels:
                raise ValueError(f"FCOSCriterion: {name} must hold one tensor per level ({levels})")
            for t, ref in zip(ts, cls_lr):
                if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError(f"FCOSCriterion: {name} must hold contiguous fp32 tensors on the device "
                                     f"([N,h,w,{cols}]; a channels_last conv output viewed with permute(0, 2, 3, 1))")
                if t.dim() != 4 or t.shape[3] != cols or tuple(t.shape[:3]) != tuple(ref.shape[:3]):
                    raise ValueError(f"FCOSCriterion: expected {name}[l] [N,h,w,{cols}] on the levels of cls_lr")
        if not isinstance(targets, ops.FcosTargets):
            raise ValueError("FCOSCriterion: targets must be an ops.FcosTargets (ops.pack_fcos_targets)")
        heads = list(cls_lr) + list(reg_ctr) + (list(ext) if self.ext else [])
        values, fg = _FCOSLoss.apply(targets, self.strides, self.num_classes, self.radius, levels, self.ext, *heads)
        keys = ops.FCOS_LOSS_KEYS if self.ext else ops.FCOS_LOSS_KEYS[:4]
        return {k: values[i] for i, k in enumerate(keys)}, fg
