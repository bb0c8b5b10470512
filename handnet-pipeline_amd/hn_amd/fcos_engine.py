"""FCOS hand detector on MI355X: ResNet-34-FPN + GroupNorm towers + on-device post-process.

Arithmetic follows fcos_utils/fcos.py:675-767 of the reference (eval branch); default precision "f16x3":
  transform (torchvision GeneralizedRCNNTransform)   -> hn_fcos_preprocess_split (the stem's split fp16 image;
                                                         hn_fcos_preprocess_list for mixed-size batches)
  resnet34 body + FrozenBatchNorm (folded) + FPN      -> hn_conv_stem_f16x3, hn_conv2d_nhwc_f16x3(_ws / _grouped)
                                                         on S32 split activations (+ residual / nearest-2x
                                                         top-down add epilogues)
  4 x (conv3x3 + GroupNorm(32) + ReLU) towers          -> grouped conv launches write the raw fp32 output AND the
                                                         GroupNorm partial sums; hn_groupnorm_finalize_rows32
                                                         builds per-(image, channel) scale/shift tables,
                                                         hn_affine_split_f32 applies them (+ReLU) and emits the
                                                         next conv's S32 input
  cls_logits+hand_lr / bbox_reg+ctrness               -> one Cout=C+2 and one Cout=5 conv
  score/threshold/decode/compaction, batched NMS      -> hn_fcos_candidates, hn_fcos_nms(_ratios)
precision "f32" keeps every convolution on the exact f32-MFMA kernel (hn_conv2d_nhwc_f32; GroupNorm applied on
load by the next conv).  Everything stays on the device; nothing here synchronises with the host.
"""
from __future__ import annotations

import math

import torch

from . import ops
from .forms import engine_forms
from .weights import ConvW, bn_scale_shift, concat_cout, pack_conv, pack_stem_split

IMAGE_MEAN = (0.485, 0.456, 0.406)
IMAGE_STD = (0.229, 0.224, 0.225)
SCORE_THRESH = 0.7  # hard-coded in the reference, fcos_utils/fcos.py:600 (ctor args are ignored)
NMS_THRESH = 0.3    # hard-coded, fcos_utils/fcos.py:635
_R34 = [(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)]


def resized_size(h: int, w: int, min_size: int = 800, max_size: int = 1333):
    """Size after GeneralizedRCNNTransform.resize.  torchvision evaluates
    `float / tensor` = tensor.reciprocal() * float in fp32, then floor(size * scale) in fp64."""
    inv_min = torch.tensor(float(min(h, w))).reciprocal()
    inv_max = torch.tensor(float(max(h, w))).reciprocal()
    scale = torch.min(inv_min * float(min_size), inv_max * float(max_size)).item()
    return int(h * scale), int(w * scale)


class FCOSEngine:
    def __init__(self, state_dict, num_classes: int, device="cuda", min_size=800, max_size=1333,
                 precision="f16x3", ext=False, head_streams=None, image_mean=None, image_std=None, forms=None):
        """precision: "f16x3" (split-fp16 operands, fp32-grade; default) or "f32" (exact f32 MFMA).
        image_mean / image_std: the transform's normalisation (fcos.py:501-505; default: ImageNet's)."""
        if precision not in ("f32", "f16x3", "f16x1"):
            raise ValueError("precision must be 'f32', 'f16x3' or 'f16x1'")
        # "f16x1": the f16x3 engine with the hi*hi term alone (plain fp16 operands, one MFMA per MAC): the throughput mode
        # SURVEY D6 plans BESIDE the parity mode -- misses the 1e-3 keypoint contract, never a default
        self.terms = 1 if precision == "f16x1" else 3
        precision = "f16x3" if precision == "f16x1" else precision
        self.precision = precision
        sd = state_dict
        ops.clear_plan_caches()   # plans are keyed by weight addresses; a rebuilt engine starts clean
        dev = torch.device(device)
        self.device = dev
        self.num_classes = num_classes
        self.min_size, self.max_size = min_size, max_size
        self.image_mean = tuple(float(v) for v in (IMAGE_MEAN if image_mean is None else image_mean))
        self.image_std = tuple(float(v) for v in (IMAGE_STD if image_std is None else image_std))
        if len(self.image_mean) != 3 or len(self.image_std) != 3 or any(v == 0.0 for v in self.image_std):
            raise ValueError("image_mean / image_std must hold three values (std non-zero)")
        p = "backbone.body."

        def cbn(conv, bn, **kw):
            return pack_conv(sd[conv + ".weight"], None, bn_scale_shift(sd, bn), **kw).to(dev)

        self.stem = cbn(p + "conv1", p + "bn1", stride=2, pad=3)  # Cin 3 -> padded to 4
        # f16x3 mode: the stem runs on the split kernel too, one filter row (7 taps x 4 channels) per k tile
        self.stem16 = pack_stem_split(sd[p + "conv1.weight"], bn_scale_shift(sd, p + "bn1")).to(dev) \
            if precision == "f16x3" else None
        self.blocks = []
        for li, (planes, blocks, stride) in enumerate(_R34, start=1):
            for b in range(blocks):
                q = f"{p}layer{li}.{b}."
                st = stride if b == 0 else 1
                self.blocks.append({
                    "c1": cbn(q + "conv1", q + "bn1", stride=st, pad=1),
                    "c2": cbn(q + "conv2", q + "bn2", pad=1),
                    "ds": cbn(q + "downsample.0", q + "downsample.1", stride=st)
                    if (q + "downsample.0.weight") in sd else None,
                    "layer": li, "last": b == blocks - 1,
                })
        f = "backbone.fpn."
        self.inner = [pack_conv(sd[f"{f}inner_blocks.{i}.weight"], sd[f"{f}inner_blocks.{i}.bias"]).to(dev)
                      for i in range(3)]
        self.layer = [pack_conv(sd[f"{f}layer_blocks.{i}.weight"], sd[f"{f}layer_blocks.{i}.bias"], pad=1).to(dev)
                      for i in range(3)]
        c, r = "head.classification_head", "head.regression_head"

        def tconv(t, i):
            return pack_conv(sd[f"{t}.conv.{3 * i}.weight"], sd[f"{t}.conv.{3 * i}.bias"], pad=1)

        # layer 0 of both towers reads the same FPN level -> one 256->512 conv, one GN(64 groups)
        self.tower0 = concat_cout([tconv(c, 0), tconv(r, 0)]).to(dev)
        self.cls_tower = [tconv(c, i).to(dev) for i in range(1, 4)]
        self.reg_tower = [tconv(r, i).to(dev) for i in range(1, 4)]
        gn = lambda t, i, k: sd[f"{t}.conv.{3 * i + 1}.{k}"].float()  # noqa: E731
        self.gn0_gamma = torch.cat([gn(c, 0, "weight"), gn(r, 0, "weight")]).to(dev)
        self.gn0_beta = torch.cat([gn(c, 0, "bias"), gn(r, 0, "bias")]).to(dev)
        self.cls_gn = [(gn(c, i, "weight").to(dev), gn(c, i, "bias").to(dev)) for i in range(1, 4)]
        self.reg_gn = [(gn(r, i, "weight").to(dev), gn(r, i, "bias").to(dev)) for i in range(1, 4)]
        self.both_gn = [(torch.cat([gc, gr]), torch.cat([bc, br])) for (gc, bc), (gr, br) in zip(self.cls_gn, self.reg_gn)]
        self.cls_out = concat_cout([
            pack_conv(sd[c + ".cls_logits.weight"], sd[c + ".cls_logits.bias"], pad=1),
            pack_conv(sd[c + ".hand_lr_layer.weight"], sd[c + ".hand_lr_layer.bias"], pad=1)]).to(dev)
        self.reg_out = concat_cout([
            pack_conv(sd[r + ".bbox_reg.weight"], sd[r + ".bbox_reg.bias"], pad=1),
            pack_conv(sd[r + ".bbox_ctrness.weight"], sd[r + ".bbox_ctrness.bias"], pad=1)]).to(dev)
        if self.cls_out.cout != num_classes + 2:
            raise ValueError("checkpoint does not match num_classes")
        # ext=True heads (fcos.py:255-264): dxdy-magnitude (3, ReLU) and contact state (5) from the cls tower
        self.ext = ext
        self.ext_out = concat_cout([
            pack_conv(sd[c + ".hand_dydx_layer.weight"], sd[c + ".hand_dydx_layer.bias"], pad=1),
            pack_conv(sd[c + ".hand_contact_state_layer.weight"], sd[c + ".hand_contact_state_layer.bias"], pad=1),
        ]).to(dev) if ext else None
        self._gn_scratch = {}
        self._side = None
        # launch-structure switches (hn_amd/forms.py: defaults unless a development host changed them; never the environment)
        fm = engine_forms(forms)
        self.head_streams = fm["head_streams"] if head_streams is None else head_streams
        self.group_towers = fm["group_convs"]
        self.fuse_stem_pool = fm["fuse_stem_pool"]   # (the pooled values are bit-identical either way: ops.conv_stem_pool_split)
        self.fuse_last_gn = fm["fuse_last_gn"]       # bit-identical
        self.thin_outputs = fm["thin_outputs"] and self.cls_out.cout <= 16   # (tap form bit-identical, P form to fp32 rounding)
        # conv1 of a downsampling block together with its 1x1 downsample (ops.conv2d_nhwc_multi)
        self.multi = fm["conv_multi_fcos"] and precision == "f16x3"
        # the towers' apply passes in the tails of the other tower's convolutions, where those passes are HBM streams
        # (heads_grouped; True = always, for tests of the schedule at small shapes; results are bit-identical either way)
        self.tower_carry = fm["tower_carry"]
        self.tower_carry_force = False
        self.tower_tile = 0   # development / tests: HN_TILE_* id of the tower layers' launches in heads_grouped (0 = the heuristic)
        # output_grads: a list that receives, per heads() call, the S32 activations that feed the output convolutions
        # ({"cls": [per level], "reg": [per level]}); None (always, outside that call): nothing is kept
        self._capture = None
        # tower_grads: under _capture, heads_grouped also keeps every tower layer's S32 inputs, raw outputs and GroupNorm tables
        # (and runs the lock-step schedule, whose tensors are the carried schedule's bit for bit)
        self._capture_towers = False
        self._tower_cap = None
        # fpn_grads: backbone() appends, per call, the S32 tensors the FPN read and wrote ({"c": [c3, c4, c5], "lat": [lat3,
        # lat4, lat5]}) to _fpn_cap; off (always, outside that call): nothing is kept and nothing else differs
        self._capture_fpn = False
        self._fpn_cap = None

    def _keep(self, kind, a):
        if self._capture is not None:
            self._capture[-1][kind].append(a)

    def _keep_layer(self, a, y, aff):
        if self._capture is not None and self._capture_towers:
            self._capture[-1]["layers"].append({"a": list(a), "y": list(y), "aff": list(aff)})

    # -----------------------------------------------------------------------------------
    def _conv(self, x, cw: ConvW, relu=False, out_f32=False, **kw):
        """f16x3 mode: activations travel in the S32 split format (written by each epilogue, read by
        LDS-DMA); the stem (Cin = 4) runs on the f32 kernel; tower outputs that feed GroupNorm and
        the final head outputs are fp32."""
        s16 = self.precision == "f16x3"
        return ops.conv2d_nhwc(x, cw.w, cw.bias, stride=cw.stride, pad=cw.pad, dil=cw.dil, relu=relu,
                               w16=cw.w16 if s16 else None, out_split=s16 and not out_f32, **kw)

    def geometry(self, h, w):
        oh, ow = resized_size(h, w, self.min_size, self.max_size)
        ph, pw = int(math.ceil(oh / 32) * 32), int(math.ceil(ow / 32) * 32)
        return oh, ow, ph, pw

    def backbone(self, x):
        """x: preprocessed canvas -- fp32 [N,PH,PW,4], or the fp16 stem image [2,N,PH+6,PW+6,4] of
        ops.fcos_preprocess_split (f16x3 mode) -> [P3, P4, P5] (256 channels, strides 8/16/32; S32 in f16x3 mode)."""
        ops.PROFILE_STAGE = "resnet34_body"
        if x.dtype == torch.float16 and self.fuse_stem_pool:
            # conv1 + bn1 + relu + maxpool as one kernel: the 64-channel half-resolution map never reaches HBM
            x = ops.conv_stem_pool_split(x, self.stem16.w16, self.stem16.bias, 64, r=7, stride=2)
        else:
            if x.dtype == torch.float16:
                x = ops.conv_stem_split(x, self.stem16.w16, self.stem16.bias, 64, r=7, stride=2, relu=True)
            else:
                x = self._conv(x, self.stem, relu=True, algo_cin=3)
            x = ops.maxpool3x3s2_nhwc(x)
        feats = []
        for blk in self.blocks:
            if blk["ds"] is not None and self.multi and x.dtype == torch.float16:
                # both read the block input and neither reads the other: one grid (same bits as the two launches)
                o, idn = ops.conv2d_nhwc_multi([(x, blk["c1"], dict(relu=True)), (x, blk["ds"], dict(relu=False))])
            else:
                o = self._conv(x, blk["c1"], relu=True)
                idn = self._conv(x, blk["ds"]) if blk["ds"] is not None else x
            x = self._conv(o, blk["c2"], relu=True, residual=idn)
            if blk["last"] and blk["layer"] >= 2:
                feats.append(x)
        c3, c4, c5 = feats
        ops.PROFILE_STAGE = "fpn"
        lat5 = self._conv(c5, self.inner[2])
        lat4 = self._conv(c4, self.inner[1], residual=lat5, res_upsample=True)
        lat3 = self._conv(c3, self.inner[0], residual=lat4, res_upsample=True)
        if self._capture_fpn and self._fpn_cap is not None:
            self._fpn_cap.append({"c": [c3, c4, c5], "lat": [lat3, lat4, lat5]})
        if self.precision == "f16x3" and self.group_towers:
            # the three FPN output convs (own weights, own map size) are independent: one grouped launch
            return ops.conv2d_nhwc_grouped([lat3, lat4, lat5], self.layer, pad=1, out_split=True)
        return [self._conv(lat3, self.layer[0]), self._conv(lat4, self.layer[1]), self._conv(lat5, self.layer[2])]

    def _scratch(self, key, need, device):
        """Per-chain GroupNorm scratch (chains may run on different streams)."""
        buf = self._gn_scratch.get(key)
        if buf is None or buf.numel() < need:
            buf = self._gn_scratch[key] = torch.empty((need,), device=device, dtype=torch.float32)
        return buf

    def _gn(self, x, gamma, beta, groups, key=0):
        n, h, w, c = x.shape
        need = ops._lib.load().hn_groupnorm_scratch_floats(n, h * w, c, groups)
        return ops.groupnorm_affine(x, gamma, beta, groups=groups, scratch=self._scratch(key, need, x.device))

    # -----------------------------------------------------------------------------------
    # head: conv -> GroupNorm -> ReLU -> conv.  Each tower conv writes its raw fp32 output, GroupNorm becomes
    # a per-(image, channel) affine, and
    #   f16x3: the conv epilogue also emits the GroupNorm partial sums (no second read of its output), a
    #          tiny finalize kernel builds the tables, and one hn_affine_split_f32 pass applies affine + ReLU
    #          and emits the S32 input of the next conv (whose hot loop is then pure DMA + MFMA);
    #   f32  : a statistics pass reads the output back; the next conv applies the affine + ReLU while
    #          staging its input (in_affine).
    # -----------------------------------------------------------------------------------
    def _conv_gn(self, a, cw, gamma, beta, groups, n, hw, key):
        """tower conv + the GroupNorm tables of its output -> (raw output, scale, shift)"""
        s16 = self.precision == "f16x3"
        if s16 and hw >= 32:
            part = self._scratch(key, ops.gn_rows32_scratch_floats(n * hw, cw.cout), cw.w.device)
            y = self._conv(a, cw, out_f32=True, gn_partial=part)
            return (y, *ops.groupnorm_finalize_rows32(part, gamma, beta, n, hw, groups))
        y = self._conv(a, cw, out_f32=True) if s16 else self._conv(a[0], cw, in_scale=a[1], in_shift=a[2])
        return (y, *self._gn(y, gamma, beta, groups, key))

    def _act(self, x, scale, shift):
        """GroupNorm affine + ReLU, materialised (S32) or deferred to the next conv's load (f32 mode)."""
        return ops.to_split(x, scale, shift, relu=True) if self.precision == "f16x3" else (x, scale, shift)

    def _out_conv(self, a, cw, **kw):
        prev, ops.PROFILE_STAGE = ops.PROFILE_STAGE, "head_outputs"
        try:
            return self._out_conv_impl(a, cw, **kw)
        finally:
            ops.PROFILE_STAGE = prev

    def _out_conv_impl(self, a, cw, **kw):
        if self.precision == "f16x3":
            return self._conv(a, cw, out_f32=True, **kw)
        return self._conv(a[0], cw, in_scale=a[1], in_shift=a[2], **kw)

    def _tower0(self, feat, key):
        """Layer 0 of BOTH towers on one FPN level: one 256->512 conv, one GroupNorm with 64 groups."""
        n, fh, fw = feat.shape[:3]
        if self.precision == "f16x3":
            return self._conv_gn(feat, self.tower0, self.gn0_gamma, self.gn0_beta, 64, n, fh * fw, key)
        t0 = self._conv(feat, self.tower0, out_f32=True)
        return (t0, *self._gn(t0, self.gn0_gamma, self.gn0_beta, 64, key))

    def _cls_chain(self, t0, sc, sh, key):
        n, fh, fw = t0.shape[:3]
        x, sc, sh = t0[..., :256], sc[:, :256], sh[:, :256]
        for cw, (g, b) in zip(self.cls_tower, self.cls_gn):
            x, sc, sh = self._conv_gn(self._act(x, sc, sh), cw, g, b, 32, n, fh * fw, key)
        a = self._act(x, sc, sh)
        self._keep("cls", a)
        cls_lr = self._out_conv(a, self.cls_out)
        ext = self._out_conv(a, self.ext_out, relu_cols=3) if self.ext else None
        return cls_lr, ext

    def _reg_chain(self, t0, sc, sh, key):
        n, fh, fw = t0.shape[:3]
        x, sc, sh = t0[..., 256:], sc[:, 256:], sh[:, 256:]
        for cw, (g, b) in zip(self.reg_tower, self.reg_gn):
            x, sc, sh = self._conv_gn(self._act(x, sc, sh), cw, g, b, 32, n, fh * fw, key)
        a = self._act(x, sc, sh)
        self._keep("reg", a)
        return self._out_conv(a, self.reg_out, relu_cols=4)

    def head_level(self, feat, key=0):
        """One FPN level -> (cls_lr [N,h,w,C+2], reg_ctr [N,h,w,5], ext [N,h,w,8] or None) raw fp32 conv outputs."""
        t0, sc, sh = self._tower0(feat, key)
        n, fh, fw = t0.shape[:3]
        hw = fh * fw
        if self.precision != "f16x3" or hw < 32 or not self.group_towers:
            cls_lr, ext = self._cls_chain(t0, sc, sh, key)
            return cls_lr, self._reg_chain(t0, sc, sh, key), ext
        # f16x3: layer k of the cls tower and of the reg tower are independent and identical in shape -> ONE
        # launch each (gridDim.z = 2) whose two outputs stay stacked as [N,h,w,512] like tower0's, so that
        # ONE GroupNorm finalize (64 groups) and ONE affine+split pass serve both towers of a layer.
        part = self._scratch((key, "g2"), ops.gn_rows32_scratch_floats(n * hw, 512), t0.device)
        for cwc, cwr, (g2, b2) in zip(self.cls_tower, self.reg_tower, self.both_gn):
            a = self._act(t0, sc, sh)                                   # S32 [N,h,w,16,2,32]
            t0 = torch.empty((n, fh, fw, 512), device=t0.device, dtype=torch.float32)
            ops.conv2d_nhwc_grouped([a[:, :, :, :8], a[:, :, :, 8:]], [cwc, cwr], pad=1, outs=[t0, t0],
                                    out_channel_offsets=[0, 256], gn=[(part, 0), (part, 32)], gn_units=64)
            sc, sh = ops.groupnorm_finalize_rows32(part, g2, b2, n, hw, 64)
        a = self._act(t0, sc, sh)
        ac, ar = a[:, :, :, :8], a[:, :, :, 8:]
        self._keep("cls", ac)
        self._keep("reg", ar)
        cls_lr = self._out_conv(ac, self.cls_out)
        ext = self._out_conv(ac, self.ext_out, relu_cols=3) if self.ext else None
        reg_ctr = self._out_conv(ar, self.reg_out, relu_cols=4)
        return cls_lr, reg_ctr, ext

    def heads_grouped(self, feats):
        """All FPN levels in lockstep (f16x3): the tower weights are shared across levels and the cls / reg towers are
        independent, so layer k of both towers on all levels is ONE grouped launch (gridDim.z = 2 x levels, members of
        different map sizes); tower0 and each output conv are one launch over the levels.  6 conv launches per frame
        batch instead of 18 -- and grids that fill the chip at batch 1."""
        L = len(feats)
        n = feats[0].shape[0]
        dev = feats[0].device
        dims = [tuple(f.shape[1:3]) for f in feats]
        hw = [h * w for h, w in dims]
        parts = [self._scratch(("lv", l), ops.gn_rows32_scratch_floats(n * hw[l], 512), dev) for l in range(L)]
        new_t = lambda: [torch.empty((n, h, w, 512), device=dev, dtype=torch.float32) for h, w in dims]  # noqa: E731
        t = new_t()
        ops.PROFILE_STAGE = "towers"
        ops.conv2d_nhwc_grouped(feats, [self.tower0] * L, pad=1, outs=t, gn=[(parts[l], 0) for l in range(L)], gn_units=64)
        # GroupNorm finalize and the affine + ReLU + split pass: ONE launch each over the levels (the library falls back
        # to per-level launches of the apply pass for tensors beyond the caches, where streaming stores win)
        aff = ops.groupnorm_finalize_rows32_levels(parts, self.gn0_gamma, self.gn0_beta, n, hw, 64)
        self._keep_layer(feats, t, aff)
        if self.tower_carry and not self._capture_towers and (self.tower_carry_force or ops.split_levels_stream(n, hw, 512)):
            t, aff = self._towers_carried(t, aff, parts, new_t, n, hw)
            if t is not None:
                return self._head_outputs(t, aff, L)
            t, aff = aff   # (the launches would not carry at this shape: nothing was issued)
        for cwc, cwr, (g2, b2) in zip(self.cls_tower, self.reg_tower, self.both_gn):
            a = ops.to_split_levels(t, aff, relu=True)                  # S32 [N,h,w,16,2,32]: cls blocks 0-7, reg 8-15
            t = new_t()
            ops.conv2d_nhwc_grouped([x[:, :, :, :8] for x in a] + [x[:, :, :, 8:] for x in a], [cwc] * L + [cwr] * L,
                                    pad=1, outs=t + t, out_channel_offsets=[0] * L + [256] * L,
                                    gn=[(parts[l], 0) for l in range(L)] + [(parts[l], 32) for l in range(L)], gn_units=64,
                                    tile=self.tower_tile)
            aff = ops.groupnorm_finalize_rows32_levels(parts, g2, b2, n, hw, 64)
            self._keep_layer(a, t, aff)
        return self._head_outputs(t, aff, L)

    def _towers_carried(self, t, aff, parts, new_t, n, hw):
        """Tower layers 1-3 as one launch per TOWER (cls, then reg) instead of one per layer: the two towers are independent
        chains, so the launch of one carries the GroupNorm apply pass of the other's last output -- a pure HBM stream that
        otherwise runs alone between two convolutions that leave HBM idle -- in the tails of its workgroups
        (ops.conv2d_nhwc_grouped(carry=...)):
            apply(y0 cls) alone;  C1 + apply(y0 reg);  R1 + apply(y1 cls);  C2 + apply(y1 reg);  ...  C3 + apply(y2 reg);  R3
        Tensors, GroupNorm slabs and arithmetic are those of the lock-step schedule: same bits.  The finalize runs over the
        whole slab after each launch; only the half that launch completed is read from its tables.
        -> (stacked outputs of layer 3, their tables), or (None, (t, aff)) when the launches would not carry."""
        L = len(t)
        dev = t[0].device
        half = lambda xs, k: [x[..., 256 * k:256 * (k + 1)] for x in xs]                        # noqa: E731
        blocks = lambda xs, k: [x[:, :, :, 8 * k:8 * (k + 1)] for x in xs]                      # noqa: E731
        tabs = lambda af, k: [(sc[:, 256 * k:256 * (k + 1)], sh[:, 256 * k:256 * (k + 1)]) for sc, sh in af]   # noqa: E731
        new_a = lambda: [torch.empty(tuple(x.shape[:3]) + (16, 2, 32), device=dev, dtype=torch.float16) for x in t]  # noqa: E731

        def tower(k, cw, a, y, carry=None, query=False):
            return ops.conv2d_nhwc_grouped(blocks(a, k), [cw] * L, pad=1, outs=y, out_channel_offsets=[256 * k] * L,
                                           gn=[(parts[l], 32 * k) for l in range(L)], gn_units=64, tile=self.tower_tile,
                                           carry=carry, carry_query=query)

        a = new_a()
        if not tower(0, self.cls_tower[0], a, t, query=True):
            return None, (t, aff)
        ops.to_split_levels(half(t, 0), tabs(aff, 0), relu=True, outs=blocks(a, 0))      # needed at once: stays a pass of its own
        layers = list(zip(self.cls_tower, self.reg_tower, self.both_gn))
        for i, (cwc, cwr, (g2, b2)) in enumerate(layers):
            y = new_t()
            tower(0, cwc, a, y, carry=(half(t, 1), tabs(aff, 1), blocks(a, 1), True))      # C: reads a[cls], completes a[reg]
            aff_c = ops.groupnorm_finalize_rows32_levels(parts, g2, b2, n, hw, 64)         # (cls half valid)
            if i + 1 < len(layers):
                a_next = new_a()
                tower(1, cwr, a, y, carry=(half(y, 0), tabs(aff_c, 0), blocks(a_next, 0), True))   # R: completes a_next[cls]
            else:
                a_next = None
                tower(1, cwr, a, y)                                     # the last layer's pass stays in the head-output kernels
            t, a = y, a_next
            aff = ops.groupnorm_finalize_rows32_levels(parts, g2, b2, n, hw, 64)           # both halves valid
        return t, aff

    def _head_outputs(self, t, aff, L):
        ops.PROFILE_STAGE = "head_outputs"
        if (self.thin_outputs and self.fuse_last_gn and self.terms == 3 and not self.ext and self._capture is None
                and ops.thin_affine_applies(t, self.cls_out) and ops.thin_affine_applies(t, self.reg_out)):
            # the last GroupNorm apply pass happens on the head-output kernels' fragments (no 8 bytes per element round trip)
            cls_lr = ops.conv3x3_thin_affine_levels(t, aff, 0, self.cls_out)
            reg_ctr = ops.conv3x3_thin_affine_levels(t, aff, 256, self.reg_out, relu_cols=4)
            return list(zip(cls_lr, reg_ctr, [None] * L))
        ops.PROFILE_STAGE = "towers"
        a = ops.to_split_levels(t, aff, relu=True)
        ac, ar = [x[:, :, :, :8] for x in a], [x[:, :, :, 8:] for x in a]
        for c, r in zip(ac, ar):
            self._keep("cls", c)
            self._keep("reg", r)
        ops.PROFILE_STAGE = "head_outputs"
        if self.thin_outputs and self.terms == 3:   # <= 16 output channels: the thin-N kernels (csrc/conv3x3_thin.hip)
            # one launch for the two (ext: three) filter banks where they run the tap kernel (a single frame); else one each
            members = [(ac, self.cls_out, 0)] + ([(ac, self.ext_out, 3)] if self.ext else []) + [(ar, self.reg_out, 4)]
            outs = ops.conv3x3_thin_levels_group(members)
            cls_lr, reg_ctr = outs[0], outs[-1]
            ext = outs[1] if self.ext else [None] * L
        else:
            cls_lr = ops.conv2d_nhwc_grouped(ac, [self.cls_out] * L, pad=1)
            ext = ops.conv2d_nhwc_grouped(ac, [self.ext_out] * L, pad=1, relu_cols=3) if self.ext else [None] * L
            reg_ctr = ops.conv2d_nhwc_grouped(ar, [self.reg_out] * L, pad=1, relu_cols=4)
        return list(zip(cls_lr, reg_ctr, ext))

    def heads(self, feats):
        """All levels.  With head_streams > 1 the 2 x levels independent tower chains are spread over side
        streams so that the tail of one convolution's grid (e.g. 1700 workgroups on 512 slots at the
        stride-16 level) is filled by another chain's workgroups."""
        ops.PROFILE_STAGE = "towers"
        if self._capture is not None:
            self._capture.append({"cls": [], "reg": [], "layers": []})
        if (self.head_streams <= 1 and self.group_towers and self.precision == "f16x3" and 2 * len(feats) <= 6
                and all(f.shape[1] * f.shape[2] >= 32 for f in feats)):
            return self.heads_grouped(feats)
        if self.head_streams <= 1:
            return [self.head_level(f, key=i) for i, f in enumerate(feats)]
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = [torch.cuda.Stream(device=self.device) for _ in range(self.head_streams)]
        lv = [self._tower0(f, ("t0", i)) for i, f in enumerate(feats)]
        fork = torch.cuda.Event()
        fork.record(main)
        chains = [(i, kind) for i in range(len(feats)) for kind in ("cls", "reg")]
        results = {}
        for ci, (i, kind) in enumerate(chains):
            st = self._side[ci % len(self._side)]
            st.wait_event(fork)
            with torch.cuda.stream(st):
                if kind == "cls":
                    results[(i, "cls")] = self._cls_chain(*lv[i], key=("cls", i))
                else:
                    results[(i, "reg")] = self._reg_chain(*lv[i], key=("reg", i))
        for st in self._side:
            main.wait_stream(st)
        outs = []
        for i in range(len(feats)):
            cls_lr, ext = results[(i, "cls")]
            reg_ctr = results[(i, "reg")]
            for t in (cls_lr, ext, reg_ctr):
                if t is not None:
                    t.record_stream(main)  # allocated on a side stream, consumed on the main one
            outs.append((cls_lr, reg_ctr, ext))
        return outs

    def list_geometry(self, images):
        """torchvision batch_images for a list of [3,h_i,w_i] images: per-image (h, w, oh, ow) and the common
        canvas (max resized size rounded up to 32), fcos_utils/fcos.py:702-709."""
        geom = []
        for img in images:
            if img.dim() != 3 or img.shape[0] != 3:
                raise ValueError("expected a list of [3,H,W] images")
            h, w = int(img.shape[1]), int(img.shape[2])
            geom.append((h, w) + resized_size(h, w, self.min_size, self.max_size))
        ph = int(math.ceil(max(g[2] for g in geom) / 32) * 32)
        pw = int(math.ceil(max(g[3] for g in geom) / 32) * 32)
        return geom, ph, pw

    @ops.device_guarded
    def forward_heads(self, images):
        with ops.f16_terms(self.terms):
            return self._forward_heads(images)

    def _forward_heads(self, images):
        """images [N,3,H,W] fp32 0..1 on the GPU (or a list of [3,h_i,w_i] images of different sizes)
        -> per-level head tensors + geometry."""
        if not torch.is_tensor(images):
            geom, ph, pw = self.list_geometry(images)
            x = ops.fcos_preprocess_list(images, geom, ph, pw, self.image_mean, self.image_std, split=self.precision == "f16x3")
            oh, ow = [g[2] for g in geom], [g[3] for g in geom]
        else:
            if images.dim() != 4 or images.shape[1] != 3:
                raise ValueError("expected [N,3,H,W]")
            n, _, h, w = images.shape
            oh, ow, ph, pw = self.geometry(h, w)
            pre = ops.fcos_preprocess_split if self.precision == "f16x3" else ops.fcos_preprocess
            x = pre(images.float().contiguous(), oh, ow, ph, pw, self.image_mean, self.image_std)
        feats = self.backbone(x)
        outs = self.heads(feats)
        strides = [ph // f.shape[1] for f in feats]
        self._ext_levels = [o[2] for o in outs] if self.ext else None
        return [o[0] for o in outs], [o[1] for o in outs], strides, (oh, ow, ph, pw)

    @ops.device_guarded
    def forward_heads_each(self, images):
        """forward_heads for a list of [3,h_i,w_i] images with the network run image by image on the list's common canvas.
        The convolutions pick their forms by problem size (split-K by workgroup count), so an image's head tensors in a batch
        of two differ in their last bits from those of the image alone; here every image's rows are the bytes of that image
        alone on this canvas, whatever else the list holds -- what a per-image validation number needs (FCOS.loss_step).
        One preprocess launch for the list; the price is the batch-1 convolution forms once per image."""
        with ops.f16_terms(self.terms):
            geom, ph, pw = self.list_geometry(images)
            split = self.precision == "f16x3"
            x = ops.fcos_preprocess_list(images, geom, ph, pw, self.image_mean, self.image_std, split=split)
            per = []
            for i in range(len(images)):
                xi = x[:, i:i + 1].contiguous() if split else x[i:i + 1]
                feats = self.backbone(xi)
                # (copies: the engine may hand the same buffers out again on the next image)
                per.append([tuple(None if t is None else t.clone() for t in o) for o in self.heads(feats)])
            strides = [ph // o[0].shape[1] for o in per[0]]
            cat = lambda l, k: torch.cat([p[l][k] for p in per])
            levels = range(len(per[0]))
            self._ext_levels = [cat(l, 2) for l in levels] if self.ext else None
            return [cat(l, 0) for l in levels], [cat(l, 1) for l in levels], strides, ([g[2] for g in geom], [g[3] for g in geom], ph, pw)

    @ops.device_guarded
    def head_grads(self, images, targets, radius=1.5, upstream=None):
        """The heads, the criterion and its backward at this engine's own head tensors (ops.fcos_loss_grad; DESIGN.md section
        9s) -> (losses, fg, (d_cls_lr, d_reg_ctr, d_ext or None)), all on the device: losses = the reference's dict (0-d fp32
        tensors, four keys without ext) and fg int32 [N] are the bytes ops.fcos_loss gives on the same heads, the gradients are
        per-level lists in the heads' layouts.  images: [N,3,H,W] (the batched forms) or a list of [3,h_i,w_i] images of
        different sizes (forward_heads_each); targets: an ops.FcosTargets on the canvas's scale.  output_grads carries these
        gradients on through the output convolutions."""
        heads = self.forward_heads if torch.is_tensor(images) else self.forward_heads_each
        cls_lr, reg_ctr, strides, _ = heads(images)
        return self._grads_at_heads(cls_lr, reg_ctr, strides, targets, radius, upstream)

    def _grads_at_heads(self, cls_lr, reg_ctr, strides, targets, radius, upstream):
        *grads, res = ops.fcos_loss_grad(cls_lr, reg_ctr, strides, self.num_classes, targets,
                                         ext=self._ext_levels if self.ext else None, radius=radius, upstream=upstream,
                                         want_forward=True)
        keys = ops.FCOS_LOSS_KEYS if self.ext else ops.FCOS_LOSS_KEYS[:4]
        return {k: res.losses[i] for i, k in enumerate(keys)}, res.fg, tuple(grads)

    @ops.device_guarded
    def output_grads(self, images, targets, radius=1.5, upstream=None, want_inputs=False):
        """head_grads plus the backward of the output convolutions (ops.conv3x3_thin_backward_levels) on
        the engine's own tensors -> (losses, fg, head_grads, param_grads, d_towers): the first three are head_grads' bytes;
        param_grads = {"cls_out": (dW, db), "reg_out": ..., "ext_out": ... with ext} in the engine's layout (dW [Cout,3,3,256]
        over the concatenated rows of the bank, ONE sum over levels and images); d_towers = per level fp32 [N,h,w,512], the
        gradient at the ReLU'd activations of the last tower layer, cls half then reg half like the engine's stacked tower
        tensor (the cls half holds the ext bank's share too).  tower_grads carries it on through the towers.  For this call the heads keep the S32 activations that feed the output convolutions, and where the
        last GroupNorm apply is fused into the thin kernel the unfused, bit-identical path runs; inference is untouched.
        images / targets as head_grads takes them (a list of different sizes: image by image, concatenated per level).
        want_inputs: also return {"a_cls", "a_reg", "cls_lr", "reg_ctr", "ext"}, what the backward read.  f16x3 engines only;
        with ext the cls and ext banks must have at most 16 columns together (num_classes <= 6)."""
        if self.precision != "f16x3" or self.terms != 3:
            raise RuntimeError("output_grads needs the f16x3 engine (the backward reads the S32 activations)")
        if self.ext and self.cls_out.cout + self.ext_out.cout > 16:   # (refused here, before the heads run)
            raise ValueError(f"output_grads: the cls and ext banks have {self.cls_out.cout} + {self.ext_out.cout} output columns, "
                             "more than the 16 the backward kernel takes on one map (with ext: num_classes <= 6)")
        batched = torch.is_tensor(images)
        self._capture = []
        try:
            cls_lr, reg_ctr, strides, _ = (self.forward_heads if batched else self.forward_heads_each)(images)
        finally:
            cap, self._capture = self._capture, None
        if self._capture_towers:
            self._tower_cap = cap
        losses, fg, grads = self._grads_at_heads(cls_lr, reg_ctr, strides, targets, radius, upstream)
        levels = range(len(cls_lr))
        # (the image-by-image path: one capture per image, concatenated per level like forward_heads_each does)
        join = lambda kind, l: cap[0][kind][l] if len(cap) == 1 else torch.cat([c[kind][l] for c in cap])   # noqa: E731
        a_cls, a_reg = [join("cls", l) for l in levels], [join("reg", l) for l in levels]
        ext = self._ext_levels if self.ext else None
        d_towers = [torch.empty(tuple(t.shape[:3]) + (512,), device=t.device, dtype=torch.float32) for t in cls_lr]
        prev, ops.PROFILE_STAGE = ops.PROFILE_STAGE, "head_outputs"
        try:
            cls_members = [(self.cls_out, 0, cls_lr, grads[0])] + ([(self.ext_out, 3, ext, grads[2])] if self.ext else [])
            pg_cls, _ = ops.conv3x3_thin_backward_levels(a_cls, cls_members, dx_out=d_towers, dx_channel_offset=0)
            pg_reg, _ = ops.conv3x3_thin_backward_levels(a_reg, [(self.reg_out, 4, reg_ctr, grads[1])], dx_out=d_towers,
                                                         dx_channel_offset=256)
        finally:
            ops.PROFILE_STAGE = prev
        param_grads = {"cls_out": pg_cls[0], "reg_out": pg_reg[0]}
        if self.ext:
            param_grads["ext_out"] = pg_cls[1]
        out = (losses, fg, grads, param_grads, d_towers)
        if want_inputs:
            out += (dict(a_cls=a_cls, a_reg=a_reg, cls_lr=cls_lr, reg_ctr=reg_ctr, ext=ext),)
        return out

    def refresh_outputs(self, sd):
        """Repack the output convolutions from the reference-layout values in sd (cls_logits, hand_lr_layer, bbox_reg,
        bbox_ctrness and, with ext, hand_dydx_layer, hand_contact_state_layer: .weight / .bias) into cls_out / reg_out /
        ext_out, the way the constructor packs them (pack_conv, concat_cout, split_f16x3 with its range check).  The new values
        are COPIED INTO the banks' existing tensors (w, bias, w16): every address stays what it was, so whatever holds this
        engine -- launch plans keyed by weight addresses, a HandNetEngine's captured graphs with the banks' addresses baked in
        -- reads the new weights from its next launch or replay on.  Every bank is built and checked before any is written: a
        refusal leaves the engine as it was.  Nothing else is rebuilt."""
        c, r = "head.classification_head", "head.regression_head"

        def bank(*names):
            return concat_cout([pack_conv(sd[n + ".weight"].detach().cpu(), sd[n + ".bias"].detach().cpu(), pad=1)
                                for n in names]).to(self.device)

        cls_out = bank(c + ".cls_logits", c + ".hand_lr_layer")
        reg_out = bank(r + ".bbox_reg", r + ".bbox_ctrness")
        ext_out = bank(c + ".hand_dydx_layer", c + ".hand_contact_state_layer") if self.ext else None
        pairs = [(self.cls_out, cls_out), (self.reg_out, reg_out)] + ([(self.ext_out, ext_out)] if self.ext else [])
        fields = lambda cw: (cw.w, cw.bias, cw.w16)                      # noqa: E731
        for old, new in pairs:
            if any((a is None) != (b is None) or (a is not None and (a.shape != b.shape or a.dtype != b.dtype))
                   for a, b in zip(fields(old), fields(new))):
                raise ValueError("refresh_outputs: the values do not have the engine's shapes")
        # (inference mode: the banks may be inference tensors -- an engine first built under torch.inference_mode() -- and
        # those take an in-place write only there; ordinary tensors take it too)
        with torch.inference_mode(), ops.on_device(self.device):
            for old, new in pairs:
                for a, b in zip(fields(old), fields(new)):
                    if a is not None:
                        a.copy_(b)

    def _tower_route_check(self, images):
        """tower_grads' refusals, before the heads run: the backward walks the tensors of the grouped lock-step route only"""
        if self.precision != "f16x3" or self.terms != 3:
            raise RuntimeError("tower_grads needs the f16x3 engine with three terms (the backward reads the S32 activations)")
        if self.head_streams > 1 or not self.group_towers:
            raise RuntimeError("tower_grads needs the grouped tower route (head_streams <= 1, group_convs on)")
        if torch.is_tensor(images):
            if images.dim() != 4 or images.shape[1] != 3:
                raise ValueError("expected [N,3,H,W]")
            _, _, ph, pw = self.geometry(*images.shape[-2:])
        else:
            _, ph, pw = self.list_geometry(images)
        if (ph // 32) * (pw // 32) < 32:
            raise ValueError(f"tower_grads: the coarsest level of a {ph} x {pw} canvas has fewer than 32 pixels, where the heads "
                             "leave the grouped route")

    @ops.device_guarded
    def tower_grads(self, images, targets, radius=1.5, upstream=None, want_inputs=False):
        """output_grads carried on through the four tower layers (conv3x3 -> GroupNorm -> ReLU, twice: cls and reg) down to the
        FPN outputs -> output_grads' five results, then tower_param_grads and d_feats:
        tower_param_grads = {"tower0": (dW [512,3,3,256], db [512]), "cls_tower" / "reg_tower": [(dW [256,3,3,256], db [256])] x 3,
        "gn0": (d_gamma [512], d_beta [512]), "cls_gn" / "reg_gn": [(d_gamma [256], d_beta [256])] x 3} in the engine's layouts,
        every one ONE sum over levels and images; d_feats = per level fp32 [N,h,w,256], the gradient at the FPN outputs.
        Per layer, from the last to the first: the statistics of the layer's raw output (ops.groupnorm_stats_levels), one
        GroupNorm + ReLU backward over the stacked 512 channels / 64 groups (ops.groupnorm_relu_backward_levels), then per filter
        bank the weight gradient on the f32 MFMA (ops.conv3x3_wgrad_levels) and the input gradient as a forward convolution with
        the flipped, transposed bank (ops.conv3x3_dgrad_levels) into that bank's half of the next gradient.  For this call the
        heads keep every layer's S32 inputs, raw outputs and tables and run the lock-step schedule; inference is untouched.
        Only the grouped route is supported (f16x3, three terms, head_streams <= 1, grouped towers, every level >= 32 pixels):
        anything else is refused before the heads run.  images / targets as output_grads takes them.  want_inputs: also return
        what the backward read and wrote, output_grads' dict plus "feats" and "layers" = per layer {"a", "y", "aff", "stats",
        "g", "dy"}."""
        self._tower_route_check(images)
        self._capture_towers = True
        try:
            losses, fg, grads, param_grads, d_towers, inp = self.output_grads(images, targets, radius, upstream, want_inputs=True)
        finally:
            cap, self._tower_cap, self._capture_towers = self._tower_cap, None, False
        if not cap or any(len(c["layers"]) != 4 for c in cap):
            raise RuntimeError("tower_grads: the heads did not take the grouped route")
        nl = len(d_towers)
        if len(cap) == 1:
            layers = cap[0]["layers"]
        else:   # the image-by-image path: one capture per image, concatenated per level like forward_heads_each does
            cat = lambda ts: torch.cat(list(ts))                                                    # noqa: E731
            layers = [{"a": [cat(c["layers"][k]["a"][l] for c in cap) for l in range(nl)],
                       "y": [cat(c["layers"][k]["y"][l] for c in cap) for l in range(nl)],
                       "aff": [(cat(c["layers"][k]["aff"][l][0] for c in cap), cat(c["layers"][k]["aff"][l][1] for c in cap))
                               for l in range(nl)]} for k in range(4)]
        from .weights import dgrad_bank
        dev = d_towers[0].device
        tg = {"cls_tower": [None] * 3, "reg_tower": [None] * 3, "cls_gn": [None] * 3, "reg_gn": [None] * 3}
        half = lambda ts, k: [t[..., 256 * k:256 * (k + 1)] for t in ts]                            # noqa: E731
        prev, ops.PROFILE_STAGE = ops.PROFILE_STAGE, "towers"
        try:
            d = d_towers
            for k in (3, 2, 1, 0):
                lay = layers[k]
                gamma = self.gn0_gamma if k == 0 else self.both_gn[k - 1][0]
                lay["stats"] = ops.groupnorm_stats_levels(lay["y"], 64)
                lay["g"] = d
                dys, d_gamma, d_beta = ops.groupnorm_relu_backward_levels(lay["y"], d, lay["aff"], lay["stats"], gamma, 64)
                lay["dy"] = dys
                if k == 0:
                    tg["gn0"] = (d_gamma, d_beta)
                    tg["tower0"] = ops.conv3x3_wgrad_levels(lay["a"], dys)
                    d_feats = ops.conv3x3_dgrad_levels(dys, dgrad_bank(self.tower0.w))
                    break
                tg["cls_gn"][k - 1], tg["reg_gn"][k - 1] = (d_gamma[:256], d_beta[:256]), (d_gamma[256:], d_beta[256:])
                d = [torch.empty(tuple(t.shape), device=dev, dtype=torch.float32) for t in dys]
                for h, (name, tower) in enumerate((("cls_tower", self.cls_tower), ("reg_tower", self.reg_tower))):
                    tg[name][k - 1] = ops.conv3x3_wgrad_levels([a[:, :, :, 8 * h:8 * (h + 1)] for a in lay["a"]], half(dys, h))
                    ops.conv3x3_dgrad_levels(half(dys, h), dgrad_bank(tower[k - 1].w), outs=d, out_channel_offset=256 * h)
        finally:
            ops.PROFILE_STAGE = prev
        out = (losses, fg, grads, param_grads, d_towers, tg, d_feats)
        if want_inputs:
            out += (dict(inp, feats=layers[0]["a"], layers=layers),)
        return out

    def refresh_towers(self, sd):
        """refresh_outputs' twin for the towers: repack the reference-layout values in sd -- head.classification_head.conv.{0,3,6,9}
        and head.regression_head.conv.{0,3,6,9} (.weight / .bias: the convolutions) and conv.{1,4,7,10} (the GroupNorms) -- into
        tower0, cls_tower, reg_tower and every GroupNorm tensor, the concatenated copies gn0_gamma / gn0_beta / both_gn included,
        the way the constructor packs them.  Everything is built and checked first (shapes, the f16x3 range check), then COPIED
        INTO the existing tensors: addresses, launch plans and captured graphs survive; a refusal leaves the engine as it was."""
        c, r = "head.classification_head", "head.regression_head"
        val = lambda k: sd[k].detach().cpu()                                                         # noqa: E731
        tconv = lambda t, i: pack_conv(val(f"{t}.conv.{3 * i}.weight"), val(f"{t}.conv.{3 * i}.bias"), pad=1)   # noqa: E731
        gn = lambda t, i, k: val(f"{t}.conv.{3 * i + 1}.{k}").float()                                # noqa: E731
        convs = [(self.tower0, concat_cout([tconv(c, 0), tconv(r, 0)]).to(self.device))]
        convs += [(old, tconv(t, i).to(self.device)) for t, tower in ((c, self.cls_tower), (r, self.reg_tower))
                  for i, old in enumerate(tower, start=1)]
        pairs = [(a, b) for old, new in convs for a, b in zip((old.w, old.bias, old.w16), (new.w, new.bias, new.w16))]
        pairs += [(self.gn0_gamma, torch.cat([gn(c, 0, "weight"), gn(r, 0, "weight")])),
                  (self.gn0_beta, torch.cat([gn(c, 0, "bias"), gn(r, 0, "bias")]))]
        for i in range(1, 4):
            gc, bc, gr, br = gn(c, i, "weight"), gn(c, i, "bias"), gn(r, i, "weight"), gn(r, i, "bias")
            pairs += [(self.cls_gn[i - 1][0], gc), (self.cls_gn[i - 1][1], bc), (self.reg_gn[i - 1][0], gr), (self.reg_gn[i - 1][1], br),
                      (self.both_gn[i - 1][0], torch.cat([gc, gr])), (self.both_gn[i - 1][1], torch.cat([bc, br]))]
        for a, b in pairs:
            if (a is None) != (b is None) or (a is not None and (a.shape != b.shape or a.dtype != b.dtype)):
                raise ValueError("refresh_towers: the values do not have the engine's shapes")
            if a is not None and a.dtype == torch.float32 and not bool(torch.isfinite(b).all()):
                raise ValueError("refresh_towers: non-finite values")
        with torch.inference_mode(), ops.on_device(self.device):
            for a, b in pairs:
                if a is not None:
                    a.copy_(b)

    @ops.device_guarded
    def fpn_grads(self, images, targets, radius=1.5, upstream=None, want_inputs=False):
        """tower_grads carried on through the FPN -- the three 3x3 output convolutions, the top-down nearest-neighbour read and
        the three 1x1 laterals -- down to the outputs of the ResNet body -> tower_grads' seven results,
        then fpn_param_grads and d_body: fpn_param_grads = {"inner": [(dW [256,Cin_l], db [256])] x 3, "layer": [(dW
        [256,3,3,256], db [256])] x 3} in the engine's layouts, level order P3, P4, P5; d_body = per level fp32 [N,h,w,Cin_l],
        the gradient at C3 / C4 / C5 (Cin 128 / 256 / 512).  With G_l = d_feats[l]: the output convolutions' weight gradients are
        ops.conv3x3_wgrad_levels on (lat_l, G_l), one call per level (each level has its own bank); D3 = dgrad(G3), D4 =
        dgrad(G4) + upT(D3), D5 = dgrad(G5) + upT(D4), where upT is ops.upsample_nearest_backward and goes in as the f32 kernel's
        dense residual; the laterals' gradients are ops.conv1x1_wgrad on (c_l, D_l) and dC_l = the 1x1 convolution of D_l with
        weights.dgrad_bank_1x1.  The S32 rounding of lat_l is passed straight through.  For this call only, backbone() keeps
        c3..c5 and lat3..lat5; inference is untouched.  Refusals are tower_grads'.  images / targets as tower_grads takes them (a
        list of different sizes: image by image, concatenated per level).  want_inputs: tower_grads' dict plus, per level, "c",
        "lat", "D" and "U" (U[l] = upT(D[l - 1]), the residual of D[l]'s launch; None at P3)."""
        self._tower_route_check(images)
        self._capture_fpn, self._fpn_cap = True, []
        try:
            res = self.tower_grads(images, targets, radius, upstream, want_inputs=True)
        finally:
            cap, self._fpn_cap, self._capture_fpn = self._fpn_cap, None, False
        *res, inp = res
        d_feats = res[6]
        nl = len(d_feats)
        if not cap or nl != 3:
            raise RuntimeError("fpn_grads: the backbone kept nothing")
        join = lambda kind, l: cap[0][kind][l] if len(cap) == 1 else torch.cat([c[kind][l] for c in cap])   # noqa: E731
        cs, lats = [join("c", l) for l in range(nl)], [join("lat", l) for l in range(nl)]
        from .weights import dgrad_bank, dgrad_bank_1x1
        prev, ops.PROFILE_STAGE = ops.PROFILE_STAGE, "fpn"
        try:
            layer = [ops.conv3x3_wgrad_levels([lats[l]], [d_feats[l]]) for l in range(nl)]
            ds, ups = [], [None]
            for l in range(nl):
                ds.append(ops.conv3x3_dgrad_levels([d_feats[l]], dgrad_bank(self.layer[l].w), residuals=[ups[l]])[0])
                if l + 1 < nl:
                    ups.append(ops.upsample_nearest_backward(ds[l], tuple(lats[l + 1].shape[1:3])))
            inner = [ops.conv1x1_wgrad(cs[l], ds[l]) for l in range(nl)]
            d_body = [ops.conv2d_nhwc(ds[l], dgrad_bank_1x1(self.inner[l].w)) for l in range(nl)]
        finally:
            ops.PROFILE_STAGE = prev
        out = tuple(res) + ({"inner": inner, "layer": layer}, d_body)
        if want_inputs:
            out += (dict(inp, c=cs, lat=lats, D=ds, U=ups),)
        return out

    def refresh_fpn(self, sd):
        """refresh_towers' twin for the FPN: repack the reference-layout values in sd -- backbone.fpn.inner_blocks.{0,1,2} and
        backbone.fpn.layer_blocks.{0,1,2} (.weight / .bias) -- into the six banks of inner and layer, the way the constructor
        packs them.  Everything is built and checked first (shapes, finiteness, the f16x3 range check), then COPIED INTO the
        existing tensors: addresses, launch plans and captured graphs survive; a refusal leaves the engine as it was."""
        f = "backbone.fpn."
        val = lambda k: sd[k].detach().cpu()                                                         # noqa: E731
        convs = [(self.inner[i], pack_conv(val(f"{f}inner_blocks.{i}.weight"), val(f"{f}inner_blocks.{i}.bias")).to(self.device))
                 for i in range(3)]
        convs += [(self.layer[i], pack_conv(val(f"{f}layer_blocks.{i}.weight"), val(f"{f}layer_blocks.{i}.bias"), pad=1).to(self.device))
                  for i in range(3)]
        pairs = [(a, b) for old, new in convs for a, b in zip((old.w, old.bias, old.w16), (new.w, new.bias, new.w16))]
        for a, b in pairs:
            if (a is None) != (b is None) or (a is not None and (a.shape != b.shape or a.dtype != b.dtype)):
                raise ValueError("refresh_fpn: the values do not have the engine's shapes")
            if a is not None and a.dtype == torch.float32 and not bool(torch.isfinite(b).all()):
                raise ValueError("refresh_fpn: non-finite values")
        with torch.inference_mode(), ops.on_device(self.device):
            for a, b in pairs:
                if a is not None:
                    a.copy_(b)

    @ops.device_guarded
    def detect(self, images, cand=None, det=None, nms_scratch=None):
        """Full detector on the device -> ops.Detections (fixed capacity, score-ordered).  images: [N,3,H,W], or a
        list of [3,h_i,w_i] tensors of different sizes (each resized on its own, boxes rescaled per image)."""
        cls_lr, reg_ctr, strides, (oh, ow, ph, pw) = self.forward_heads(images)
        cand = ops.fcos_candidates(cls_lr, reg_ctr, strides, self.num_classes, SCORE_THRESH, out=cand)
        if det is None:   # (rows at or beyond count[i] stay undefined: nobody downstream reads them)
            det = ops.alloc_detections(cand.scores.shape[0], cand.scores.shape[1], cand.scores.device, zero=False)
        # resize_boxes (fcos.py:770-783): fp32 tensor / fp32 tensor
        if not torch.is_tensor(images):
            hs = torch.tensor([float(i.shape[1]) for i in images]) / torch.tensor([float(v) for v in oh])
            ws = torch.tensor([float(i.shape[2]) for i in images]) / torch.tensor([float(v) for v in ow])
            ratios = torch.stack([hs, ws], dim=1).contiguous().to(self.device)
            return ops.fcos_nms(cand, NMS_THRESH, 1.0, 1.0, scratch=nms_scratch, out=det, ratios=ratios), cand
        n, _, h, w = images.shape
        ratio_h = (torch.tensor(float(h)) / torch.tensor(float(oh))).item()
        ratio_w = (torch.tensor(float(w)) / torch.tensor(float(ow))).item()
        det = ops.fcos_nms(cand, NMS_THRESH, ratio_h, ratio_w, scratch=nms_scratch, out=det)
        return det, cand

    @ops.device_guarded
    def detect_ext(self, images, zero=True):
        """ext=True detector: (Detections, Candidates, contacts [N,cap] int32, dxdymags [N,cap,3]).  zero=False: no fill
        launches -- the two tensors' rows at or beyond count[i] are then undefined, like the detections' (the engines' steps,
        which only ever read the rows below it, ask for this)."""
        if not self.ext:
            raise RuntimeError("engine was built without the ext heads")
        det, cand = self.detect(images)
        out = None
        if not zero:
            n, cap = det.scores.shape
            out = (torch.empty((n, cap), device=det.scores.device, dtype=torch.int32),
                   torch.empty((n, cap, 3), device=det.scores.device, dtype=torch.float32))
        contacts, dxdymags = ops.fcos_ext_gather(self._ext_levels, det, cand, out=out)
        return det, cand, contacts, dxdymags

    # -----------------------------------------------------------------------------------
    def macs_per_frame(self, h=480, w=640) -> int:
        """Algorithmic conv MACs exactly as the reference executes them (3-channel stem, padded canvas)."""
        _, _, ph, pw = self.geometry(h, w)
        total = 0
        sh, sw = ph // 2, pw // 2
        total += sh * sw * 64 * 49 * 3
        sh, sw = sh // 2, sw // 2
        sizes = {}
        for blk in self.blocks:
            st = blk["c1"].stride
            sh, sw = sh // st, sw // st
            total += sh * sw * (blk["c1"].macs_per_pixel() + blk["c2"].macs_per_pixel())
            if blk["ds"] is not None:
                total += sh * sw * blk["ds"].macs_per_pixel()
            sizes[blk["layer"]] = (sh, sw)
        pts = 0
        for i, li in enumerate((2, 3, 4)):
            a, b = sizes[li]
            total += a * b * (self.inner[i].macs_per_pixel() + self.layer[i].macs_per_pixel())
            pts += a * b
        per_pt = self.tower0.macs_per_pixel() + sum(c.macs_per_pixel() for c in self.cls_tower + self.reg_tower)
        per_pt += self.cls_out.macs_per_pixel() + self.reg_out.macs_per_pixel()
        per_pt += self.ext_out.macs_per_pixel() if self.ext else 0
        return total + pts * per_pt
