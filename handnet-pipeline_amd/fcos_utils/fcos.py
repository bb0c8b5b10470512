"""Drop-in `fcos_utils.fcos.FCOS` running on MI355X HIP kernels.

Same constructor arguments, state_dict layout and eval-mode call contract as the
reference class (fcos_utils/fcos.py:398-767): `model(images: list of [3,H,W] in 0..1)`
returns one dict per image with `boxes [k,4]` (original-image pixels, unclipped),
`scores [k]`, `labels [k] int64`, `sides [k] int64`, `feature_idx [k] float32`, sorted by
descending score; with `ext=True` (the class default, used by trainval_net_fcos.py --test-only) the dicts hold
`dxdymags [k,3]`, `contacts [k] int64` and `sides` instead of `feature_idx` (fcos.py:637-647).  As in the reference, `score_thresh / nms_thresh / topk_candidates /
detections_per_img` are accepted and IGNORED: post-processing hard-codes score > 0.7 and
NMS IoU 0.3 (fcos.py:600,635).

The criterion is an opt-in: after `device_loss()`, `model.train(); model(images, targets)` returns the reference's loss dict
(fcos.py:523-570 the matching, :44-178 the six terms) computed on the device from the detector's own head tensors, and
`loss_step` is the same for a validation loop in either mode (hn_amd.ops.fcos_loss).  `head_grads` adds the
criterion's backward at those head tensors in one more launch (hn_amd.ops.fcos_loss_grad), and
`output_grads` carries it through the output convolutions to the gradients of their weights and biases under the reference's
parameter names (hn_amd.ops.conv3x3_thin_backward_levels); after a step on those parameters,
`refresh_outputs()` repacks them into the engine.  `tower_grads` carries the backward on through the four tower layers (GroupNorm
and 256 -> 256 convolution gradients), so that every parameter of the head has a gradient, and
`refresh_towers()` is `refresh_outputs()` for them.  `fpn_grads` carries it on through the FPN (the 3x3 output convolutions, the
top-down read and the 1x1 laterals) with `refresh_fpn()` as its refresh: head + FPN on a frozen ResNet-34 is
a complete step, and the gradient at C3 / C4 / C5 comes out.  The backward stops at the body's outputs: there is none through the
ResNet body and no optimizer on the device; without the opt-in, train mode and targets raise as before.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from hn_amd import ops, synth
from hn_amd.fcos_engine import FCOSEngine
from hn_amd.state import EngineOwner, build_state_tree


class FCOS(EngineOwner):
    def __init__(self, num_classes: int, ext: bool = True, min_size: int = 800, max_size: int = 1333,
                 image_mean: Optional[List[float]] = None, image_std: Optional[List[float]] = None,
                 anchor_generator=None, head=None, center_sampling_radius: float = 1.5,
                 score_thresh: float = 0.2, nms_thresh: float = 0.6, detections_per_img: int = 100,
                 topk_candidates: int = 1000):
        super().__init__()
        if anchor_generator is not None or head is not None:
            # (the reference accepts torch modules here, fcos.py:483-494; this class runs fixed HIP layer graphs --
            # listed under "deviations" in INTEGRATION.md)
            raise NotImplementedError("custom anchor_generator / head modules are not supported")
        # forwarded to the transform like the reference does (fcos.py:501-505)
        self.image_mean = [0.485, 0.456, 0.406] if image_mean is None else [float(v) for v in image_mean]
        self.image_std = [0.229, 0.224, 0.225] if image_std is None else [float(v) for v in image_std]
        self.ext = ext
        self.num_classes = num_classes
        self.min_size, self.max_size = min_size, max_size
        # the criterion's centre sampling radius (fcos.py:545); the four below are stored and ignored, exactly like the reference
        # (fcos.py:507-511)
        self.center_sampling_radius = center_sampling_radius
        self.score_thresh, self.nms_thresh = score_thresh, nms_thresh
        self.detections_per_img, self.topk_candidates = detections_per_img, topk_candidates
        tree = build_state_tree(synth.make_fcos_state_dict(seed=0, num_classes=num_classes, ext=ext))
        for name, child in tree.named_children():
            self.add_module(name, child)

    def engine(self) -> FCOSEngine:
        dev = self._require_gpu()
        if self._engine is None:
            sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
            self._engine = FCOSEngine(sd, self.num_classes, device=dev, min_size=self.min_size,
                                      max_size=self.max_size, ext=self.ext, image_mean=self.image_mean,
                                      image_std=self.image_std)
        return self._engine

    _detection_ap = None   # the module's hn_amd.metrics.DetectionAP once device_metrics() was called

    def device_metrics(self, annotations, image_index, **options):
        """Opt in to the evaluation's numbers computed on the device (hn_amd.metrics.DetectionAP): the six
        AP tables `evaluate()` of trainval_net_fcos.py gets from the VOC text files and voc_eval.py.  annotations: the reference's
        annotation cache dict (image name -> records) or its flattened form; image_index: the image names, position = the id a
        batch carries; options: max_dets, hand_label, object_label, score_min, ovthresh.  Returns the accumulator and keeps it
        for `eval_step` / `eval_results`.  `forward` is untouched."""
        if not self.ext:
            raise RuntimeError("the evaluation needs the ext heads (contacts, dxdymags): FCOS(ext=True)")
        from hn_amd.metrics import DetectionAP
        self._detection_ap = DetectionAP(self._require_gpu(), annotations, image_index, **options)
        return self._detection_ap

    def _require_metrics(self):
        if self._detection_ap is None:
            raise RuntimeError("call device_metrics(annotations, image_index) before eval_step / eval_results")
        return self._detection_ap

    def eval_step(self, images: List[torch.Tensor], image_ids) -> None:
        """One batch of the evaluation loop (trainval_net_fcos.py:121-169) without its host side: the detector, then ONE more
        launch that files the batch's records under their image ids.  No dicts are built, no count is copied to the host and
        nothing waits.  image_ids: int32 [N] on the device (anything else is converted and uploaded)."""
        ap = self._require_metrics()
        if self.training:
            raise NotImplementedError("training (fcos.py:543-570 losses) is outside the inference hot path")
        det, _, contacts, dxdymags = self.engine().detect_ext(self._batch(images))
        if not (torch.is_tensor(image_ids) and image_ids.is_cuda and image_ids.dtype == torch.int32):
            image_ids = torch.as_tensor(image_ids).to(dtype=torch.int32).reshape(-1).to(det.scores.device)
        ap.update(det, contacts, dxdymags, image_ids.contiguous())

    def eval_results(self, use_07_metric: bool = False):
        """The epoch's end: {name: {'ap', 'rec', 'prec'}} for targetobject, hand and hand + handstate / handside / objectbbox /
        all, plus mean_ap, npos and fed (one device -> host copy); the accumulator then starts the next epoch from zero."""
        ap = self._require_metrics()
        results = ap.compute(use_07_metric)
        ap.reset()
        return results

    _device_loss = False   # device_loss(): train-mode forward(images, targets) returns the loss dict

    def device_loss(self, on: bool = True):
        """Opt in to (or out of) the criterion on the device.  On and in train mode, `forward(images, targets)` returns the
        reference's loss dict; off (the default) every path behaves as before.  Returns self."""
        self._device_loss = bool(on)
        return self

    def loss_step(self, images: List[torch.Tensor], targets, want_terms: bool = False):
        """The detector's heads plus the criterion's two launches, in either mode: -> (losses, fg) with losses the reference's
        dict (classification, bbox_regression, bbox_ctrness, hand_lr and, with ext, hand_contact_state, hand_dxdy: 0-d fp32
        tensors on the device) and fg int32 [N], the foreground points per image.  Nothing is copied to the host and nothing
        waits.  targets: the reference's list of dicts ('boxes' in image pixels, 'labels', 'box_info'), scaled per image like
        torchvision's transform scales them, or an ops.FcosTargets already on the canvas's scale.  Equal-size batches and lists
        of differently sized images (per-image ratios, anchors on the common canvas) both work; a list of different sizes runs
        the network image by image (FCOSEngine.forward_heads_each), so that an image's terms and fg are the bytes of that
        image alone on the same canvas, whatever else the list holds.  want_terms: also return the per-image sums [N, 6] before
        any factor or division."""
        return self._loss_step(images, targets, want_terms, False)

    def head_grads(self, images: List[torch.Tensor], targets):
        """loss_step(images, targets) and the criterion's backward at the engine's own head tensors in one more launch
        (ops.fcos_loss_grad) -> (losses, fg, (d_cls_lr, d_reg_ctr, d_ext or None)): losses and fg are
        loss_step's bytes, the gradients are those of the sum of the dict's values (what trainval_net_fcos.py:56-57
        back-propagates) with respect to the per-level head tensors, in their layouts ([N,h,w,C+2], [N,h,w,5], [N,h,w,8]) and
        on the device.  Equal-size batches and lists of differently sized images take loss_step's paths.  Nothing is copied to
        the host and nothing waits."""
        return self._loss_step(images, targets, False, True)

    # the reference's modules behind the engine's output banks, in the banks' row order
    _OUTPUT_BANKS = (("cls_out", ("head.classification_head.cls_logits", "head.classification_head.hand_lr_layer")),
                     ("reg_out", ("head.regression_head.bbox_reg", "head.regression_head.bbox_ctrness")),
                     ("ext_out", ("head.classification_head.hand_dydx_layer", "head.classification_head.hand_contact_state_layer")))

    def _output_banks(self):
        return [(bank, names) for bank, names in self._OUTPUT_BANKS if self.ext or bank != "ext_out"]

    def output_grads(self, images: List[torch.Tensor], targets, assign: bool = False):
        """head_grads(images, targets) carried on through the output convolutions (FCOSEngine.output_grads; DESIGN.md section
        9t) -> (losses, fg, grads): losses and fg are head_grads' bytes; grads maps the reference's parameter names -- .weight
        [Cout,Cin,3,3] and .bias [Cout] of head.classification_head.cls_logits / hand_lr_layer, head.regression_head.bbox_reg /
        bbox_ctrness and, with ext, head.classification_head.hand_dydx_layer / hand_contact_state_layer -- to the gradient of
        the sum of the dict's values, on the device: the engine bank's rows un-concatenated and permuted to the reference's
        layout.  assign: also set .grad of the module's own parameters, so that torch.optim.SGD over them followed by
        refresh_outputs() is a fine-tuning step of the output layers (a linear probe on frozen towers).  There is no backward
        through the towers or the backbone."""
        dev = self._require_gpu()
        eng = self.engine()
        batch = self._batch(images)
        if torch.is_tensor(batch):
            oh, ow = eng.geometry(*batch.shape[-2:])[:2]
        else:
            oh, ow = zip(*[g[2:] for g in eng.list_geometry(batch)[0]])
        targets = self._packed_targets(images, batch, targets, oh, ow, dev)
        losses, fg, _, param_grads, _ = eng.output_grads(batch, targets, radius=self.center_sampling_radius)
        return losses, fg, self._named_grads(self._named_output_grads(param_grads), assign)

    def _named_output_grads(self, param_grads):
        """the engine's output banks' (dW, db) -> the reference's names and layouts: rows un-concatenated, [Cout,Cin,3,3]"""
        grads = {}
        params = dict(self.named_parameters())
        for bank, names in self._output_banks():
            d_w, d_b = param_grads[bank]
            row = 0
            for name in names:
                cout = params[name + ".weight"].shape[0]
                grads[name + ".weight"] = d_w[row:row + cout].permute(0, 3, 1, 2).contiguous()
                grads[name + ".bias"] = d_b[row:row + cout].clone()
                row += cout
        return grads

    def _named_grads(self, grads, assign):
        if assign:
            params = dict(self.named_parameters())
            for key, g in grads.items():
                params[key].grad = g
        return grads

    _TOWERS = (("head.classification_head", "cls_tower", "cls_gn", 0), ("head.regression_head", "reg_tower", "reg_gn", 1))

    def tower_grads(self, images: List[torch.Tensor], targets, assign: bool = False):
        """output_grads(images, targets) carried on through the towers (FCOSEngine.tower_grads) ->
        (losses, fg, grads): grads holds output_grads' entries and, under head.classification_head and head.regression_head,
        conv.{0,3,6,9}.weight [256,256,3,3] / .bias [256] (the tower convolutions) and conv.{1,4,7,10}.weight / .bias [256] (their
        GroupNorms): the engine's gradients permuted to the reference's layout, the stacked layer 0 (one 256 -> 512 bank, one
        512-channel GroupNorm) un-concatenated into the two towers' halves.  With it every parameter of the head has a gradient.
        assign: also set .grad of the module's own parameters, so that an optimizer step over the head followed by
        refresh_towers() and refresh_outputs() is a fine-tuning step on a frozen backbone.  fpn_grads carries the backward on
        through the FPN; there is none through the ResNet body."""
        eng, batch, targets = self._grads_args(images, targets)
        losses, fg, _, param_grads, _, tg, _ = eng.tower_grads(batch, targets, radius=self.center_sampling_radius)
        return losses, fg, self._named_grads(self._named_tower_grads(param_grads, tg), assign)

    def _grads_args(self, images, targets):
        """-> (engine, batch, packed targets) the way output_grads prepares them"""
        dev = self._require_gpu()
        eng = self.engine()
        batch = self._batch(images)
        if torch.is_tensor(batch):
            oh, ow = eng.geometry(*batch.shape[-2:])[:2]
        else:
            oh, ow = zip(*[g[2:] for g in eng.list_geometry(batch)[0]])
        return eng, batch, self._packed_targets(images, batch, targets, oh, ow, dev)

    def _named_tower_grads(self, param_grads, tg):
        """the engine's output and tower gradients -> the reference's names and layouts"""
        grads = self._named_output_grads(param_grads)
        for head, tower, gn, h in self._TOWERS:
            rows = slice(256 * h, 256 * (h + 1))
            convs = [(tg["tower0"][0][rows], tg["tower0"][1][rows])] + list(tg[tower])
            norms = [(tg["gn0"][0][rows], tg["gn0"][1][rows])] + list(tg[gn])
            for i, ((d_w, d_b), (d_gamma, d_beta)) in enumerate(zip(convs, norms)):
                grads[f"{head}.conv.{3 * i}.weight"] = d_w.permute(0, 3, 1, 2).contiguous()
                grads[f"{head}.conv.{3 * i}.bias"] = d_b.clone()
                grads[f"{head}.conv.{3 * i + 1}.weight"] = d_gamma.clone()
                grads[f"{head}.conv.{3 * i + 1}.bias"] = d_beta.clone()
        return grads

    def fpn_grads(self, images: List[torch.Tensor], targets, assign: bool = False):
        """tower_grads(images, targets) carried on through the FPN (FCOSEngine.fpn_grads) -> (losses, fg,
        grads): grads holds tower_grads' entries and backbone.fpn.inner_blocks.{0,1,2}.weight [256,Cin,1,1] / .bias [256] (the
        1x1 laterals, Cin 128 / 256 / 512) and backbone.fpn.layer_blocks.{0,1,2}.weight [256,256,3,3] / .bias [256] (the output
        convolutions): every parameter the reference trains outside the ResNet body.  assign: also set .grad, so that an optimizer
        step followed by refresh_fpn(), refresh_towers() and refresh_outputs() is a fine-tuning step of head + FPN on a frozen
        ResNet-34.  The backward stops at the body's outputs (FCOSEngine.fpn_grads also returns the gradient there)."""
        eng, batch, targets = self._grads_args(images, targets)
        res = eng.fpn_grads(batch, targets, radius=self.center_sampling_radius)
        losses, fg, param_grads, tg, fg_fpn = res[0], res[1], res[3], res[5], res[7]
        grads = self._named_tower_grads(param_grads, tg)
        for i in range(3):
            d_w, d_b = fg_fpn["inner"][i]
            grads[f"backbone.fpn.inner_blocks.{i}.weight"] = d_w.reshape(d_w.shape[0], d_w.shape[1], 1, 1).clone()
            grads[f"backbone.fpn.inner_blocks.{i}.bias"] = d_b.clone()
            d_w, d_b = fg_fpn["layer"][i]
            grads[f"backbone.fpn.layer_blocks.{i}.weight"] = d_w.permute(0, 3, 1, 2).contiguous()
            grads[f"backbone.fpn.layer_blocks.{i}.bias"] = d_b.clone()
        return losses, fg, self._named_grads(grads, assign)

    def refresh_fpn(self):
        """Repack the module's CURRENT values of the FPN's twelve parameters (those fpn_grads names) into the engine's inner and
        layer banks, with the f16x3 range check; like refresh_towers() the engine is kept and its tensors keep their addresses.  A
        value beyond the fp16 range raises and leaves the engine as it was."""
        params = dict(self.named_parameters())
        sd = {f"backbone.fpn.{b}.{i}.{k}": params[f"backbone.fpn.{b}.{i}.{k}"] for b in ("inner_blocks", "layer_blocks")
              for i in range(3) for k in ("weight", "bias")}
        self.engine().refresh_fpn(sd)
        return self

    def refresh_towers(self):
        """Repack the module's CURRENT values of the towers' parameters (the convolutions and GroupNorms tower_grads names) into
        the engine's tower banks and GroupNorm tensors, with the f16x3 range check; like refresh_outputs() the engine is kept and
        its tensors keep their addresses.  A value beyond the fp16 range raises and leaves the engine as it was."""
        params = dict(self.named_parameters())
        sd = {f"{head}.conv.{j}.{k}": params[f"{head}.conv.{j}.{k}"] for head, _, _, _ in self._TOWERS
              for i in range(4) for j in (3 * i, 3 * i + 1) for k in ("weight", "bias")}
        self.engine().refresh_towers(sd)
        return self

    def refresh_outputs(self):
        """Repack the module's CURRENT values of the output layers' parameters (those output_grads names) into the engine's
        cls_out / reg_out / ext_out banks, with the f16x3 range check; the engine itself is kept, not rebuilt, and the banks' tensors keep
        their addresses (the values are copied into them), so a HandNet that shares this engine and its captured graphs run with
        the new weights from their next step on.  A value beyond
        the fp16 range raises and leaves the engine's banks as they were."""
        eng = self.engine()
        params = dict(self.named_parameters())
        sd = {name + k: params[name + k] for _, names in self._output_banks() for name in names for k in (".weight", ".bias")}
        eng.refresh_outputs(sd)
        return self

    def _packed_targets(self, images, batch, targets, oh, ow, dev):
        """The reference's list of target dicts, scaled per image like torchvision's transform scales them -> ops.FcosTargets on
        the canvas's scale (an ops.FcosTargets passes through).  oh, ow: the resized size, one pair for an equal-size batch, one
        per image for a list of different sizes."""
        if isinstance(targets, ops.FcosTargets):
            return targets
        if len(targets) != len(images):
            raise ValueError("one target dict per image")
        new = [(oh, ow)] * len(images) if torch.is_tensor(batch) else list(zip(oh, ow))
        ratios = ops.fcos_target_ratios([tuple(i.shape[-2:]) for i in images], new)
        return ops.pack_fcos_targets(targets, ratios, num_classes=self.num_classes, ext=self.ext, device=dev)

    def _loss_step(self, images, targets, want_terms, head_grads):
        dev = self._require_gpu()
        eng = self.engine()
        batch = self._batch(images)
        heads = eng.forward_heads if torch.is_tensor(batch) else eng.forward_heads_each
        cls_lr, reg_ctr, strides, (oh, ow, _, _) = heads(batch)
        targets = self._packed_targets(images, batch, targets, oh, ow, dev)
        ext = eng._ext_levels if self.ext else None
        grads = None
        with ops.on_device(dev):
            if head_grads:
                *grads, res = ops.fcos_loss_grad(cls_lr, reg_ctr, strides, self.num_classes, targets, ext=ext,
                                                 radius=self.center_sampling_radius, want_forward=True)
            else:
                res = ops.fcos_loss(cls_lr, reg_ctr, strides, self.num_classes, targets, ext=ext,
                                    radius=self.center_sampling_radius)
        keys = ops.FCOS_LOSS_KEYS if self.ext else ops.FCOS_LOSS_KEYS[:4]
        losses = {k: res.losses[i] for i, k in enumerate(keys)}
        if head_grads:
            return losses, res.fg, tuple(grads)
        return (losses, res.fg, res.terms) if want_terms else (losses, res.fg)

    @staticmethod
    def _batch(images):
        if len({tuple(i.shape) for i in images}) != 1:
            # torchvision batch_images (fcos.py:702-709): every image is resized on its own, padded to the common
            # canvas, and its boxes are scaled back by its own ratios
            return [i.float() for i in images]
        return torch.stack([i.float() for i in images])

    def forward(self, images: List[torch.Tensor], targets=None) -> List[Dict[str, torch.Tensor]]:
        if self._device_loss and self.training:
            if targets is None:
                raise ValueError("In training mode, targets should be passed")
            return self.loss_step(images, targets)[0]
        if self.training or targets is not None:
            raise NotImplementedError("training (fcos.py:543-570 losses) is outside the inference hot path")
        if len({tuple(i.shape) for i in images}) != 1:
            # torchvision batch_images (fcos.py:702-709): every image is resized on its own, padded to the common
            # canvas, and its boxes are scaled back by its own ratios
            batch = [i.float() for i in images]
        else:
            batch = torch.stack([i.float() for i in images])
        if self.ext:
            det, _, contacts, dxdymags = self.engine().detect_ext(batch)
        else:
            det, _ = self.engine().detect(batch)
        counts = det.count.cpu().tolist()  # the list-of-dicts contract needs lengths on the host
        out = []
        for i, k in enumerate(counts):
            if self.ext:  # fcos.py:637-647
                out.append({
                    "boxes": det.boxes[i, :k].clone(),
                    "scores": det.scores[i, :k].clone(),
                    "labels": det.labels[i, :k].to(torch.int64),
                    "dxdymags": dxdymags[i, :k].clone(),
                    "contacts": contacts[i, :k].to(torch.int64),
                    "sides": det.sides[i, :k].to(torch.int64),
                })
                continue
            out.append({
                "boxes": det.boxes[i, :k].clone(),
                "scores": det.scores[i, :k].clone(),
                "labels": det.labels[i, :k].to(torch.int64),
                "sides": det.sides[i, :k].to(torch.int64),
                "feature_idx": det.level[i, :k].to(torch.float32),
            })
        return out
