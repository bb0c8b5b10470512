"""The FCOS criterion on the device (csrc/fcos_loss.hip through ops.fcos_loss, FCOS.device_loss / loss_step) against the rule of
tests/fcos_loss_ref.py: the matching bit for bit, the terms inside the derived bound, the same bytes on a second run and image by
image, refusals that launch nothing, and the drop-in's train-mode forward on the engine's own head tensors."""
import numpy as np
import pytest
import torch

import fcos_loss_cases as lc
import fcos_loss_ref as fr

pytestmark = pytest.mark.gpu


def _dev(ts):
    return None if ts is None else [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in ts]


def _targets(gt):
    from hn_amd import ops
    return ops.FcosTargets(*(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in gt))


def _run(a, want_matched=True, out=None):
    from hn_amd import ops
    cls_lr, reg_ctr, ext, strides, c = a[:5]
    return ops.fcos_loss(_dev(cls_lr), _dev(reg_ctr), strides, c, _targets(a[5:]), ext=_dev(ext), want_matched=want_matched, out=out)


def _host(res):
    return dict(matched=None if res.matched is None else res.matched.cpu().numpy(), fg=res.fg.cpu().numpy(),
                terms=res.terms.cpu().numpy(), losses=res.losses.cpu().numpy())


@pytest.mark.parametrize("name", lc.NAMES)
def test_case_against_the_rule(name):
    c = lc.BY_NAME[name]
    got = _host(_run(lc.args(name)))
    detail = {}
    ratio = fr.check(got, lc.reference(name), detail=detail)
    print(f"fcos loss {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    again = _host(_run(lc.args(name)))
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    plain = _host(_run(lc.args(name), want_matched=False))
    assert plain["matched"] is None and all(plain[k].tobytes() == got[k].tobytes() for k in ("terms", "fg", "losses"))
    for i in range(c.n):
        one = _host(_run(lc.image(name, i)))
        assert one["terms"][0].tobytes() == got["terms"][i].tobytes() and one["fg"][0] == got["fg"][i]
        assert one["matched"][0].tobytes() == got["matched"][i].tobytes()
    if name == "nofg":
        assert not got["fg"].any() and not got["terms"][:, 1:3].any()
    if name == "sat":
        assert np.isfinite(got["losses"]).all()


def test_refusals_launch_nothing():
    from hn_amd import ops
    cls_lr, reg_ctr, ext, strides, c = lc.args("edge")[:5]
    gt = lc.args("edge")[5:]
    n, p = 2, lc.points(lc.BY_NAME["edge"])
    out = ops.alloc_fcos_loss(n, p, "cuda", want_matched=True)
    for t in (out.terms, out.losses):
        t.fill_(-7.0)
    out.fg.fill_(-7); out.matched.fill_(-7)

    def untouched():
        torch.cuda.synchronize()
        return bool((out.terms == -7).all() and (out.losses == -7).all() and (out.fg == -7).all() and (out.matched == -7).all())
    wide = lc.pad_targets([(np.zeros((0, 4), fr.F), np.zeros((0,), np.int32), np.zeros((0, 5), fr.F))] * n, g=65)
    with pytest.raises(ValueError, match="G = 65"):
        ops.fcos_loss(_dev(cls_lr), _dev(reg_ctr), strides, c, _targets(wide), ext=_dev(ext), want_matched=True, out=out)
    assert untouched()
    nine = [torch.zeros(t.shape[:3] + (11,), device="cuda") for t in cls_lr]
    with pytest.raises(ValueError, match="num_classes = 9"):
        ops.fcos_loss(nine, _dev(reg_ctr), strides, 9, _targets(gt), ext=_dev(ext), want_matched=True, out=out)
    assert untouched()
    with pytest.raises(ValueError, match="per level"):
        ops.fcos_loss(_dev(cls_lr), _dev(reg_ctr), strides, c, _targets(gt), ext=_dev(ext)[:2], want_matched=True, out=out)
    assert untouched()
    with pytest.raises(TypeError):
        ops.fcos_loss([t.double() for t in _dev(cls_lr)], _dev(reg_ctr), strides, c, _targets(gt), ext=_dev(ext), want_matched=True, out=out)
    t64 = _targets(gt)
    t64.boxes = t64.boxes.double()
    with pytest.raises(TypeError):
        ops.fcos_loss(_dev(cls_lr), _dev(reg_ctr), strides, c, t64, ext=_dev(ext), want_matched=True, out=out)
    assert untouched()
    # ... and the same call with nothing wrong fills it
    ops.fcos_loss(_dev(cls_lr), _dev(reg_ctr), strides, c, _targets(gt), ext=_dev(ext), want_matched=True, out=out)
    assert not untouched()


# fixed boxes on a 480 x 640 frame (resized to 800 x 1067: ratios 1.667): foreground on P3 (sides < 64 px on the canvas),
# P4 (64..128) and P5 (beyond 128)
def _model_targets(ext):
    rows = [(100, 100, 130, 136, 1, (1.0, 0.0, 0.5, 0.06, -0.08)), (300, 200, 360, 270, 2, (3.0, 1.0, 0.2, 0.0, 0.1)),
            (50, 40, 400, 420, 1, (0.0, 1.0, 0.0, 0.0, 0.0)), (420, 300, 470, 330, 0, lc.OBJ)]
    b, l, f = lc._t(rows)
    l = np.minimum(l, 2 if ext else 1)
    return [{"boxes": torch.from_numpy(b), "labels": torch.from_numpy(l.astype(np.int64)), "box_info": torch.from_numpy(f)}]


def _second_image(rgb):
    """480 x 648 (resized to 800 x 1080: another ratio, the same 800 x 1088 canvas, so an image alone has the pair's points) and
    its targets"""
    wide = torch.cat([rgb[0], rgb[0][:, :, :8]], dim=2).contiguous()
    return wide, [{"boxes": torch.tensor([[60.0, 50.0, 200.0, 260.0], [300.0, 100.0, 340.0, 150.0]]), "labels": torch.tensor([1, 0]),
                   "box_info": torch.tensor([[2.0, 1.0, 0.3, 0.1, 0.0], list(lc.OBJ)])}]


@pytest.mark.parametrize("num_classes,ext", [(3, True), (2, False)])
def test_list_of_two_sizes_gives_each_image_alone(num_classes, ext):
    """A list of two images of different sizes gives, for terms and fg, the bytes of each image run alone through the model.
    (The convolutions pick their forms by batch size, so loss_step runs such a list image by image: forward_heads_each.)"""
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model = FCOS(num_classes=num_classes, ext=ext).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    wide, t2 = _second_image(rgb)
    targets = _model_targets(ext)
    with torch.inference_mode():
        _, fg_pair, terms_pair = model.loss_step([rgb[0], wide], targets + t2, want_terms=True)
        rows = [model.loss_step([img], tg, want_terms=True) for img, tg in ((rgb[0], targets), (wide, t2))]
    for i, (_, fg_one, terms_one) in enumerate(rows):
        print(f"  image {i} alone: fg {int(fg_one[0])} terms {terms_one[0].tolist()}; in the pair: fg {int(fg_pair[i])} terms {terms_pair[i].tolist()}")
    for i, (_, fg_one, terms_one) in enumerate(rows):
        assert torch.equal(fg_one[0], fg_pair[i]) and torch.equal(terms_one[0], terms_pair[i])


@pytest.mark.parametrize("num_classes,ext", [(3, True), (2, False)])
def test_model_level(num_classes, ext):
    from fcos_utils.fcos import FCOS
    from hn_amd import ops, synth
    model = FCOS(num_classes=num_classes, ext=ext).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    images, targets = [rgb[0]], _model_targets(ext)
    with torch.inference_mode():
        before = model(images)
        with pytest.raises(NotImplementedError):
            model(images, targets)
        model.train()
        with pytest.raises(NotImplementedError):
            model(images, targets)
        model.device_loss()
        with pytest.raises(ValueError, match="targets should be passed"):
            model(images)
        losses = model(images, targets)
        keys = list(fr.KEYS if ext else fr.KEYS[:4])
        assert list(losses) == keys
        assert all(v.is_cuda and v.dtype == torch.float32 and v.dim() == 0 for v in losses.values())
        # the same bytes as ops.fcos_loss on the engine's own heads, and inside the bound of the rule on those heads
        eng = model.engine()
        cls_lr, reg_ctr, strides, (oh, ow, ph, pw) = eng.forward_heads(torch.stack(images))
        ex = eng._ext_levels if ext else None
        packed = ops.pack_fcos_targets(targets, ops.fcos_target_ratios([(480, 640)], [(oh, ow)]), num_classes=num_classes, ext=ext)
        res = ops.fcos_loss(cls_lr, reg_ctr, strides, num_classes, packed, ext=ex, want_matched=True)
        got = _host(res)
        assert np.array_equal(np.array([float(v) for v in losses.values()], np.float32), got["losses"][:len(keys)])
        host = lambda ts: None if ts is None else [t.cpu().numpy() for t in ts]
        a = (host(cls_lr), host(reg_ctr), host(ex), tuple(strides), num_classes) + tuple(t.cpu().numpy() for t in
                                                                                       (packed.boxes, packed.labels, packed.info, packed.count))
        detail = {}
        fr.check(got, (fr.rule(*a), fr.bound(*a)), detail=detail)
        print(f"fcos loss model C={num_classes} ext={ext}: fg {got['fg']}, |err| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
        lvl = np.searchsorted(np.cumsum([t.shape[1] * t.shape[2] for t in cls_lr]), np.nonzero(got["matched"][0] >= 0)[0], side="right")
        assert set(lvl.tolist()) == {0, 1, 2}, "foreground on all three levels"
        # loss_step: the same bytes in eval mode
        model.eval()
        step, fg = model.loss_step(images, targets)
        assert all(torch.equal(step[k], losses[k]) for k in keys) and torch.equal(fg, res.fg)
        # a list of two images of different sizes: per-image ratios, and each row is the criterion alone on that image's heads
        wide, t2 = _second_image(rgb)
        _, fg_pair, terms_pair = model.loss_step([rgb[0], wide], targets + t2, want_terms=True)
        cls_lr, reg_ctr, strides, (oh, ow, ph, pw) = eng.forward_heads_each([rgb[0], wide])
        ex = eng._ext_levels if ext else None
        for i, (img, tg) in enumerate(((rgb[0], targets), (wide, t2))):
            one = lambda ts: None if ts is None else [t[i:i + 1].contiguous() for t in ts]
            packed = ops.pack_fcos_targets(tg, ops.fcos_target_ratios([tuple(img.shape[-2:])], [(oh[i], ow[i])]), num_classes=num_classes, ext=ext)
            alone = ops.fcos_loss(one(cls_lr), one(reg_ctr), strides, num_classes, packed, ext=one(ex))
            assert torch.equal(alone.fg[0], fg_pair[i]) and torch.equal(alone.terms[0], terms_pair[i])
        assert int(fg_pair[0]) > 0 and int(fg_pair[1]) > 0
        # ... and inference is untouched
        after = model(images)
        assert all(torch.equal(after[0][k], before[0][k]) for k in before[0])
        with pytest.raises(NotImplementedError):
            model(images, targets)
