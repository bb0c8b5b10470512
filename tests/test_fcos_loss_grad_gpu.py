"""hn_fcos_loss_grad_f32 (the FCOS criterion's backward at the detector heads, one launch after the forward's two) against the
float64 rule (tests/fcos_loss_grad_ref.py) on every case of tests/fcos_loss_cases.py plus g3 and both upstream settings, its
forward outputs against ops.fcos_loss's bytes, FCOSCriterion under torch's autograd, and head_grads of the drop-in module.  The
assertion is |err| <= the derived worst-case bound and nothing tighter; the ratios are printed and DESIGN.md section 9s holds the
table measured on the MI355X."""
import numpy as np
import pytest
import torch

import fcos_loss_cases as lc
import fcos_loss_grad_cases as gc
import fcos_loss_grad_ref as gr
import fcos_loss_ref as fr
from test_fcos_loss_gpu import _model_targets, _second_image

pytestmark = pytest.mark.gpu

IDS = [gc.case_id(c) for c in gc.CASES]


def _dev(ts):
    return None if ts is None else [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in ts]


def _targets(gt):
    from hn_amd import ops
    return ops.FcosTargets(*(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in gt))


def _upstream(u):
    up = gc.UPSTREAMS[u]
    return None if up is None else torch.tensor(up, dtype=torch.float32).cuda()


def _run(name, upstream=None, **kw):
    from hn_amd import ops
    cls_lr, reg_ctr, ext, strides, c = gc.args(name)[:5]
    return ops.fcos_loss_grad(_dev(cls_lr), _dev(reg_ctr), strides, c, _targets(gc.args(name)[5:]), ext=_dev(ext), upstream=upstream, **kw)


def _host(grads):
    """per-level lists -> the rule's flat arrays"""
    d_cls, d_reg, d_ext = ([t.cpu().numpy() for t in g] if g is not None else None for g in grads[:3])
    cls, reg, ex, _ = fr.flatten(d_cls, d_reg, d_ext)
    return dict(d_cls=cls, d_reg=reg, d_ext=ex)


def _same(a, b):
    return all((x is None and y is None) or all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_gradients_are_inside_the_bound_and_the_forward_is_the_loss_entrys(case):
    from hn_amd import ops
    name, u = case
    grads = _run(name, _upstream(u))
    a = gc.args(name)
    assert len(grads) == 3 and (grads[2] is None) == (a[2] is None)
    for g, heads in zip(grads, a[:3]):
        assert g is None or all(t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == h.shape for t, h in zip(g, heads))
    got = _host(grads)
    detail = {}
    ratio = gr.check(got, gr.reference(case), detail=detail)
    print(f"fcos loss grad gpu {gc.case_id(case)}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    # a second run, with the forward: the same gradient bytes, and ops.fcos_loss's bytes
    again = _run(name, _upstream(u), want_forward=True)
    assert len(again) == 4 and _same(again, grads)
    cls_lr, reg_ctr, ext, strides, c = a[:5]
    want = ops.fcos_loss(_dev(cls_lr), _dev(reg_ctr), strides, c, _targets(a[5:]), ext=_dev(ext))
    assert torch.equal(again[3].terms, want.terms) and torch.equal(again[3].fg, want.fg) and torch.equal(again[3].losses, want.losses)
    if u == 0:   # upstream = None is six ones
        assert _same(_run(name, torch.ones((6,), device="cuda")), grads)
    if name == "nofg":
        assert not got["d_reg"].any() and int(want.fg.sum()) == 0
        # the divisor is 1: the background focal gradient of one element is its derivative itself
        x = np.float64(a[0][0][0, 0, 0, 0])
        w0 = 1.0 if u == 0 else gc.UPSTREAMS[1][0]
        assert abs(got["d_cls"][0, 0, 0] - w0 * gr._focal_grad(np.array([[x]]), np.array([-1]))[0, 0]) <= gr.reference(case)[1]["d_cls"][0, 0, 0]
    if name == "sat":
        assert all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("name", ["edge", "chunks-ext", "g3"])
def test_a_unit_upstream_leaves_the_other_terms_elements_at_zero(name):
    """upstream = e_k: every gradient element the k-th term does not touch is exactly zero"""
    a = gc.args(name)
    c = a[4]
    fg = fr.rule(*a)["matched"] >= 0
    got = [_host(_run(name, torch.eye(6, device="cuda")[k].contiguous())) for k in range(6)]
    zero = lambda t: not t.any()                                           # noqa: E731
    e0, e1, e2, e3, e4, e5 = got
    assert e0["d_cls"][..., :c].all() and zero(e0["d_cls"][..., c:]) and zero(e0["d_reg"]) and zero(e0["d_ext"])
    assert zero(e1["d_cls"]) and zero(e1["d_reg"][..., 4]) and zero(e1["d_reg"][~fg]) and zero(e1["d_ext"]) and e1["d_reg"][fg][:, :4].any()
    assert zero(e2["d_cls"]) and zero(e2["d_reg"][..., :4]) and zero(e2["d_reg"][~fg]) and zero(e2["d_ext"]) and e2["d_reg"][fg][:, 4].all()
    assert zero(e3["d_cls"][..., :c]) and e3["d_cls"][..., c:].all() and zero(e3["d_reg"]) and zero(e3["d_ext"])
    assert zero(e4["d_cls"]) and zero(e4["d_reg"]) and zero(e4["d_ext"][..., :3]) and e4["d_ext"][..., 3:].all()
    assert zero(e5["d_cls"]) and zero(e5["d_reg"]) and zero(e5["d_ext"][..., 3:]) and e5["d_ext"][..., 0].any()


def test_refusals_leave_prefilled_outputs_untouched():
    from hn_amd import ops
    a = gc.args("edge")
    cls_lr, reg_ctr, ext, strides, c = a[:5]
    gt = a[5:]
    out = tuple([torch.full(t.shape, -7.0, device="cuda") for t in h] for h in (cls_lr, reg_ctr, ext))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for o in out for t in o)
    call = lambda **kw: ops.fcos_loss_grad(**dict(dict(cls_lr=_dev(cls_lr), reg_ctr=_dev(reg_ctr), strides=strides, num_classes=c,     # noqa: E731
                                                       targets=_targets(gt), ext=_dev(ext), out=out), **kw))
    wide = lc.pad_targets([(np.zeros((0, 4), fr.F), np.zeros((0,), np.int32), np.zeros((0, 5), fr.F))] * 2, g=65)
    with pytest.raises(ValueError, match="G = 65"):
        call(targets=_targets(wide))
    with pytest.raises(ValueError, match="num_classes = 9"):
        call(num_classes=9)
    with pytest.raises(ValueError, match="per level"):
        call(ext=_dev(ext)[:2])
    with pytest.raises(TypeError):
        call(cls_lr=[t.double() for t in _dev(cls_lr)])
    with pytest.raises(ValueError, match="upstream"):
        call(upstream=torch.ones((5,), device="cuda"))
    with pytest.raises(TypeError):
        call(upstream=torch.ones((6,), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="out must"):
        call(out=(out[0], out[1], None))
    with pytest.raises(ValueError, match="out must"):
        call(out=(out[0], out[1][:2], out[2]))
    with pytest.raises(ValueError, match="contiguous"):
        call(reg_ctr=[t.transpose(1, 2) for t in _dev([np.ascontiguousarray(t.transpose(0, 2, 1, 3)) for t in reg_ctr])])
    assert untouched()
    # ... and the same call with nothing wrong fills them, with the bytes of a call that allocates
    res = call()
    assert res[0] is out[0] and not untouched() and _same(res, _run("edge"))


def test_criterion_under_autograd():
    """FCOSCriterion on leaf level tensors: sum(losses).backward() leaves the bytes of ops.fcos_loss_grad(upstream=None) in .grad;
    a weighted sum those of that upstream; the loss values are ops.fcos_loss's bytes; a relu before the heads receives a masked
    gradient; a second backward raises; a layout other than contiguous fp32 raises ValueError."""
    from hn_amd import ops
    from hn_amd.criterion import FCOSCriterion
    name = "g3"
    a = gc.args(name)
    cls_lr, reg_ctr, ext, strides, c = a[:5]
    targets = _targets(a[5:])
    crit = FCOSCriterion(c, strides, ext=True)

    def leaves():
        return [[t.requires_grad_(True) for t in _dev(h)] for h in (cls_lr, reg_ctr, ext)]
    heads = leaves()
    losses, fg = crit(heads[0], heads[1], targets, ext=heads[2])
    want = ops.fcos_loss(_dev(cls_lr), _dev(reg_ctr), strides, c, targets, ext=_dev(ext))
    assert list(losses) == list(ops.FCOS_LOSS_KEYS) and torch.equal(fg, want.fg) and not fg.requires_grad
    assert all(v.is_cuda and v.dtype == torch.float32 and v.dim() == 0 for v in losses.values())
    assert all(torch.equal(losses[k].detach(), want.losses[i]) for i, k in enumerate(ops.FCOS_LOSS_KEYS))
    total = sum(losses.values())
    total.backward()
    plain = _run(name)
    assert all(torch.equal(t.grad, w) for h, g in zip(heads, plain) for t, w in zip(h, g))
    with pytest.raises(RuntimeError):
        total.backward()
    heads = leaves()
    losses, _ = crit(heads[0], heads[1], targets, ext=heads[2])
    w = gc.UPSTREAMS[1]
    sum(wk * losses[k] for wk, k in zip(w, ops.FCOS_LOSS_KEYS) if wk != 0).backward()     # the third value takes no part: weight 0
    weighted = _run(name, _upstream(1))
    assert all(torch.equal(t.grad, g) for h, gs in zip(heads, weighted) for t, g in zip(h, gs))
    gr.check(_host([[t.grad for t in h] for h in heads]), gr.reference((name, 1)))
    # a relu in front of the regressions: its input's gradient is the head's, masked where the input was not positive
    pre = [(t.detach() - 0.5).requires_grad_(True) for t in _dev(reg_ctr)]
    act = [torch.cat([torch.relu(p[..., :4]), p[..., 4:]], dim=3) for p in pre]
    losses, _ = crit(_dev(cls_lr), act, targets, ext=_dev(ext))
    sum(losses.values()).backward()
    at_heads = ops.fcos_loss_grad(_dev(cls_lr), [t.detach() for t in act], strides, c, targets, ext=_dev(ext))[1]
    for p, g in zip(pre, at_heads):
        mask = torch.cat([(p[..., :4] > 0).float(), torch.ones_like(p[..., 4:])], dim=3)
        assert torch.equal(p.grad, g * mask)
    assert any(bool(((p[..., :4] <= 0) & (g[..., :4] != 0)).any()) for p, g in zip(pre, at_heads))
    # without ext: four keys, and the weights beyond them are ignored
    a2 = gc.args("golden-2")
    crit2 = FCOSCriterion(a2[4], a2[3])
    h2 = [[t.requires_grad_(True) for t in _dev(h)] for h in a2[:2]]
    losses, _ = crit2(h2[0], h2[1], _targets(a2[5:]))
    assert list(losses) == list(ops.FCOS_LOSS_KEYS[:4])
    sum(losses.values()).backward()
    assert all(torch.equal(t.grad, g) for h, gs in zip(h2, _run("golden-2")[:2]) for t, g in zip(h, gs))
    with pytest.raises(ValueError):
        crit2([t.detach().double() for t in h2[0]], [t.detach() for t in h2[1]], _targets(a2[5:]))
    with pytest.raises(ValueError):
        crit2([t.detach().transpose(1, 2) for t in h2[0]], [t.detach() for t in h2[1]], _targets(a2[5:]))
    with pytest.raises(ValueError):
        crit2([t.detach() for t in h2[0]], [t.detach() for t in h2[1]], a2[5:])


@pytest.mark.parametrize("num_classes,ext", [(3, True), (2, False)])
def test_model_head_grads(num_classes, ext):
    """FCOS.head_grads on synthetic weights, one 480 x 640 frame: losses and fg are loss_step's bytes, the gradients the bytes of
    ops.fcos_loss_grad on the engine's own head tensors and inside the bound of the rule on those heads; a list of two sizes
    takes loss_step's image-by-image path; inference is untouched and targets without the opt-in keep raising."""
    from fcos_utils.fcos import FCOS
    from hn_amd import ops, synth
    model = FCOS(num_classes=num_classes, ext=ext).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    images, targets = [rgb[0]], _model_targets(ext)
    keys = list(fr.KEYS if ext else fr.KEYS[:4])
    with torch.inference_mode():
        before = model(images)
        want_losses, want_fg = model.loss_step(images, targets)
        losses, fg, grads = model.head_grads(images, targets)
        assert list(losses) == keys and all(torch.equal(losses[k], want_losses[k]) for k in keys) and torch.equal(fg, want_fg)
        eng = model.engine()
        cls_lr, reg_ctr, strides, (oh, ow, _, _) = eng.forward_heads(torch.stack(images))
        ex = eng._ext_levels if ext else None
        packed = ops.pack_fcos_targets(targets, ops.fcos_target_ratios([(480, 640)], [(oh, ow)]), num_classes=num_classes, ext=ext)
        want = ops.fcos_loss_grad(cls_lr, reg_ctr, strides, num_classes, packed, ext=ex)
        assert len(grads) == 3 and (grads[2] is None) == (not ext) and _same(grads, want)
        e_losses, e_fg, e_grads = eng.head_grads(torch.stack(images), packed)
        assert all(torch.equal(e_losses[k], want_losses[k]) for k in keys) and torch.equal(e_fg, want_fg) and _same(e_grads, want)
        host = lambda ts: None if ts is None else [t.cpu().numpy() for t in ts]             # noqa: E731
        a = (host(cls_lr), host(reg_ctr), host(ex), tuple(strides), num_classes) + tuple(t.cpu().numpy() for t in
                                                                                       (packed.boxes, packed.labels, packed.info, packed.count))
        detail = {}
        gr.check(_host(grads), (gr.rule(*a), gr.bound(*a)), detail=detail)
        print(f"fcos loss grad gpu model C={num_classes} ext={ext}: fg {fg.tolist()}, |err| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
        # a list of two sizes: per-image ratios, the network image by image, one criterion call on the common canvas
        wide, t2 = _second_image(rgb)
        step, fg_pair = model.loss_step([rgb[0], wide], targets + t2)
        m_losses, m_fg, m_grads = model.head_grads([rgb[0], wide], targets + t2)
        assert all(torch.equal(m_losses[k], step[k]) for k in keys) and torch.equal(m_fg, fg_pair)
        cls_lr, reg_ctr, strides, (oh, ow, _, _) = eng.forward_heads_each([rgb[0], wide])
        ex = eng._ext_levels if ext else None
        packed = ops.pack_fcos_targets(targets + t2, ops.fcos_target_ratios([(480, 640), (480, 648)], list(zip(oh, ow))),
                                       num_classes=num_classes, ext=ext)
        assert _same(m_grads, ops.fcos_loss_grad(cls_lr, reg_ctr, strides, num_classes, packed, ext=ex))
        assert all(t.shape[0] == 2 for t in m_grads[0])
        after = model(images)
        assert all(torch.equal(after[0][k], before[0][k]) for k in before[0])
        with pytest.raises(NotImplementedError):
            model(images, targets)
        with pytest.raises(NotImplementedError):
            model.train()(images, targets)
