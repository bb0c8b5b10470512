"""hn_conv3x3_thin_backward_f32 (the output convolutions' weight, bias and input gradients: a sweep and a fixed-order reduction)
against the float64 rule of tests/thin_bwd_ref.py on every case of tests/thin_bwd_cases.py, ThinConv3x3Levels under torch's
autograd, and output_grads / refresh_outputs of the drop-in detector.  The assertion is |err| <= the derived worst-case bound and
nothing tighter (planted cases: bit for bit); the ratios are printed and DESIGN.md section 9t holds the table measured on the
MI355X."""
import numpy as np
import pytest
import torch

import fcos_loss_cases as lc
import fcos_loss_ref as fr
import thin_bwd_cases as tc
import thin_bwd_ref as tr
from test_fcos_loss_gpu import _model_targets, _second_image

pytestmark = pytest.mark.gpu


def _cuda(t):
    return torch.from_numpy(np.array(t)).cuda()   # (a copy: the cases' arrays are read-only)


class _W:
    """what ops.conv3x3_thin_backward_levels reads of a filter bank"""

    def __init__(self, w):
        self.w = w if torch.is_tensor(w) else _cuda(w)


def _inputs(name):
    """the case on the device: S32 maps (a channel slice of a wider map where the case says so) and the members"""
    c = tc.args(name)
    a16 = []
    for hi, lo in zip(c["hi"], c["lo"]):
        t = _cuda(tr.pack_s32(hi, lo))
        if c["blocks"]:
            first, total = c["blocks"]
            wide = torch.full(tuple(t.shape[:3]) + (total, 2, 32), float("nan"), device="cuda", dtype=torch.float16)
            wide[:, :, :, first:first + t.shape[3]] = t
            t = wide[:, :, :, first:first + t.shape[3]]
        a16.append(t)
    members = [(_W(w), relu, [_cuda(y) for y in ys], [_cuda(g) for g in gs]) for w, relu, ys, gs in c["members"]]
    return c, a16, members


def _dx_out(c, fill):
    if not c["dx"]:
        return None, 0
    width, off = c["dx"]
    return [torch.full(a.shape[:3] + (width,), fill, device="cuda", dtype=torch.float32) for a in c["a"]], off


def _run(name, fill=float("nan"), **kw):
    from hn_amd import ops
    c, a16, members = _inputs(name)
    dx_out, off = _dx_out(c, fill)
    res, d_a = ops.conv3x3_thin_backward_levels(a16, members, dx_out=dx_out, dx_channel_offset=off, **kw)
    return c, res, d_a, dx_out


def _host(c, res, d_a):
    got = {}
    for m, (d_w, d_b) in enumerate(res):
        got[f"dW{m}"], got[f"db{m}"] = d_w.cpu().numpy(), d_b.cpu().numpy()
    off = c["dx"][1] if c["dx"] else 0
    for l, t in enumerate(d_a):
        got[f"dA{l}"] = np.ascontiguousarray(t.cpu().numpy()[..., off:off + c["cin"]])
    return got


@pytest.mark.parametrize("name", tc.NAMES)
def test_every_case_is_inside_the_bound_and_a_second_run_gives_the_same_bytes(name):
    c, res, d_a, dx_out = _run(name)
    assert all(d_w.is_cuda and d_w.dtype == torch.float32 and tuple(d_w.shape) == m[0].shape and tuple(d_b.shape) == m[0].shape[:1]
               for (d_w, d_b), m in zip(res, c["members"]))
    got = _host(c, res, d_a)
    detail = {}
    ratio = tr.check(got, tc.reference(name), detail=detail)
    print(f"thin bwd gpu {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    if c["planted"]:
        want = tc.reference(name)[0]
        for key in want:
            assert np.array_equal(got[key], want[key].astype(np.float32)), key
    if c["dx"]:   # the other half of the wide tensor is left alone (NaN prefill), this half is written everywhere
        width, off = c["dx"]
        for t in dx_out:
            rest = torch.cat([t[..., :off], t[..., off + c["cin"]:]], dim=3)
            assert bool(torch.isnan(rest).all()) and not bool(torch.isnan(t[..., off:off + c["cin"]]).any())
    _, res2, d_a2, _ = _run(name)
    again = _host(c, res2, d_a2)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    # without the input gradient: the same dW and db
    _, res3, none, _ = _run(name, want_dx=False)
    assert none is None and all(torch.equal(a, b) for r3, r in zip(res3, res) for a, b in zip(r3, r))


def test_zero_gradients_overwrite_a_nan_prefill():
    """g all zero: every output element comes back zero -- dA in a caller's NaN-filled tensor, dW and db in blocks of the
    allocator that held NaN just before"""
    from hn_amd import ops
    c, a16, members = _inputs("gzero")
    dx_out = [torch.full(a.shape, float("nan"), device="cuda", dtype=torch.float32) for a in c["a"]]
    stale = [torch.full(m[0].w.shape, float("nan"), device="cuda") for m in members] + \
            [torch.full((m[0].w.shape[0],), float("nan"), device="cuda") for m in members]
    torch.cuda.synchronize()
    del stale
    res, d_a = ops.conv3x3_thin_backward_levels(a16, members, dx_out=dx_out)
    assert all(x is y for x, y in zip(d_a, dx_out))
    for t in list(d_a) + [t for r in res for t in r]:
        assert not bool(t.any()) and not bool(torch.isnan(t).any())


def test_refusals_leave_prefilled_outputs_untouched():
    from hn_amd import _lib, ops
    import ctypes as C
    c, a16, members = _inputs("three")
    dx_out = [torch.full(a.shape, -7.0, device="cuda", dtype=torch.float32) for a in c["a"]]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in dx_out)
    call = lambda a=a16, ms=members, **kw: ops.conv3x3_thin_backward_levels(a, ms, **dict(dict(dx_out=dx_out), **kw))   # noqa: E731
    big = (_W(np.zeros((17, 3, 3, 32), np.float32)), 0, [torch.zeros(t.shape[:3] + (17,), device="cuda") for t in a16],
           [torch.zeros(t.shape[:3] + (17,), device="cuda") for t in a16])
    with pytest.raises(ValueError, match="<= 16 output channels"):
        call(ms=[big])                                                              # Cout > 16
    with pytest.raises(ValueError, match="one or two members"):
        call(ms=members + members[:1])                                              # three members on a map
    with pytest.raises(ValueError, match="one or two members"):
        call(ms=[])
    wide = lambda cout: (_W(np.zeros((cout, 3, 3, 32), np.float32)), 0, [torch.zeros(t.shape[:3] + (cout,), device="cuda") for t in a16],  # noqa: E731
                         [torch.zeros(t.shape[:3] + (cout,), device="cuda") for t in a16])
    with pytest.raises(RuntimeError, match="columns together"):
        call(ms=[wide(16), wide(1)])                                                # more than 16 columns on a map
    with pytest.raises(ValueError, match="S32 tensors of one"):
        call(ms=[(_W(np.zeros((5, 3, 3, 48), np.float32)),) + members[0][1:]])      # Cin not a multiple of 32: no such S32 map
    with pytest.raises(TypeError):
        call(a=[t[..., :16] for t in a16])                                          # not an S32 map
    with pytest.raises(ValueError, match="per level"):
        call(ms=[(members[0][0], members[0][1], members[0][2][:2], members[0][3])])    # a missing level
    with pytest.raises(TypeError):
        call(ms=[(members[0][0], members[0][1], [t.double() for t in members[0][2]], members[0][3])])
    with pytest.raises(ValueError):
        call(ms=[(members[0][0], 6, members[0][2], members[0][3])])                 # relu_cols > Cout
    with pytest.raises(ValueError, match="dx_out"):
        call(dx_out=dx_out[:2])
    with pytest.raises(ValueError, match="dx_channel_offset"):
        call(dx_channel_offset=32)
    # the C entry's own refusals, with a workspace one byte short and with a null level
    lib = _lib.load()
    nl = len(a16)
    lv = ops._thin_levels_of(a16, inputs=True)
    for l, t in enumerate(dx_out):
        lv.y[l] = t.data_ptr()
    couts, relus = (C.c_int32 * 2)(5, 8), (C.c_int32 * 2)(4, 3)
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])                # noqa: E731
    wp = arr([m[0].w for m in members])
    yp, gp = arr([t for m in members for t in m[2]]), arr([t for m in members for t in m[3]])
    d_w = [torch.full(m[0].w.shape, -7.0, device="cuda") for m in members]
    d_b = [torch.full((m[0].w.shape[0],), -7.0, device="cuda") for m in members]
    need = lib.hn_conv3x3_thin_backward_ws_bytes(C.byref(lv), c["n"], 32, 2, couts)
    units, _, _ = tr.plan(c["sizes"], c["n"])
    assert need == 4 * (units * 9 * 13 * 256 + units * 13)
    ws = torch.empty((need // 4,), device="cuda")
    go = lambda lv_, nbytes, cin=32: lib.hn_conv3x3_thin_backward_f32(C.byref(lv_), c["n"], cin, 0, 2, couts, relus, wp, yp, gp,   # noqa: E731
                                                                      arr(d_w), arr(d_b), 0, 0, ws.data_ptr(), nbytes, None)
    assert go(lv, need - 1) != 0 and b"workspace" in lib.hn_last_error()
    assert go(lv, need, cin=48) != 0
    assert lib.hn_conv3x3_thin_backward_ws_bytes(C.byref(lv), c["n"], 48, 2, couts) == -1
    null = ops._thin_levels_of(a16, inputs=True)
    for l, t in enumerate(dx_out):
        null.y[l] = t.data_ptr()
    null.x16[1] = None
    assert go(null, need) != 0 and b"null" in lib.hn_last_error()
    assert untouched() and all(bool((t == -7).all()) for t in d_w + d_b)
    # ... and the same call with nothing wrong fills them, with the bytes of a call that allocates
    torch.cuda.synchronize()
    assert go(lv, need) == 0
    res, d_a = ops.conv3x3_thin_backward_levels(a16, members)
    assert not untouched()
    assert all(torch.equal(a, b) for a, b in zip(d_w + d_b + dx_out, [r[0] for r in res] + [r[1] for r in res] + d_a))
    assert nl == 3


def _module_case(name="three"):
    """a ThinConv3x3Levels with member 0's weights, and the case's a as its fp32 inputs"""
    from hn_amd.autograd import ThinConv3x3Levels
    c = tc.args(name)
    w, relu, _, gs = c["members"][0]
    conv = ThinConv3x3Levels(c["cin"], w.shape[0], relu_cols=relu).cuda()
    with torch.no_grad():
        conv.weight.copy_(_cuda(w).permute(0, 3, 1, 2))
        conv.bias.copy_(torch.linspace(-0.2, 0.2, w.shape[0]))
    xs = [_cuda(a).requires_grad_(True) for a in c["a"]]
    return c, conv, xs, [_cuda(g) for g in gs]


def test_module_under_autograd():
    """.grad of weight, bias and inputs: the bytes of a direct ops call on the module's own split maps and outputs, inside the
    bound of the rule on them; layouts other than contiguous fp32 on the device raise ValueError"""
    from hn_amd import ops
    from hn_amd.autograd import ThinConv3x3Levels
    c, conv, xs, gs = _module_case()
    ys = conv(xs)
    assert len(ys) == len(xs) and all(y.requires_grad and tuple(y.shape) == tuple(x.shape[:3]) + (conv.cout,) for y, x in zip(ys, xs))
    total = sum((y * g).sum() for y, g in zip(ys, gs))
    total.backward()
    a16 = [ops.to_split(x.detach()) for x in xs]
    w = conv.weight.detach().permute(0, 2, 3, 1).contiguous()
    [(d_w, d_b)], d_a = ops.conv3x3_thin_backward_levels(a16, [(_W(w), conv.relu_cols, [y.detach() for y in ys], gs)])
    assert torch.equal(conv.weight.grad, d_w.permute(0, 3, 1, 2)) and torch.equal(conv.bias.grad, d_b)
    assert all(torch.equal(x.grad, d) for x, d in zip(xs, d_a))
    a_val = [ops.from_split(t).cpu().numpy() for t in a16]
    members = [(w.cpu().numpy(), conv.relu_cols, [y.detach().cpu().numpy() for y in ys], [g.cpu().numpy() for g in gs])]
    got = {"dW0": d_w.cpu().numpy(), "db0": d_b.cpu().numpy(), **{f"dA{l}": t.cpu().numpy() for l, t in enumerate(d_a)}}
    ratio = tr.check(got, (tr.rule(a_val, members), tr.bound(a_val, members)))
    print(f"thin bwd gpu module: max |err| / bound = {ratio:.4f}")
    with pytest.raises(RuntimeError):
        total.backward()
    # the packed bank is cached on the weight's version: the same object between two steps, a new one after a write, and the
    # outputs after the write are those of a module that never cached
    bank = conv._bank()
    conv([x.detach() for x in xs])
    assert conv._bank() is bank
    with torch.no_grad():
        conv.weight.mul_(0.5)
        conv.bias.add_(0.125)
    assert conv._bank() is not bank
    other = ThinConv3x3Levels(conv.cin, conv.cout, relu_cols=conv.relu_cols).cuda()
    other.load_state_dict(conv.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(conv([x.detach() for x in xs]), other([x.detach() for x in xs])))
    # a level that takes no part gets a zero gradient; an input that does not ask gets none
    c, conv, xs, gs = _module_case()
    xs[1].requires_grad_(False)
    ys = conv(xs)
    (ys[0] * gs[0]).sum().backward()
    assert xs[1].grad is None and not bool(xs[2].grad.any()) and bool(xs[0].grad.any()) and bool(conv.weight.grad.any())
    for bad in ([x.detach().cpu() for x in xs], [x.detach().double() for x in xs],
                [x.detach().transpose(1, 2) for x in xs], [x.detach()[..., :16] for x in xs], xs[0]):
        with pytest.raises(ValueError):
            conv(bad)
    with pytest.raises(ValueError):
        ThinConv3x3Levels(48, 5)
    with pytest.raises(ValueError):
        ThinConv3x3Levels(32, 17)


def test_module_composes_with_the_criterion():
    """torch towers -> ThinConv3x3Levels heads -> FCOSCriterion -> backward, on case "edge" of tests/fcos_loss_cases.py: every
    head parameter and every level input receives a finite gradient: the heads' the bytes of the direct calls, the inputs' the
    sum of the three banks' direct input gradients"""
    from hn_amd import ops
    from hn_amd.autograd import ThinConv3x3Levels
    from hn_amd.criterion import FCOSCriterion
    cls_lr, reg_ctr, ext, strides, num_classes, gt_boxes, gt_labels, gt_info, gt_count = lc.args("edge")
    targets = ops.FcosTargets(*(_cuda(t) for t in (gt_boxes, gt_labels, gt_info, gt_count)))
    torch.manual_seed(3)
    n = cls_lr[0].shape[0]
    feats = [(torch.randn((n,) + t.shape[1:3] + (32,), device="cuda") * 0.5).requires_grad_(True) for t in cls_lr]
    heads = [ThinConv3x3Levels(32, num_classes + 2).cuda(), ThinConv3x3Levels(32, 5, relu_cols=4).cuda(),
             ThinConv3x3Levels(32, 8, relu_cols=3).cuda()]
    crit = FCOSCriterion(num_classes, strides, ext=ext is not None)
    outs = [h(feats) for h in heads[:3 if ext is not None else 2]]
    losses, fg = crit(outs[0], outs[1], targets, ext=outs[2] if ext is not None else None)
    sum(losses.values()).backward()
    for h in heads[:len(outs)]:
        assert bool(torch.isfinite(h.weight.grad).all()) and bool(h.weight.grad.any()) and bool(torch.isfinite(h.bias.grad).all())
    assert all(bool(torch.isfinite(f.grad).all()) and bool(f.grad.any()) for f in feats)
    # the same numbers from the direct calls: the criterion's gradients at the heads, then one backward call per bank, summed
    d = ops.fcos_loss_grad([t.detach() for t in outs[0]], [t.detach() for t in outs[1]], strides, num_classes, targets,
                           ext=[t.detach() for t in outs[2]] if ext is not None else None)
    a16 = [ops.to_split(f.detach()) for f in feats]
    parts = []
    for h, ys, gs in zip(heads, outs, d):
        bank = _W(h.weight.detach().permute(0, 2, 3, 1).contiguous())
        [(d_w, d_b)], d_a = ops.conv3x3_thin_backward_levels(a16, [(bank, h.relu_cols, [y.detach() for y in ys], gs)])
        assert torch.equal(h.weight.grad, d_w.permute(0, 3, 1, 2)) and torch.equal(h.bias.grad, d_b)
        parts.append(d_a)
    # autograd adds the three banks' input gradients in an order of its own: two fp32 additions, so within gamma(2) of the sum
    # of the magnitudes around the exact sum
    for l, f in enumerate(feats):
        exact = sum(p[l].double() for p in parts)
        mag = sum(p[l].double().abs() for p in parts)
        assert bool(((f.grad.double() - exact).abs() <= tr.gamma(2) * mag).all())


_BANKS = {"cls_out": ("head.classification_head.cls_logits", "head.classification_head.hand_lr_layer"),
          "reg_out": ("head.regression_head.bbox_reg", "head.regression_head.bbox_ctrness"),
          "ext_out": ("head.classification_head.hand_dydx_layer", "head.classification_head.hand_contact_state_layer")}


@pytest.mark.parametrize("num_classes,ext", [(3, True), (2, False)])
def test_model_output_grads(num_classes, ext):
    """FCOS.output_grads on synthetic weights, one 480 x 640 frame: losses, fg and the head gradients are head_grads' bytes, the
    parameter gradients the un-concatenated, permuted bytes of the engine call, which is inside the bound of the rule on the
    engine's own a, y and g; a list of two sizes takes the image-by-image path; inference is untouched."""
    from fcos_utils.fcos import FCOS
    from hn_amd import ops, synth
    model = FCOS(num_classes=num_classes, ext=ext).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    images, targets = [rgb[0]], _model_targets(ext)
    keys = list(fr.KEYS if ext else fr.KEYS[:4])
    with torch.inference_mode():
        before = model(images)
        want_losses, want_fg, want_grads = model.head_grads(images, targets)
        losses, fg, grads = model.output_grads(images, targets)
        assert list(losses) == keys and all(torch.equal(losses[k], want_losses[k]) for k in keys) and torch.equal(fg, want_fg)
        eng = model.engine()
        oh, ow, _, _ = eng.geometry(480, 640)
        packed = ops.pack_fcos_targets(targets, ops.fcos_target_ratios([(480, 640)], [(oh, ow)]), num_classes=num_classes, ext=ext)
        e_losses, e_fg, e_grads, param_grads, d_towers, inp = eng.output_grads(torch.stack(images), packed, want_inputs=True)
        assert all(torch.equal(e_losses[k], want_losses[k]) for k in keys) and torch.equal(e_fg, want_fg)
        for a, b in zip(e_grads, want_grads):
            assert (a is None and b is None) or all(torch.equal(s, t) for s, t in zip(a, b))
        banks = [b for b in _BANKS if ext or b != "ext_out"]
        assert sorted(param_grads) == sorted(banks) and len(grads) == 4 * len(banks)
        for bank in banks:
            d_w, d_b = param_grads[bank]
            row = 0
            for name in _BANKS[bank]:
                cout = model.state_dict()[name + ".weight"].shape[0]
                assert tuple(grads[name + ".weight"].shape) == (cout, 256, 3, 3)
                assert torch.equal(grads[name + ".weight"], d_w[row:row + cout].permute(0, 3, 1, 2))
                assert torch.equal(grads[name + ".bias"], d_b[row:row + cout])
                row += cout
            assert row == d_w.shape[0]
        assert all(tuple(t.shape) == tuple(c.shape[:3]) + (512,) for t, c in zip(d_towers, inp["cls_lr"]))
        # the engine call against the rule on its own tensors, map by map
        host = lambda ts: [t.cpu().numpy() for t in ts]                                     # noqa: E731
        for kind, bank_names, off in (("a_cls", ["cls_out"] + (["ext_out"] if ext else []), 0), ("a_reg", ["reg_out"], 256)):
            a_val = host([ops.from_split(t) for t in inp[kind]])
            members, got = [], {}
            for m, bank in enumerate(bank_names):
                cw, relu, ys, gs = {"cls_out": (eng.cls_out, 0, inp["cls_lr"], e_grads[0]), "reg_out": (eng.reg_out, 4, inp["reg_ctr"], e_grads[1]),
                                    "ext_out": (eng.ext_out, 3, inp["ext"], e_grads[2])}[bank]
                members.append((cw.w.cpu().numpy(), relu, host(ys), host(gs)))
                got[f"dW{m}"], got[f"db{m}"] = (t.cpu().numpy() for t in param_grads[bank])
            for l, t in enumerate(d_towers):
                got[f"dA{l}"] = np.ascontiguousarray(t[..., off:off + 256].cpu().numpy())
            detail = {}
            tr.check(got, (tr.rule(a_val, members), tr.bound(a_val, members)), detail=detail)
            print(f"thin bwd gpu model C={num_classes} ext={ext} {kind}: |err| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
        # a list of two sizes: the image-by-image path, N = 2 tower gradients
        wide, t2 = _second_image(rgb)
        h_losses, h_fg, h_grads = model.head_grads([rgb[0], wide], targets + t2)
        m_losses, m_fg, m_grads = model.output_grads([rgb[0], wide], targets + t2)
        assert all(torch.equal(m_losses[k], h_losses[k]) for k in keys) and torch.equal(m_fg, h_fg)
        oh2, ow2 = zip(*[g[2:] for g in eng.list_geometry([rgb[0], wide])[0]])
        packed2 = ops.pack_fcos_targets(targets + t2, ops.fcos_target_ratios([(480, 640), (480, 648)], list(zip(oh2, ow2))),
                                        num_classes=num_classes, ext=ext)
        out2 = eng.output_grads([rgb[0], wide], packed2)
        assert all(t.shape[0] == 2 and t.shape[3] == 512 for t in out2[4])
        for a, b in zip(out2[2], h_grads):
            assert (a is None and b is None) or all(torch.equal(s, t) for s, t in zip(a, b))
        assert all(bool(torch.isfinite(v).all()) for v in m_grads.values())
        after = model(images)
        assert all(torch.equal(after[0][k], before[0][k]) for k in before[0])
        with pytest.raises(NotImplementedError):
            model(images, targets)
        with pytest.raises(NotImplementedError):
            model.train()(images, targets)


def test_refresh_outputs():
    """a step on the output layers' parameters, then refresh_outputs(): forward_heads gives the bytes of a fresh FCOS that loaded
    the same state_dict, on the SAME engine object and in the SAME bank tensors (their addresses are what launch plans and captured
    graphs hold), and so does the module's own forward; a value beyond the fp16 range raises and leaves the banks as they were"""
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model = FCOS(num_classes=3, ext=True).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    images, targets = [rgb[0]], _model_targets(True)
    with torch.inference_mode():
        eng = model.engine()
        _, _, grads = model.output_grads(images, targets, assign=True)
    params = dict(model.named_parameters())
    assert all(torch.equal(params[k].grad, g) for k, g in grads.items())
    with torch.no_grad():
        for k in grads:
            params[k].sub_(1e-3 * params[k].grad)
    with torch.inference_mode():
        stale = eng.forward_heads(torch.stack(images))[0]
        banks = (eng.cls_out, eng.reg_out, eng.ext_out)
        fields = lambda: [t for b in banks for t in (b.w, b.bias, b.w16)]                # noqa: E731
        where = [t.data_ptr() for t in fields()]
        assert model.refresh_outputs() is model and model.engine() is eng
        assert all(a is b for a, b in zip((eng.cls_out, eng.reg_out, eng.ext_out), banks)) and [t.data_ptr() for t in fields()] == where
        cls_lr, reg_ctr, _, _ = eng.forward_heads(torch.stack(images))
        ex = eng._ext_levels
        fresh = FCOS(num_classes=3, ext=True)
        fresh.load_state_dict(model.state_dict())
        fresh = fresh.cuda().eval()
        f_cls, f_reg, _, _ = fresh.engine().forward_heads(torch.stack(images))
        f_ex = fresh.engine()._ext_levels
        assert fresh.engine() is not eng
        assert all(torch.equal(a, b) for xs, ys in ((cls_lr, f_cls), (reg_ctr, f_reg), (ex, f_ex)) for a, b in zip(xs, ys))
        assert not all(torch.equal(a, b) for a, b in zip(stale, cls_lr))
        # the module's own forward (another path to the same engine) against the fresh module's
        got, want = model(images)[0], fresh(images)[0]
        assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
        kept = [t.clone() for t in fields()]
        with torch.no_grad():
            params["head.regression_head.bbox_reg.weight"][0, 0, 0, 0] = 7.0e4
        with pytest.raises(ValueError, match="fp16 range"):
            model.refresh_outputs()
        assert all(a is b for a, b in zip((eng.cls_out, eng.reg_out, eng.ext_out), banks)) and model.engine() is eng
        assert all(torch.equal(a, b) for a, b in zip(fields(), kept))


def test_refresh_outputs_reaches_a_captured_graph():
    """a second holder of the engine: a graph captured BEFORE the step has the banks' addresses baked in; replayed after
    refresh_outputs() it gives the heads of a fresh FCOS with the new state (HandNetEngine keeps such graphs while the detector's
    engine object stays the same)"""
    from fcos_utils.fcos import FCOS
    from hn_amd import ops, synth
    model = FCOS(num_classes=3, ext=True).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    frame = torch.stack([rgb[0]])
    with torch.no_grad():
        eng = model.engine()
        with ops.on_device(eng.device):
            graph, out = ops.capture_step(lambda: eng.forward_heads(frame)[:2])
        graph.replay()
        eager = eng.forward_heads(frame)[:2]
        assert all(torch.equal(a, b) for xs, ys in zip(out, eager) for a, b in zip(xs, ys))
        before = [t.clone() for t in out[0]]
        for name in ("head.classification_head.cls_logits", "head.regression_head.bbox_reg"):
            dict(model.named_parameters())[name + ".weight"].mul_(0.5)
            dict(model.named_parameters())[name + ".bias"].add_(0.25)
        model.refresh_outputs()
        graph.replay()
        fresh = FCOS(num_classes=3, ext=True)
        fresh.load_state_dict(model.state_dict())
        want = fresh.cuda().eval().engine().forward_heads(frame)[:2]
        assert all(torch.equal(a, b) for xs, ys in zip(out, want) for a, b in zip(xs, ys))
        assert not all(torch.equal(a, b) for a, b in zip(out[0], before))


def test_output_grads_refuses_too_many_columns_before_any_launch():
    """with ext, C + 2 + 8 columns on the cls tower's map: num_classes = 7 is beyond the kernel's 16 and is refused in Python,
    with nothing run (no heads kept, no criterion)"""
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model = FCOS(num_classes=7, ext=True).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    with torch.inference_mode():
        eng = model.engine()
        eng._ext_levels = "untouched"
        with pytest.raises(ValueError, match=r"9 \+ 8 output columns"):
            model.output_grads([rgb[0]], _model_targets(True))
        assert eng._ext_levels == "untouched" and eng._capture is None
