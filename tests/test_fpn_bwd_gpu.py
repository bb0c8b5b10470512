"""The FPN's backward on the device -- hn_conv1x1_wgrad_f32 (the laterals' weight and bias gradient on the f32-input MFMA),
hn_upsample_nearest_backward_f32 (the adjoint of the top-down read) and the reused kernels of section 9u -- against the float64 rule
of tests/fpn_bwd_ref.py on every case of tests/fpn_bwd_cases.py, then fpn_grads / refresh_fpn of the engine and of the drop-in
detector.  The assertion is |err| <= the derived worst-case bound and nothing tighter (planted cases: bit for bit); the ratios are
printed and DESIGN.md section 9v holds the table measured on the MI355X."""
import numpy as np
import pytest
import torch

import fpn_bwd_cases as fc
import fpn_bwd_ref as fr
import tower_bwd_ref as tr

pytestmark = pytest.mark.gpu
NAN = float("nan")
D = np.float64


def _cuda(t):
    return torch.from_numpy(np.array(t)).cuda()   # (a copy: the cases' arrays are read-only)


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _sliced(t, cols, fill=NAN):
    """t [N,h,w,C] on the device as columns first .. first + C of a `total`-wide tensor prefilled with `fill` -> (view, wide)"""
    if not cols:
        return t, None
    first, total = cols
    wide = torch.full(tuple(t.shape[:3]) + (total,), fill, device="cuda", dtype=t.dtype)
    wide[..., first:first + t.shape[3]] = t
    return wide[..., first:first + t.shape[3]], wide


def _w1_inputs(name):
    c = fc.w1_args(name)
    a16 = _cuda(tr.pack_s32(c["hi"], c["lo"]))
    if c["blocks"]:
        first, total = c["blocks"]
        wide = torch.full(tuple(a16.shape[:3]) + (total, 2, 32), NAN, device="cuda", dtype=torch.float16)
        wide[:, :, :, first:first + a16.shape[3]] = a16
        a16 = wide[:, :, :, first:first + a16.shape[3]]
    return c, a16, _sliced(_cuda(c["dy"]), c["cols"])[0]


def _w1_run(name):
    from hn_amd import ops, weights
    c, a16, dy = _w1_inputs(name)
    d_w, d_b = ops.conv1x1_wgrad(a16, dy)
    d_c = ops.conv2d_nhwc(dy, weights.dgrad_bank_1x1(_cuda(c["w"])[:, None, None, :]))
    return c, {"dW": _host(d_w), "db": _host(d_b), "dC": _host(d_c)}, (d_w, d_b)


@pytest.mark.parametrize("name", fc.W1_NAMES)
def test_lateral_backward_is_inside_the_bound_and_a_second_run_gives_the_same_bytes(name):
    """dW and db of the MFMA kernel inside gamma(m_W), dC through the f32 implicit GEMM inside gamma(Cout); planted cases bit for
    bit; operands that are channel slices read nothing of the NaN around them"""
    c, got, (d_w, d_b) = _w1_run(name)
    assert d_w.dtype == torch.float32 and tuple(d_w.shape) == (c["cout"], c["cin"]) and tuple(d_b.shape) == (c["cout"],)
    detail = {}
    ratio = fr.check(got, fc.w1_reference(name), detail=detail)
    print(f"fpn bwd gpu lateral {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    if c["planted"]:
        want = fc.w1_reference(name)[0]
        for key in want:
            assert np.array_equal(got[key], want[key].astype(np.float32)), key
    if name == "dy-zero":
        assert all(v.tobytes() == bytes(v.nbytes) for v in got.values())
    _, again, _ = _w1_run(name)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def _up_run(name):
    from hn_amd import ops
    c = fc.up_args(name)
    g = _sliced(_cuda(c["g"]), c["cols"])[0]
    wide = None
    if c["cols"]:
        view, wide = _sliced(torch.zeros((c["n"],) + tuple(c["size"]) + (c["c"],), device="cuda"), c["cols"])
        out = ops.upsample_nearest_backward(g, c["size"], out=view)
        assert out is view
    else:
        out = ops.upsample_nearest_backward(g, c["size"])
    return c, {"U": _host(out)}, wide


@pytest.mark.parametrize("name", fc.UP_NAMES)
def test_adjoint_is_inside_the_bound_and_a_second_run_gives_the_same_bytes(name):
    c, got, wide = _up_run(name)
    assert got["U"].shape == (c["n"],) + tuple(c["size"]) + (c["c"],)
    detail = {}
    ratio = fr.check(got, fc.up_reference(name), detail=detail)
    print(f"fpn bwd gpu adjoint {name}: max |err| / bound = {detail['U']:.4f}")
    assert ratio <= 1.0
    want = fc.up_reference(name)[0]["U"]
    if c["planted"]:
        assert np.array_equal(got["U"], want.astype(np.float32))
    if name == "same":           # the identity: the gradient's own bytes
        assert got["U"].tobytes() == np.ascontiguousarray(c["g"]).tobytes()
    if wide is not None:         # the slice is written everywhere, the NaN around it is left alone
        first, _ = c["cols"]
        assert bool(torch.isnan(wide[..., :first]).all()) and bool(torch.isnan(wide[..., first + c["c"]:]).all())
        assert not bool(torch.isnan(wide[..., first:first + c["c"]]).any())
    _, again, _ = _up_run(name)
    assert got["U"].tobytes() == again["U"].tobytes()


def test_dgrad_adds_its_residual_after_the_chain():
    """conv3x3_dgrad_levels(residuals=): D = dgrad(G) + U inside gamma(9 Cout + 1); None changes nothing"""
    from hn_amd import ops, weights
    import tower_bwd_cases as tc
    c = tc.conv_args("cross")
    dys = [_cuda(d) for d in c["dy"]]
    bank = weights.dgrad_bank(_cuda(c["w"]))
    rng = np.random.default_rng(77)
    us = [None, rng.standard_normal(c["a"][1].shape).astype(np.float32)]
    got = ops.conv3x3_dgrad_levels(dys, bank, residuals=[None, _cuda(us[1])])
    plain = ops.conv3x3_dgrad_levels(dys, bank)
    assert torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1])
    for l in range(2):
        ratio = fr.check({"D": _host(got[l])}, fr.d_stage(c["dy"][l], c["w"], us[l]))
        print(f"fpn bwd gpu dgrad residual level {l}: max |err| / bound = {ratio:.4f}")
    with pytest.raises(ValueError, match="per level"):
        ops.conv3x3_dgrad_levels(dys, bank, residuals=[None])


def test_device_side_refusals_leave_the_outputs_untouched():
    from hn_amd import _lib, ops
    lib = _lib.load()
    c, a16, dy = _w1_inputs("odd")
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv1x1_wgrad(a16, dy[..., :16])
    with pytest.raises(ValueError, match="batch size"):
        ops.conv1x1_wgrad(a16, dy[:1])
    with pytest.raises((TypeError, ValueError)):
        ops.conv1x1_wgrad(a16[..., :16], dy)                                     # not an S32 map
    with pytest.raises(ValueError):
        ops.conv1x1_wgrad(a16, torch.zeros((2, 3, 5, 64), device="cuda")[..., ::2])       # not NHWC-dense
    rows, cin, cout = c["rows"], c["cin"], c["cout"]
    need = lib.hn_conv1x1_wgrad_ws_bytes(rows, cin, cout)
    assert need == fr.w1_ws_bytes(rows, cin, cout)
    ws = torch.empty((need // 4,), device="cuda")
    d_w, d_b = torch.full((cout, cin), -7.0, device="cuda"), torch.full((cout,), -7.0, device="cuda")
    go = lambda a=a16.data_ptr(), g=dy.data_ptr(), rows_=rows, cin_=cin, cout_=cout, astride=0, dstride=0, dw=d_w.data_ptr(), nbytes=need: \
        lib.hn_conv1x1_wgrad_f32(a, g, rows_, cin_, cout_, astride, dstride, dw, d_b.data_ptr(), ws.data_ptr(), nbytes, None)   # noqa: E731
    assert go(nbytes=need - 1) != 0 and b"workspace" in lib.hn_last_error()
    assert go(cin_=48) != 0 and go(cout_=16) != 0 and go(cin_=544) != 0 and go(rows_=0) != 0
    assert go(astride=96) != 0 and b"stride" in lib.hn_last_error()
    assert go(dstride=34) != 0 and b"stride" in lib.hn_last_error() and go(dstride=16) != 0
    assert go(a=None) != 0 and b"null" in lib.hn_last_error() and go(g=None) != 0 and go(dw=None) != 0
    assert go(a=a16.data_ptr() + 4) != 0 and b"unaligned" in lib.hn_last_error()
    assert go(g=dy.data_ptr() + 8) != 0 and b"unaligned" in lib.hn_last_error()
    # the adjoint
    cu = fc.up_args("5x7")
    g = _cuda(cu["g"])
    out = torch.full((cu["n"],) + tuple(cu["size"]) + (cu["c"],), -7.0, device="cuda")
    up = lambda g_=g.data_ptr(), rh=3, rw=4, ch=cu["c"], gs=0, os_=0, o=out.data_ptr(): \
        lib.hn_upsample_nearest_backward_f32(g_, cu["n"], 5, 7, rh, rw, ch, gs, os_, o, None)              # noqa: E731
    assert up(rh=6) != 0 and b"larger" in lib.hn_last_error() and up(rw=8) != 0
    assert up(ch=10) != 0 and up(gs=8) != 0 and b"stride" in lib.hn_last_error() and up(os_=14) != 0
    assert up(g_=None) != 0 and b"null" in lib.hn_last_error() and up(o=None) != 0
    assert up(g_=g.data_ptr() + 4) != 0 and b"unaligned" in lib.hn_last_error()
    with pytest.raises(ValueError, match="no larger"):
        ops.upsample_nearest_backward(g, (6, 4))
    torch.cuda.synchronize()
    assert bool((d_w == -7).all()) and bool((d_b == -7).all()) and bool((out == -7).all())
    # ... and the same calls with nothing wrong fill them, with the bytes of the calls that allocate
    assert go() == 0 and up() == 0
    w2, b2 = ops.conv1x1_wgrad(a16, dy)
    assert torch.equal(d_w, w2) and torch.equal(d_b, b2) and torch.equal(out, ops.upsample_nearest_backward(g, cu["size"]))


# ---- the engine and the drop-in detector ----
_SIZES = [(24, 32), (12, 16), (6, 8)]
_CINS = (128, 256, 512)


def _model(num_classes=2, ext=False):
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model = FCOS(num_classes=num_classes, ext=ext, min_size=192, max_size=256).cuda().eval()
    frame = synth.make_rgb(1, seed=1000).cuda()[0][:, :192, :256].contiguous()
    targets = [{"boxes": torch.tensor([[20.0, 20.0, 120.0, 150.0], [150.0, 60.0, 230.0, 170.0]]), "labels": torch.tensor([1, 0]),
                "box_info": torch.tensor([[2.0, 1.0, 0.3, 0.1, 0.0], [-1.0, -1.0, 0.0, 0.0, 0.0]])}]
    return model, frame, targets


def _check_stages(eng, d_feats, fpn_pg, d_body, inp):
    """every stage of fpn_grads against the rule on its own captured tensors -> {stage: max |err| / bound}"""
    from hn_amd import ops
    worst = {}
    for l in range(3):
        c, lat = _host(ops.from_split(inp["c"][l])), _host(ops.from_split(inp["lat"][l]))
        g, d = _host(d_feats[l]), _host(inp["D"][l])
        u = None if inp["U"][l] is None else _host(inp["U"][l])
        assert (u is None) == (l == 0)
        (d_wl, d_bl), (d_wi, d_bi) = fpn_pg["layer"][l], fpn_pg["inner"][l]
        assert tuple(d_wl.shape) == (256, 3, 3, 256) and tuple(d_wi.shape) == (256, c.shape[3]) and tuple(d_body[l].shape) == c.shape
        worst[f"P{l + 3} layer"] = fr.check({"dWlayer": _host(d_wl), "dblayer": _host(d_bl)}, fr.layer_stage(lat, g))
        worst[f"P{l + 3} D"] = fr.check({"D": d}, fr.d_stage(g, _host(eng.layer[l].w), u))
        if l:
            worst[f"P{l + 3} upT"] = fr.check({"U": u}, fr.up_t_stage(_host(inp["D"][l - 1]), d.shape[1:3]))
        worst[f"P{l + 3} inner"] = fr.check({"dW": _host(d_wi), "db": _host(d_bi)}, fr.w1_stage(c, d))
        worst[f"P{l + 3} dC"] = fr.check({"dC": _host(d_body[l])}, fr.dc_stage(d, _host(eng.inner[l].w)[:, 0, 0, :]))
    return worst


@pytest.mark.parametrize("num_classes,ext", [(2, False), (3, True)])
def test_model_fpn_grads(num_classes, ext):
    """FCOS.fpn_grads on synthetic weights, one 192 x 256 frame (levels 24 x 32, 12 x 16, 6 x 8): its first results are
    tower_grads' bytes; every stage -- layer dW / db, D_l, upT, lateral dW / db, dC_l -- is inside the bound of the rule applied to
    that stage's own captured tensors; the named gradients are the permuted bytes of the engine's; inference is untouched; forward
    with targets keeps raising"""
    from hn_amd import ops
    model, frame, targets = _model(num_classes, ext)
    images = [frame]
    with torch.inference_mode():
        before = model(images)
        t_losses, t_fg, t_grads = model.tower_grads(images, targets)
        losses, fg, grads = model.fpn_grads(images, targets)
        assert list(losses) == list(t_losses) and all(torch.equal(losses[k], t_losses[k]) for k in losses) and torch.equal(fg, t_fg)
        assert set(t_grads) < set(grads) and all(torch.equal(grads[k], t_grads[k]) for k in t_grads)
        params = dict(model.named_parameters())
        names = {k for k in params if k.startswith("head.") or k.startswith("backbone.fpn.")}
        assert set(grads) == names and len(set(grads) - set(t_grads)) == 12
        assert all(tuple(grads[k].shape) == tuple(params[k].shape) for k in names)
        eng = model.engine()
        oh, ow, _, _ = eng.geometry(192, 256)
        packed = ops.pack_fcos_targets(targets, ops.fcos_target_ratios([(192, 256)], [(oh, ow)]), num_classes=num_classes, ext=ext)
        want_t = eng.tower_grads(torch.stack(images), packed)
        res = eng.fpn_grads(torch.stack(images), packed, want_inputs=True)
        assert len(res) == 10
        fpn_pg, d_body, inp = res[7], res[8], res[9]
        assert all(torch.equal(res[0][k], want_t[0][k]) for k in res[0]) and torch.equal(res[1], want_t[1])
        assert all(torch.equal(a, b) for k in res[3] for a, b in zip(res[3][k], want_t[3][k]))
        assert all(torch.equal(a, b) for a, b in zip(res[4], want_t[4])) and all(torch.equal(a, b) for a, b in zip(res[6], want_t[6]))
        assert torch.equal(res[5]["tower0"][0], want_t[5]["tower0"][0])
        assert len(eng.fpn_grads(torch.stack(images), packed)) == 9
        assert [tuple(t.shape[1:3]) for t in inp["lat"]] == _SIZES and [ops.channels(t) for t in inp["c"]] == list(_CINS)
        for i in range(3):      # the named gradients: the engine's, in the reference's layouts
            assert torch.equal(grads[f"backbone.fpn.inner_blocks.{i}.weight"][:, :, 0, 0], fpn_pg["inner"][i][0])
            assert torch.equal(grads[f"backbone.fpn.inner_blocks.{i}.bias"], fpn_pg["inner"][i][1])
            assert torch.equal(grads[f"backbone.fpn.layer_blocks.{i}.weight"], fpn_pg["layer"][i][0].permute(0, 3, 1, 2))
            assert torch.equal(grads[f"backbone.fpn.layer_blocks.{i}.bias"], fpn_pg["layer"][i][1])
        worst = _check_stages(eng, res[6], fpn_pg, d_body, inp)
        print(f"fpn bwd gpu model C={num_classes} ext={ext}: max |err| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0 and all(_host(t).any() for t in d_body)
        after = model(images)
        assert all(torch.equal(after[0][k], before[0][k]) for k in before[0])
        assert eng._capture is None and eng._capture_towers is False and eng._capture_fpn is False and eng._fpn_cap is None
        with pytest.raises(NotImplementedError):
            model(images, targets)
        with pytest.raises(NotImplementedError):
            model.train()(images, targets)


def test_wiring_against_torch_float64_autograd():
    """One 192 x 256 frame: torch float64 autograd on the CPU through the reference's FPN layers (F.conv2d, F.interpolate nearest,
    +, F.conv2d padding 1) with the engine's parameters, on from_split of the captured c3..c5; the scalar is sum <captured
    d_feats[l], P_l>.  max |got - want|_inf / |want|_inf over the twelve parameter gradients and d_body <= 1e-2 and nothing tighter
    (section 9u's wiring threshold): a wrong level, a missing flip or a transposed bank gives O(1); the per-stage bounds are the
    accuracy assertion."""
    import torch.nn.functional as fn
    from hn_amd import ops
    model, frame, targets = _model()
    with torch.inference_mode():
        eng = model.engine()
        oh, ow, _, _ = eng.geometry(192, 256)
        packed = ops.pack_fcos_targets(targets, ops.fcos_target_ratios([(192, 256)], [(oh, ow)]), num_classes=2, ext=False)
        res = eng.fpn_grads(torch.stack([frame]), packed, want_inputs=True)
        d_feats, fpn_pg, d_body, inp = res[6], res[7], res[8], res[9]
        cs = [ops.from_split(t).double().cpu().permute(0, 3, 1, 2) for t in inp["c"]]
        gs = [t.double().cpu().permute(0, 3, 1, 2) for t in d_feats]
        got = {}
        for i in range(3):
            got[f"inner_blocks.{i}.weight"] = fpn_pg["inner"][i][0][:, :, None, None].double().cpu()
            got[f"inner_blocks.{i}.bias"] = fpn_pg["inner"][i][1].double().cpu()
            got[f"layer_blocks.{i}.weight"] = fpn_pg["layer"][i][0].permute(0, 3, 1, 2).double().cpu()
            got[f"layer_blocks.{i}.bias"] = fpn_pg["layer"][i][1].double().cpu()
            got[f"d_body[{i}]"] = d_body[i].double().cpu().permute(0, 3, 1, 2)
    # (copies made outside inference mode: ordinary tensors that autograd may save)
    p = {k[len("backbone.fpn."):]: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters()
         if k.startswith("backbone.fpn.")}
    assert len(p) == 12
    cs = [t.clone().requires_grad_(True) for t in cs]
    gs = [t.clone() for t in gs]
    lats = [None] * 3
    lats[2] = fn.conv2d(cs[2], p["inner_blocks.2.weight"], p["inner_blocks.2.bias"])
    for l in (1, 0):
        lats[l] = fn.conv2d(cs[l], p[f"inner_blocks.{l}.weight"], p[f"inner_blocks.{l}.bias"]) \
            + fn.interpolate(lats[l + 1], size=cs[l].shape[-2:], mode="nearest")
    total = sum((fn.conv2d(lats[l], p[f"layer_blocks.{l}.weight"], p[f"layer_blocks.{l}.bias"], padding=1) * gs[l]).sum() for l in range(3))
    total.backward()
    want = {k: v.grad for k, v in p.items()}
    want.update({f"d_body[{i}]": cs[i].grad for i in range(3)})
    assert set(want) == set(got)
    worst, where = 0.0, None
    for k in want:
        assert got[k].shape == want[k].shape, k
        q = float((got[k] - want[k]).abs().max() / want[k].abs().max())
        worst, where = (q, k) if q > worst else (worst, where)
    print(f"fpn bwd gpu wiring: max |got - want|_inf / |want|_inf = {worst:.3e} at {where}")
    assert worst <= 1e-2


def test_list_of_two_sizes_runs_image_by_image_and_obeys_the_rule():
    """a list of two differently sized images: the captured tensors are the per-image ones concatenated per level, and every stage
    obeys the rule on them inside the bounds"""
    model, frame, targets = _model()
    second = frame[:, :176, :].contiguous()
    images = [frame, second]
    both = targets + [{"boxes": torch.tensor([[30.0, 25.0, 140.0, 160.0]]), "labels": torch.tensor([1]),
                       "box_info": torch.tensor([[1.0, 0.0, 0.5, 0.1, -0.1]])}]
    with torch.inference_mode():
        eng, batch, packed = model._grads_args(images, both)
        assert not torch.is_tensor(batch)
        res = eng.fpn_grads(batch, packed, want_inputs=True)
        d_feats, fpn_pg, d_body, inp = res[6], res[7], res[8], res[9]
        assert all(t.shape[0] == 2 for t in inp["c"] + inp["lat"] + inp["D"] + list(d_feats) + list(d_body))
        assert [tuple(t.shape[1:3]) for t in inp["lat"]] == _SIZES
        worst = _check_stages(eng, d_feats, fpn_pg, d_body, inp)
        print("fpn bwd gpu list of two sizes: max |err| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0
        assert eng._capture_fpn is False and eng._fpn_cap is None
        _, _, grads = model.fpn_grads(images, both)
        assert torch.equal(grads["backbone.fpn.inner_blocks.0.weight"][:, :, 0, 0], fpn_pg["inner"][0][0])


def _fpn_fields(eng):
    return [t for b in eng.inner + eng.layer for t in (b.w, b.bias, b.w16)]


def test_refresh_fpn_after_a_step():
    """fpn_grads(assign=True) + SGD.step() + refresh_fpn() (+ the head's two refreshes): the six banks keep their addresses and
    loss_step gives, bit for bit, the losses of a fresh FCOS loaded with the updated state dict; a weight beyond the fp16 range
    raises and leaves every bank's bytes unchanged"""
    from fcos_utils.fcos import FCOS
    model, frame, targets = _model()
    with torch.inference_mode():
        eng = model.engine()
        stale, _ = model.loss_step([frame], targets)
        _, _, grads = model.fpn_grads([frame], targets, assign=True)
    params = dict(model.named_parameters())
    assert len(grads) == 52 and all(torch.equal(params[k].grad, g) for k, g in grads.items())
    torch.optim.SGD([params[k] for k in grads], lr=1e-3).step()
    with torch.inference_mode():
        where = [t.data_ptr() for t in _fpn_fields(eng)]
        assert len(where) == 18 and all(where)
        assert model.refresh_fpn() is model and model.refresh_towers() is model and model.refresh_outputs() is model
        assert model.engine() is eng and [t.data_ptr() for t in _fpn_fields(eng)] == where
        losses, fg = model.loss_step([frame], targets)
        fresh = FCOS(num_classes=2, ext=False, min_size=192, max_size=256)
        fresh.load_state_dict(model.state_dict())
        fresh = fresh.cuda().eval()
        f_losses, f_fg = fresh.loss_step([frame], targets)
        assert fresh.engine() is not eng
        assert list(losses) == list(f_losses) and all(torch.equal(losses[k], f_losses[k]) for k in losses) and torch.equal(fg, f_fg)
        assert all(torch.equal(a, b) for a, b in zip(_fpn_fields(eng), _fpn_fields(fresh.engine())))
        assert not all(torch.equal(losses[k], stale[k]) for k in losses)
        kept = [t.clone() for t in _fpn_fields(eng)]
        with torch.no_grad():
            params["backbone.fpn.layer_blocks.2.weight"][0, 0, 0, 0] = 7.0e4
        with pytest.raises(ValueError, match="fp16 range"):
            model.refresh_fpn()
        with torch.no_grad():
            params["backbone.fpn.layer_blocks.2.weight"][0, 0, 0, 0] = 0.0
            params["backbone.fpn.inner_blocks.0.bias"][3] = float("inf")
        with pytest.raises(ValueError):
            model.refresh_fpn()
        assert model.engine() is eng and [t.data_ptr() for t in _fpn_fields(eng)] == where
        assert all(torch.equal(a, b) for a, b in zip(_fpn_fields(eng), kept))


def test_fpn_grads_is_refused_wherever_tower_grads_is():
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    from hn_amd.fcos_engine import FCOSEngine
    model, frame, targets = _model()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    with torch.inference_mode():
        eng = model.engine()
        eng._ext_levels = "untouched"
        eng.head_streams = 2
        with pytest.raises(RuntimeError, match="grouped tower route"):
            model.fpn_grads([frame], targets)
        eng.head_streams = 1
        tiny = FCOS(num_classes=2, ext=False, min_size=96, max_size=128).cuda().eval()
        tiny.engine()._ext_levels = "untouched"
        with pytest.raises(ValueError, match="fewer than 32 pixels"):
            tiny.fpn_grads([rgb[0][:, :96, :128].contiguous()], targets)
        assert eng._ext_levels == "untouched" and tiny.engine()._ext_levels == "untouched"
        assert eng._capture is None and not eng._capture_towers and not eng._capture_fpn and eng._fpn_cap is None
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    e32 = FCOSEngine(sd, 2, device="cuda", min_size=192, max_size=256, precision="f32")
    with pytest.raises(RuntimeError, match="f16x3"):
        e32.fpn_grads(torch.stack([frame]), None)
