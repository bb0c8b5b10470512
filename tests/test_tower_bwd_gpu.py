"""The tower layers' backward on the device -- hn_conv3x3_wgrad_f32 (weight and bias gradient on the f32-input MFMA),
hn_groupnorm_stats_levels_f32 / hn_groupnorm_relu_backward_f32 and the input gradient through the f32 implicit GEMM -- against the
float64 rule of tests/tower_bwd_ref.py on every case of tests/tower_bwd_cases.py, then tower_grads / refresh_towers of the engine
and of the drop-in detector.  The assertion is |err| <= the derived worst-case bound and nothing tighter (planted cases: bit for
bit); the ratios are printed and DESIGN.md section 9u holds the table measured on the MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import tower_bwd_cases as tc
import tower_bwd_ref as tr

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _cuda(t):
    return torch.from_numpy(np.array(t)).cuda()   # (a copy: the cases' arrays are read-only)


def _sliced(t, cols, fill=NAN):
    """t [N,h,w,C] on the device as columns first .. first + C of a `total`-wide tensor prefilled with `fill` -> (view, wide)"""
    if not cols:
        return t, None
    first, total = cols
    wide = torch.full(tuple(t.shape[:3]) + (total,), fill, device="cuda", dtype=t.dtype)
    wide[..., first:first + t.shape[3]] = t
    return wide[..., first:first + t.shape[3]], wide


def _conv_inputs(name):
    c = tc.conv_args(name)
    a16, dys = [], []
    for hi, lo, dy in zip(c["hi"], c["lo"], c["dy"]):
        t = _cuda(tr.pack_s32(hi, lo))
        if c["blocks"]:
            first, total = c["blocks"]
            wide = torch.full(tuple(t.shape[:3]) + (total, 2, 32), NAN, device="cuda", dtype=torch.float16)
            wide[:, :, :, first:first + t.shape[3]] = t
            t = wide[:, :, :, first:first + t.shape[3]]
        a16.append(t)
        dys.append(_sliced(_cuda(dy), c["cols"])[0])
    return c, a16, dys


def _conv_run(name):
    from hn_amd import ops, weights
    c, a16, dys = _conv_inputs(name)
    d_w, d_b = ops.conv3x3_wgrad_levels(a16, dys)
    d_a = ops.conv3x3_dgrad_levels(dys, weights.dgrad_bank(_cuda(c["w"])))
    got = {"dW": d_w.cpu().numpy(), "db": d_b.cpu().numpy()}
    got.update({f"dA{l}": t.cpu().numpy() for l, t in enumerate(d_a)})
    return c, got, (d_w, d_b)


@pytest.mark.parametrize("name", tc.CONV_NAMES)
def test_convolution_backward_is_inside_the_bound_and_a_second_run_gives_the_same_bytes(name):
    """dW and db of the MFMA kernel inside gamma(m_W), dA through the f32 implicit GEMM inside gamma(9 Cout); planted cases bit
    for bit; operands that are channel slices read nothing of the NaN around them"""
    c, got, (d_w, d_b) = _conv_run(name)
    assert d_w.dtype == torch.float32 and tuple(d_w.shape) == (c["cout"], 3, 3, c["cin"]) and tuple(d_b.shape) == (c["cout"],)
    detail = {}
    ratio = tr.check(got, tc.conv_reference(name), detail=detail)
    print(f"tower bwd gpu conv {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    if c["planted"]:
        want = tc.conv_reference(name)[0]
        for key in want:
            assert np.array_equal(got[key], want[key].astype(np.float32)), key
    if name == "1x1":
        off = np.ones((3, 3), bool)
        off[1, 1] = False
        assert not got["dW"][:, off].any() and got["dW"][:, off].tobytes() == bytes(got["dW"][:, off].nbytes)
    if name == "dy-zero":
        assert all(v.tobytes() == bytes(v.nbytes) for v in got.values())
    _, again, _ = _conv_run(name)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_dgrad_writes_its_half_of_a_wide_tensor_only():
    from hn_amd import ops, weights
    c, _, dys = _conv_inputs("cross")
    bank = weights.dgrad_bank(_cuda(c["w"]))
    outs = [torch.full(tuple(d.shape[:3]) + (96,), NAN, device="cuda") for d in dys]
    res = ops.conv3x3_dgrad_levels(dys, bank, outs=outs, out_channel_offset=64)
    alone = ops.conv3x3_dgrad_levels(dys, bank)
    for o, r, a in zip(outs, res, alone):
        assert r.data_ptr() == o[..., 64:].data_ptr() and torch.equal(o[..., 64:], a) and bool(torch.isnan(o[..., :64]).all())
    with pytest.raises(ValueError):
        ops.conv3x3_dgrad_levels(dys, bank, outs=outs, out_channel_offset=80)
    with pytest.raises(ValueError):
        ops.conv3x3_dgrad_levels(dys, bank, out_channel_offset=32)


def test_wgrad_refusals_launch_nothing():
    from hn_amd import _lib, ops
    c, a16, dys = _conv_inputs("cross")
    with pytest.raises(ValueError, match="1..5 levels"):
        ops.conv3x3_wgrad_levels(a16 * 3, dys * 3)
    with pytest.raises(ValueError, match="1..5 levels"):
        ops.conv3x3_wgrad_levels([], [])
    with pytest.raises(ValueError, match="one gradient per level"):
        ops.conv3x3_wgrad_levels(a16, dys[:1])
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv3x3_wgrad_levels(a16, [d[..., :48] for d in dys])                   # Cout off the rule
    with pytest.raises(ValueError):
        ops.conv3x3_wgrad_levels(a16, [d[:2] for d in dys])                         # another batch size
    with pytest.raises(ValueError, match="map sizes"):
        ops.conv3x3_wgrad_levels(a16, dys[::-1])
    with pytest.raises((TypeError, ValueError)):
        ops.conv3x3_wgrad_levels([t[..., :16] for t in a16], dys)                   # not an S32 map
    # the C entry's own refusals: prefilled outputs stay as they were
    lib = _lib.load()
    lv = _lib.WgradLevels()
    lv.count = 2
    for i, (a, d) in enumerate(zip(a16, dys)):
        lv.h[i], lv.w[i], lv.a16[i], lv.dy[i] = a.shape[1], a.shape[2], a.data_ptr(), d.data_ptr()
    need = lib.hn_conv3x3_wgrad_ws_bytes(C.byref(lv), c["n"], 32, 64)
    ranges, _, _ = tr.wgrad_plan(c["sizes"], c["n"], 32, 64)
    assert need == 4 * (ranges * 64 * 9 * 32 + ranges * 64)
    ws = torch.empty((need // 4,), device="cuda")
    d_w, d_b = torch.full((64, 3, 3, 32), -7.0, device="cuda"), torch.full((64,), -7.0, device="cuda")
    go = lambda lv_, nbytes=need, cin=32, cout=64, astride=0, dstride=0: lib.hn_conv3x3_wgrad_f32(   # noqa: E731
        C.byref(lv_), c["n"], cin, cout, astride, dstride, d_w.data_ptr(), d_b.data_ptr(), ws.data_ptr(), nbytes, None)
    assert go(lv, nbytes=need - 1) != 0 and b"workspace" in lib.hn_last_error()
    assert go(lv, cin=48) != 0 and go(lv, cout=16) != 0 and go(lv, cin=544) != 0
    assert lib.hn_conv3x3_wgrad_ws_bytes(C.byref(lv), c["n"], 48, 64) == -1
    assert go(lv, astride=96) != 0 and b"stride" in lib.hn_last_error()             # breaks the S32 block alignment
    assert go(lv, dstride=66) != 0 and b"stride" in lib.hn_last_error()             # breaks the 8-byte loads
    assert go(lv, dstride=32) != 0                                                  # below Cout
    bad = _lib.WgradLevels.from_buffer_copy(lv)
    bad.dy[1] = None
    assert go(bad) != 0 and b"null" in lib.hn_last_error()
    bad = _lib.WgradLevels.from_buffer_copy(lv)
    bad.count = 6
    assert go(bad) != 0 and b"level count" in lib.hn_last_error()
    bad.count = 0
    assert go(bad) != 0
    bad = _lib.WgradLevels.from_buffer_copy(lv)
    bad.h[0] = 0
    assert go(bad) != 0
    torch.cuda.synchronize()
    assert bool((d_w == -7).all()) and bool((d_b == -7).all())
    # ... and the same call with nothing wrong fills them, with the bytes of the call that allocates
    assert go(lv) == 0
    w2, b2 = ops.conv3x3_wgrad_levels(a16, dys)
    assert torch.equal(d_w, w2) and torch.equal(d_b, b2)


def _gn_inputs(name, fill=NAN):
    c = tc.gn_args(name)
    ys = [_sliced(_cuda(y), c["cols"], fill)[0] for y in c["y"]]
    gs = [_sliced(_cuda(g), c["cols"], fill)[0] for g in c["g"]]
    tables = [(_cuda(sc), _cuda(sh)) for sc, sh in c["tables"]]
    stats = [(_cuda(m), _cuda(r)) for m, r in c["stats"]]
    return c, ys, gs, tables, stats, _cuda(c["gamma"])


def _gn_run(name):
    from hn_amd import ops
    c, ys, gs, tables, stats, gam = _gn_inputs(name)
    wides = None
    if c["cols"]:
        pairs = [_sliced(torch.zeros(tuple(y.shape), device="cuda"), c["cols"]) for y in ys]
        dy_out, wides = [p[0] for p in pairs], [p[1] for p in pairs]
        dys, d_gamma, d_beta = ops.groupnorm_relu_backward_levels(ys, gs, tables, stats, gam, c["groups"], dy_out=dy_out)
        assert all(a is b for a, b in zip(dys, dy_out))
    else:
        dys, d_gamma, d_beta = ops.groupnorm_relu_backward_levels(ys, gs, tables, stats, gam, c["groups"])
    got = {"dgamma": d_gamma.cpu().numpy(), "dbeta": d_beta.cpu().numpy()}
    got.update({f"dy{l}": np.ascontiguousarray(t.cpu().numpy()) for l, t in enumerate(dys)})
    return c, got, wides


@pytest.mark.parametrize("name", tc.GN_NAMES)
def test_groupnorm_backward_is_inside_the_bound_and_a_second_run_gives_the_same_bytes(name):
    c, got, wides = _gn_run(name)
    detail = {}
    ratio = tr.check(got, tc.gn_reference(name), detail=detail)
    print(f"tower bwd gpu groupnorm {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    want = tc.gn_reference(name)[0]
    cpg = c["c"] // c["groups"]
    if name == "gzero":          # every element written, every one +0
        assert all(v.tobytes() == bytes(v.nbytes) for v in got.values())
    if name == "gint":
        assert np.array_equal(got["dbeta"], want["dbeta"].astype(np.float32))
    if c["masked"]:              # a group that passes no gradient: dy exactly 0 there, and its parameters' gradients
        assert not got["dy0"][..., :cpg].any() and not got["dgamma"][:cpg].any() and not got["dbeta"][:cpg].any()
        assert got["dy0"][..., cpg:].any()
    if c["gamma0"] is not None:
        assert got["dgamma"][c["gamma0"]] != 0 and np.isfinite(got["dgamma"]).all()
    if wides is not None:        # the slice is written everywhere, the NaN around it is left alone
        first, total = c["cols"]
        for t in wides:
            assert bool(torch.isnan(t[..., :first]).all()) and not bool(torch.isnan(t[..., first:first + c["c"]]).any())
    _, again, _ = _gn_run(name)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


@pytest.mark.parametrize("name", ["1x1", "cross", "512", "slice"])
def test_groupnorm_stats_levels_is_inside_its_bound(name):
    from hn_amd import ops
    c, ys, _, _, _, _ = _gn_inputs(name)
    stats = ops.groupnorm_stats_levels(ys, c["groups"])
    want, bound = tr.gn_stats(c["y"], c["groups"]), tr.gn_stats_bound(c["y"], c["groups"])
    worst = 0.0
    for (mean, rstd), (wm, wr), (bm, br) in zip(stats, want, bound):
        assert tuple(mean.shape) == tuple(rstd.shape) == (c["n"], c["groups"]) and mean.dtype == torch.float32
        for g_, w_, b_ in ((mean, wm, bm), (rstd, wr, br)):
            q = np.abs(g_.cpu().numpy().astype(np.float64) - w_) / b_
            worst = max(worst, float(q.max()))
    print(f"tower bwd gpu stats {name}: max |err| / bound = {worst:.4f}")
    assert worst <= 1.0
    again = ops.groupnorm_stats_levels(ys, c["groups"])
    assert all(torch.equal(a, b) for p, q in zip(stats, again) for a, b in zip(p, q))


def test_groupnorm_refusals_launch_nothing():
    from hn_amd import _lib, ops
    c, ys, gs, tables, stats, gam = _gn_inputs("cross")
    call = lambda **kw: ops.groupnorm_relu_backward_levels(*[kw.get(k, v) for k, v in (("ys", ys), ("gs", gs), ("tables", tables),   # noqa: E731
                                                            ("stats", stats), ("gamma", gam), ("groups", c["groups"]))])
    with pytest.raises(ValueError, match="1..5 levels"):
        call(ys=ys * 3, gs=gs * 3, tables=tables * 3, stats=stats * 3)
    with pytest.raises(ValueError, match="per level"):
        call(gs=gs[:1])
    with pytest.raises(ValueError, match="multiple of 8"):
        call(groups=16)                                                             # 4 channels per group
    with pytest.raises(ValueError, match="multiple of 8"):
        call(groups=5)
    with pytest.raises(ValueError):
        call(gs=[g[..., :32] for g in gs])
    with pytest.raises(ValueError, match="tables"):
        call(tables=[(sc[:, :32], sh[:, :32]) for sc, sh in tables])
    with pytest.raises(ValueError, match="mean / rstd"):
        call(stats=[(m[:, :4], r[:, :4]) for m, r in stats])
    with pytest.raises(ValueError, match="gamma"):
        call(gamma=gam[:32])
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.groupnorm_stats_levels(ys, 16)
    lib = _lib.load()
    n, ch, groups = c["n"], c["c"], c["groups"]
    dys = [torch.full(tuple(y.shape), -7.0, device="cuda") for y in ys]
    outs = [torch.full((ch,), -7.0, device="cuda") for _ in range(2)]
    lv = _lib.GnBwdLevels()
    lv.count = 2
    for i in range(2):
        lv.h[i], lv.w[i] = ys[i].shape[1], ys[i].shape[2]
        for k, t in (("y", ys[i]), ("g", gs[i]), ("scale", tables[i][0]), ("shift", tables[i][1]), ("mean", stats[i][0]),
                     ("rstd", stats[i][1]), ("dy", dys[i])):
            getattr(lv, k)[i] = t.data_ptr()
    need = lib.hn_groupnorm_relu_backward_ws_bytes(C.byref(lv), n, ch, groups)
    slots = n * sum(-(-h * w // tr.CHUNK) for h, w in c["sizes"])
    assert need == 4 * (slots * ch * 2 + 2 * n * groups * 2)
    ws = torch.empty((need // 4,), device="cuda")
    go = lambda lv_, nbytes=need, ch_=ch, groups_=groups, strides=(0, 0, 0, 0): lib.hn_groupnorm_relu_backward_f32(   # noqa: E731
        C.byref(lv_), n, ch_, groups_, *strides, gam.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), ws.data_ptr(), nbytes, None)
    assert go(lv, nbytes=need - 1) != 0 and b"workspace" in lib.hn_last_error()
    assert go(lv, groups_=16) != 0 and go(lv, ch_=60) != 0 and go(lv, ch_=1024, groups_=64) != 0
    assert lib.hn_groupnorm_relu_backward_ws_bytes(C.byref(lv), n, ch, 16) == -1
    assert go(lv, strides=(66, 0, 0, 0)) != 0 and b"stride" in lib.hn_last_error()
    assert go(lv, strides=(0, 0, 32, 0)) != 0 and go(lv, strides=(0, 0, 0, 70)) != 0
    for field in ("g", "mean", "dy"):
        bad = _lib.GnBwdLevels.from_buffer_copy(lv)
        getattr(bad, field)[1] = None
        assert go(bad) != 0 and b"null" in lib.hn_last_error()
    bad = _lib.GnBwdLevels.from_buffer_copy(lv)
    bad.y[0] = ys[0].data_ptr() + 4
    assert go(bad) != 0 and b"aligned" in lib.hn_last_error()
    bad = _lib.GnBwdLevels.from_buffer_copy(lv)
    bad.count = 6
    assert go(bad) != 0 and b"level count" in lib.hn_last_error()
    assert lib.hn_groupnorm_stats_levels_f32(C.byref(lv), n, ch, groups, 0, 1e-5, ws.data_ptr(), 8, None) != 0
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in dys + outs)
    assert go(lv) == 0
    want = ops.groupnorm_relu_backward_levels(ys, gs, tables, stats, gam, groups)
    assert all(torch.equal(a, b) for a, b in zip(dys + [outs[0], outs[1]], want[0] + [want[1], want[2]]))


# ---- the engine and the drop-in detector ----
_HEADS = ("head.classification_head", "head.regression_head")


def _conv_sums_device(a_levels, dys, w, absolute):
    """tr._conv_sums, line by line, in torch float64 on the device (the model's 6300 pixels x 512 x 256 x 9 would take numpy
    many seconds); test_device_rule_is_the_numpy_rule holds the two together"""
    f = torch.abs if absolute else (lambda t: t)
    cin, cout = a_levels[0].shape[3], dys[0].shape[3]
    out = {"dW": torch.zeros((cout, 3, 3, cin), device="cuda", dtype=torch.float64),
           "db": torch.zeros((cout,), device="cuda", dtype=torch.float64)}
    wd = f(w.double())
    for l, (a, dy) in enumerate(zip(a_levels, dys)):
        n, h, wdt, _ = a.shape
        g = f(dy.double())
        ap = torch.zeros((n, h + 2, wdt + 2, cin), device="cuda", dtype=torch.float64)
        ap[:, 1:-1, 1:-1] = f(a.double())
        gp = torch.zeros((n, h + 2, wdt + 2, cout), device="cuda", dtype=torch.float64)
        gp[:, 1:-1, 1:-1] = g
        out["db"] += g.sum((0, 1, 2))
        d_a = torch.zeros(tuple(a.shape), device="cuda", dtype=torch.float64)
        for r in range(3):
            for s in range(3):
                out["dW"][:, r, s] += g.reshape(-1, cout).T @ ap[:, r:r + h, s:s + wdt].reshape(-1, cin)
                d_a += gp[:, 2 - r:2 - r + h, 2 - s:2 - s + wdt] @ wd[:, r, s]
        out[f"dA{l}"] = d_a
    return {k: v.cpu().numpy() for k, v in out.items()}


def _conv_reference_device(a_levels, dys, w):
    """(rule, bound) like tr.conv_rule / tr.conv_bound, from the device sums and tr's plan"""
    want, mag = _conv_sums_device(a_levels, dys, w, False), _conv_sums_device(a_levels, dys, w, True)
    cin, cout = a_levels[0].shape[3], dys[0].shape[3]
    ranges, most, k = tr.wgrad_plan([tuple(a.shape[1:3]) for a in a_levels], a_levels[0].shape[0], cin, cout)
    m_w, m_a = most + ranges - 1, 9 * cout
    assert m_w <= k + 9
    bound = {key: tr.gamma(m_a if key.startswith("dA") else m_w) * s + (m_a if key.startswith("dA") else m_w) * 2.0 ** -149
             for key, s in mag.items()}
    return want, bound


def test_device_rule_is_the_numpy_rule():
    c = tc.conv_args("cross")
    args = ([_cuda(a) for a in c["a"]], [_cuda(d) for d in c["dy"]], _cuda(c["w"]))
    want, bound = tc.conv_reference("cross")
    got, gb = _conv_reference_device(*args)
    mag = tr._conv_sums(c["a"], c["dy"], c["w"], True)
    for key in want:
        assert np.all(np.abs(got[key] - want[key]) <= 1e-12 * mag[key] + 1e-300), key
        assert np.allclose(gb[key], bound[key], rtol=1e-12, atol=0), key


def _frame_targets(ext):
    from test_fcos_loss_gpu import _model_targets
    return _model_targets(ext)


@pytest.mark.parametrize("num_classes,ext", [(3, True), (2, False)])
def test_model_tower_grads(num_classes, ext):
    """FCOS.tower_grads on synthetic weights, one 480 x 640 frame: its first results are output_grads' bytes; every layer's dy,
    dgamma, dbeta, dW, db and dA is inside the bound of the rule applied to that layer's own captured tensors; the named
    gradients are the permuted, un-concatenated bytes of the engine's; inference is untouched; forward with targets raises"""
    from fcos_utils.fcos import FCOS
    from hn_amd import ops, synth
    model = FCOS(num_classes=num_classes, ext=ext).cuda().eval()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    images, targets = [rgb[0]], _frame_targets(ext)
    host = lambda t: t.cpu().numpy()                                                     # noqa: E731
    with torch.inference_mode():
        before = model(images)
        o_losses, o_fg, o_grads = model.output_grads(images, targets)
        losses, fg, grads = model.tower_grads(images, targets)
        assert list(losses) == list(o_losses) and all(torch.equal(losses[k], o_losses[k]) for k in losses) and torch.equal(fg, o_fg)
        assert set(o_grads) < set(grads) and all(torch.equal(grads[k], o_grads[k]) for k in o_grads)
        head = {k for k, _ in model.named_parameters() if k.startswith("head.")}
        assert set(grads) == head and all(tuple(grads[k].shape) == tuple(dict(model.named_parameters())[k].shape) for k in head)
        eng = model.engine()
        oh, ow, _, _ = eng.geometry(480, 640)
        packed = ops.pack_fcos_targets(targets, ops.fcos_target_ratios([(480, 640)], [(oh, ow)]), num_classes=num_classes, ext=ext)
        want_o = eng.output_grads(torch.stack(images), packed)
        res = eng.tower_grads(torch.stack(images), packed, want_inputs=True)
        e_losses, e_fg, e_grads, param_grads, d_towers, tg, d_feats, inp = res
        assert all(torch.equal(e_losses[k], want_o[0][k]) for k in e_losses) and torch.equal(e_fg, want_o[1])
        for a, b in zip(e_grads, want_o[2]):
            assert (a is None and b is None) or all(torch.equal(s, t) for s, t in zip(a, b))
        assert all(torch.equal(a, b) for k in param_grads for a, b in zip(param_grads[k], want_o[3][k]))
        assert all(torch.equal(a, b) for a, b in zip(d_towers, want_o[4]))
        # the named gradients: the engine's, permuted and un-concatenated
        for h, (hd, tower, gn) in enumerate(zip(_HEADS, ("cls_tower", "reg_tower"), ("cls_gn", "reg_gn"))):
            rows = slice(256 * h, 256 * (h + 1))
            convs = [(tg["tower0"][0][rows], tg["tower0"][1][rows])] + list(tg[tower])
            norms = [(tg["gn0"][0][rows], tg["gn0"][1][rows])] + list(tg[gn])
            for i, ((d_w, d_b), (d_g, d_be)) in enumerate(zip(convs, norms)):
                assert torch.equal(grads[f"{hd}.conv.{3 * i}.weight"], d_w.permute(0, 3, 1, 2)) and tuple(d_w.shape) == (256, 3, 3, 256)
                assert torch.equal(grads[f"{hd}.conv.{3 * i}.bias"], d_b)
                assert torch.equal(grads[f"{hd}.conv.{3 * i + 1}.weight"], d_g) and torch.equal(grads[f"{hd}.conv.{3 * i + 1}.bias"], d_be)
        assert tuple(tg["tower0"][0].shape) == (512, 3, 3, 256) and len(inp["layers"]) == 4
        assert [tuple(t.shape) for t in d_feats] == [tuple(f.shape[:3]) + (256,) for f in inp["feats"]]
        # layer by layer against the rule on the layer's own captured tensors
        worst = {}
        for k in (3, 2, 1, 0):
            lay = inp["layers"][k]
            gamma = eng.gn0_gamma if k == 0 else eng.both_gn[k - 1][0]
            ys, gs = [host(t) for t in lay["y"]], [host(t) for t in lay["g"]]
            tables = [(host(a), host(b)) for a, b in lay["aff"]]
            stats = [(host(a), host(b)) for a, b in lay["stats"]]
            sw, sb = tr.gn_stats(ys, 64), tr.gn_stats_bound(ys, 64)
            for (m_, r_), (wm, wr), (bm, br) in zip(stats, sw, sb):
                assert np.all(np.abs(m_ - wm) <= bm) and np.all(np.abs(r_ - wr) <= br)
            parts = (ys, gs, tables, stats, host(gamma), 64)
            got = {f"dy{l}": host(t) for l, t in enumerate(lay["dy"])}
            d_g, d_be = (tg["gn0"] if k == 0 else tuple(torch.cat([tg["cls_gn"][k - 1][j], tg["reg_gn"][k - 1][j]]) for j in (0, 1)))
            got.update(dgamma=host(d_g), dbeta=host(d_be))
            detail = {}
            tr.check(got, (tr.gn_rule(*parts), tr.gn_bound(*parts)), detail=detail)
            worst[f"L{k} gn"] = max(detail.values())
            banks = [("tower0", eng.tower0, None)] if k == 0 else [("cls_tower", eng.cls_tower[k - 1], 0), ("reg_tower", eng.reg_tower[k - 1], 1)]
            nxt = d_feats if k == 0 else inp["layers"][k - 1]["g"]
            for name, cw, h in banks:
                a = [ops.from_split(t if h is None else t[:, :, :, 8 * h:8 * (h + 1)]) for t in lay["a"]]
                dy = [t if h is None else t[..., 256 * h:256 * (h + 1)].contiguous() for t in lay["dy"]]
                d_w, d_b = tg[name] if k == 0 else tg[name][k - 1]
                got = {"dW": host(d_w), "db": host(d_b)}
                got.update({f"dA{l}": host(t if h is None else t[..., 256 * h:256 * (h + 1)].contiguous()) for l, t in enumerate(nxt)})
                detail = {}
                tr.check(got, _conv_reference_device(a, dy, cw.w), detail=detail)
                worst[f"L{k} {name}"] = max(detail.values())
        print(f"tower bwd gpu model C={num_classes} ext={ext}: max |err| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
        after = model(images)
        assert all(torch.equal(after[0][k], before[0][k]) for k in before[0])
        assert eng._capture is None and eng._capture_towers is False and eng._tower_cap is None
        with pytest.raises(NotImplementedError):
            model(images, targets)
        with pytest.raises(NotImplementedError):
            model.train()(images, targets)


def _small_model():
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model = FCOS(num_classes=2, ext=False, min_size=192, max_size=256).cuda().eval()
    frame = synth.make_rgb(1, seed=1000).cuda()[0][:, :192, :256].contiguous()
    targets = [{"boxes": torch.tensor([[20.0, 20.0, 120.0, 150.0], [150.0, 60.0, 230.0, 170.0]]), "labels": torch.tensor([1, 0]),
                "box_info": torch.tensor([[2.0, 1.0, 0.3, 0.1, 0.0], [-1.0, -1.0, 0.0, 0.0, 0.0]])}]
    return model, frame, targets


def test_wiring_against_torch_float64_autograd():
    """One 192 x 256 frame (levels 24 x 32, 12 x 16, 6 x 8): torch float64 autograd on the CPU through the reference's head layers
    with the engine's parameters, on from_split of the captured FPN outputs; the scalar is sum <captured head gradient, head
    output>.  max |got - want|_inf / |want|_inf over all parameter gradients and d_feats <= 1e-2 and nothing tighter: a swapped
    half, a missing flip or a transposed bank gives O(1); the per-layer bounds are the accuracy assertion."""
    import torch.nn.functional as fn
    from hn_amd import ops
    model, frame, targets = _small_model()
    with torch.inference_mode():
        eng = model.engine()
        oh, ow, _, _ = eng.geometry(192, 256)
        packed = ops.pack_fcos_targets(targets, ops.fcos_target_ratios([(192, 256)], [(oh, ow)]), num_classes=2, ext=False)
        res = eng.tower_grads(torch.stack([frame]), packed, want_inputs=True)
        _, _, (g_cls, g_reg, _), _, _, _, d_feats, inp = res
        assert [tuple(f.shape[1:3]) for f in inp["feats"]] == [(24, 32), (12, 16), (6, 8)]
        _, _, grads = model.tower_grads([frame], targets)
        feats = [ops.from_split(f).double().cpu().permute(0, 3, 1, 2) for f in inp["feats"]]
        up = [(a.double().cpu().permute(0, 3, 1, 2), b.double().cpu().permute(0, 3, 1, 2)) for a, b in zip(g_cls, g_reg)]
    # (copies made outside inference mode: ordinary tensors that autograd may save)
    params = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters() if k.startswith("head.")}
    feats = [f.clone().requires_grad_(True) for f in feats]
    up = [(a.clone(), b.clone()) for a, b in up]
    c, r = _HEADS
    conv = lambda x, name: fn.conv2d(x, params[name + ".weight"], params[name + ".bias"], padding=1)      # noqa: E731
    total = 0.0
    for x0, (u_cls, u_reg) in zip(feats, up):
        for hd in _HEADS:
            x = x0
            for i in range(4):
                x = torch.relu(fn.group_norm(conv(x, f"{hd}.conv.{3 * i}"), 32, params[f"{hd}.conv.{3 * i + 1}.weight"],
                                             params[f"{hd}.conv.{3 * i + 1}.bias"], eps=1e-5))
            if hd == c:
                total = total + (torch.cat([conv(x, c + ".cls_logits"), conv(x, c + ".hand_lr_layer")], 1) * u_cls).sum()
            else:
                total = total + (torch.cat([torch.relu(conv(x, r + ".bbox_reg")), conv(x, r + ".bbox_ctrness")], 1) * u_reg).sum()
    total.backward()
    worst, where = 0.0, None
    rel = lambda got, want: float((got.double().cpu() - want).abs().max() / want.abs().max())               # noqa: E731
    for k, p in params.items():
        q = rel(grads[k], p.grad)
        worst, where = (q, k) if q > worst else (worst, where)
    for l, (g, f) in enumerate(zip(d_feats, feats)):
        q = rel(g.permute(0, 3, 1, 2), f.grad)
        worst, where = (q, f"d_feats[{l}]") if q > worst else (worst, where)
    print(f"tower bwd gpu wiring: max |got - want|_inf / |want|_inf = {worst:.3e} at {where}")
    assert worst <= 1e-2


def _tower_fields(eng):
    banks = [eng.tower0] + eng.cls_tower + eng.reg_tower
    gns = [eng.gn0_gamma, eng.gn0_beta] + [t for trio in (eng.cls_gn, eng.reg_gn, eng.both_gn) for pair in trio for t in pair]
    return [t for b in banks for t in (b.w, b.bias, b.w16)] + gns


def test_refresh_towers_after_a_step_and_under_a_captured_graph():
    """an SGD step on every head parameter, then refresh_towers() + refresh_outputs(): the heads are the bytes of a fresh FCOS
    loaded from the same state_dict, on the same engine object and at the same tensor addresses; a graph captured before the step
    replays with the new weights; a value beyond the fp16 range raises and leaves every tensor as it was"""
    from fcos_utils.fcos import FCOS
    from hn_amd import ops
    model, frame, targets = _small_model()
    batch = torch.stack([frame])
    with torch.no_grad():
        eng = model.engine()
        with ops.on_device(eng.device):
            graph, out = ops.capture_step(lambda: eng.forward_heads(batch)[:2])
        graph.replay()
        stale = [t.clone() for t in out[0]]
    with torch.inference_mode():
        _, _, grads = model.tower_grads([frame], targets, assign=True)
    params = dict(model.named_parameters())
    assert all(torch.equal(params[k].grad, g) for k, g in grads.items()) and len(grads) == 40
    opt = torch.optim.SGD([params[k] for k in grads], lr=1e-3)
    opt.step()
    with torch.inference_mode():
        where = [t.data_ptr() for t in _tower_fields(eng)]
        assert model.refresh_towers() is model and model.refresh_outputs() is model and model.engine() is eng
        assert [t.data_ptr() for t in _tower_fields(eng)] == where
        cls_lr, reg_ctr, _, _ = eng.forward_heads(batch)
        fresh = FCOS(num_classes=2, ext=False, min_size=192, max_size=256)
        fresh.load_state_dict(model.state_dict())
        fresh = fresh.cuda().eval()
        f_cls, f_reg, _, _ = fresh.engine().forward_heads(batch)
        assert fresh.engine() is not eng
        assert all(torch.equal(a, b) for xs, ys in ((cls_lr, f_cls), (reg_ctr, f_reg)) for a, b in zip(xs, ys))
        assert all(torch.equal(a, b) for a, b in zip(_tower_fields(eng), _tower_fields(fresh.engine())))
        assert not all(torch.equal(a, b) for a, b in zip(stale, cls_lr))
        graph.replay()   # captured before the step: the banks' addresses are baked in, the values are the new ones
        assert all(torch.equal(a, b) for xs, ys in zip(out, (f_cls, f_reg)) for a, b in zip(xs, ys))
        kept = [t.clone() for t in _tower_fields(eng)]
        with torch.no_grad():
            params["head.regression_head.conv.9.weight"][0, 0, 0, 0] = 7.0e4
        with pytest.raises(ValueError, match="fp16 range"):
            model.refresh_towers()
        assert model.engine() is eng and [t.data_ptr() for t in _tower_fields(eng)] == where
        assert all(torch.equal(a, b) for a, b in zip(_tower_fields(eng), kept))


def test_tower_grads_refuses_other_routes_before_the_heads_run():
    from fcos_utils.fcos import FCOS
    from hn_amd import synth
    model, frame, targets = _small_model()
    rgb = synth.make_rgb(1, seed=1000).cuda()
    with torch.inference_mode():
        eng = model.engine()
        eng._ext_levels = "untouched"
        eng.head_streams = 2
        with pytest.raises(RuntimeError, match="grouped tower route"):
            model.tower_grads([frame], targets)
        eng.head_streams = 1
        tiny = FCOS(num_classes=2, ext=False, min_size=96, max_size=128).cuda().eval()
        tiny.engine()._ext_levels = "untouched"
        with pytest.raises(ValueError, match="fewer than 32 pixels"):
            tiny.tower_grads([rgb[0][:, :96, :128].contiguous()], targets)
        assert eng._ext_levels == "untouched" and tiny.engine()._ext_levels == "untouched"
        assert eng._capture is None and not eng._capture_towers
    f32 = FCOS(num_classes=2, ext=False, min_size=192, max_size=256).cuda().eval()
    from hn_amd.fcos_engine import FCOSEngine
    sd = {k: v.detach().cpu() for k, v in f32.state_dict().items()}
    e32 = FCOSEngine(sd, 2, device="cuda", min_size=192, max_size=256, precision="f32")
    with pytest.raises(RuntimeError, match="f16x3"):
        e32.tower_grads(torch.stack([frame]), None)
