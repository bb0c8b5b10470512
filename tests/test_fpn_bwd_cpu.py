"""The rule of the FPN's backward (tests/fpn_bwd_ref.py) against torch's float64 autograd through the reference's own layer arithmetic
-- F.conv2d, F.interpolate(mode="nearest", size=...), + and F.conv2d(padding=1) (torchvision's FeaturePyramidNetwork) --, the plans
of the two new kernels, the planted cases' expected values, weights.dgrad_bank_1x1, the new header's declaration, export and binding,
and every refusal of the new front ends that needs no device.  No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as fn

import fpn_bwd_cases as fc
import fpn_bwd_ref as fr
import tower_bwd_ref as tr

REPO = Path(__file__).resolve().parent.parent
D = np.float64
NEW = ["hn_conv1x1_wgrad_f32", "hn_conv1x1_wgrad_ws_bytes", "hn_upsample_nearest_backward_f32"]


def _nchw(t):
    return torch.from_numpy(np.array(t, D)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _close(got, want, mag):
    return np.all(np.abs(got - want) <= 1e-12 * mag + 1e-300)


@pytest.mark.parametrize("name", fc.FPN_NAMES)
def test_rule_equals_torch_float64_autograd(name):
    """loss = sum_l <G_l, P_l> through the reference's FPN layers: its gradients at the twelve parameters and at c3..c5 are the
    rule fed with the forward's own lat_l, to 1e-12 of the sum of |terms| on every element"""
    c = fc.fpn_args(name)
    cs = [_nchw(t).requires_grad_(True) for t in c["c"]]
    wi = [torch.from_numpy(np.array(w))[:, :, None, None].requires_grad_(True) for w in c["w_inner"]]
    bi = [torch.from_numpy(np.array(b)).requires_grad_(True) for b in c["b_inner"]]
    wl = [_nchw(w).requires_grad_(True) for w in c["w_layer"]]     # [Cout,3,3,Cin] -> [Cout,Cin,3,3]
    bl = [torch.from_numpy(np.array(b)).requires_grad_(True) for b in c["b_layer"]]
    lats = [None] * 3
    lats[2] = fn.conv2d(cs[2], wi[2], bi[2])
    for l in (1, 0):
        lats[l] = fn.conv2d(cs[l], wi[l], bi[l]) + fn.interpolate(lats[l + 1], size=c["sizes"][l], mode="nearest")
    loss = sum((fn.conv2d(lat, w, b, padding=1) * _nchw(g)).sum() for lat, w, b, g in zip(lats, wl, bl, c["g"]))
    loss.backward()
    lat_np = [_nhwc(t.detach()) for t in lats]
    # the forward's top-down read is the rule's `up`
    for l in (1, 0):
        own = lat_np[l] - _nhwc(fn.conv2d(cs[l], wi[l], bi[l]).detach())
        assert np.allclose(own, fr.up(lat_np[l + 1], c["sizes"][l]), rtol=0, atol=1e-12)
    parts = (c["c"], lat_np, c["g"], c["w_inner"], c["w_layer"])
    want, mag = fr.fpn_rule(*parts), fr._fpn_sums(*parts, True)
    got = {}
    for l in range(3):
        got[f"dWlayer{l}"], got[f"dblayer{l}"] = _nhwc(wl[l].grad), bl[l].grad.numpy()
        got[f"dWinner{l}"], got[f"dbinner{l}"] = wi[l].grad[:, :, 0, 0].numpy(), bi[l].grad.numpy()
        got[f"dC{l}"] = _nhwc(cs[l].grad)
    assert set(got) == {k for k in want if not k.startswith("D")}
    for key in got:
        assert got[key].shape == want[key].shape and _close(got[key], want[key], mag[key]), key
    # D_l itself: the gradient at lat_l
    lats2 = [torch.from_numpy(t).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in lat_np]
    tot = 0.0
    for l in range(3):
        x = lats2[l]
        for k in range(l, 0, -1):     # lat_l also feeds every finer level through the top-down reads
            x = fn.interpolate(x, size=c["sizes"][k - 1], mode="nearest")
            tot = tot + (fn.conv2d(x, wl[k - 1].detach(), None, padding=1) * _nchw(c["g"][k - 1])).sum()
        tot = tot + (fn.conv2d(lats2[l], wl[l].detach(), None, padding=1) * _nchw(c["g"][l])).sum()
    tot.backward()
    for l in range(3):
        assert _close(_nhwc(lats2[l].grad), want[f"D{l}"], mag[f"D{l}"]), l


@pytest.mark.parametrize("name", fc.W1_NAMES)
def test_lateral_rule_equals_torch_float64_autograd(name):
    c = fc.w1_args(name)
    a = _nchw(c["a"]).requires_grad_(True)
    w = torch.from_numpy(np.array(c["w"], D))[:, :, None, None].requires_grad_(True)
    b = torch.zeros(c["cout"], dtype=torch.float64, requires_grad=True)
    (fn.conv2d(a, w, b) * _nchw(c["dy"])).sum().backward()
    want, _ = fc.w1_reference(name)
    mag = dict(fr._w1_sums(c["a"], c["dy"], True), dC=np.abs(c["dy"].astype(D)) @ np.abs(c["w"].astype(D)))
    got = {"dW": w.grad[:, :, 0, 0].numpy(), "db": b.grad.numpy(), "dC": _nhwc(a.grad)}
    for key in want:
        assert _close(got[key], want[key], mag[key]), key


@pytest.mark.parametrize("name", fc.UP_NAMES)
def test_adjoint_rule_equals_torch_float64_autograd(name):
    """x -> F.interpolate(x, size, 'nearest') reads by the floor rule, and its autograd is upT"""
    c = fc.up_args(name)
    x = torch.randn((c["n"], c["c"]) + tuple(c["size"]), dtype=torch.float64, requires_grad=True)
    y = fn.interpolate(x, size=c["fine"], mode="nearest")
    assert np.array_equal(_nhwc(y.detach()), fr.up(_nhwc(x.detach()), c["fine"]))
    (y * _nchw(c["g"])).sum().backward()
    want = fr.up_t(c["g"], c["size"])
    assert _close(_nhwc(x.grad), want, fr.up_t(c["g"], c["size"], True))
    ref, b = fc.up_reference(name)
    assert np.array_equal(ref["U"], want) and np.all(b["U"] >= 0)


def test_adjoint_plan():
    """the source ranges per axis: contiguous, never empty while r <= O, exactly the floor rule's sets"""
    assert [hi - lo for lo, hi in fr.up_ranges(5, 3)] == [2, 2, 1]
    assert [hi - lo for lo, hi in fr.up_ranges(7, 4)] == [2, 2, 2, 1]
    assert fr.up_ranges(4, 2) == [(0, 2), (2, 4)] and fr.up_ranges(3, 3) == [(0, 1), (1, 2), (2, 3)] and fr.up_ranges(2, 1) == [(0, 2)]
    for o in range(1, 40):
        for r in range(1, o + 1):
            rs = fr.up_ranges(o, r)
            assert rs[0][0] == 0 and rs[-1][1] == o and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
    with pytest.raises(AssertionError):
        fr.up_ranges(3, 4)                           # a coarse index that nothing reads
    # m_U = terms - 1 is the any-order count; the identity rounds nothing
    _, b = fc.up_reference("same")
    assert not b["U"].any()
    _, b = fc.up_reference("all")
    c = fc.up_args("all")
    assert np.allclose(b["U"], tr.gamma(3) * np.abs(c["g"].astype(D)).sum((1, 2), keepdims=True) + 3 * 2.0 ** -149, rtol=1e-15, atol=0)


def test_lateral_plan():
    assert fr.w1_plan(1, 32, 32) == (1, 1, [1])
    assert fr.w1_plan(80, 32, 32) == (3, 32, [32, 32, 16])                       # the planted map
    ranges, most, sizes = fr.w1_plan(fc.w1_args("ranges")["rows"], 32, 32)
    assert (ranges, most) == (37, 64) and ranges >= 3 and sizes[-1] == 6 and set(sizes[:-1]) == {64}
    assert fr.w1_plan(20, 128, 256) == (1, 20, [20]) and fr.w1_plan(9, 512, 256)[0] == 1
    # the 480 x 640 frame on its 800 x 1088 canvas: 100 x 136, 50 x 68, 25 x 34, at batch 1 and 16
    assert fr.w1_plan(13600, 128, 256)[:2] == (61, 224) and fr.w1_plan(3400, 256, 256)[:2] == (54, 64) and fr.w1_plan(850, 512, 256)[:2] == (27, 32)
    assert fr.w1_plan(16 * 13600, 128, 256)[:2] == (64, 3424)
    assert fr.w1_plan(1 << 20, 512, 512)[0] == 16                                # 32 groups: the cap is 16 ranges
    for name in fc.W1_NAMES:
        c = fc.w1_args(name)
        ranges, most, sizes = fr.w1_plan(c["rows"], c["cin"], c["cout"])
        assert most + ranges - 1 <= c["rows"]                                    # never beyond the any-order bound
        want, b = fc.w1_reference(name)
        mag = fr._w1_sums(c["a"], c["dy"], True)
        for key in ("dW", "db"):
            assert np.all(b[key] <= tr.gamma(c["rows"]) * mag[key] + c["rows"] * 2.0 ** -149), (name, key)
    assert fr.w1_ws_bytes(80, 32, 32) == 4 * (3 * 32 * 32 + 3 * 32)
    for bad in ((0, 32, 32), (5, 48, 32), (5, 32, 16), (5, 544, 32)):
        with pytest.raises(AssertionError):
            fr.w1_plan(*bad)


@pytest.mark.parametrize("name", fc.W1_NAMES)
def test_operands_are_exact_in_fp32(name):
    c = fc.w1_args(name)
    assert c["a"].dtype == np.float32 and np.array_equal(c["a"].astype(D), c["hi"].astype(D) + c["lo"].astype(D))
    assert tr.pack_s32(c["hi"], c["lo"]).shape == c["a"].shape[:3] + (c["cin"] // 32, 2, 32)


@pytest.mark.parametrize("name", list(fc.W1_PLANTED))
def test_planted_cases_expected_values(name):
    """the planted cases' values written down by hand are what the rule gives, and every one of them is an fp32 number"""
    want, _ = fc.w1_reference(name)
    exp = fc.w1_planted_expected(name)
    assert set(exp) == set(want)
    for key in want:
        assert np.array_equal(exp[key], want[key]), key
        assert np.array_equal(want[key].astype(np.float32).astype(D), want[key]), key
    if name == "dy-zero":
        assert not any(v.any() for v in want.values())
    if name == "hot":
        assert np.count_nonzero(want["dW"]) == 1 and want["dW"][5, 7] == 6.0 and want["db"][5] == 2.0
    if name == "pair-range":      # rows 31 and 32: the last of range 0, the first of range 1
        assert fr.w1_plan(80, 32, 32)[2][0] == 32 and want["db"][3] == -2.0
    if name == "pair-image":      # rows 39 and 40: the last of image 0, the first of image 1
        assert fc._PH * fc._PW == 40 and want["db"][2] == 9.0


def test_planted_adjoint_case_is_exact():
    want, b = fc.up_reference("ints")
    assert np.array_equal(want["U"], np.round(want["U"])) and want["U"].any() and np.abs(want["U"]).max() < 2 ** 20


@pytest.mark.parametrize("name", ["odd", "c128", "pair-image"])
def test_dgrad_bank_1x1_is_the_forward_bank_of_the_input_gradient(name):
    """conv2d(dy, dgrad_bank_1x1(w)) in float64 is the gradient F.conv2d's autograd gives at the input"""
    from hn_amd import weights
    c = fc.w1_args(name)
    w4 = torch.from_numpy(np.array(c["w"]))[:, None, None, :]                    # the engine's [Cout,1,1,Cin]
    bank = weights.dgrad_bank_1x1(w4)
    assert tuple(bank.shape) == (c["cin"], 1, 1, c["cout"]) and bank.is_contiguous() and bank[3, 0, 0, 5] == c["w"][5, 3]
    a = _nchw(c["a"]).requires_grad_(True)
    (fn.conv2d(a, w4.double().permute(0, 3, 1, 2)) * _nchw(c["dy"])).sum().backward()
    got = fn.conv2d(_nchw(c["dy"]), bank.double().permute(0, 3, 1, 2))
    mag = np.abs(c["dy"].astype(D)) @ np.abs(c["w"].astype(D))
    assert _close(_nhwc(got), _nhwc(a.grad), mag) and _close(_nhwc(got), fc.w1_reference(name)[0]["dC"], mag)
    with pytest.raises(ValueError):
        weights.dgrad_bank_1x1(torch.zeros(4, 3, 3, 4))
    with pytest.raises(ValueError):
        weights.dgrad_bank(w4)                                                   # dgrad_bank itself stays 3x3 only


def _header_symbols(name):
    text = (REPO / "include" / name).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(hn_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_for_gfx950_with_the_new_sources():
    from hn_amd import _lib, build
    assert build.ARCH == "gfx950"
    path = build.build_library()
    assert path.exists() and _lib.load().hn_abi_version() == 36
    kernels = {"conv1x1_wgrad_f32": 2, "upsample_bwd": 1}
    for stem, count in kernels.items():
        text = (build.CSRC / "build" / f"{stem}.resources.txt").read_text()
        assert len(text.splitlines()) == count
        assert text.count("vgpr_spill 0") == count and text.count("sgpr_spill 0") == count and text.count("scratch 0 ") == count, text
        names = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", (build.CSRC / f"{stem}.hip").read_text(), flags=re.S)
        assert len(names) == count and not any(k in n for n in names for k in build.NO_SPILL_KERNELS)   # compiler-scheduled code
    # the new kernels live in the two new files only: the files of section 9u hold what they held
    old = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", (build.CSRC / "conv3x3_wgrad_f32.hip").read_text()
                     + (build.CSRC / "gn_relu_bwd.hip").read_text(), flags=re.S)
    assert len(old) == 7


def test_fpn_header_is_declared_exported_and_bound():
    from hn_amd import _lib
    text, declared = _header_symbols("handnet_hip_train_fpn.h")
    assert declared == sorted(NEW)
    assert '#include "handnet_hip_train.h"' in text and "struct" not in text and "typedef" not in text
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hn_[a-z0-9_]+)", out))
    assert not [s for s in declared if s not in exported]
    assert sorted(_lib.TRAIN_FPN_SIGNATURES) == declared
    lib = _lib.load()
    for name, (res, args) in _lib.TRAIN_FPN_SIGNATURES.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args
    # the pinned tables and headers are what they were
    main = (REPO / "include" / "handnet_hip.h").read_text()
    assert _lib.ABI_VERSION == 36 and re.search(r"#define\s+HN_ABI_VERSION\s+36\b", main)
    assert len(_lib.SIGNATURES) == 136 and len(_lib.TRAIN_SIGNATURES) == 5
    assert not (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES)) & set(_lib.TRAIN_FPN_SIGNATURES)
    train_text, train = _header_symbols("handnet_hip_train.h")
    assert len(train) == 5 and sorted(_lib.TRAIN_SIGNATURES) == train
    assert not any(re.search(r"\b" + s + r"\s*\(", main + train_text) for s in declared)


def test_c_entries_refuse_before_any_launch():
    """the refusals of the three entry points that need no device: every one returns before a launch (the pointers are never
    dereferenced on the host)"""
    from hn_amd import _lib
    lib = _lib.load()
    assert lib.hn_conv1x1_wgrad_ws_bytes(80, 32, 32) == fr.w1_ws_bytes(80, 32, 32)
    assert lib.hn_conv1x1_wgrad_ws_bytes(2310, 32, 32) == fr.w1_ws_bytes(2310, 32, 32)
    assert lib.hn_conv1x1_wgrad_ws_bytes(16 * 4800, 128, 256) == fr.w1_ws_bytes(16 * 4800, 128, 256)
    assert lib.hn_conv1x1_wgrad_ws_bytes(1 << 20, 512, 512) == fr.w1_ws_bytes(1 << 20, 512, 512)
    for bad in ((0, 32, 32), (-1, 32, 32), (1 << 30, 32, 32), (5, 48, 32), (5, 32, 16), (5, 544, 32), (5, 32, 0)):
        assert lib.hn_conv1x1_wgrad_ws_bytes(*bad) == -1, bad
    p, need = 0x10000, fr.w1_ws_bytes(80, 32, 32)
    go = lambda a=p, dy=p, rows=80, cin=32, cout=32, astride=0, dstride=0, dw=p, db=p, ws=p, nbytes=need: \
        lib.hn_conv1x1_wgrad_f32(a, dy, rows, cin, cout, astride, dstride, dw, db, ws, nbytes, None)      # noqa: E731
    for kw in (dict(a=None), dict(dy=None), dict(dw=None), dict(db=None), dict(ws=None)):
        assert go(**kw) != 0 and b"null" in lib.hn_last_error(), kw
    assert go(rows=0) != 0 and b"rows" in lib.hn_last_error()
    assert go(cin=48) != 0 and go(cout=16) != 0 and go(cin=544) != 0
    assert go(nbytes=need - 1) != 0 and b"workspace" in lib.hn_last_error()
    assert go(astride=96) != 0 and b"stride" in lib.hn_last_error()               # breaks the S32 block alignment
    assert go(astride=32) != 0                                                    # below 2 Cin
    assert go(dstride=34) != 0 and b"stride" in lib.hn_last_error()               # breaks the 16-byte loads
    assert go(dstride=16) != 0                                                    # below Cout
    assert go(a=p + 4) != 0 and b"unaligned" in lib.hn_last_error()               # breaks the 8-byte loads
    assert go(dy=p + 8) != 0 and b"unaligned" in lib.hn_last_error()
    up = lambda g=p, n=1, oh=4, ow=6, rh=2, rw=3, c=8, gs=0, os_=0, out=p: \
        lib.hn_upsample_nearest_backward_f32(g, n, oh, ow, rh, rw, c, gs, os_, out, None)                 # noqa: E731
    assert up(g=None) != 0 and b"null" in lib.hn_last_error() and up(out=None) != 0
    assert up(rh=5) != 0 and b"larger" in lib.hn_last_error() and up(rw=7) != 0
    assert up(c=6) != 0 and up(c=0) != 0 and up(n=0) != 0 and up(rh=0) != 0
    assert up(gs=10) != 0 and b"stride" in lib.hn_last_error() and up(os_=4) != 0
    assert up(g=p + 4) != 0 and b"unaligned" in lib.hn_last_error()


def test_front_ends_refuse_without_a_device():
    from hn_amd import ops
    a16 = torch.zeros((1, 3, 4, 2, 2, 32), dtype=torch.float16)
    dy = torch.zeros((1, 3, 4, 32))
    with pytest.raises(TypeError):
        ops.conv1x1_wgrad(torch.zeros((1, 3, 4, 64)), dy)                        # not an S32 map
    with pytest.raises(TypeError):
        ops.conv1x1_wgrad(a16, dy.half())
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv1x1_wgrad(a16, torch.zeros((1, 3, 4, 48)))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv1x1_wgrad(torch.zeros((1, 3, 4, 17, 2, 32), dtype=torch.float16), dy)      # Cin 544
    with pytest.raises(ValueError, match="map size"):
        ops.conv1x1_wgrad(a16, torch.zeros((1, 4, 3, 32)))
    with pytest.raises(ValueError, match="batch size"):
        ops.conv1x1_wgrad(a16, torch.zeros((2, 3, 4, 32)))
    with pytest.raises(ValueError, match="empty"):
        ops.conv1x1_wgrad(a16[:0], dy[:0])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.conv1x1_wgrad(a16, dy)                                               # no CPU fallback
    g = torch.zeros((1, 4, 6, 8))
    with pytest.raises(TypeError):
        ops.upsample_nearest_backward(g.half(), (2, 3))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.upsample_nearest_backward(g[..., :6], (2, 3))
    for size in ((5, 3), (2, 7), (0, 3)):
        with pytest.raises(ValueError, match="no larger"):
            ops.upsample_nearest_backward(g, size)
    with pytest.raises(ValueError, match="out must be"):
        ops.upsample_nearest_backward(g, (2, 3), out=torch.zeros((1, 3, 2, 8)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.upsample_nearest_backward(g, (2, 3))
    with pytest.raises(ValueError, match="per level"):
        ops.conv3x3_dgrad_levels([g], torch.zeros((8, 3, 3, 8)), residuals=[None, None])


def test_the_model_names_the_fpn_parameters():
    """FCOS has the twelve parameters under the reference's names with the reference's shapes, and the opt-ins exist"""
    from fcos_utils.fcos import FCOS
    model = FCOS(num_classes=2, ext=False, min_size=192, max_size=256)
    params = dict(model.named_parameters())
    for i, cin in enumerate((128, 256, 512)):
        assert tuple(params[f"backbone.fpn.inner_blocks.{i}.weight"].shape) == (256, cin, 1, 1)
        assert tuple(params[f"backbone.fpn.layer_blocks.{i}.weight"].shape) == (256, 256, 3, 3)
        assert tuple(params[f"backbone.fpn.inner_blocks.{i}.bias"].shape) == tuple(params[f"backbone.fpn.layer_blocks.{i}.bias"].shape) == (256,)
    assert callable(model.fpn_grads) and callable(model.refresh_fpn)
