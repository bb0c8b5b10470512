"""The rule of the tower layers' backward (tests/tower_bwd_ref.py) against torch's float64 autograd through the reference's own layer
arithmetic -- F.conv2d(padding=1), F.group_norm, relu, parameters shared over the levels (fcos_utils/fcos.py:232-239) --, the
cases' operands and masks, the planted cases' expected values, weights.dgrad_bank, and the new header's declaration, export and
binding.  No GPU."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as fn

import tower_bwd_cases as tc
import tower_bwd_ref as tr

REPO = Path(__file__).resolve().parent.parent
D = np.float64


def _nchw(t):
    return torch.from_numpy(np.asarray(t, D)).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("name", tc.CONV_NAMES)
def test_conv_rule_equals_torch_float64_autograd(name):
    """loss = sum_l <dy_l, conv2d(a_l, w, b, padding=1)>: its gradients at w, b and a_l are the rule, to 1e-12 of the sum of
    |terms| on every element"""
    c = tc.conv_args(name)
    a = [_nchw(t).requires_grad_(True) for t in c["a"]]
    wt = _nchw(c["w"]).requires_grad_(True)
    b = torch.zeros(c["cout"], dtype=torch.float64, requires_grad=True)
    loss = sum((fn.conv2d(x, wt, b, padding=1) * _nchw(dy)).sum() for x, dy in zip(a, c["dy"]))
    loss.backward()
    want, mag = tr.conv_rule(c["a"], c["dy"], c["w"]), tr._conv_sums(c["a"], c["dy"], c["w"], True)
    got = {"dW": wt.grad.permute(0, 2, 3, 1).numpy(), "db": b.grad.numpy()}
    for l, x in enumerate(a):
        got[f"dA{l}"] = x.grad.permute(0, 2, 3, 1).numpy()
    assert set(got) == set(want)
    for key in want:
        assert np.all(np.abs(got[key] - want[key]) <= 1e-12 * mag[key] + 1e-300), key


@pytest.mark.parametrize("name", tc.GN_NAMES)
def test_groupnorm_rule_equals_torch_float64_autograd(name):
    """loss = sum_l <g_l, relu(group_norm(y_l, G, gamma, beta))> in float64: its gradients at y_l, gamma and beta are the rule
    fed with float64 statistics, to 1e-12 of the sum of |terms|"""
    c = tc.gn_args(name, f64_stats=True)
    ys = [_nchw(t).requires_grad_(True) for t in c["y"]]
    gam = torch.from_numpy(c["gamma"].astype(D)).requires_grad_(True)
    beta = torch.from_numpy(c["beta"].astype(D)).requires_grad_(True)
    loss = sum((torch.relu(fn.group_norm(y, c["groups"], gam, beta, eps=tr.EPS)) * _nchw(g)).sum() for y, g in zip(ys, c["g"]))
    loss.backward()
    parts = (c["y"], c["g"], c["tables"], c["stats"], c["gamma"], c["groups"])
    want, mag = tr.gn_rule(*parts), tr._gn_sums(*parts, True)
    got = {"dgamma": gam.grad.numpy(), "dbeta": beta.grad.numpy()}
    for l, y in enumerate(ys):
        got[f"dy{l}"] = y.grad.permute(0, 2, 3, 1).numpy()
    assert set(got) == set(want)
    for key in want:
        assert np.all(np.abs(got[key] - want[key]) <= 1e-12 * mag[key] + 1e-300), key


@pytest.mark.parametrize("name", tc.GN_NAMES)
def test_groupnorm_cases_stay_away_from_the_kink(name):
    """|z| >= 1e-3 on every element, with the fp32 tables and with the float64 ones: the two masks are the same mask, and both
    signs occur"""
    c32, c64 = tc.gn_args(name), tc.gn_args(name, f64_stats=True)
    pos = neg = False
    for z32, z64 in zip(tr.z_of(c32["y"], c32["tables"]), tr.z_of(c64["y"], c64["tables"])):
        assert np.abs(z32).min() >= 1e-3 and np.abs(z64).min() >= 1e-3
        assert np.array_equal(z32 > 0, z64 > 0)
        pos, neg = pos or (z32 > 0).any(), neg or (z32 < 0).any()
    assert pos and neg
    # the fp32 tables are the forward's own: the same sign from the fp32 fma of the kernels
    for y, (sc, sh), z in zip(c32["y"], c32["tables"], tr.z_of(c32["y"], c32["tables"])):
        zf = y.astype(np.float32) * sc[:, None, None] + sh[:, None, None]
        assert np.array_equal(zf > 0, z > 0)
    if c32["masked"]:
        cpg = c32["c"] // c32["groups"]
        assert all((z[..., :cpg] < 0).all() and (z[..., cpg:] > 0).any() for z in tr.z_of(c32["y"], c32["tables"]))
    if c32["gamma0"] is not None:
        assert c32["gamma"][c32["gamma0"]] == 0 and all((z[..., c32["gamma0"]] > 0).all() for z in tr.z_of(c32["y"], c32["tables"]))


@pytest.mark.parametrize("name", tc.CONV_NAMES)
def test_operands_are_exact_in_fp32(name):
    """a = float(hi) + float(lo) is exact in fp32: the kernel's one addition rounds nothing"""
    c = tc.conv_args(name)
    for a, hi, lo in zip(c["a"], c["hi"], c["lo"]):
        exact = hi.astype(D) + lo.astype(D)
        assert a.dtype == np.float32 and np.array_equal(a.astype(D), exact)
        assert tr.pack_s32(hi, lo).shape == a.shape[:3] + (a.shape[3] // 32, 2, 32)


@pytest.mark.parametrize("name", list(tc.CONV_PLANTED))
def test_planted_convolution_cases_expected_values(name):
    """the planted cases' values written down by hand are what the rule gives, and every one of them is an fp32 number"""
    want, _ = tc.conv_reference(name)
    exp = tc.conv_planted_expected(name)
    assert set(exp) == set(want)
    for key in want:
        assert np.array_equal(exp[key], want[key]), key
        assert np.array_equal(want[key].astype(np.float32).astype(D), want[key]), key
    if name == "dy-zero":
        assert not any(v.any() for v in want.values())
    if name.startswith("hot-"):     # ONE element of dW: tap (r, s), column 5, channel 7
        r, s = int(name[4]), int(name[5])
        assert np.count_nonzero(want["dW"]) == 1 and want["dW"][5, r, s, 7] == 6.0 and want["db"][5] == 2.0
    if name == "pair-range":
        assert tr.wgrad_plan(tc.CONV_CASES[name][3], 1, 32, 32)[0] == 27      # every segment its own range
        assert want["db"][3] == -2.0


def test_one_pixel_case_has_only_the_centre_tap():
    want, _ = tc.conv_reference("1x1")
    off = np.ones((3, 3), bool)
    off[1, 1] = False
    assert not want["dW"][:, off].any() and want["dW"][:, 1, 1].all()


def test_planted_groupnorm_cases_are_exact():
    want, _ = tc.gn_reference("gzero")
    assert not any(v.any() for v in want.values())
    want, _ = tc.gn_reference("gint")
    assert np.array_equal(want["dbeta"], np.round(want["dbeta"])) and want["dbeta"].any() and np.abs(want["dbeta"]).max() < 2 ** 20
    want, _ = tc.gn_reference("masked")
    c = tc.gn_args("masked")
    cpg = c["c"] // c["groups"]
    assert not want["dy0"][..., :cpg].any() and want["dy0"][..., cpg:].any()
    assert not want["dgamma"][:cpg].any() and not want["dbeta"][:cpg].any()


def test_bounds_are_never_beyond_the_any_order_bounds():
    for name in tc.CONV_NAMES:
        c = tc.conv_args(name)
        ranges, most, k = tr.wgrad_plan(c["sizes"], c["n"], c["cin"], c["cout"])
        assert most + ranges - 1 <= k + 9
        _, b = tc.conv_reference(name)
        mag = tr._conv_sums(c["a"], c["dy"], c["w"], True)
        for key in b:
            m = 9 * c["cout"] if key.startswith("dA") else k + 9
            assert np.all(b[key] <= tr.gamma(m) * mag[key] + m * 2.0 ** -149), (name, key)
    for name in tc.GN_NAMES:
        c = tc.gn_args(name)
        parts = (c["y"], c["g"], c["tables"], c["stats"], c["gamma"], c["groups"])
        _, b = tc.gn_reference(name)
        mag = tr._gn_sums(*parts, True)
        ms = [h * w * (c["c"] // c["groups"]) for h, w in c["sizes"]]
        for key in b:
            m = (ms[int(key[2:])] if key.startswith("dy") else max(ms)) + 16
            assert np.all(b[key] <= tr.gamma(m) * mag[key] + m * 2.0 ** -149), (name, key)
    assert tr.wgrad_plan([(20, 35)], 2, 32, 32) == (60, 32, 2 * 20 * 35)          # two segments per range
    assert tr.wgrad_plan([(8, 8)], 1, 256, 512)[0] == 8 and tr.wgrad_plan([(16, 16)], 1, 256, 256)[0] == 16


@pytest.mark.parametrize("name", ["2x3", "cross", "pair-level"])
def test_dgrad_bank_is_the_forward_bank_of_the_input_gradient(name):
    """conv2d(dy, dgrad_bank(w), padding=1) in float64 is the rule's dA"""
    from hn_amd import weights
    c = tc.conv_args(name)
    bank = weights.dgrad_bank(torch.from_numpy(np.array(c["w"])))
    assert tuple(bank.shape) == (c["cin"], 3, 3, c["cout"]) and bank.is_contiguous()
    assert bank[3, 0, 2, 5] == c["w"][5, 2, 0, 3]
    want, mag = tc.conv_reference(name)[0], tr._conv_sums(c["a"], c["dy"], c["w"], True)
    for l, dy in enumerate(c["dy"]):
        got = fn.conv2d(_nchw(dy), bank.double().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).numpy()
        assert np.all(np.abs(got - want[f"dA{l}"]) <= 1e-12 * mag[f"dA{l}"] + 1e-300)
    with pytest.raises(ValueError):
        weights.dgrad_bank(torch.zeros(4, 1, 1, 4))


def _train_header_symbols():
    text = (REPO / "include" / "handnet_hip_train.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hn_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_for_gfx950_with_the_new_sources():
    from hn_amd import _lib, build
    assert build.ARCH == "gfx950"
    path = build.build_library()
    assert path.exists() and _lib.load().hn_abi_version() == 36
    for stem in ("conv3x3_wgrad_f32", "gn_relu_bwd"):
        text = (build.CSRC / "build" / f"{stem}.resources.txt").read_text()
        assert "vgpr_spill 0" in text and not re.search(r"vgpr_spill [1-9]", text)
        assert not re.search(r"scratch [1-9]", text), text
    names = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", (build.CSRC / "conv3x3_wgrad_f32.hip").read_text()
                       + (build.CSRC / "gn_relu_bwd.hip").read_text(), flags=re.S)
    assert len(names) == 7 and not any(k in n for n in names for k in build.NO_SPILL_KERNELS)   # compiler-scheduled code


def test_train_header_is_declared_exported_and_bound():
    from hn_amd import _lib
    declared = _train_header_symbols()
    assert declared == sorted(["hn_groupnorm_stats_levels_f32", "hn_groupnorm_relu_backward_f32", "hn_groupnorm_relu_backward_ws_bytes",
                               "hn_conv3x3_wgrad_f32", "hn_conv3x3_wgrad_ws_bytes"])
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hn_[a-z0-9_]+)", out))
    assert not [s for s in declared if s not in exported]
    assert sorted(_lib.TRAIN_SIGNATURES) == declared
    lib = _lib.load()
    for name, (res, args) in _lib.TRAIN_SIGNATURES.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args
    # the inference header and its table are what they were
    main = (REPO / "include" / "handnet_hip.h").read_text()
    assert _lib.ABI_VERSION == 36 and re.search(r"#define\s+HN_ABI_VERSION\s+36\b", main)
    assert len(_lib.SIGNATURES) == 136 and not set(_lib.SIGNATURES) & set(_lib.TRAIN_SIGNATURES)
    assert not any(re.search(r"\b" + s + r"\s*\(", main) for s in declared)


def test_train_structs_have_the_ctypes_layout(tmp_path):
    """sizeof and every offsetof of the new header's structs, from a C probe, against their ctypes mirrors"""
    from hn_amd import _lib
    pairs = {"hn_gn_bwd_levels": _lib.GnBwdLevels, "hn_wgrad_levels": _lib.WgradLevels}
    header = REPO / "include" / "handnet_hip_train.h"
    assert set(re.findall(r"typedef struct (\w+) \{", header.read_text())) == set(pairs)
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "handnet_hip_train.h"', "int main(void) {"]
    for cname, ct in pairs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in ct._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run([gcc, f"-I{REPO / 'include'}", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, ct in pairs.items():
        assert int(got[cname]) == __import__("ctypes").sizeof(ct)
        for f, _ in ct._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(ct, f).offset, (cname, f)
