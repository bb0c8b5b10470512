"""The rule of the output convolutions' backward (tests/thin_bwd_ref.py) against torch's float64 autograd through the reference's own
head arithmetic -- F.conv2d(padding=1), ReLU on the column prefix, one weight shared over the levels (fcos_utils/fcos.py:247-264,
362-363) --, the cases' operands, the planted cases' expected values, and the two entry points' declaration and binding.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as fn

import thin_bwd_cases as tc
import thin_bwd_ref as tr

REPO = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", tc.NAMES)
def test_rule_equals_torch_float64_autograd(name):
    """loss = sum_l sum_members <g_l, relu_prefix(conv2d(a_l, w, padding=1))>; its gradients at w, the bias and a_l are the rule
    evaluated on the stored results of that forward, to 1e-12 of the sum of |terms| on every element"""
    c = tc.args(name)
    a = [torch.from_numpy(np.asarray(t, np.float64)).permute(0, 3, 1, 2).requires_grad_(True) for t in c["a"]]
    rng = np.random.default_rng(1)
    loss, params, stored = 0.0, [], []
    for w, relu, _ys, gs in c["members"]:
        wt = torch.from_numpy(np.asarray(w, np.float64)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        b = torch.from_numpy(rng.standard_normal(w.shape[0]) * 0.1).requires_grad_(True)
        ys = []
        for x, g in zip(a, gs):
            y = fn.conv2d(x, wt, b, padding=1)
            y = torch.cat([torch.relu(y[:, :relu]), y[:, relu:]], dim=1)
            ys.append(y.detach().permute(0, 2, 3, 1).numpy())
            loss = loss + (y * torch.from_numpy(np.asarray(g, np.float64)).permute(0, 3, 1, 2)).sum()
        params.append((wt, b))
        stored.append(ys)
    loss.backward()
    members = [(w, relu, ys, gs) for (w, relu, _y, gs), ys in zip(c["members"], stored)]
    want, mag = tr.rule(c["a"], members), tr._sums(c["a"], members, True)
    got = {}
    for m, (wt, b) in enumerate(params):
        got[f"dW{m}"], got[f"db{m}"] = wt.grad.permute(0, 2, 3, 1).numpy(), b.grad.numpy()
    for l, x in enumerate(a):
        got[f"dA{l}"] = x.grad.permute(0, 2, 3, 1).numpy()
    assert set(got) == set(want)
    for key in want:
        assert np.all(np.abs(got[key] - want[key]) <= 1e-12 * mag[key] + 1e-300), key


@pytest.mark.parametrize("name", ["16x16", "relu-all", "three", "five-256"])
def test_random_cases_meet_the_mask_both_ways(name):
    """on the cases' own y: a ReLU column with y exactly 0 (and y < 0) under g != 0, and, where a column is free, y < 0 there"""
    for w, relu, ys, gs in tc.args(name)["members"]:
        assert any(((y[..., :relu] == 0) & (g[..., :relu] != 0)).any() for y, g in zip(ys, gs))
        assert any(((y[..., :relu] < 0) & (g[..., :relu] != 0)).any() for y, g in zip(ys, gs))
        if relu < w.shape[0]:
            assert any((y[..., relu:] < 0).any() for y in ys)


@pytest.mark.parametrize("name", tc.NAMES)
def test_operands_are_exact_in_fp32(name):
    """a = float(hi) + float(lo) is exact in fp32: the kernel's one addition rounds nothing"""
    c = tc.args(name)
    for a, hi, lo in zip(c["a"], c["hi"], c["lo"]):
        exact = hi.astype(np.float64) + lo.astype(np.float64)
        assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), exact)
        assert tr.pack_s32(hi, lo).shape == a.shape[:3] + (a.shape[3] // 32, 2, 32)


@pytest.mark.parametrize("name", list(tc.PLANTED))
def test_planted_cases_expected_values(name):
    """the planted cases' values written down by hand are what the rule gives, and every one of them is an fp32 number"""
    want, _ = tc.reference(name)
    exp = tc.planted_expected(name)
    assert set(exp) == set(want)
    for key in want:
        assert np.array_equal(exp[key], want[key]), key
        assert np.array_equal(want[key].astype(np.float32).astype(np.float64), want[key]), key
    if name == "gzero":
        assert not any(v.any() for v in want.values())
    if name == "mask":
        assert not want["dW0"][:4].any() and not want["db0"][:4].any() and want["db0"][4] > 0 and want["dW0"][4].any()
    if name.startswith("hot-"):
        assert want["dW0"][1].any() and not want["dW0"][0].any() and want["db0"][1] == 3.0


def test_bound_is_never_beyond_the_any_order_bound():
    for name in tc.NAMES:
        c = tc.args(name)
        units, most, k = tr.plan(c["sizes"], c["n"])
        assert most + units - 1 <= k + 9
        _, b = tc.reference(name)
        mag = tr._sums(c["a"], c["members"], True)
        for key in b:
            if not key.startswith("dA"):
                assert np.all(b[key] <= tr.gamma(k + 9) * mag[key] + (k + 9) * 2.0 ** -149)
    assert tr.plan([(72, 352)], 2) == (396, 128, 2 * 72 * 352)          # two tiles per workgroup


def test_entry_points_are_declared_and_bound():
    from hn_amd import _lib
    header = (REPO / "include" / "handnet_hip.h").read_text()
    assert _lib.ABI_VERSION == 36 and re.search(r"#define\s+HN_ABI_VERSION\s+36\b", header)
    for name in ("hn_conv3x3_thin_backward_ws_bytes", "hn_conv3x3_thin_backward_f32"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES
    assert (REPO / "handnet-pipeline_amd" / "csrc" / "conv3x3_thin_bwd.hip").exists()
