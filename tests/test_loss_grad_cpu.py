"""The A2J criterion's backward (tests/loss_grad_ref.py) without a GPU: the rule against the imported reference's autograd in
float64 (tests/golden/a2j_loss_grad.npz: full gradients, the gt-NaN mask, directional derivatives at the model's shape), the fp32
emulation of the kernel inside the derived bound on every case and both upstream settings, every mutant of the emulation outside
it, the depth differences' distance from sign's jump, and the surface: the C entry's export, ABI and argument refusals."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_grad_ref as gr
import loss_ref as lr

F = np.float32
IDS = [gr.case_id(c) for c in gr.CASES]


def _to_nhwc(t, k, fh, fw, last):
    """reference layout [B, (w*fh+h)*16+a, J(, 2)] -> NHWC [B, h, w, (a*J+j)(*2)] (tests/test_loss_cpu.py's permutation)"""
    return t.reshape(k, fw, fh, 16, *last).permute(0, 2, 1, 3, *range(4, 4 + len(last))).reshape(k, fh, fw, -1).contiguous().numpy()


def _golden(g, name):
    """(heads in NHWC from the golden's seed, rule kwargs, (k, fh, fw, joints))"""
    k, joints = int(g[f"{name}_k"]), int(g[f"{name}_joints"])
    fh, fw = (int(v) for v in g[f"{name}_shape"])
    gen = torch.Generator().manual_seed(int(g[f"{name}_seed"]))
    n = fh * fw * 16
    cls = torch.randn((k, n, joints), generator=gen) * 2.0
    reg = torch.randn((k, n, joints, 2), generator=gen) * 8.0
    dep = 0.8 + 0.2 * torch.randn((k, n, joints), generator=gen)
    heads = _to_nhwc(cls, k, fh, fw, (joints,)), _to_nhwc(reg, k, fh, fw, (joints, 2)), _to_nhwc(dep, k, fh, fw, (joints,))
    kw = dict(gt=g[f"{name}_gt"], joints=joints, stride=int(g[f"{name}_stride"]), spatial_factor=float(g[f"{name}_spatial_factor"]),
              reg_loss_factor=float(g["reg_loss_factor"]), upstream=tuple(float(x) for x in g[f"{name}_upstream"]))
    return heads, kw, (k, fh, fw, joints)


def _golden_grads(g, name, dims):
    k, fh, fw, joints = dims
    return {key: _to_nhwc(torch.from_numpy(g[f"{name}_{key}"]), k, fh, fw, (joints, 2) if key == "d_reg" else (joints,)) for key in gr.KEYS}


def _directional(g, name, got, dims):
    """the golden's sums from the rule's gradients: ([3, 8] sums of grad * direction, [3] sums of |grad|), NaN entries left out"""
    k, fh, fw, joints = dims
    dots, mags = np.empty((3, int(g["directions"]))), np.empty((3,))
    for h, key in enumerate(gr.KEYS):
        last = (joints, 2) if key == "d_reg" else (joints,)
        ok = ~np.isnan(got[key])
        mags[h] = np.abs(got[key][ok]).sum()
        for d in range(dots.shape[1]):
            v = torch.randn((k, fh * fw * 16, *last), generator=torch.Generator().manual_seed(int(g[f"{name}_dir_seed"]) + 8 * h + d),
                            dtype=torch.float64)
            dots[h, d] = (got[key][ok] * _to_nhwc(v, k, fh, fw, last)[ok]).sum()
    return dots, mags


def test_rule_is_the_references_autograd_full_gradients(golden_dir):
    """1e-12 relative, element by element.  d_reg and d_dep are single products: relative to the element.  d_cls is w times a
    bracket of five products that cancel (its sum over the anchors is 0): both float64 evaluations, autograd's and the rule's,
    round in proportion to the products' magnitudes, so an element is compared relative to w * sum |product| (rule(magnitude=True));
    the plain elementwise figure is printed."""
    g = np.load(golden_dir / "a2j_loss_grad.npz")
    heads, kw, dims = _golden(g, "t")
    got, want, size = gr.rule(*heads, **kw), _golden_grads(g, "t", dims), gr.rule(*heads, **kw, magnitude=True)
    for key in gr.KEYS:
        assert want[key].dtype == np.float64 and not np.isnan(want[key]).any()
        err = np.abs(got[key] - want[key])
        print(f"loss grad golden t {key}: max |err| / |golden| = {(err / np.abs(want[key])).max():.2e}, "
              f"max |err| / magnitude = {(err / size[key]).max():.2e}, max |err| = {err.max():.2e}")
        assert (err <= 1e-12 * size[key]).all(), (key, float((err / size[key]).max()))
        if key != "d_cls":
            assert np.array_equal(size[key], np.abs(got[key]))
    assert kw["upstream"] == (0.7, 1.9)


def test_rule_is_the_references_autograd_with_a_nan_in_gt(golden_dir):
    """the NaN masks are the reference's: the joint's d_cls and one coordinate of its d_reg, nothing of d_dep, no other joint;
    the stored float32 gradients are the rule's rounded (to one float32 ulp), the float64 sums agree to 1e-12"""
    g = np.load(golden_dir / "a2j_loss_grad.npz")
    heads, kw, dims = _golden(g, "n")
    assert np.isnan(kw["gt"]).sum() == 1 and np.isnan(kw["gt"][1, 2, 0])
    got, want = gr.rule(*heads, **kw), _golden_grads(g, "n", dims)
    k, fh, fw, joints = dims
    for key in gr.KEYS:
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
        ok = ~np.isnan(want[key])
        err = np.abs(got[key][ok] - want[key][ok].astype(np.float64))
        assert (err <= 2.0 ** -23 * np.abs(got[key][ok])).all(), key
    nan_cls = np.isnan(got["d_cls"]).reshape(k, fh * fw, 16, joints)
    nan_reg = np.isnan(got["d_reg"]).reshape(k, fh * fw, 16, joints, 2)
    assert nan_cls[1, :, :, 2].all() and nan_cls.sum() == fh * fw * 16
    assert nan_reg[1, :, :, 2, 0].all() and nan_reg.sum() == fh * fw * 16 and not np.isnan(got["d_dep"]).any()
    dots, mags = _directional(g, "n", got, dims)
    assert (np.abs(dots - g["n_dots"]) <= 1e-12 * mags[:, None]).all() and (np.abs(mags - g["n_mags"]) <= 1e-12 * mags).all()


def test_rule_is_the_references_autograd_at_the_models_shape(golden_dir):
    """[11, 11], stride 16, J = 21: eight directional derivatives per head to 1e-12 of the head's sum |grad| (a sum of products
    with unit-variance directions: the scale of its rounding), and that sum itself to 1e-12 relative"""
    g = np.load(golden_dir / "a2j_loss_grad.npz")
    heads, kw, dims = _golden(g, "m")
    assert dims == (2, 11, 11, 21) and kw["stride"] == 16
    dots, mags = _directional(g, "m", gr.rule(*heads, **kw), dims)
    assert (np.abs(mags - g["m_mags"]) <= 1e-12 * mags).all(), (mags, g["m_mags"])
    assert (np.abs(dots - g["m_dots"]) <= 1e-12 * mags[:, None]).all(), np.abs(dots - g["m_dots"]).max()


def test_the_cases_and_the_depth_condition():
    assert [c.name for c in lc.CASES] == [n for n, u in gr.CASES if u == 0] and len(gr.CASES) == 30
    assert gr.UPSTREAMS == ((1.0, 1.0), (0.7, 1.9))
    assert set(gr.MUTANT_CASE) == set(gr.MUTANTS) and len(gr.MUTANTS) == 9
    for c in lc.CASES:
        margin = gr.conditions(c.name)
        print(f"loss grad case {c.name}: min |gt_d - Ed| / its difference bound = {margin:.1f}")
        assert margin > gr.SIGN_GUARD


@pytest.mark.parametrize("case", gr.CASES, ids=IDS)
def test_emulation_is_inside_the_bound(case):
    detail = {}
    out = gr.emulate(*lc.heads(case[0]), **gr.kwargs(case))
    ratio = gr.check(out, gr.reference(case), detail=detail)
    print(f"loss grad emulate {gr.case_id(case)}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    # the first two phases are the loss form's: the same keypoints bit for bit
    if case[1] == 0:
        assert np.array_equal(out["uvd"], lr.emulate(*lc.heads(case[0]), **lc.kwargs(case[0]))["uvd"])


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_every_mutant_fails_on_its_case(mutant):
    name, u = gr.MUTANT_CASE[mutant]
    case = (name, u)
    with pytest.raises(AssertionError, match="bound"):
        gr.check(gr.mutants()[mutant](*lc.heads(name), **gr.kwargs(case)), gr.reference(case))


def test_valid_rows_and_linearity_in_the_rule():
    want, b = gr.reference(("3x5x7-valid", 0))
    full = gr.rule(*lc.heads("3x5x7-valid"), **dict(gr.kwargs(("3x5x7-valid", 0)), valid=None))
    for key in gr.KEYS:
        assert not want[key][1].any() and not b[key][1].any()
        # n = 2 against n = 3 (float64 roundings apart; d_cls's bracket cancels, hence the absolute part)
        assert np.allclose(want[key][[0, 2]] * 2.0, full[key][[0, 2]] * 3.0, rtol=1e-12, atol=1e-15 * np.abs(full[key]).max())
    two = gr.rule(*lc.heads("3x5x7"), **dict(gr.kwargs(("3x5x7", 0)), valid=np.array([1, 2, 1], np.int32)))
    assert all(np.isnan(two[key][1]).all() and np.isfinite(two[key][[0, 2]]).all() for key in gr.KEYS)
    # the gradient is linear in (wa, wr): (0.7, 1.9) = 0.7 * (1, 0) + 1.9 * (0, 1)
    kw = gr.kwargs(("5x3x6", 1))
    a, r = (gr.rule(*lc.heads("5x3x6"), **dict(kw, upstream=u)) for u in ((1.0, 0.0), (0.0, 1.0)))
    both = gr.rule(*lc.heads("5x3x6"), **kw)
    for key in gr.KEYS:
        assert np.allclose(both[key], 0.7 * a[key] + 1.9 * r[key], rtol=1e-12, atol=1e-300)
    assert not a["d_reg"].any() and not a["d_dep"].any() and a["d_cls"].any()


def test_the_closed_forms_sums_over_the_anchors():
    """the sum over the anchors of d_cls is 0 (a softmax's gradient), and the sum of d_dep is the coefficient gd (the weights sum
    to 1): |gd| = wr R / n / J"""
    name = "3x5x7"
    kw = gr.kwargs((name, 1))
    got = gr.rule(*lc.heads(name), **kw)
    a = lc.agg(name)
    k, cells = a.k, 15
    d_cls = got["d_cls"].reshape(k, cells * 16, a.joints)
    assert (np.abs(d_cls.sum(axis=1)) <= 1e-14 * np.abs(d_cls).sum(axis=1)).all()
    d_dep = got["d_dep"].reshape(k, cells * 16, a.joints).sum(axis=1)
    assert np.allclose(np.abs(d_dep), 1.9 * 3.0 / k / a.joints, rtol=1e-13, atol=0)


def test_check_refuses_a_nan_and_a_wrong_type():
    case = ("3x5x7", 0)
    out = gr.emulate(*lc.heads(case[0]), **gr.kwargs(case))
    bad = {k: v.copy() for k, v in out.items()}
    bad["d_cls"][1, 2, 0, 5] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        gr.check(bad, gr.reference(case))
    with pytest.raises(AssertionError):
        gr.check(dict(out, d_dep=out["d_dep"].astype(np.float64)), gr.reference(case))
    nan_case = ("3x5x7-gt-nan", 0)
    fine = gr.emulate(*lc.heads(nan_case[0]), **gr.kwargs(nan_case))
    gr.check(fine, gr.reference(nan_case))
    fine["d_reg"][np.isnan(fine["d_reg"])] = 0.0                    # numbers where the rule has NaN
    with pytest.raises(AssertionError, match="NaN"):
        gr.check(fine, gr.reference(nan_case))


def test_the_c_entry_is_exported_under_abi_36_and_refuses_bad_arguments():
    """hn_a2j_loss_grad_f32: declared, bound and exported; the ABI stays 36; null pointers, joints outside [1, 64], fh * fw == 0, a
    crop slice of 2^31 elements and unaligned outputs are refused with status 1 and a message before any launch (the pointers are
    never followed: 16 stands for any aligned address)."""
    import re

    from hn_amd import _lib, build
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    proto = re.search(r"int\s+hn_a2j_loss_grad_f32\s*\(([^;]*)\)\s*;", text)
    assert proto and "hn_a2j_loss_grad_f32" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["hn_a2j_loss_grad_f32"]
    assert res is C.c_int and len(args) == len(proto.group(1).split(",")) == 19
    assert "#define HN_ABI_VERSION 36" in text
    p = 16

    def call(cls=p, gt=p, d_cls=p, d_reg=p, d_dep=p, k=1, fh=2, fw=2, joints=21, stride=16, upstream=None, uvd=None, terms=None):
        return lib.hn_a2j_loss_grad_f32(cls, p, p, None, gt, k, fh, fw, joints, stride, 0.5, 3.0, upstream, d_cls, d_reg, d_dep, uvd,
                                        terms, None)
    for kw, word in ((dict(cls=None), b"null pointer"), (dict(gt=None), b"null pointer"), (dict(d_cls=None), b"null pointer"),
                     (dict(d_reg=None), b"null pointer"), (dict(d_dep=None), b"null pointer"), (dict(joints=0), b"[1, 64]"),
                     (dict(joints=65), b"[1, 64]"), (dict(fh=0), b"fh * fw"), (dict(fw=0), b"fh * fw"), (dict(k=-1), b"bad dims"),
                     (dict(stride=0), b"bad dims"), (dict(fh=1 << 10, fw=1 << 10, joints=64), b"2^31"),
                     (dict(d_reg=p + 4), b"8-byte aligned"), (dict(terms=p + 8), b"16-byte aligned")):
        assert call(**kw) == 1 and word in lib.hn_last_error(), (kw, lib.hn_last_error())
    assert call(k=0) == 0                                          # no crop: nothing is launched
    rows = (build.CSRC / "build" / "a2j_ops.resources.txt").read_text().splitlines()
    for kernel in ("a2j_aggregate_kernel", "a2j_loss_aggregate_kernel", "a2j_loss_grad_kernel"):   # the three of the one sweep
        row = [r for r in rows if kernel in r]
        assert len(row) == 1 and " vgpr_spill 0 " in row[0] and " scratch 0 " in row[0], row
        assert kernel in build.NO_SCRATCH_KERNELS


def test_the_python_surface():
    """ops.a2j_loss_grad carries ops.a2j_loss's arguments and refusals (host tensors are refused like a2j_loss refuses them: there
    is no CPU fallback; the shape and dtype refusals need device tensors and are in tests/test_loss_grad_gpu.py); A2JCriterion is a
    parameter-free module that refuses anything but contiguous fp32 device tensors; the training-side hooks keep raising."""
    from a2j.a2j import A2JModel, A2JModelLightning
    from hn_amd import a2j_engine, criterion, ops
    sig = inspect.signature(ops.a2j_loss_grad)
    assert list(sig.parameters) == ["cls", "reg", "dep", "gt", "joints", "stride", "spatial_factor", "reg_loss_factor", "valid",
                                    "upstream", "want_forward"]
    want = inspect.signature(ops.a2j_loss).parameters
    for name in ("joints", "stride", "spatial_factor", "reg_loss_factor", "valid"):
        assert sig.parameters[name].default == want[name].default
    assert sig.parameters["upstream"].default is None and sig.parameters["want_forward"].default is False
    heads = torch.zeros((1, 2, 2, 16 * 21)), torch.zeros((1, 2, 2, 32 * 21)), torch.zeros((1, 2, 2, 16 * 21))
    for fn in (ops.a2j_loss, ops.a2j_loss_grad):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(*heads, torch.zeros((1, 21, 3)))
    crit = criterion.A2JCriterion(joints=21, stride=16, spatial_factor=0.25, reg_loss_factor=2.0)
    assert isinstance(crit, torch.nn.Module) and not list(crit.parameters()) and not list(crit.buffers())
    assert (crit.joints, crit.stride, crit.spatial_factor, crit.reg_loss_factor) == (21, 16, 0.25, 2.0)
    assert "channels_last" in criterion.A2JCriterion.__doc__ and "permute(0, 2, 3, 1)" in criterion.A2JCriterion.__doc__
    with pytest.raises(ValueError, match="contiguous fp32"):
        crit(*heads, torch.zeros((1, 21, 3)))
    assert callable(A2JModel.head_grads) and callable(a2j_engine.A2JEngine.head_grads)
    net = A2JModelLightning()
    for hook in (net.training_step, net.configure_optimizers, net.validation_step):
        with pytest.raises(NotImplementedError):
            hook(None, 0)
