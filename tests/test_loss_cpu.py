"""The A2J criterion's rule (tests/loss_ref.py) without a GPU: the rule against the imported reference's A2J_loss in float64
(tests/golden/a2j_loss.npz, whole batch and sample by sample, on a square and a non-square map), the fp32 emulation of the two
kernels inside the derived bound on every case, every mutant of the emulation outside it -- so check() is known to be able to
fail --, the C entry's argument refusals, and the training-side hooks that keep raising."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_ref as lr

NAMES = [c.name for c in lc.CASES]


def _golden_heads(g, name):
    """the golden's seeded heads (tests/golden/make_golden_loss.py heads()) in the NHWC layout, through the permutation of
    tests/test_agg_cpu.py::to_nhwc for an fh x fw map"""
    k, joints = int(g[f"{name}_k"]), int(g[f"{name}_joints"])
    fh, fw = (int(v) for v in g[f"{name}_shape"])
    gen = torch.Generator().manual_seed(int(g[f"{name}_seed"]))
    n = fh * fw * 16
    cls = torch.randn((k, n, joints), generator=gen) * 2.0
    reg = torch.randn((k, n, joints, 2), generator=gen) * 8.0
    dep = 0.8 + 0.2 * torch.randn((k, n, joints), generator=gen)

    def to_nhwc(t, last):   # reference layout [B, (w*fh+h)*16+a, J] -> NHWC [B, h, w, a*J+j]
        return t.reshape(k, fw, fh, 16, *last).permute(0, 2, 1, 3, *range(4, 4 + len(last))).reshape(k, fh, fw, -1).contiguous().numpy()
    return to_nhwc(cls, (joints,)), to_nhwc(reg, (joints, 2)), to_nhwc(dep, (joints,))


@pytest.mark.parametrize("name", ["a", "b"])
def test_rule_is_the_references_criterion(golden_dir, name):
    g = np.load(golden_dir / "a2j_loss.npz")
    heads = _golden_heads(g, name)
    kw = dict(gt=g[f"{name}_gt"], joints=int(g[f"{name}_joints"]), stride=int(g[f"{name}_stride"]),
              spatial_factor=float(g[f"{name}_spatial_factor"]))
    got = lr.rule(*heads, **kw)
    want_b, want_s = g[f"{name}_f64_batch"], g[f"{name}_f64_sample"]
    assert (np.abs(got["batch"][:2] - want_b) <= 1e-12 * np.abs(want_b)).all(), (got["batch"][:2], want_b)
    assert (np.abs(got["sample"] - want_s) <= 1e-12 * np.abs(want_s)).all()
    assert got["batch"][2] == got["batch"][1] * 3.0 and got["batch"][3] == got["batch"][0] + got["batch"][2]
    # the reference's own float32 run, for the record only (its additions are torch's, not the kernels': the bound is not its bound)
    b = lr.bound(*heads, **kw)
    print(f"golden {name}: the reference's float32 run, max |err| / bound = {(np.abs(g[f'{name}_f32_sample'] - want_s) / b['sample']).max():.4f}")
    # ... and sample by sample == the batch of one
    for i in range(int(g[f"{name}_k"])):
        one = lr.rule(*(t[i:i + 1] for t in heads), **dict(kw, gt=kw["gt"][i:i + 1]))
        assert np.array_equal(one["sample"][0], got["sample"][i])


def test_the_cases_meet_their_conditions():
    assert [c.name for c in lc.CASES[:12]] == ["11x11x21", "11x11x21-peaked-flat", "1x1x1", "3x5x7", "5x3x6", "9x14x5", "1x127x5",
                                               "23x31x64", "6x6x63", "4x7x21-stride8", "11x11x21-cls30", "11x11x21-big"]
    assert {c.special for c in lc.CASES} >= {"gt-nan", "valid"} and any(c.spatial_factor == 0.1 for c in lc.CASES)
    for name in NAMES:
        gap, below = lc.conditions(name)
        print(f"loss case {name}: nearest uv difference to the knee {gap:.4f}, Lr share below the knee {below:.3f}")
    assert set(lc.MUTANT_CASE) == set(lr.MUTANTS)
    assert np.isnan(lc.make("3x5x7-gt-nan")[0]).sum() == 1


@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_inside_the_bound(name):
    detail = {}
    ratio = lr.check(lr.emulate(*lc.heads(name), **lc.kwargs(name)), lc.reference(name), detail=detail)
    print(f"loss emulate {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", lr.MUTANTS)
def test_every_mutant_fails_on_its_case(mutant):
    name = lc.MUTANT_CASE[mutant]
    with pytest.raises(AssertionError, match="bound"):
        lr.check(lr.mutants()[mutant](*lc.heads(name), **lc.kwargs(name)), lc.reference(name))


def test_nan_and_valid_rows_in_the_rule():
    want, _ = lc.reference("3x5x7-gt-nan")
    assert np.isnan(want["batch"]).all() and np.isnan(want["sample"][1]).all() and not np.isnan(want["sample"][[0, 2]]).any()
    assert np.isnan(want["terms"]).sum() == 3                      # La_h, Lr_h and the squared u difference of that joint
    want, b = lc.reference("3x5x7-valid")
    full = lr.rule(*lc.heads("3x5x7-valid"), **dict(lc.kwargs("3x5x7-valid"), valid=None))
    assert not want["terms"][1].any() and not b["terms"][1].any() and np.array_equal(want["sample"][[0, 2]], full["sample"][[0, 2]])
    assert want["batch"][0] == (full["sample"][0, 0] + full["sample"][2, 0]) / 2.0
    none = lr.rule(*lc.heads("3x5x7"), **dict(lc.kwargs("3x5x7"), valid=np.zeros((3,), np.int32)))
    assert np.isnan(none["batch"]).all()


def test_check_refuses_a_nan_and_a_wrong_type():
    name = "3x5x7"
    out = lr.emulate(*lc.heads(name), **lc.kwargs(name))
    bad = {k: v.copy() for k, v in out.items()}
    bad["terms"][1, 2, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        lr.check(bad, lc.reference(name))
    with pytest.raises(AssertionError):
        lr.check(dict(out, sample=out["sample"].astype(np.float64)), lc.reference(name))
    nan_case = "3x5x7-gt-nan"
    fine = lr.emulate(*lc.heads(nan_case), **lc.kwargs(nan_case))
    fine["batch"][4] = 1.0                                         # a number where the rule has NaN
    with pytest.raises(AssertionError, match="NaN"):
        lr.check(fine, lc.reference(nan_case))


def test_argument_errors_do_not_need_a_gpu():
    """hn_a2j_aggregate_loss_f32 refuses null pointers, joints outside [1, 64] and fh * fw == 0 with status 1 and a message,
    before any launch (the pointers are never followed: 16 stands for any aligned address)."""
    from hn_amd import _lib
    lib = _lib.load()
    p = 16

    def call(cls=p, gt=p, terms=p, batch=p, k=1, fh=2, fw=2, joints=21, box=None, img=None):
        return lib.hn_a2j_aggregate_loss_f32(cls, p, p, None, gt, k, fh, fw, joints, 16, 0.5, 3.0, box, 176.0, 176.0, None, None, p,
                                             img, None, terms, p, batch, None)
    for kw, word in ((dict(cls=None), b"null pointer"), (dict(gt=None), b"null pointer"), (dict(terms=None), b"null pointer"),
                     (dict(batch=None), b"null pointer"), (dict(joints=0), b"[1, 64]"), (dict(joints=65), b"[1, 64]"),
                     (dict(fh=0), b"fh * fw"), (dict(fw=0), b"fh * fw"), (dict(k=-1), b"bad dims"),
                     (dict(box=p), b"no converted output"), (dict(img=p), b"need boxes")):
        assert call(**kw) == 1 and word in lib.hn_last_error(), (kw, lib.hn_last_error())
    assert call(k=0) == 0                                          # no crop: nothing is launched
    assert C.sizeof(C.c_void_p) == 8


def test_training_side_hooks_keep_raising_without_the_opt_in():
    from a2j.a2j import A2JModelLightning
    net = A2JModelLightning()
    for hook in (net.validation_step, net.training_step):
        with pytest.raises(NotImplementedError):
            hook(None, 0)
    assert net.device_loss() is net and net.device_loss(False) is net
    with pytest.raises(NotImplementedError):
        net.validation_step(None, 0)
    net.device_loss()
    for hook in (net.training_step, net.configure_optimizers):     # these raise either way
        with pytest.raises(NotImplementedError):
            hook(None, 0)
