"""The aggregation rule (tests/agg_ref.py) without a GPU: the rule against the oracle's post_process in float64 (which ties it
to the reference's anchor order independently of the kernel), the fp32 emulation inside the bound on every case, and every
mutant of the emulation outside it -- so check() is known to be able to fail."""
import numpy as np
import pytest
import torch

import agg_cases as ac
import agg_ref as ar

NAMES = [c.name for c in ac.CASES]


def _oracle(cls, reg, dep, joints, stride):
    """oracle.a2j_ref.post_process in float64 on the NHWC heads, through the reference's own permutation"""
    from oracle import a2j_ref
    fh, fw = cls.shape[1:3]
    nchw = [torch.from_numpy(t.copy()).double().permute(0, 3, 1, 2) for t in (cls, reg, dep)]
    c1, r1, d1 = a2j_ref.heads_to_reference_layout(*nchw, joints=joints)
    return a2j_ref.post_process(c1, r1, d1, a2j_ref.all_anchors(shape=(fh, fw), stride=stride).double()).numpy()


def test_geometry_is_launch_aggregates():
    for name, want in ac.GEOMETRY.items():
        assert ar.geometry(ac.BY_NAME[name].joints) == want, name
    assert {c.k for c in ac.CASES} <= {2, 3}


@pytest.mark.parametrize("name", NAMES)
def test_rule_is_the_oracles_post_process(name):
    c = ac.BY_NAME[name]
    want = _oracle(*ac.make(name), c.joints, c.stride)
    got = ac.reference(name)[0]
    assert got.shape == (c.k, c.joints, 3)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_rule_on_the_golden_post_process(golden_dir):
    """the inputs of test_aggregate_matches_reference_post_process, within that test's 2e-4 of the imported reference's output"""
    g = np.load(golden_dir / "a2j_post_process.npz")
    gen = torch.Generator().manual_seed(int(g["seed"]))
    cls = torch.randn((4, 1936, 21), generator=gen) * 2.0
    reg = torch.randn((4, 1936, 21, 2), generator=gen) * 8.0
    dep = 0.8 + 0.2 * torch.randn((4, 1936, 21), generator=gen)
    cls[3, 100, :] += 30.0
    cls[2] *= 0.0

    def to_nhwc(t, last):   # reference layout [B, (w*11+h)*16+a, J] -> NHWC [B, h, w, a*J+j]
        return t.reshape(4, 11, 11, 16, *last).permute(0, 2, 1, 3, *range(4, 4 + len(last))).reshape(4, 11, 11, -1).contiguous().numpy()
    out = ar.rule(to_nhwc(cls, (21,)), to_nhwc(reg, (21, 2)), to_nhwc(dep, (21,)), 21, 16)
    assert np.abs(out - g["out"]).max() < 2e-4


@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_inside_the_bound(name):
    c = ac.BY_NAME[name]
    heads = ac.make(name)
    ratio = ar.check(ar.emulate(*heads, c.joints, c.stride), *heads, c.joints, c.stride, ref=ac.reference(name))
    print(f"agg emulate {name}: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_every_mutant_fails_on_its_case(mutant):
    fn = ar.mutants()[mutant]
    name = ac.MUTANT_CASE[mutant]
    c = ac.BY_NAME[name]
    heads = ac.make(name)
    with pytest.raises(AssertionError, match="bound"):
        ar.check(fn(*heads, c.joints, c.stride), *heads, c.joints, c.stride, ref=ac.reference(name))


def test_div_fh_hides_on_a_square_map():
    """why the table holds non-square maps: decomposing the cell index with fh instead of fw is invisible at 11 x 11"""
    c = ac.BY_NAME["11x11x21"]
    heads = ac.make(c.name)
    assert np.array_equal(ar.emulate(*heads, c.joints, c.stride, mutant="div_fh"), ar.emulate(*heads, c.joints, c.stride))


def test_check_refuses_a_nan_and_a_wrong_type():
    c = ac.BY_NAME["3x5x7"]
    heads = ac.make(c.name)
    out = ar.emulate(*heads, c.joints, c.stride)
    bad = out.copy()
    bad[1, 2, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        ar.check(bad, *heads, c.joints, c.stride)
    with pytest.raises(AssertionError):
        ar.check(out.astype(np.float64), *heads, c.joints, c.stride)
