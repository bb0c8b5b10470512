"""The GroupNorm statistics rule (tests/gn_ref.py) without a GPU: the rule against torch's float64 group_norm, the two-pass
emulation inside the bound on every case, every mutant outside it on its named case -- so check() is known to be able to fail --
and the rows32 slab through a numpy finalize."""
import numpy as np
import pytest
import torch

import gn_cases as gc
import gn_ref as gr

F = np.float32


@pytest.mark.parametrize("shape", list(gc.AFFINE))
def test_rule_is_torch_group_norm_in_float64(shape):
    groups = gc.AFFINE[shape][4]
    for kind in gc.INPUTS:
        x, gamma, beta = gc.make(shape, kind)
        scale, shift, mean, var = gc.reference(shape, kind)[0]
        xd = torch.from_numpy(x.copy()).double()
        # a CONTIGUOUS NCHW tensor: torch's CPU kernel for channels-last strides forms the variance from sum and sum of squares
        # (5e-10 off at ratio 100), the contiguous one does not
        want = torch.nn.functional.group_norm(xd.permute(0, 3, 1, 2).contiguous(), groups, torch.from_numpy(gamma.copy()).double(),
                                              torch.from_numpy(beta.copy()).double(), eps=float(F(gc.EPS))).permute(0, 2, 3, 1).numpy()
        got = x.astype(np.float64) * scale[:, None, None, :] + shift[:, None, None, :]
        assert np.abs(got - want).max() <= 1e-12, (shape, kind)
        assert mean.shape == var.shape == (x.shape[0], groups) and (var >= 0).all()


@pytest.mark.parametrize("shape", list(gc.AFFINE))
def test_emulation_is_inside_the_bound(shape):
    groups = gc.AFFINE[shape][4]
    worst = {}
    for kind in gc.INPUTS:
        x, gamma, beta = gc.make(shape, kind)
        sc, sh = gr.emulate(x, gamma, beta, groups, gc.EPS)
        worst[kind] = gr.check(sc, sh, x, gamma, beta, groups, gc.EPS, ref=gc.reference(shape, kind))
    print(f"gn emulate {shape}: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_constant_tensor_has_zero_variance_exactly():
    """var = 0: scale = gamma * fl32(1/sqrt(eps)), shift = beta - mean*scale, with every partial sum exact"""
    for shape in gc.AFFINE:
        groups = gc.AFFINE[shape][4]
        x, gamma, beta = gc.make(shape, "constant")
        sc, sh = gr.emulate(x, gamma, beta, groups, gc.EPS)
        rstd = F(1.0 / np.sqrt(float(F(gc.EPS))))
        assert np.array_equal(sc, np.broadcast_to(gamma * rstd, sc.shape)), shape
        assert np.array_equal(sh, beta[None, :] - F(0.75) * sc), shape
        assert (gc.reference(shape, "constant")[0][3] == 0).all()


def test_the_limit_of_the_one_pass_variance_at_the_tower_shape():
    """rstd from E[x^2] - mean^2 with fp32 partials loses accuracy as (mean/std)^2: the emulation's relative error of rstd at
    hw 850, c 256, 32 groups for |mean|/std = 0, 10, 100, 1000 (printed; the emulation stays inside the bound at each)."""
    for ratio, ceiling in zip(gc.LIMIT_RATIOS, (1e-6, 1e-4, 1e-2, 1.0)):
        x, gamma, beta, groups = gc.make_limit(ratio)
        sc, sh = gr.emulate(x, gamma, beta, groups, 0.0)
        want = gr.rule(x, gamma, beta, groups, 0.0)[0]
        rel = float(np.abs(sc / want - 1.0).max())
        r = gr.check(sc, sh, x, gamma, beta, groups, 0.0)
        print(f"gn emulate tower ratio {ratio}: relative error of rstd {rel:.2e}, |err| / bound {r:.4f}")
        assert rel < ceiling        # (orders of magnitude only: a ceiling of (ratio^2 + 1) * 1e-6)


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_every_mutant_fails_on_its_case(mutant):
    fn, form = gr.mutants()[mutant]
    if form == "affine":
        shape, kind = gc.MUTANT_CASE[mutant]
        groups = gc.AFFINE[shape][4]
        x, gamma, beta = gc.make(shape, kind)
        with pytest.raises(AssertionError, match="bound"):
            gr.check(*fn(x, gamma, beta, groups, gc.EPS), x, gamma, beta, groups, gc.EPS, ref=gc.reference(shape, kind))
    else:
        name = gc.MUTANT_CASE[mutant]
        n, hw, c, groups = gc.ROWS32[name]
        for poison in (True, False):        # reading the NaN half, and reading the other image's sums
            slab, _x, gamma, beta = gc.make_rows32(name, poison=poison)
            with pytest.raises(AssertionError, match="non-finite" if poison else "bound"):
                gr.check_rows32(*fn(slab, gamma, beta, n, hw, groups, gc.EPS), slab, gamma, beta, n, hw, groups, gc.EPS)


@pytest.mark.parametrize("name", list(gc.ROWS32))
def test_rows32_slab_through_a_numpy_finalize_reproduces_the_rule(name):
    n, hw, c, groups = gc.ROWS32[name]
    slab, x, gamma, beta = gc.make_rows32(name)
    assert slab.size == -(-n * hw // 32) * (c // 8) * 4
    got = gr.rule_rows32(slab, gamma, beta, n, hw, groups, gc.EPS)
    want = gr.rule(x.reshape(n, hw, c), gamma, beta, groups, gc.EPS)
    # the records are float64 sums rounded to fp32: u on each, (1 + (mean/std)^2) u on the variance, with ratios below 2 here
    assert np.abs(got[0] / want[0] - 1.0).max() < 1e-6
    assert np.abs(got[1] - want[1]).max() < 1e-6 * max(1.0, np.abs(want[1]).max())
    sc, sh = gr.emulate_rows32(slab, gamma, beta, n, hw, groups, gc.EPS)
    ratio = gr.check_rows32(sc, sh, slab, gamma, beta, n, hw, groups, gc.EPS)
    print(f"gn rows32 emulate {name}: max |err| / bound = {ratio:.4f}")
    clean = gc.make_rows32(name, poison=False)[0]
    sc0, sh0 = gr.emulate_rows32(clean, gamma, beta, n, hw, groups, gc.EPS)
    assert np.array_equal(sc, sc0) and np.array_equal(sh, sh0)      # the poisoned halves are not read
    if n * hw % 32 or hw % 32:
        assert np.isnan(slab).any()
