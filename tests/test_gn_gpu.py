"""hn_groupnorm_affine_f32 and hn_groupnorm_finalize_rows32(_levels) against the float64 rule (tests/gn_ref.py) at the shapes
where the reduction tree, the chunk tail and the write loop change (tests/gn_cases.py).  The assertion is |err| <= the derived
worst-case bound and nothing tighter; the ratios are printed and DESIGN.md section 5 holds the table measured on the MI355X."""
import numpy as np
import pytest
import torch

import gn_cases as gc
import gn_ref as gr

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
GUARD = 16


def _d(t):
    return torch.from_numpy(t.copy()).cuda()


@pytest.mark.parametrize("shape", list(gc.AFFINE))
def test_groupnorm_affine_is_inside_the_bound(shape):
    """the ladder of |mean| / std x scale, images and groups that differ, the constant tensor; then one run into pre-allocated
    scratch / scale / shift of exactly the needed size, cut out of a sentinel-filled arena whose rest must come back untouched"""
    from hn_amd import ops
    n, h, w, c, groups = gc.AFFINE[shape]
    worst = {}
    for kind in gc.INPUTS:
        x, gamma, beta = gc.make(shape, kind)
        sc, sh = ops.groupnorm_affine(_d(x), _d(gamma), _d(beta), groups=groups, eps=gc.EPS)
        assert sc.shape == sh.shape == (n, c)
        sc, sh = sc.cpu().numpy(), sh.cpu().numpy()
        if kind == "constant":      # var = 0 exactly (every partial sum is exact): the bound is void there, the values are known
            rstd = np.float32(1.0 / np.sqrt(float(np.float32(gc.EPS))))
            assert np.array_equal(sc, np.broadcast_to(gamma * rstd, sc.shape)), shape
            want_sh = beta.astype(np.float64)[None, :] - 0.75 * sc.astype(np.float64)
            assert np.abs(sh - want_sh).max() <= 2 * gr.U * np.abs(0.75 * sc).max() + gr.U * np.abs(want_sh).max(), shape
        worst[kind] = gr.check(sc, sh, x, gamma, beta, groups, gc.EPS, ref=gc.reference(shape, kind))
    print(f"gn gpu {shape}: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
    # pre-allocated buffers of exactly the needed size
    kind = "groups"
    x, gamma, beta = gc.make(shape, kind)
    need = n * -(-h * w // 64) * groups * 2
    arena = torch.full((need + 2 * n * c + 4 * GUARD,), SENTINEL, device="cuda")
    cuts, at = [], GUARD
    for size in (need, n * c, n * c):
        cuts.append((at, at + size))
        at += size + GUARD
    scratch = arena[cuts[0][0]:cuts[0][1]]
    scale, shift = (arena[a:b].view(n, c) for a, b in cuts[1:])
    sc, sh = ops.groupnorm_affine(_d(x), _d(gamma), _d(beta), groups=groups, eps=gc.EPS, scratch=scratch, scale=scale, shift=shift)
    assert sc.data_ptr() == scale.data_ptr() and sh.data_ptr() == shift.data_ptr()
    plain = ops.groupnorm_affine(_d(x), _d(gamma), _d(beta), groups=groups, eps=gc.EPS)
    assert torch.equal(sc, plain[0]) and torch.equal(sh, plain[1])
    assert not bool((scratch == SENTINEL).any())        # the given scratch was used, all of it
    keep = torch.ones(arena.numel(), dtype=torch.bool, device="cuda")
    for a, b in cuts:
        keep[a:b] = False
    assert bool((arena[keep] == SENTINEL).all())


@pytest.mark.parametrize("name", list(gc.ROWS32))
def test_finalize_rows32_is_inside_the_bound_and_reads_no_poisoned_half(name):
    """the slab of tests/gn_ref.pack_rows32 with NaN in every half the kernel must not read: the result is finite (check()
    compares the masks) and within a few u of the slab's own float64 statistics; the levels launch gets the same slab and a
    second level and must return the same bits"""
    from hn_amd import ops
    n, hw, c, groups = gc.ROWS32[name]
    slab, _x, gamma, beta = gc.make_rows32(name)
    sc, sh = ops.groupnorm_finalize_rows32(_d(slab), _d(gamma), _d(beta), n, hw, groups=groups, eps=gc.EPS)
    ratio = gr.check_rows32(sc.cpu().numpy(), sh.cpu().numpy(), slab, gamma, beta, n, hw, groups, gc.EPS)
    hw2 = hw + 31
    slab2 = gc.make_rows32(name, hw_extra=31)[0]
    (lsc, lsh), (lsc2, lsh2) = ops.groupnorm_finalize_rows32_levels([_d(slab), _d(slab2)], _d(gamma), _d(beta), n, [hw, hw2],
                                                                    groups=groups, eps=gc.EPS)
    assert torch.equal(lsc, sc) and torch.equal(lsh, sh)
    ratio2 = gr.check_rows32(lsc2.cpu().numpy(), lsh2.cpu().numpy(), slab2, gamma, beta, n, hw2, groups, gc.EPS)
    print(f"gn rows32 gpu {name}: max |err| / bound = {ratio:.4f}, second level (hw {hw2}) {ratio2:.4f}")
    assert max(ratio, ratio2) <= 1.0


def test_the_limit_of_the_one_pass_variance_at_the_tower_shape():
    """the kernel's relative error of rstd at hw 850, c 256, 32 groups, eps = 0 for |mean|/std = 0, 10, 100, 1000: PRINTED (the
    figures of DESIGN.md section 5, next to test_gn_cpu.py's for the emulation); asserted is check() alone"""
    from hn_amd import ops
    for ratio in gc.LIMIT_RATIOS:
        x, gamma, beta, groups = gc.make_limit(ratio)
        sc, sh = ops.groupnorm_affine(_d(x), _d(gamma), _d(beta), groups=groups, eps=0.0)
        sc, sh = sc.cpu().numpy(), sh.cpu().numpy()
        want = gr.rule(x, gamma, beta, groups, 0.0)[0]
        rel = float(np.abs(sc / want - 1.0).max())
        r = gr.check(sc, sh, x, gamma, beta, groups, 0.0)
        print(f"gn gpu tower ratio {ratio}: relative error of rstd {rel:.2e}, |err| / bound {r:.4f}")


def test_refusals_launch_nothing():
    """c/4 not a divisor of 256, 6 channels per group, 512 groups, hw = 31 for rows32: refused before any launch (the
    sentinel-filled tables come back untouched).  512 groups are refused by `c <= 1024`: with at least 4 channels per group no
    shape reaches the library's own `groups <= 256` check, so that line cannot be tested by itself."""
    from hn_amd import ops
    for n, hw, c, groups in ((1, 64, 48, 4), (1, 64, 24, 4), (1, 8, 2048, 512)):
        scale, shift = (torch.full((n, c), SENTINEL, device="cuda") for _ in range(2))
        with pytest.raises(RuntimeError):
            ops.groupnorm_affine(torch.ones((n, hw, 1, c), device="cuda"), torch.ones(c, device="cuda"), torch.zeros(c, device="cuda"),
                                 groups=groups, scale=scale, shift=shift)
        torch.cuda.synchronize()
        assert bool((scale == SENTINEL).all()) and bool((shift == SENTINEL).all()), (c, groups)
    n, hw, c, groups = 2, 31, 64, 8
    scale, shift = (torch.full((n, c), SENTINEL, device="cuda") for _ in range(2))
    with pytest.raises(RuntimeError):
        ops.groupnorm_finalize_rows32(torch.zeros((4 * (c // 8) * 4,), device="cuda"), torch.ones(c, device="cuda"),
                                      torch.zeros(c, device="cuda"), n, hw, groups=groups, scale=scale, shift=shift)
    torch.cuda.synchronize()
    assert bool((scale == SENTINEL).all()) and bool((shift == SENTINEL).all())
