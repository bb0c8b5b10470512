"""The candidate and ext-gather rules (tests/cand_ref.py) without a GPU: the guards of the case generator, the rules against the
reference's chain of torch operations in float64 (fcos_utils/fcos.py:591-628 and :299-320; anchors and decode as
anchor_utils.py:82-132 and det_utils.py:266-294 state them), the fp32 emulations against the rules, and every mutant of the
emulations failing on its named case with the property it breaks -- so the checks are known to be able to fail."""
import numpy as np
import pytest
import torch

import cand_cases as cc
import cand_ref as cr

NAMES = [c.name for c in cc.CASES]


def _args(name):
    c = cc.BY_NAME[name]
    cls_lr, reg_ctr, _ = cc.make(name)
    return (cls_lr, reg_ctr, c.strides, c.num_classes, c.thresh), dict(cap=c.cap or None)


@pytest.mark.parametrize("name", NAMES)
def test_guards_hold_and_plants_survive(name):
    c = cc.BY_NAME[name]
    cls_lr, reg_ctr, planted = cc.make(name)
    assert not cr.guards(cls_lr, reg_ctr, c.num_classes, c.thresh).any()          # nothing is left out of a comparison
    cls, reg, sizes = cr.flatten(cls_lr, reg_ctr)
    assert tuple(tuple(s) for s in sizes) == c.sizes and cls.shape == (c.n, cc.points(c), c.num_classes + 2)
    cls2, reg2 = cls.copy(), reg.copy()
    cc._plant(c, cls2, reg2, [])
    assert np.array_equal(cls2, cls) and np.array_equal(reg2, reg) and (len(planted) > 0) == bool(c.special and c.special != ("neg-reg",))
    ref = cc.reference(name)
    modes = c.images or ("mixed",) * c.n
    for r, mode in zip(ref, modes):
        assert mode != "none" or r["total"] == 0
        assert mode != "all" or r["total"] == cc.points(c)
        assert mode != "mixed" or 0 < r["total"] and (c.thresh < 0) == (r["total"] == cc.points(c))
        assert r["count"] == min(r["total"], c.cap or cc.points(c))
    if c.cap:
        assert ref[0]["total"] > c.cap and ref[2]["total"] > c.cap and ref[1]["total"] == 0
    if "ties" in c.special:
        assert {int(ref[0]["label"][list(ref[0]["point"]).index(p)]) for p in planted[:4]} == {0, 1}


def test_the_table_holds_every_loop_bound():
    pts = {c.name: cc.points(c) for c in cc.CASES}
    assert [pts[f"P{p}"] for p in (1023, 1024, 1025, 4095, 4096, 4097, 8193)] == [1023, 1024, 1025, 4095, 4096, 4097, 8193]
    for name in ("P1023", "P1024", "P1025", "P4095", "P4096", "P4097", "P8193"):      # a level boundary inside a chunk
        assert cr.starts_of(cc.BY_NAME[name].sizes)[1] % 1024 != 0
    assert -(-pts["260x260"] // 1024) == 67
    assert {c.num_classes for c in cc.CASES} == {1, 3, 64} and max(len(c.sizes) for c in cc.CASES) == 5
    assert [float(np.rint(np.float32(s) * np.float32(0.5))) for s in (5, 7, 1)] == [2.0, 4.0, 0.0]


def _torch_anchors(sizes, strides):
    """anchor_utils.py:82-132 with one size per level equal to its stride and aspect ratio 1, in fp32"""
    out = []
    for (h, w), s in zip(sizes, strides):
        base = (torch.tensor([-s, -s, s, s], dtype=torch.float32) / 2).round()
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.int32) * s, torch.arange(w, dtype=torch.int32) * s, indexing="ij")
        shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), 1)
        out.append((shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4))
    return torch.cat(out)


@pytest.mark.parametrize("name", NAMES)
def test_rule_is_the_references_chain_in_float64(name):
    """fcos.py:591-628 with torch in float64: the same set of points in the same order, the same labels and sides; the boxes of
    det_utils' decode_single on torch's fp32 anchors bit for bit"""
    from oracle import fcos_ref
    c = cc.BY_NAME[name]
    (cls_lr, reg_ctr, strides, C, thresh), _ = _args(name)
    cls, reg, sizes = cr.flatten(cls_lr, reg_ctr)
    tc, tr = torch.from_numpy(cls.copy()), torch.from_numpy(reg.copy())
    scores = torch.sqrt(torch.sigmoid(tc[..., :C].double()) * torch.sigmoid(tr[..., 4:5].double()))
    smax, lmax = torch.max(scores, dim=-1)
    masks = smax > float(np.float32(thresh))
    _, sides = torch.max(torch.sigmoid(tc[..., C:].double()), dim=-1)
    anchors = _torch_anchors(sizes, strides)
    starts = cr.starts_of(sizes)
    level = np.searchsorted(starts, np.arange(starts[-1]), side="right") - 1
    full = cr.rule64(cls_lr, reg_ctr, strides, C, thresh)
    for i, (r, kept) in enumerate(zip(full, cc.reference(name))):
        idx = torch.where(masks[i])[0]
        assert np.array_equal(idx.numpy(), r["point"]) and r["count"] == r["total"] == len(idx)
        assert np.array_equal(lmax[i][idx].numpy(), r["label"]) and np.array_equal(sides[i][idx].numpy(), r["side"])
        assert np.array_equal(level[idx.numpy()], r["level"])
        assert np.abs(smax[i][idx].numpy() - r["score"]).max(initial=0.0) <= 1e-15
        assert torch.equal(fcos_ref.decode_single(tr[i, :, :4], anchors)[idx], torch.from_numpy(r["box"]))
        k = kept["count"]                                   # the shared reference: the first cap rows of that
        assert k == min(len(idx), c.cap or len(idx)) and all(np.array_equal(kept[f], r[f][:k]) for f in cr.FIELDS)


@pytest.mark.parametrize("name", NAMES)
def test_emulation_matches_the_rule(name):
    args, kw = _args(name)
    dev = cr.check(cr.emulate(*args, **kw), cc.reference(name))
    print(f"cand emulate {name}: max |score - rule| = {dev:.3e}")
    assert dev <= cr.SCORE_TOL


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_every_mutant_fails_on_its_case_with_its_property(mutant):
    name, prop = cc.MUTANT_CASE[mutant]
    args, kw = _args(name)
    with pytest.raises(AssertionError, match=prop + r" (differs|\d+ !=)"):
        cr.check(cr.mutants()[mutant](*args, **kw), cc.reference(name))


def test_gy_by_h_hides_on_a_square_level():
    """why the table holds levels with h != w"""
    args, kw = _args("P1025")
    a, b = cr.emulate(*args, mutant="gy_by_h", **kw), cr.emulate(*args, **kw)
    assert np.array_equal(a[0]["box"][a[0]["point"] < 961], b[0]["box"][b[0]["point"] < 961]) and (b[0]["point"] < 961).any()


# --------------------------------------------------------------------------------------------------------------------------
# ext gather
# --------------------------------------------------------------------------------------------------------------------------
def test_ext_rule_is_the_references_chain_in_float64():
    """fcos.py:301-303: cat(d[0], 0.1 * F.normalize(d[1:], p=2)) with the fp32 constants, :605-607: argmax of the sigmoids; then
    the gather through keep and the candidates' point"""
    ext, point, keep, count = cc.make_ext()
    contacts, mags, bound = cc.ext_reference()
    flat = torch.from_numpy(np.concatenate([t.reshape(3, -1, 8) for t in ext], 1)).double()
    d = torch.cat([flat[..., :1], cr.TENTH * torch.nn.functional.normalize(flat[..., 1:3], p=2, dim=-1, eps=cr.EPS32)], -1)
    _, con = torch.max(torch.sigmoid(flat[..., 3:]), dim=-1)
    seen = set()
    for i in range(3):
        k = int(count[i])
        rows = torch.from_numpy(point[i][keep[i, :k]].astype(np.int64))
        seen |= set(rows.tolist()) if i == 2 else set()
        assert np.abs(d[i][rows].numpy() - mags[i, :k]).max(initial=0.0) <= 1e-15
        assert np.array_equal(con[i][rows].numpy(), contacts[i, :k])
        assert not mags[i, k:].any() and not contacts[i, k:].any()
    starts = cr.starts_of(cc.EXT_SIZES)
    assert seen >= set(starts[:-1].tolist()) | set((starts[1:] - 1).tolist())       # the first and the last point of every level
    assert not np.isnan(mags).any() and (mags[2, np.nonzero(keep[2] == np.nonzero(point[2] == 0)[0][0])[0][0], 1:] == 0).all()
    assert int(point[1][keep[1, 0]]) == 12 and bound[..., 0].max() == cr.TINY


def test_ext_emulation_is_inside_the_bound():
    args = cc.make_ext()
    contacts, mags = cr.ext_emulate(*args)
    ratio = cr.ext_check(contacts, mags, args[3], cc.ext_reference())
    print(f"ext emulate: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", cr.EXT_MUTANTS)
def test_every_ext_mutant_fails_with_its_property(mutant):
    args = cc.make_ext()
    contacts, mags = cr.ext_mutants()[mutant](*args)
    with pytest.raises(AssertionError, match=cc.EXT_MUTANT_PROPERTY[mutant]):
        cr.ext_check(contacts, mags, args[3], cc.ext_reference())


def test_saturated_contacts_keep_the_first():
    """logits 20 and 30 both give sigmoid == 1.0f: fp32 torch.sigmoid (the reference's type) ties them and the first wins"""
    logits = cc.SATURATED
    want = int(torch.max(torch.sigmoid(torch.from_numpy(logits.copy())), dim=-1)[1])
    assert want == 1 and int(np.argmax(logits)) == 3
    ext, point, keep, count = cc.make_saturated()
    assert int(cr.ext_emulate(ext, point, keep, count)[0][0, 0]) == want
