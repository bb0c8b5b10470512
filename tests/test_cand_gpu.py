"""hn_fcos_candidates (one workgroup per image), hn_fcos_candidates_ws (count + scatter over 1024-point chunks) and
hn_fcos_ext_gather against the float64 rules (tests/cand_ref.py) on the cases of tests/cand_cases.py: level boundaries inside a
chunk, P around 1024 and 4 x 1024, 67 chunks, 1 / 3 / 64 classes, odd strides, planted class and side ties, logits at expf's
overflow and underflow, a cap below the passing count.  Each form is compared with the rule, not with the other form: membership,
order, labels, sides, levels and boxes exactly, scores to 2e-7.  Outputs are filled with a sentinel first; rows at and beyond
count must come back untouched.  DESIGN.md section 5 holds the deviations measured on the MI355X."""
import numpy as np
import pytest
import torch

import cand_cases as cc
import cand_ref as cr

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cc.CASES]
SENTINEL_F, SENTINEL_I = -77.25, -7


def _run(name, chunked):
    """the case through ops.fcos_candidates into a sentinel-filled Candidates of the case's cap -> (per-image rows, Candidates)"""
    from hn_amd import ops
    c = cc.BY_NAME[name]
    cls_lr, reg_ctr, _ = cc.make(name)
    cls_lr = [torch.from_numpy(t.copy()).cuda() for t in cls_lr]
    reg_ctr = [torch.from_numpy(t.copy()).cuda() for t in reg_ctr]
    cap = c.cap or cc.points(c)
    out = ops.alloc_candidates(c.n, cap, "cuda")
    for t in (out.boxes, out.scores):
        t.fill_(SENTINEL_F)
    for t in (out.labels, out.sides, out.level, out.point, out.count):
        t.fill_(SENTINEL_I)
    before = ops.CANDIDATES_CHUNKED
    ops.CANDIDATES_CHUNKED = chunked
    try:
        got = ops.fcos_candidates(cls_lr, reg_ctr, list(c.strides), c.num_classes, c.thresh, out=out)
        torch.cuda.synchronize()
    finally:
        ops.CANDIDATES_CHUNKED = before
    assert got is out
    count = out.count.cpu().numpy()
    f = {k: getattr(out, a).cpu().numpy() for k, a in (("point", "point"), ("score", "scores"), ("label", "labels"), ("side", "sides"),
                                                       ("level", "level"), ("box", "boxes"))}
    rows = []
    for i in range(c.n):
        k = int(count[i])
        assert 0 <= k <= cap, (i, k)
        rows.append(dict(count=k, **{key: v[i, :k] for key, v in f.items()}))
        # rows at and beyond count: untouched (with count == cap that is the next image's rows, checked as that image's own)
        assert (f["box"][i, k:] == SENTINEL_F).all() and (f["score"][i, k:] == SENTINEL_F).all(), (name, i)
        assert all((f[key][i, k:] == SENTINEL_I).all() for key in ("point", "label", "side", "level")), (name, i)
    return rows


@pytest.mark.parametrize("chunked", [True, False], ids=["chunked", "one-workgroup"])
@pytest.mark.parametrize("name", NAMES)
def test_candidates_are_the_rules(name, chunked):
    dev = cr.check(_run(name, chunked), cc.reference(name))
    print(f"cand gpu {name} {'chunked' if chunked else 'one-workgroup'}: max |score - rule| = {dev:.3e} (bar {cr.SCORE_TOL:.0e})")
    assert dev <= cr.SCORE_TOL


def _ext_run(ext, point, keep, count):
    from hn_amd import ops
    n, cap = keep.shape
    cand = ops.alloc_candidates(n, cap, "cuda")
    det = ops.alloc_detections(n, cap, "cuda")
    cand.point.copy_(torch.from_numpy(point.copy()))
    det.keep.copy_(torch.from_numpy(keep.copy()))
    det.count.copy_(torch.from_numpy(count.copy()))
    contacts, mags = ops.fcos_ext_gather([torch.from_numpy(t.copy()).cuda() for t in ext], det, cand)
    return contacts.cpu().numpy(), mags.cpu().numpy()


def test_ext_gather_is_the_rule():
    """keep and point are permutations other than the identity; det_count = 0, 1 and cap; dx = dy = 0, one of them 0, 1e-20, norms on
    either side of the 1e-12 clamp; first-max contact ties"""
    ext, point, keep, count = cc.make_ext()
    contacts, mags = _ext_run(ext, point, keep, count)
    assert contacts.dtype == np.int32
    ratio = cr.ext_check(contacts, mags, count, cc.ext_reference())
    print(f"ext gpu: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_saturated_contacts_keep_the_first():
    """logits 20 and 30 both give sigmoid == 1.0f, so the first of them wins: the expectation is fp32 torch.sigmoid on the CPU"""
    want = int(torch.max(torch.sigmoid(torch.from_numpy(cc.SATURATED.copy())), dim=-1)[1])
    contacts, mags = _ext_run(*cc.make_saturated())
    assert int(contacts[0, 0]) == want == 1 and int(contacts[0, 1]) == 0
    assert mags[0, 0, 0] == np.float32(0.5) and not mags[0, 1].any()
