"""hn_a2j_aggregate_f32 and its fused epilogue against the float64 rule (tests/agg_ref.py) at every branch of the launch geometry
(tests/agg_cases.py): joint split with a short last workgroup, idle thread slots, the batched cell loops' tail, non-square maps,
the stride argument, logits near expf's underflow.  The assertion is |err| <= the derived worst-case bound and nothing tighter;
the ratios are printed and DESIGN.md section 5 holds the table measured on the MI355X."""
import numpy as np
import pytest
import torch

import agg_cases as ac
import agg_ref as ar

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ac.CASES]
PARAS = (475.065948, 475.065857, 315.944855, 245.287079)
BOXES = torch.tensor([[100, 50, 420, 430], [-5, -3, 700, 500], [7, 9, 8, 10]], dtype=torch.int64)
SENTINEL = -77.25


def _dev(name):
    return [torch.from_numpy(t.copy()).cuda() for t in ac.make(name)]


@pytest.mark.parametrize("name", NAMES)
def test_aggregate_is_inside_the_bound_and_rows_do_not_depend_on_the_batch(name):
    from hn_amd import ops
    c = ac.BY_NAME[name]
    cls, reg, dep = _dev(name)
    out = ops.a2j_aggregate(cls, reg, dep, joints=c.joints, stride=c.stride)
    ratio = ar.check(out.cpu().numpy(), *ac.make(name), c.joints, c.stride, ref=ac.reference(name))
    print(f"agg gpu {name}: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    for k in range(c.k):        # row k of the batched launch == the K = 1 launch of that row
        one = ops.a2j_aggregate(cls[k:k + 1].contiguous(), reg[k:k + 1].contiguous(), dep[k:k + 1].contiguous(),
                                joints=c.joints, stride=c.stride)
        assert torch.equal(one[0], out[k]), (name, k)


@pytest.mark.parametrize("name", ["9x14x5", "3x5x7", "23x31x64"])
def test_valid_rows_are_filled_and_the_others_unchanged(name):
    """valid == 0: zero rows, valid == 2: NaN rows (every joint of every workgroup of the split, in all three outputs of the fused
    form); rows with valid == 1 bit for bit the unmasked launch's."""
    from hn_amd import ops
    c = ac.BY_NAME[name]
    cls, reg, dep = _dev(name)
    box = BOXES[:c.k].cuda()
    full = ops.a2j_aggregate(cls, reg, dep, joints=c.joints, stride=c.stride)
    _, full_img, full_xyz = ops.a2j_aggregate(cls, reg, dep, joints=c.joints, stride=c.stride, convert=dict(crop_box=box, paras=PARAS))
    seen = set()
    for pattern in ([0, 1, 2][:c.k], [2, 0, 1][:c.k]):
        valid = torch.tensor(pattern, dtype=torch.int32).cuda()
        plain = ops.a2j_aggregate(cls, reg, dep, joints=c.joints, stride=c.stride, valid=valid,
                                  out=torch.full((c.k, c.joints, 3), SENTINEL, device="cuda"))
        fused = ops.a2j_aggregate(cls, reg, dep, joints=c.joints, stride=c.stride, valid=valid,
                                  convert=dict(crop_box=box, paras=PARAS,
                                               image_uvd=torch.full((c.k, c.joints, 3), SENTINEL, device="cuda"),
                                               xyz_mm=torch.full((c.k, c.joints, 3), SENTINEL, device="cuda")))
        for k, v in enumerate(pattern):
            seen.add(v)
            for got, want in ((plain, full), (fused[0], full), (fused[1], full_img), (fused[2], full_xyz)):
                if v == 1:
                    assert torch.equal(got[k], want[k]), (name, pattern, k)
                elif v == 0:
                    assert bool((got[k] == 0).all()), (name, pattern, k)
                else:
                    assert bool(torch.isnan(got[k]).all()), (name, pattern, k)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("name", ["3x5x7", "23x31x64", "11x11x21"])
def test_fused_epilogue_is_convert_joints_on_the_returned_crop_uvd(name):
    """convert=dict(crop_box, paras) plain, with mirror set on some rows, and with the live caller's clamps: image_uvd and xyz_mm
    are ops.convert_joints of the RETURNED crop uvd, bit for bit (for the clamps: of the clamped uvd and boxes, as
    test_aggregate_epilogue_equals_convert_joints_bit_for_bit states it)."""
    from hn_amd import ops
    c = ac.BY_NAME[name]
    cls, reg, dep = _dev(name)
    box = BOXES[:c.k].cuda()
    kw = dict(joints=c.joints, stride=c.stride)
    plain = ops.a2j_aggregate(cls, reg, dep, **kw)
    uvd, img, xyz = ops.a2j_aggregate(cls, reg, dep, convert=dict(crop_box=box, paras=PARAS), **kw)
    assert torch.equal(uvd, plain)
    assert torch.equal(img, ops.convert_joints(uvd, box, None, None)) and torch.equal(xyz, ops.convert_joints(uvd, box, None, PARAS))
    # mirror on some rows: u = crop - u (one fp32 subtraction) before anything else sees the value
    flags = [1, 0, 1][:c.k]
    mirror = torch.tensor(flags, dtype=torch.int32).cuda()
    uvd_m, img_m, xyz_m = ops.a2j_aggregate(cls, reg, dep, convert=dict(crop_box=box, paras=PARAS, mirror=mirror), **kw)
    want = plain.clone()
    want[mirror != 0, :, 0] = 176.0 - want[mirror != 0, :, 0]
    assert torch.equal(uvd_m, want) and not torch.equal(uvd_m, plain)
    assert torch.equal(img_m, ops.convert_joints(uvd_m, box, None, None)) and torch.equal(xyz_m, ops.convert_joints(uvd_m, box, None, PARAS))
    # clamp_keypoints + clamp_box: identical to clamping first (torch.clamp) and converting then; the crop uvd stays unclamped
    # (crop = 32: every case has coordinates beyond the keypoint clamp's upper end, and the depths inside it)
    uvd_c, img_c, xyz_c = ops.a2j_aggregate(cls, reg, dep, convert=dict(crop_box=box, paras=PARAS, crop=32, clamp_keypoints=True,
                                                                        clamp_box=(480, 640)), **kw)
    kp_c = torch.clamp(uvd_c, min=0.0, max=32.0)
    box_c = box.clone()
    box_c[:, :2] = torch.clamp(box_c[:, :2], 0, 480)
    box_c[:, 2:] = torch.clamp(box_c[:, 2:], 0, 640)
    assert torch.equal(uvd_c, plain) and not torch.equal(box_c, box)
    moved = kp_c != uvd_c
    assert bool(moved.any()) and not bool(moved.all())         # (the case exercises both clamps)
    assert torch.equal(img_c, ops.convert_joints(kp_c, box_c, None, None, crop=32))
    assert torch.equal(xyz_c, ops.convert_joints(kp_c, box_c, None, PARAS, crop=32))


def test_refusals_launch_nothing():
    """65 joints, a cls whose last dimension is not 16 * joints, fh = 0, a valid shorter than K, a reg of another K: refused
    before any launch (the sentinel-filled output comes back untouched)."""
    from hn_amd import ops

    def heads(k, fh, fw, joints, aj=None):
        aj = 16 * joints if aj is None else aj
        return (torch.zeros((k, fh, fw, aj), device="cuda"), torch.zeros((k, fh, fw, 2 * aj), device="cuda"),
                torch.zeros((k, fh, fw, aj), device="cuda"))
    for joints, args, exc in ((65, heads(1, 2, 2, 65), RuntimeError),
                              (21, heads(1, 2, 2, 21, aj=16 * 21 + 16), ValueError),
                              (21, heads(1, 0, 3, 21), (RuntimeError, ValueError))):
        out = torch.full((1, joints, 3), SENTINEL, device="cuda")
        with pytest.raises(exc):
            ops.a2j_aggregate(*args, joints=joints, out=out)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), joints
    # fewer flags than crops (the kernel would read past the end of valid), and reg with another K: ops.a2j_loss's refusals
    out = torch.full((2, 21, 3), SENTINEL, device="cuda")
    cls, reg, dep = heads(2, 2, 2, 21)
    with pytest.raises(ValueError, match="one flag per crop"):
        ops.a2j_aggregate(cls, reg, dep, joints=21, valid=torch.ones(1, dtype=torch.int32, device="cuda"), out=out)
    with pytest.raises(ValueError, match="bad head shapes"):
        ops.a2j_aggregate(cls, reg[:1], dep, joints=21, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
