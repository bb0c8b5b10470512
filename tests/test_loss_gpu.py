"""hn_a2j_aggregate_loss_f32 (the aggregation with the A2J criterion in its sweep, and its reduction launch) against the float64
rule (tests/loss_ref.py) at every branch of the launch geometry (tests/loss_cases.py), its keypoints against the plain
aggregation's bytes, and forward(x, gt) / validation_step of the drop-in module.  The assertion is |err| <= the derived worst-case
bound and nothing tighter; the ratios are printed and DESIGN.md section 9o holds the table measured on the MI355X."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_ref as lr

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in lc.CASES]
PARAS = (475.065948, 475.065857, 315.944855, 245.287079)
BOXES = torch.tensor([[100, 50, 420, 430], [-5, -3, 700, 500], [7, 9, 8, 10]], dtype=torch.int64)
SENTINEL = -77.25


def _dev(name):
    return [torch.from_numpy(t.copy()).cuda() for t in lc.heads(name)]


def _kw(name):
    """ops.a2j_loss's arguments behind the heads, on the device"""
    kw = lc.kwargs(name)
    kw["gt"] = torch.from_numpy(kw["gt"].copy()).cuda()
    if kw["valid"] is not None:
        kw["valid"] = torch.from_numpy(kw["valid"].copy()).cuda()
    return kw


def _same(a, b):
    """equal bytes (torch.equal would call two NaN rows different)"""
    return a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _host(terms, sample, batch):
    return dict(terms=terms.cpu().numpy(), sample=sample.cpu().numpy(), batch=batch.cpu().numpy())


@pytest.mark.parametrize("name", NAMES)
def test_loss_is_inside_the_bound_and_the_keypoints_are_the_aggregations(name):
    from hn_amd import ops
    a = lc.agg(name)
    cls, reg, dep = _dev(name)
    kw = _kw(name)
    uvd, terms, sample, batch = ops.a2j_loss(cls, reg, dep, **kw)
    detail = {}
    ratio = lr.check(_host(terms, sample, batch), lc.reference(name), detail=detail)
    print(f"loss gpu {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    plain = ops.a2j_aggregate(cls, reg, dep, joints=a.joints, stride=a.stride, valid=kw["valid"])
    assert torch.equal(uvd, plain)
    assert uvd.is_cuda and terms.is_cuda and sample.is_cuda and batch.is_cuda
    # with convert=: the image uvd and the xyz are the aggregation's too
    box = BOXES[:a.k].cuda()
    (u2, img, xyz), t2, s2, b2 = ops.a2j_loss(cls, reg, dep, convert=dict(crop_box=box, paras=PARAS), **kw)
    _, want_img, want_xyz = ops.a2j_aggregate(cls, reg, dep, joints=a.joints, stride=a.stride, valid=kw["valid"],
                                              convert=dict(crop_box=box, paras=PARAS))
    assert torch.equal(u2, plain) and torch.equal(img, want_img) and torch.equal(xyz, want_xyz)
    assert _same(t2, terms) and _same(s2, sample) and _same(b2, batch)
    # row k of the batched launch == the K = 1 launch of that row
    for k in range(a.k):
        one = ops.a2j_loss(cls[k:k + 1].contiguous(), reg[k:k + 1].contiguous(), dep[k:k + 1].contiguous(),
                           **dict(kw, gt=kw["gt"][k:k + 1].contiguous(), valid=None if kw["valid"] is None else kw["valid"][k:k + 1].contiguous()))
        assert _same(one[2], sample[k:k + 1]) and _same(one[1], terms[k:k + 1]) and _same(one[0], uvd[k:k + 1]), (name, k)


@pytest.mark.parametrize("name", ["9x14x5", "3x5x7", "23x31x64"])
def test_valid_rows_the_divisor_and_the_nan_rows(name):
    """valid patterns [0,1,2] and [2,0,1]: rows with valid == 1 have the unmasked launch's sample row bit for bit, rows with 0
    are zeros and left out, a row with 2 is NaN and makes every batch value NaN; without the NaN row (2 -> 0) the batch values are
    inside the bound of the rule with that mask, whose divisor is the number of counted rows; an all-zero valid gives NaN."""
    from hn_amd import ops
    a = lc.agg(name)
    cls, reg, dep = _dev(name)
    kw = _kw(name)
    assert kw["valid"] is None
    _, terms, sample, _ = ops.a2j_loss(cls, reg, dep, **kw)
    seen = set()
    for pattern in ([0, 1, 2][:a.k], [2, 0, 1][:a.k]):
        valid = torch.tensor(pattern, dtype=torch.int32).cuda()
        uvd, t, s, b = ops.a2j_loss(cls, reg, dep, **dict(kw, valid=valid))
        assert _same(uvd, ops.a2j_aggregate(cls, reg, dep, joints=a.joints, stride=a.stride, valid=valid))
        for k, v in enumerate(pattern):
            seen.add(v)
            if v == 1:
                assert torch.equal(s[k], sample[k]) and torch.equal(t[k], terms[k]), (name, pattern, k)
            elif v == 0:
                assert bool((s[k] == 0).all()) and bool((t[k] == 0).all()) and bool((uvd[k] == 0).all()), (name, pattern, k)
            else:
                assert bool(torch.isnan(s[k]).all()) and bool(torch.isnan(t[k]).all()) and bool(torch.isnan(uvd[k]).all())
        assert bool(torch.isnan(b).all()) == (2 in pattern), (name, pattern)
        host_kw = dict(lc.kwargs(name), valid=np.array(pattern, np.int32))
        heads = lc.heads(name)
        lr.check(_host(t, s, b), (lr.rule(*heads, **host_kw), lr.bound(*heads, **host_kw)))
        # the same pattern without its NaN row: finite batch values, the divisor = the rows that count
        masked = [0 if v == 2 else v for v in pattern]
        host_kw = dict(host_kw, valid=np.array(masked, np.int32))
        _, t, s, b = ops.a2j_loss(cls, reg, dep, **dict(kw, valid=torch.tensor(masked, dtype=torch.int32).cuda()))
        want = lr.rule(*heads, **host_kw)
        if 1 in masked:
            assert np.isfinite(want["batch"]).all() and sum(masked) == 1
            assert want["batch"][0] == want["sample"][masked.index(1), 0]     # (one counted row: the mean is that row)
        else:
            assert np.isnan(want["batch"]).all()                              # (two crops: nothing is left to count)
        ratio = lr.check(_host(t, s, b), (want, lr.bound(*heads, **host_kw)))
        print(f"loss gpu {name} valid {masked}: max |err| / bound = {ratio:.4f}")
    assert seen == {0, 1, 2}
    _, _, s, b = ops.a2j_loss(cls, reg, dep, **dict(kw, valid=torch.zeros((a.k,), dtype=torch.int32).cuda()))
    assert bool(torch.isnan(b).all()) and bool((s == 0).all())


def test_refusals_launch_nothing():
    """65 joints, a cls whose last dimension is not 16 * joints, fh = 0, a gt of the wrong shape or type: refused before any launch
    (the sentinel-filled output comes back untouched)."""
    from hn_amd import ops

    def heads(k, fh, fw, joints, aj=None):
        aj = 16 * joints if aj is None else aj
        return (torch.zeros((k, fh, fw, aj), device="cuda"), torch.zeros((k, fh, fw, 2 * aj), device="cuda"),
                torch.zeros((k, fh, fw, aj), device="cuda"))

    def gt(k, joints, dtype=torch.float32):
        return torch.zeros((k, joints, 3), device="cuda", dtype=dtype)
    for joints, args, g, exc in ((65, heads(1, 2, 2, 65), gt(1, 65), RuntimeError),
                                 (21, heads(1, 2, 2, 21, aj=16 * 21 + 16), gt(1, 21), ValueError),
                                 (21, heads(1, 0, 3, 21), gt(1, 21), (RuntimeError, ValueError)),
                                 (21, heads(1, 2, 2, 21), gt(1, 20), ValueError),
                                 (21, heads(2, 2, 2, 21), gt(1, 21), ValueError),
                                 (21, heads(1, 2, 2, 21), gt(1, 21, torch.float64), TypeError)):
        out = torch.full((args[0].shape[0], joints, 3), SENTINEL, device="cuda")
        with pytest.raises(exc):
            ops.a2j_loss(*args, g, joints=joints, out=out)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), joints
    with pytest.raises(ValueError, match="mirror"):
        ops.a2j_loss(*heads(1, 2, 2, 21), gt(1, 21), convert=dict(crop_box=BOXES[:1].cuda(), mirror=torch.zeros((1,), dtype=torch.int32).cuda()))


def _gt_near(out, seed):
    g = torch.Generator().manual_seed(seed)
    off = torch.empty_like(out)
    off[..., :2] = torch.tensor([0.25, 0.9, 1.5, 6.0])[torch.randint(0, 4, out[..., :2].shape, generator=g)]
    off[..., 2] = torch.tensor([0.01, 0.2])[torch.randint(0, 2, out[..., 2].shape, generator=g)]
    return out + off * (torch.randint(0, 2, out.shape, generator=g) * 2 - 1)


@pytest.mark.parametrize("rgbd", [False, True])
def test_model_forward_with_gt_and_the_validation_step(a2j_sd, a2j_rgbd_sd, rgbd):
    """5 crops, depth-only and RGBD: (losses, out) = net.a2j(x, gt) has out torch.equal to net.a2j(x); losses are the bytes of
    ops.a2j_loss on the heads of forward_nhwc(return_heads=True) and inside the bound of the float64 rule applied to those same
    device heads (no new tolerance on the conv stack); after device_loss(), validation_step logs val_loss == float(total_loss) and
    a test_rmse inside its bound of sqrt(mean((gt - out)^2)), and returns the total."""
    from a2j.a2j import A2JModelLightning
    from hn_amd import ops, synth
    net = A2JModelLightning(is_RGBD=rgbd, spatial_factor=0.25)
    net.a2j.load_state_dict(a2j_rgbd_sd if rgbd else a2j_sd, strict=False)
    net = net.cuda().eval()
    k = 5
    x = (synth.make_rgbd_crops(k, 176, seed=77) if rgbd else synth.make_crops(k, 176, seed=77)).cuda()
    plain = net.a2j(x)
    gt = _gt_near(plain, seed=79)
    assert plain.device.type == "cpu" and gt.shape == (k, 21, 3)
    losses, out = net(x, gt.numpy())                                  # (an array on the host: any device, tensor or array)
    assert torch.equal(out, plain) and out.device.type == "cpu"
    assert set(losses) == {"classification", "regression", "total_loss"}
    assert all(v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (1,) for v in losses.values())
    losses2, out2 = net.a2j(x, gt.cuda())
    assert torch.equal(out2, plain) and all(torch.equal(losses[n], losses2[n]) for n in losses)
    # the same bytes as ops.a2j_loss on the engine's own heads
    eng = net.a2j.engine()
    xin = x[:, :4].permute(0, 2, 3, 1).contiguous() if rgbd else ops.pack_depth_nhwc(x[:, 0:1].contiguous(), cpad=4)
    valid = torch.ones((k,), device="cuda", dtype=torch.int32)
    kp, _, (cls, reg, dep) = eng.forward_nhwc(xin, valid, return_heads=True)
    assert torch.equal(kp.cpu(), plain)
    uvd, terms, sample, batch = ops.a2j_loss(cls, reg, dep, gt.cuda(), joints=21, stride=16, spatial_factor=0.25, reg_loss_factor=3.0)
    assert torch.equal(uvd.cpu(), plain)
    assert torch.equal(batch[0:1], losses["classification"]) and torch.equal(batch[2:3], losses["regression"])
    assert torch.equal(batch[3:4], losses["total_loss"])
    # ... and inside the bound of the float64 rule on those heads
    heads = [t.cpu().numpy() for t in (cls, reg, dep)]
    kw = dict(gt=gt.numpy(), joints=21, stride=16, spatial_factor=0.25, reg_loss_factor=3.0)
    detail = {}
    lr.check(_host(terms, sample, batch), (lr.rule(*heads, **kw), lr.bound(*heads, **kw)), detail=detail)
    print(f"loss gpu model rgbd={rgbd}: max |err| / bound = " + ", ".join(f"{n} {v:.4f}" for n, v in detail.items()))
    assert net.a2j.last_loss_host["total_loss"] == float(losses["total_loss"]) and net.a2j.last_loss_host["rmse"] == float(batch[4])
    # the validation step
    with pytest.raises(NotImplementedError):
        net.validation_step(None, 0)
    assert net.device_loss() is net
    step = (None, gt, None, None, None, None, x) if rgbd else (x, gt, None, None, None, None, None)
    total = net.validation_step(step, 0)
    assert torch.equal(total, losses["total_loss"])
    assert net.logged["val_loss"] == [float(losses["total_loss"])] and list(net.logged) == ["val_loss", "test_rmse"]
    want, b = lr.rmse_bound_given_out(gt.numpy(), plain.numpy())
    assert abs(net.logged["test_rmse"][0] - want) <= b, (net.logged["test_rmse"][0], want, b)
    print(f"loss gpu model rgbd={rgbd}: test_rmse |err| / bound = {abs(net.logged['test_rmse'][0] - want) / b:.4f}")
    for hook in (net.training_step, net.configure_optimizers):
        with pytest.raises(NotImplementedError):
            hook(None, 0)
    net.device_loss(False)
    with pytest.raises(NotImplementedError):
        net.validation_step(step, 0)
