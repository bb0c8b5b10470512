"""hn_a2j_loss_grad_f32 (the A2J criterion's backward at the three heads, one launch) against the float64 rule
(tests/loss_grad_ref.py) on every case of tests/loss_cases.py and both upstream settings, its forward outputs against
ops.a2j_loss's bytes, A2JCriterion under torch's autograd, and head_grads of the drop-in module.  The assertion is |err| <= the
derived worst-case bound and nothing tighter; the ratios are printed and DESIGN.md section 9r holds the table measured on the MI355X."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_grad_ref as gr

pytestmark = pytest.mark.gpu

IDS = [gr.case_id(c) for c in gr.CASES]


def _dev(name):
    return [torch.from_numpy(t.copy()).cuda() for t in lc.heads(name)]


def _kw(case):
    """ops.a2j_loss_grad's arguments behind the heads, on the device"""
    kw = gr.kwargs(case)
    kw["gt"] = torch.from_numpy(kw["gt"].copy()).cuda()
    if kw["valid"] is not None:
        kw["valid"] = torch.from_numpy(kw["valid"].copy()).cuda()
    kw["upstream"] = None if case[1] == 0 else torch.tensor(kw["upstream"], dtype=torch.float32).cuda()
    return kw


def _same(a, b):
    """equal bytes (torch.equal would call two NaN rows different)"""
    return a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _host(grads):
    return dict(zip(gr.KEYS, (t.cpu().numpy() for t in grads)))


@pytest.mark.parametrize("case", gr.CASES, ids=IDS)
def test_gradients_are_inside_the_bound_and_the_forward_is_the_loss_entrys(case):
    from hn_amd import ops
    cls, reg, dep = _dev(case[0])
    kw = _kw(case)
    grads = ops.a2j_loss_grad(cls, reg, dep, **kw)
    assert len(grads) == 3 and all(t.is_cuda and t.dtype == torch.float32 for t in grads)
    assert grads[0].shape == cls.shape and grads[1].shape == reg.shape and grads[2].shape == dep.shape
    detail = {}
    ratio = gr.check(_host(grads), gr.reference(case), detail=detail)
    print(f"loss grad gpu {gr.case_id(case)}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0
    # want_forward: the loss entry's keypoints and terms, bit for bit; the gradients do not change
    loss_kw = {k: v for k, v in kw.items() if k != "upstream"}
    uvd, terms, _, _ = ops.a2j_loss(cls, reg, dep, **loss_kw)
    again = ops.a2j_loss_grad(cls, reg, dep, want_forward=True, **kw)
    assert len(again) == 5
    if case[0].endswith("gt-nan"):
        assert _same(again[3], uvd) and _same(again[4], terms)
    else:
        assert torch.equal(again[3], uvd) and torch.equal(again[4], terms)
    # two launches: the same bytes
    assert all(_same(a, b) for a, b in zip(again[:3], grads))
    if case[1] == 0:   # upstream = None is (1, 1)
        ones = ops.a2j_loss_grad(cls, reg, dep, **dict(kw, upstream=torch.ones((2,), device="cuda")))
        assert all(_same(a, b) for a, b in zip(ones, grads))


@pytest.mark.parametrize("name", ["3x5x7", "23x31x64"])
def test_valid_rows(name):
    """valid = (1, 0, 1) (or (0, 1) on two crops): the rows with 0 have exact zero gradients and the others are inside the bound of
    the rule with that mask, whose divisor is the number of counted rows; a row with valid = 2 is all NaN and the others finite."""
    from hn_amd import ops
    a = lc.agg(name)
    cls, reg, dep = _dev(name)
    kw = _kw((name, 1))
    heads = lc.heads(name)
    for pattern in ([1, 0, 1][-a.k:], [2, 1, 1][:a.k]):
        valid = torch.tensor(pattern, dtype=torch.int32).cuda()
        grads = ops.a2j_loss_grad(cls, reg, dep, **dict(kw, valid=valid))
        for k, v in enumerate(pattern):
            for t in grads:
                if v == 0:
                    assert bool((t[k] == 0).all()), (name, pattern, k)
                elif v == 2:
                    assert bool(torch.isnan(t[k]).all()), (name, pattern, k)
                else:
                    assert bool(torch.isfinite(t[k]).all()), (name, pattern, k)
        host_kw = dict(gr.kwargs((name, 1)), valid=np.array(pattern, np.int32))
        ratio = gr.check(_host(grads), (gr.rule(*heads, **host_kw), gr.bound(*heads, **host_kw)))
        print(f"loss grad gpu {name} valid {pattern}: max |err| / bound = {ratio:.4f}")
    none = ops.a2j_loss_grad(cls, reg, dep, **dict(kw, valid=torch.zeros((a.k,), dtype=torch.int32).cuda()))
    assert all(bool((t == 0).all()) for t in none)


def test_refusals_and_the_empty_batch():
    """the bad shapes and dtypes ops.a2j_loss refuses (tests/test_loss_gpu.py), refused the same way; K = 0 launches nothing"""
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
        for fn in (ops.a2j_loss, ops.a2j_loss_grad):
            with pytest.raises(exc):
                fn(*args, g, joints=joints)
    h = heads(1, 2, 2, 21)
    with pytest.raises(ValueError, match="upstream"):
        ops.a2j_loss_grad(*h, gt(1, 21), upstream=torch.ones((3,), device="cuda"))
    with pytest.raises(ValueError, match="valid"):
        ops.a2j_loss_grad(*h, gt(1, 21), valid=torch.ones((2,), device="cuda", dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        ops.a2j_loss_grad(h[0].permute(0, 2, 1, 3), h[1], h[2], gt(1, 21))
    empty = ops.a2j_loss_grad(*heads(0, 2, 2, 21), gt(0, 21), want_forward=True)
    assert [tuple(t.shape) for t in empty] == [(0, 2, 2, 336), (0, 2, 2, 672), (0, 2, 2, 336), (0, 21, 3), (0, 21, 8)]


def test_criterion_under_autograd():
    """A2JCriterion on three leaf head tensors: total_loss.backward() leaves the bytes of ops.a2j_loss_grad(upstream=None) in
    .grad; (0.7 classification + 1.9 regression).backward() those of upstream = (0.7, 1.9); the losses are ops.a2j_loss's batch
    values; a second backward raises; gt gets no gradient; a layout other than contiguous fp32 raises ValueError."""
    from hn_amd import ops
    from hn_amd.criterion import A2JCriterion
    name = "11x11x21"
    a = lc.agg(name)
    kw = _kw((name, 0))
    crit = A2JCriterion(joints=a.joints, stride=a.stride, spatial_factor=0.5, reg_loss_factor=3.0)

    def leaves():
        return [t.requires_grad_(True) for t in _dev(name)]
    heads = leaves()
    gt = kw["gt"].clone().requires_grad_(True)
    losses, uvd = crit(*heads, gt)
    want_uvd, _, _, batch = ops.a2j_loss(*[t.detach() for t in heads], kw["gt"], joints=a.joints, stride=a.stride)
    assert set(losses) == {"classification", "regression", "total_loss"}
    assert all(v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (1,) for v in losses.values())
    assert torch.equal(losses["classification"], batch[0:1]) and torch.equal(losses["regression"], batch[2:3])
    assert torch.equal(losses["total_loss"], batch[3:4]) and torch.equal(uvd, want_uvd) and not uvd.requires_grad
    losses["total_loss"].backward()
    want = ops.a2j_loss_grad(*[t.detach() for t in heads], kw["gt"], joints=a.joints, stride=a.stride)
    assert all(torch.equal(t.grad, w) for t, w in zip(heads, want)) and gt.grad is None
    with pytest.raises(RuntimeError):
        losses["total_loss"].backward()
    heads = leaves()
    losses, _ = crit(*heads, kw["gt"])
    (0.7 * losses["classification"] + 1.9 * losses["regression"]).sum().backward()
    want = ops.a2j_loss_grad(*[t.detach() for t in heads], kw["gt"], joints=a.joints, stride=a.stride,
                             upstream=torch.tensor([0.7, 1.9], device="cuda"))
    assert all(torch.equal(t.grad, w) for t, w in zip(heads, want))
    gr.check(_host([t.grad for t in heads]), gr.reference((name, 1)))
    # a [K,C,fh,fw] head in channels_last (a 1 x 1 convolution written with torch's elementwise kernels), viewed with
    # permute(0, 2, 3, 1), is the layout; the gradient reaches the head's weights
    x = torch.randn((2, 8, 3, 5), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    weight = torch.randn((16 * 3, 8), device="cuda", generator=torch.Generator("cuda").manual_seed(6)).requires_grad_(True)
    small = A2JCriterion(joints=3, stride=8)
    nchw = (x[:, None] * weight[None, :, :, None, None]).sum(2)
    c = nchw.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    assert c.is_contiguous() and tuple(c.shape) == (2, 3, 5, 48)
    r, d = torch.zeros((2, 3, 5, 96), device="cuda"), torch.ones((2, 3, 5, 48), device="cuda")
    losses, _ = small(c, r, d, torch.zeros((2, 3, 3), device="cuda"))
    losses["total_loss"].backward()
    assert weight.grad is not None and bool(torch.isfinite(weight.grad).all()) and bool((weight.grad != 0).any())
    with pytest.raises(ValueError):
        small(nchw.detach().permute(0, 2, 3, 1), r, d, torch.zeros((2, 3, 3), device="cuda"))
    with pytest.raises(ValueError):
        small(c.detach().double(), r, d, torch.zeros((2, 3, 3), device="cuda"))


def _gt_near(out, seed):
    g = torch.Generator().manual_seed(seed)
    off = torch.empty_like(out)
    off[..., :2] = torch.tensor([0.25, 0.9, 1.5, 6.0])[torch.randint(0, 4, out[..., :2].shape, generator=g)]
    off[..., 2] = torch.tensor([0.01, 0.2])[torch.randint(0, 2, out[..., 2].shape, generator=g)]
    return out + off * (torch.randint(0, 2, out.shape, generator=g) * 2 - 1)


@pytest.mark.parametrize("rgbd", [False, True])
def test_model_head_grads(a2j_sd, a2j_rgbd_sd, rgbd):
    """5 crops, depth-only and RGBD: (losses, out, grads) = net.a2j.head_grads(x, gt) has losses and out torch.equal to
    net.a2j(x, gt)'s; the gradients are the bytes of ops.a2j_loss_grad on the heads of forward_nhwc(return_heads=True) and inside
    the bound of the float64 rule applied to those same device heads (no new tolerance on the conv stack)."""
    from a2j.a2j import A2JModelLightning
    from hn_amd import ops, synth
    net = A2JModelLightning(is_RGBD=rgbd, spatial_factor=0.25)
    net.a2j.load_state_dict(a2j_rgbd_sd if rgbd else a2j_sd, strict=False)
    net = net.cuda().eval()
    k = 5
    x = (synth.make_rgbd_crops(k, 176, seed=77) if rgbd else synth.make_crops(k, 176, seed=77)).cuda()
    gt = _gt_near(net.a2j(x), seed=79)
    want_losses, want_out = net.a2j(x, gt)
    losses, out, grads = net.a2j.head_grads(x, gt)
    assert torch.equal(out, want_out) and out.device.type == "cpu" and set(losses) == set(want_losses)
    assert all(torch.equal(losses[n], want_losses[n]) and losses[n].is_cuda for n in losses)
    eng = net.a2j.engine()
    xin = x[:, :4].permute(0, 2, 3, 1).contiguous() if rgbd else ops.pack_depth_nhwc(x[:, 0:1].contiguous(), cpad=4)
    valid = torch.ones((k,), device="cuda", dtype=torch.int32)
    _, _, (cls, reg, dep) = eng.forward_nhwc(xin, valid, return_heads=True)
    want = ops.a2j_loss_grad(cls, reg, dep, gt.cuda(), joints=21, stride=16, spatial_factor=0.25, reg_loss_factor=3.0)
    assert len(grads) == 3 and all(g.is_cuda and torch.equal(g, w) for g, w in zip(grads, want))
    e_losses, e_uvd, e_grads = eng.head_grads(x, gt.cuda(), spatial_factor=0.25)
    assert torch.equal(e_uvd.cpu(), want_out) and all(torch.equal(e_losses[n], want_losses[n]) for n in losses)
    assert all(torch.equal(g, w) for g, w in zip(e_grads, want))
    heads = [t.cpu().numpy() for t in (cls, reg, dep)]
    kw = dict(gt=gt.numpy(), joints=21, stride=16, spatial_factor=0.25, reg_loss_factor=3.0)
    assert gr.depth_margin(*heads, kw["gt"], 21, 16) > gr.SIGN_GUARD
    detail = {}
    gr.check(_host(grads), (gr.rule(*heads, **kw), gr.bound(*heads, **kw)), detail=detail)
    print(f"loss grad gpu model rgbd={rgbd}: max |err| / bound = " + ", ".join(f"{n} {v:.4f}" for n, v in detail.items()))
    for hook in (net.training_step, net.configure_optimizers):
        with pytest.raises(NotImplementedError):
            hook(None, 0)
