"""The FCOS criterion's backward (tests/fcos_loss_grad_ref.py) without a GPU: the rule against the imported reference's float64
autograd (tests/golden/fcos_loss_grad.npz) and against central differences of the forward rule, the fp32 emulation of the kernel
inside the derived bound on every case and both upstream settings, every mutant of the emulation outside it on its named case,
the cases' distance from the gradient's non-smooth points, and the surface: the C entry's export, ABI and refusals, and the
Python entry points."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import fcos_loss_cases as lc
import fcos_loss_grad_cases as gc
import fcos_loss_grad_ref as gr
import fcos_loss_ref as fr

IDS = [gc.case_id(c) for c in gc.CASES]
D = np.float64


@pytest.mark.parametrize("tag", list(gc.GOLDEN))
@pytest.mark.parametrize("u", range(len(gc.UPSTREAMS)))
def test_rule_is_the_references_autograd(golden_dir, tag, u):
    """1e-12 relative, element by element, with the golden's float32 matching.  The focal columns and the centre-ness column are
    products of positive factors or one difference: relative to sum |product|, which for the focal columns is the element itself.
    The four GIoU columns and the (dx, dy) columns are brackets that cancel (the two quotients' derivatives; G - u (u . G)): both
    float64 evaluations round in proportion to the products' magnitudes, so an element is compared relative to the sum of the
    |products| of its bracket (rule(magnitude=True)).  The plain elementwise figure is printed.  g3 pins the non-smooth points:
    the strict-overlap mask, the even split on a tie, the clamp's diagonal Jacobian, a zero regression that is not masked."""
    g = np.load(golden_dir / "fcos_loss_grad.npz")
    name = gc.GOLDEN[tag]
    a, up = gc.args(name), gc.UPSTREAMS[u]
    matched = g[f"{tag}_matched"]
    assert np.array_equal(matched, fr.rule(*a)["matched"])
    got, size = gr.rule(*a, upstream=up, matched=matched), gr.rule(*a, upstream=up, magnitude=True, matched=matched)
    rows = g["g1_rows"] if tag == "g1" else None
    if tag == "g1":
        fg = np.argwhere(matched >= 0)
        assert {tuple(r) for r in fg} <= {tuple(r) for r in rows} and len(rows) > 2 * len(fg)
    for key in gr.KEYS:
        if got[key] is None:
            assert f"{tag}_up{u}_{key}" not in g
            continue
        want = g[f"{tag}_up{u}_{key}"]
        x, m = (t[rows[:, 0], rows[:, 1]] if rows is not None else t for t in (got[key], size[key]))
        assert want.dtype == D and want.shape == x.shape and np.isfinite(want).all()
        err = np.abs(x - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel, plain = np.where(err == 0, 0.0, err / m), np.where(err == 0, 0.0, err / np.abs(want))
        print(f"fcos loss grad golden {tag} up{u} {key}: max |err| / magnitude = {rel.max():.2e}, max |err| / |golden| = "
              f"{plain.max():.2e}, max |golden| = {np.abs(want).max():.2e}")
        assert (err <= 1e-12 * m).all(), (key, float(rel.max()))
    if tag == "g3":
        p = gc.G3_POINTS
        d_reg, d_ext = g[f"g3_up{u}_d_reg"], g[f"g3_up{u}_d_ext"]
        assert d_reg[0, p["ZERO"], 1] != 0 and d_reg[0, p["APART"], 0] != 0            # a zero regression is not masked
        assert abs(d_ext[0, p["CLAMP"], 1]) > 1e4 and d_ext[0, p["DX0"], 1] != 0


@pytest.mark.parametrize("name", gc.SMOOTH)
def test_rule_agrees_with_central_differences_of_the_forward_rule(name, monkeypatch):
    """L(t) = sum_k w_k fcos_loss_ref.rule(heads + t v)["losses"][k] in float64 along three seeded directions v (unit normal clipped to
    [-4, 4] on every head element, zero on the (dx, dy) of the points below the normalisation's clamp, where the forward is not
    differentiable in the finite-difference sense), both upstream settings:
        D(h) = (L(h) - L(-h)) / 2h  against  <gradient, v>,  h = 2^-20.
    Tolerance, derived from the step and the forward's own higher derivative, not from the gradient under test:
      * truncation: D(h) - L'(0) = h^2 L'''/6 + O(h^4) and D(2h) - D(h) = h^2 L'''/2 + O(h^4), so |D(2h) - D(h)| / 3 estimates
        it; twice that is allowed.  (Every kink is TIE_GUARD = 1e-3 away; 2h |v| s stays below 2.5e-4 for |v| <= 4 at s = 32.)
      * rounding: a value of L is a pairwise sum of n P (C + 15) <= 2^17 terms, each through about ten roundings, so it is off by
        at most 32 * 2^-53 * sum_k |w_k losses[k]|; two such values over 2h: 32 * 2^-53 * sum |w losses| / h."""
    a = gc.args(name)
    cls, reg, ex, sizes = fr.flatten(*a[:3])
    flat64 = [t.astype(D) if t is not None else None for t in (cls, reg, ex)]
    all_grads = [gr.rule(*a, upstream=up) for up in gc.UPSTREAMS]
    monkeypatch.setattr(fr, "flatten", lambda c, r, e=None: (c, r, e, sizes))   # the rule on float64 heads handed in flat
    h = 2.0 ** -20
    rng = np.random.default_rng(77)
    for u, up in enumerate(gc.UPSTREAMS):
        w = gr.weights(up)
        grads = all_grads[u]

        def values(t, v):
            heads = [None if x is None else x + t * d for x, d in zip(flat64, v)]
            return fr.rule(heads[0], heads[1], heads[2], *a[3:])["losses"]
        for _ in range(3):
            v = [None if x is None else np.clip(rng.standard_normal(x.shape), -4.0, 4.0) for x in flat64]
            if ex is not None:
                v[2][..., 1:3][(ex[..., 1] == 0) & (ex[..., 2] == 0)] = 0.0
            d1 = float(w @ (values(h, v) - values(-h, v))) / (2 * h)
            d2 = float(w @ (values(2 * h, v) - values(-2 * h, v))) / (4 * h)
            dot = sum(float((grads[key] * d).sum()) for key, d in zip(gr.KEYS, v) if d is not None)
            tol = 2.0 * abs(d2 - d1) / 3.0 + 32 * 2.0 ** -53 * float(np.abs(w * values(0.0, v)).sum()) / h
            print(f"fcos loss grad fd {name} up{u}: <grad, v> = {dot:.6e}, D(h) = {d1:.6e}, |diff| = {abs(d1 - dot):.2e}, tol = {tol:.2e}")
            assert abs(d1 - dot) <= tol
            scale = sum(float(np.abs(grads[key] * d).sum()) for key, d in zip(gr.KEYS, v) if d is not None)
            assert tol <= 1e-4 * scale, "the tolerance stays four digits below the size of what <gradient, v> adds up"


def test_the_cases_meet_their_conditions():
    assert gc.NAMES == lc.NAMES + ("g3",) and len(gc.CASES) == 18 and gc.SMOOTH == lc.NAMES
    assert gc.UPSTREAMS[0] is None
    w = np.array(gc.UPSTREAMS[1])
    assert len(set(w.tolist())) == 6 and (w == 0).sum() == 1 and (w < 0).sum() == 1 and np.array_equal(w.astype(np.float32), w)
    assert set(gr.MUTANT_CASE) == set(gr.MUTANTS) and len(gr.MUTANTS) == 11
    for name in gc.NAMES:
        t = gr.conditions(name)
        print(f"fcos loss grad case {name}: nearest tie {t['near']:.4f}, ties " + ", ".join(f"{k} {len(t[k])}" for k in t if k != "near"))
        if name != "g3":
            assert t["near"] > gr.TIE_GUARD and not (t["edge"] or t["apart"] or t["zero_reg"])
    t = gr.conditions("g3")
    assert [len(t[k]) for k in ("edge", "apart", "zero_reg", "clamp", "dx0")] == [1, 1, 1, 1, 1]
    # the seeded cases meet the clamp on about a quarter of their points
    assert len(gr.ties("golden-1")["clamp"]) > 1000
    # g3's special values are exactly representable and the tie is exact in float32
    cls_lr, reg_ctr, ext, gt = gc.make("g3")
    assert reg_ctr[0][0, 2, 3, 0] == 2.0 and gt[0][0, 0, 0] == 8.0 and np.float32(24.0) - np.float32(2.0) * np.float32(8.0) == gt[0][0, 0, 0]


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_emulation_is_inside_the_bound(case):
    detail = {}
    out = gr.emulate(*gc.args(case[0]), upstream=gc.upstream(case))
    ratio = gr.check(out, gr.reference(case), detail=detail)
    print(f"fcos loss grad emulate {gc.case_id(case)}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_every_mutant_fails_on_its_case(mutant):
    name, u = gr.MUTANT_CASE[mutant]
    with pytest.raises(AssertionError, match="bound"):
        gr.check(gr.mutants()[mutant](*gc.args(name), upstream=gc.UPSTREAMS[u]), gr.reference((name, u)))


def test_linearity_in_upstream_and_the_untouched_elements():
    """the rule is linear in upstream: w = sum_k w_k e_k; a unit upstream e_k leaves every element its term does not touch at
    exactly zero; without foreground d_reg is exactly zero"""
    name = "edge"
    a = gc.args(name)
    w = np.array(gc.UPSTREAMS[1])
    units = [gr.rule(*a, upstream=np.eye(6)[k]) for k in range(6)]
    both = gr.rule(*a, upstream=w)
    size = gr.rule(*a, upstream=w, magnitude=True)
    for key in gr.KEYS:
        total = sum(w[k] * units[k][key] for k in range(6))
        assert (np.abs(both[key] - total) <= 1e-12 * size[key]).all()                # (the brackets of d_reg and d_ext cancel)
    c = gc.BY_NAME[name].num_classes
    fg = fr.rule(*a)["matched"] >= 0
    e0, e1, e5 = units[0], units[1], units[5]
    assert e0["d_cls"][..., :c].any() and not e0["d_cls"][..., c:].any() and not e0["d_reg"].any() and not e0["d_ext"].any()
    assert not e1["d_cls"].any() and not e1["d_reg"][..., 4].any() and not e1["d_reg"][~fg].any() and not e1["d_ext"].any()
    assert e1["d_reg"][fg][:, :4].any()
    assert e5["d_ext"][..., :3].any() and not e5["d_ext"][..., 3:].any() and e5["d_ext"][~fg][:, :3].any()
    nofg = gr.reference(("nofg", 0))
    assert not nofg[0]["d_reg"].any() and nofg[1]["d_reg"].max() <= gr.TINY     # (the bound keeps its flush allowance)


def test_check_refuses_a_wrong_value_and_a_wrong_type():
    case = ("g3", 0)
    out = gr.emulate(*gc.args("g3"))
    gr.check(out, gr.reference(case))
    bad = {k: v.copy() for k, v in out.items()}
    bad["d_ext"][0, 0, 1] = np.inf
    with pytest.raises(AssertionError, match="not finite"):
        gr.check(bad, gr.reference(case))
    bad = {k: v.copy() for k, v in out.items()}
    bad["d_reg"][0, gc.G3_POINTS["TIE"], 0] *= np.float32(1.001)
    with pytest.raises(AssertionError, match="bound"):
        gr.check(bad, gr.reference(case))
    with pytest.raises(AssertionError):
        gr.check(dict(out, d_cls=out["d_cls"].astype(D)), gr.reference(case))


def test_the_c_entry_is_exported_under_abi_36_and_refuses_bad_arguments():
    """hn_fcos_loss_grad_f32: declared, bound and exported; the ABI stays 36; the forward entry's refusals, a null gradient table or
    level, d_ext without ext and an unaligned d_ext are refused with a message before any launch (the pointers are never
    followed: 64 stands for any aligned address); the build refuses scratch and VGPR spills in the kernel."""
    import re

    from hn_amd import _lib, build
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    proto = re.search(r"int\s+hn_fcos_loss_grad_f32\s*\(([^;]*)\)\s*;", text)
    assert proto and "hn_fcos_loss_grad_f32" in _lib.SIGNATURES and "#define HN_ABI_VERSION 36" in text
    res, args = _lib.SIGNATURES["hn_fcos_loss_grad_f32"]
    assert res is C.c_int and len(args) == len(proto.group(1).split(",")) == 21
    assert args[:17] == _lib.SIGNATURES["hn_fcos_loss_f32"][1][:17]            # the forward entry's arguments, then four more
    lv = _lib.FcosLevels()
    lv.num_levels = 1
    lv.h[0], lv.w[0], lv.stride[0] = 1, 1, 8
    lv.cls_lr[0] = lv.reg_ctr[0] = 64                      # (never dereferenced on the host)
    p = 64
    table = lambda v: (C.c_void_p * 1)(v)

    def call(c=3, boxes=p, g=4, ws=p, ext=None, up=None, d_cls=table(p), d_reg=table(p), d_ext=None):
        return lib.hn_fcos_loss_grad_f32(C.byref(lv), ext, 1, c, boxes, p, p, p, g, 1.5, p, p, p, None, ws, 64 * 2, up, d_cls, d_reg,
                                         d_ext, None)
    for kw, word in ((dict(boxes=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(g=0), b"outside 1..64"),
                     (dict(g=65), b"outside 1..64"), (dict(c=0), b"outside 1..8"), (dict(c=9), b"outside 1..8"),
                     (dict(d_cls=None), b"null pointer"), (dict(d_reg=None), b"null pointer"), (dict(d_cls=table(None)), b"null gradient level"),
                     (dict(d_ext=table(p)), b"d_ext goes with ext"), (dict(ext=table(p)), b"d_ext goes with ext"),
                     (dict(ext=table(p), d_ext=table(p + 8)), b"16-byte aligned"), (dict(up=p + 2), b"unaligned upstream")):
        assert call(**kw) != 0 and word in lib.hn_last_error(), (kw, lib.hn_last_error())
    rows = (build.CSRC / "build" / "fcos_loss.resources.txt").read_text().splitlines()
    row = [r for r in rows if "fcos_loss_grad_kernel" in r]
    assert len(row) == 1 and " vgpr_spill 0 " in row[0] and " scratch 0 " in row[0], row
    assert "fcos_loss_grad_kernel" in build.NO_SCRATCH_KERNELS


def test_the_python_surface_exists_and_is_off_by_default():
    """ops.fcos_loss_grad carries ops.fcos_loss's arguments and refusals (host tensors are refused like fcos_loss refuses them:
    there is no CPU fallback); FCOSCriterion is a parameter-free module that refuses anything but contiguous fp32 device tensors;
    head_grads exists on the engine and the drop-in; the drop-in's forward and training paths raise as before."""
    from fcos_utils.fcos import FCOS
    from hn_amd import criterion, fcos_engine, ops
    sig = inspect.signature(ops.fcos_loss_grad)
    assert list(sig.parameters) == ["cls_lr", "reg_ctr", "strides", "num_classes", "targets", "ext", "radius", "upstream",
                                    "want_forward", "out"]
    want = inspect.signature(ops.fcos_loss).parameters
    for name in ("ext", "radius", "out"):
        assert sig.parameters[name].default == want[name].default
    assert sig.parameters["upstream"].default is None and sig.parameters["want_forward"].default is False
    cls_lr, reg_ctr = [torch.zeros((1, 1, 1, 5))], [torch.zeros((1, 1, 1, 5))]
    targets = ops.FcosTargets(torch.zeros((1, 1, 4)), torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 1, 5)),
                              torch.zeros((1,), dtype=torch.int32))
    for fn in (ops.fcos_loss, ops.fcos_loss_grad):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(cls_lr, reg_ctr, (8,), 3, targets)
        with pytest.raises(ValueError, match="per level"):
            fn(cls_lr, reg_ctr, (8, 16), 3, targets)
        with pytest.raises(ValueError, match="num_classes = 9"):
            fn(cls_lr, reg_ctr, (8,), 9, targets)
    crit = criterion.FCOSCriterion(3, (8, 16, 32), ext=True, radius=2.0)
    assert isinstance(crit, torch.nn.Module) and not list(crit.parameters()) and not list(crit.buffers())
    assert (crit.num_classes, crit.strides, crit.ext, crit.radius) == (3, (8, 16, 32), True, 2.0)
    assert criterion.FCOSCriterion(2, (8,)).ext is False
    assert "channels_last" in criterion.FCOSCriterion.__doc__ and "permute(0, 2, 3, 1)" in criterion.FCOSCriterion.__doc__
    with pytest.raises(ValueError, match="contiguous fp32"):
        criterion.FCOSCriterion(3, (8,))(cls_lr, reg_ctr, targets)
    with pytest.raises(ValueError, match="one tensor per level"):
        criterion.FCOSCriterion(3, (8, 16))(cls_lr, reg_ctr, targets)
    with pytest.raises(ValueError, match="ext levels"):
        crit(cls_lr * 3, reg_ctr * 3, targets)
    assert callable(FCOS.head_grads) and callable(fcos_engine.FCOSEngine.head_grads)
    net = FCOS(num_classes=3)
    assert net._device_loss is False
    with pytest.raises(NotImplementedError):
        net.train()(images=[], targets=[{}])
    with pytest.raises(NotImplementedError):
        net.eval()(images=[], targets=[{}])
    assert "forward only" not in inspect.getmodule(FCOS).__doc__ and "forward only" not in ops.fcos_loss.__doc__
