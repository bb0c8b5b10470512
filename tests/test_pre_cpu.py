"""The preprocess rule (tests/pre_ref.py) without a GPU: the rule against torch's bilinear resize in float64, the fp32 emulation
inside the bound on every case (and equal to F.interpolate where ATen's kernel takes the same order), the contract of the fp32
source coordinate, the dispatch mirror, the LDS patch sizes, and every mutant of the emulation outside the bound -- so check()
is known to be able to fail."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import pre_cases as pc
import pre_ref as pr

NAMES = [c.name for c in pc.CASES]
# largest source patch of any tile, over border 3 and 0, as emulated for the issue's table
PATCH = {"15x219-21x300": (7, 95), "10x186-14x254": (7, 95), "5x93-7x127": (5, 93), "15x220-21x300": (7, 95),
         "16x219-21x300": (8, 95), "13x157-7x127": (13, 157), "40x330-33x270": (11, 158), "3x2-41x259": (3, 2)}
CAPACITY = {"t8": (8, 96), "t16": (16, 160)}


def _norm(x, dtype):
    m = torch.tensor(pc.MEAN, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    s = torch.tensor(pc.STD, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return (torch.from_numpy(x.copy()).to(dtype) - m) / s


@pytest.mark.parametrize("name", NAMES)
def test_rule_is_torchs_bilinear_resize_in_float64(name):
    """The rule takes its taps and weights from the fp32 coordinate; torch in float64 computes the coordinate in float64.  The
    two differ by what the coordinate differs (pre_ref.coordinate_bound) times the local slope: |d out| <= dy |dv/dy| + dx |dv/dx|
    with the slopes bounded by the largest difference of neighbouring normalised pixels, plus 1e-12 for float64's own rounding."""
    c = pc.BY_NAME[name]
    h, w, oh, ow, ph, pw = c.geom
    v = _norm(pc.make(name), torch.float64)
    want = TF.interpolate(v, size=(oh, ow), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    got = pc.reference(name)[0]
    assert got.shape == (c.n, ph, pw, 4)
    dv_y = float((v[:, :, 1:] - v[:, :, :-1]).abs().max()) if h > 1 else 0.0
    dv_x = float((v[:, :, :, 1:] - v[:, :, :, :-1]).abs().max()) if w > 1 else 0.0
    tol = pr.coordinate_bound(h, oh)[None, :, None, None] * dv_y + pr.coordinate_bound(w, ow)[None, None, :, None] * dv_x + 1e-12
    assert (np.abs(got[:, :oh, :ow, :3] - want) <= tol).all()
    rest = got.copy()
    rest[:, :oh, :ow, :3] = 0
    assert not rest.any()


@pytest.mark.parametrize("h,w,oh,ow", [g[:4] for g in (c.geom for c in pc.CASES)] + list(pc.ATEN_AGREES))
def test_fp32_coordinate_is_within_its_bound_of_the_float64_one(h, w, oh, ow):
    """the contract: scale = (float)in / (float)out, real = fmaf(scale, dst + 0.5, -0.5); against (in / out)(dst + 0.5) - 0.5"""
    for n_in, n_out in ((h, oh), (w, ow)):
        scale = np.float32(n_in) / np.float32(n_out)
        dst = np.arange(n_out).astype(np.float32)
        real = pr.fma(np.full_like(dst, scale), dst + np.float32(0.5), np.full_like(dst, np.float32(-0.5)))
        exact = (float(n_in) / float(n_out)) * (np.arange(n_out) + 0.5) - 0.5
        assert (np.abs(real.astype(np.float64) - exact) <= pr.coordinate_bound(n_in, n_out)).all()
        i0, i1, l0, l1 = pr.src_index(n_in, n_out)
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0 + 1) | (i1 == n_in - 1)).all()
        assert l1.min() >= 0 and l1.max() < 1 and (l0.astype(np.float64) + l1 <= 1 + 2.0 ** -24).all()
        # l1 = real - i0 is exact
        r0 = np.maximum(real, np.float32(0))
        assert np.array_equal(l1.astype(np.float64), np.clip(r0.astype(np.float64) - i0, 0.0, 1.0))


@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_inside_the_bound_and_meets_no_midpoint(name):
    c = pc.BY_NAME[name]
    stats = {}
    out = pr.emulate(pc.make(name), *c.geom[2:], pc.MEAN, pc.STD, stats=stats)
    assert np.array_equal(out, pc.emulated(name))
    ratio = pr.check(out, pc.reference(name))
    print(f"pre emulate {name}: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert stats["midpoints"] == 0          # so the float64 emulation of fmaf rounds as a fused multiply-add does
    for b in pc.BORDERS:
        assert pr.check_split(pr.split(out, b), pc.reference(name), b) <= 1.0


def test_emulation_of_the_list_is_inside_the_bound():
    rule, bound, emu = pc.list_reference()
    assert pr.check(emu, (rule, bound)) <= 1.0
    for b in (0, 3):
        assert pr.check_split(pr.split(emu, b), (rule, bound), b) <= 1.0


@pytest.mark.parametrize("h,w,oh,ow", pc.ATEN_AGREES)
def test_emulation_is_f_interpolate_bit_for_bit_where_aten_takes_this_order(h, w, oh, ow):
    x = np.random.default_rng(h * 1000 + w).random((1, 3, h, w), dtype=np.float32)
    want = TF.interpolate(_norm(x, torch.float32), size=(oh, ow), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    stats = {}
    got = pr.emulate(x, oh, ow, oh, ow, pc.MEAN, pc.STD, stats=stats)
    assert stats["midpoints"] == 0
    assert np.array_equal(got[..., :3], want)


def test_a_constant_image_stays_constant_inside_the_rectangle():
    name = "30x40-50x66-const"
    c = pc.BY_NAME[name]
    h, w, oh, ow, ph, pw = c.geom
    out = pc.emulated(name)
    m, s = np.asarray(pc.MEAN, np.float32), np.asarray(pc.STD, np.float32)
    v = ((pc.make(name)[0, :, 0, 0] - m) / s).astype(np.float32)
    assert np.array_equal(out[:, :oh, :ow, :3], np.broadcast_to(v, (c.n, oh, ow, 3)))


@pytest.mark.parametrize("name", NAMES)
def test_form_of_names_the_kernel_of_each_row(name):
    c = pc.BY_NAME[name]
    for b in pc.BORDERS:
        assert pc.form_of(*c.geom, border=b, n=c.n) == c.form, (name, b)
        assert pc.form_of(*c.geom, border=b, n=c.n, generic=True) == "pp"
    if c.form != "pp":
        rows, cols = (max(pc.patch_of(*c.geom, b)[i] for b in pc.BORDERS) for i in (0, 1))
        assert rows <= CAPACITY[c.form][0] and cols <= CAPACITY[c.form][1], (name, rows, cols)
        if name in PATCH:
            assert (rows, cols) == PATCH[name]


def test_the_table_holds_every_form_and_the_limits():
    assert {c.form for c in pc.CASES} == {"t8", "t16", "pp"} and {c.n for c in pc.CASES} >= {1, 3}
    assert {c.kind for c in pc.CASES} == {"uniform", "const", "corners"}
    # an even canvas takes the tiled kernel where the odd one of the same geometry does not
    assert pc.form_of(13, 157, 7, 127, 9, 132) == "t16" and pc.form_of(37, 53, 97, 139, 97, 140) == "t8"
    # the workload's frame and the frames of test_tiled_preprocess_is_bit_identical_to_the_per_pixel_kernel
    assert pc.form_of(480, 640, 800, 1066, 800, 1088) == "t8"
    assert pc.form_of(1200, 1600, 800, 1066, 800, 1088) == "pp" and pc.form_of(900, 1200, 800, 1066, 800, 1088) == "t16"
    assert 1.0 < 900 / 800 <= 1.236 and 1.0 < 1200 / 1066 <= 1.236


@pytest.mark.parametrize("mutant", pr.MUTANTS)
def test_every_mutant_fails_on_its_case(mutant):
    name = pc.MUTANT_CASE[mutant]
    c = pc.BY_NAME[name]
    ref = pc.reference(name)
    if mutant in ("border_off_by_one", "lo_from_rounded"):       # mistakes of the split form: the fp32 canvas is right
        canvas = pr.emulate(pc.make(name), *c.geom[2:], pc.MEAN, pc.STD, mutant=mutant)
        assert np.array_equal(canvas, pc.emulated(name))
        with pytest.raises(AssertionError, match="bound"):
            pr.check_split(pr.split(canvas, 3, mutant=mutant), ref, 3)
    else:
        with pytest.raises(AssertionError, match="bound"):
            pr.check(pr.emulate(pc.make(name), *c.geom[2:], pc.MEAN, pc.STD, mutant=mutant), ref)


def test_clamp_mutants_hide_on_a_downscale():
    """why the table holds upscaling frames: below scale 1 the first coordinate is negative and the last lies past in - 1"""
    c = pc.BY_NAME["40x330-33x270"]
    for m in ("no_clamp0", "no_clamp_i1"):
        assert np.array_equal(pr.emulate(pc.make(c.name), *c.geom[2:], pc.MEAN, pc.STD, mutant=m), pc.emulated(c.name))


def test_check_refuses_a_nan_and_a_wrong_type():
    name = "3x2-41x259"
    out = pc.emulated(name)
    bad = out.copy()
    bad[0, 2, 3, 1] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        pr.check(bad, pc.reference(name))
    with pytest.raises(AssertionError):
        pr.check(out.astype(np.float64), pc.reference(name))
