"""hn_fcos_preprocess_f32, hn_fcos_preprocess_split (tiled <8, 96>, tiled <16, 160> and per-pixel) and hn_fcos_preprocess_list
against the float64 rule (tests/pre_ref.py) at the limits of the dispatch and of the tiled kernel's LDS patch
(tests/pre_cases.py): geometries whose need_r / need_c sit on the thresholds, fewer source pixels than a tile, image edges
inside a tile and inside the tile that holds the border, odd canvas widths, borders 0, 1 and 3, n = 1 .. 3.  Two assertions per
output: |err| <= the derived worst-case bound, and bit-equality with the fp32 emulation of the kernels' chain (every device
operation in it is a correctly rounded IEEE operation).  Every output lies in a sentinel-filled arena that must come back
untouched around it.  The ratios are printed; DESIGN.md section 5 holds the table measured on the MI355X."""
import numpy as np
import pytest
import torch

import pre_cases as pc
import pre_ref as pr

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in pc.CASES]
SENTINEL = -77.25            # an fp16 number
GUARD = 256                  # elements on either side of an output


def _arena(shape, dtype):
    size = int(np.prod(shape))
    arena = torch.full((size + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return arena, arena[GUARD:GUARD + size].view(shape)


def _intact(arena):
    torch.cuda.synchronize()
    return bool((arena[:GUARD] == SENTINEL).all()) and bool((arena[-GUARD:] == SENTINEL).all())


def _constant_inside(canvas, name):
    c = pc.BY_NAME[name]
    if c.kind == "const":
        oh, ow = c.geom[2:4]
        assert np.array_equal(canvas[:, :oh, :ow], np.broadcast_to(canvas[0, 0, 0], (c.n, oh, ow, canvas.shape[-1]))), name


@pytest.mark.parametrize("name", NAMES)
def test_fp32_canvas_is_inside_the_bound_and_equals_the_emulation(name):
    from hn_amd import ops
    c = pc.BY_NAME[name]
    h, w, oh, ow, ph, pw = c.geom
    x = torch.from_numpy(pc.make(name).copy()).cuda()
    arena, out = _arena((c.n, ph, pw, 4), torch.float32)
    got = ops.fcos_preprocess(x, oh, ow, ph, pw, pc.MEAN, pc.STD, out=out)
    assert got.data_ptr() == out.data_ptr() and _intact(arena)
    got = got.cpu().numpy()
    ratio = pr.check(got, pc.reference(name))
    print(f"pre gpu f32 {name}: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert np.array_equal(got, pc.emulated(name)), name
    _constant_inside(got, name)


@pytest.mark.parametrize("generic", [False, True], ids=["dispatch", "generic"])
@pytest.mark.parametrize("name", NAMES)
def test_split_image_is_inside_the_bound_and_equals_the_emulation(name, generic):
    """generic=False: the kernel preprocess_run picks (the case's `form`); True: the per-pixel kernel for every case"""
    from hn_amd import ops
    c = pc.BY_NAME[name]
    h, w, oh, ow, ph, pw = c.geom
    x = torch.from_numpy(pc.make(name).copy()).cuda()
    ops.set_form("preprocess_generic", generic)
    try:
        for b in pc.BORDERS:
            arena, out = _arena((2, c.n, ph + 2 * b, pw + 2 * b, 4), torch.float16)
            got = ops.fcos_preprocess_split(x, oh, ow, ph, pw, pc.MEAN, pc.STD, border=b, out=out)
            assert got.data_ptr() == out.data_ptr() and _intact(arena), (name, b)
            got = got.cpu().numpy()
            ratio = pr.check_split(got, pc.reference(name), b)
            print(f"pre gpu split {name} border {b} {'pp' if generic else c.form}: max |err| / bound = {ratio:.4f}")
            assert ratio <= 1.0
            assert np.array_equal(got, pr.split(pc.emulated(name), b)), (name, b)
            _constant_inside(got[0, :, b:, b:], name)
    finally:
        ops.set_form("preprocess_generic", False)


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split"])
def test_list_of_three_sizes_is_inside_the_bound_and_equals_the_emulation(split):
    """one upscaled, one downscaled and one 1 x 1 image on a common canvas, each with its own geometry row"""
    from hn_amd import ops
    ph, pw = pc.LIST_CANVAS
    rule, bound, emu = pc.list_reference()
    imgs = [torch.from_numpy(x.copy()).cuda() for x in pc.make_list()]
    for b in ((0, 1, 3) if split else (0,)):
        got = ops.fcos_preprocess_list(imgs, list(pc.LIST_GEOM), ph, pw, pc.MEAN, pc.STD, split=split, border=b).cpu().numpy()
        if split:
            ratio = pr.check_split(got, (rule, bound), b)
            assert np.array_equal(got, pr.split(emu, b)), b
        else:
            ratio = pr.check(got, (rule, bound))
            assert np.array_equal(got, emu)
        print(f"pre gpu list split={split} border {b}: max |err| / bound = {ratio:.4f}")
        assert ratio <= 1.0
