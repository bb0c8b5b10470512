"""The Python front ends of the convolution launches (hn_amd/ops.py): the profile record each of them appends, what an
unprofiled call leaves alone, and the launch-plan store of conv2d_nhwc / conv2d_nhwc_multi.  What the launches compute is
checked elsewhere (test_conv_gpu.py, test_stem_gpu.py); every shape here is one that those tests run the same front end on.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bank(g, cout, r, cin, stride=1, dil=1):
    from hn_amd.weights import ConvW
    wt = torch.randn((cout, r, r, cin), generator=g) * (2.0 / (r * r * cin)) ** 0.5
    return ConvW(wt, torch.randn((cout,), generator=g) * 0.1, stride, dil * (r // 2), dil).to("cuda")


def _pixels(n, sizes):
    return n * sum(h * w for h, w in sizes)


@pytest.fixture(scope="module")
def launches():
    """[(name, call, precision, MACs, shape)]: one launch through each of the eight front ends and the f32 kernel of
    conv2d_nhwc, with the record it has to leave.  MACs and shapes are written out by hand from the operand sizes."""
    from hn_amd import ops
    g = torch.Generator().manual_seed(2024)

    def s32(n, h, w, c):
        return ops.to_split(torch.randn((n, h, w, c), generator=g).cuda())

    out = []
    # conv2d_nhwc, the exact f32 kernel: 3x3 / pad 1, 8 -> 16 channels on 9 x 9 (Cin = 8 has no split bank)
    x32, b32 = torch.randn((1, 9, 9, 8), generator=g).cuda(), _bank(g, 16, 3, 8)
    assert b32.w16 is None
    out.append(("conv2d_nhwc f32", lambda: ops.conv2d_nhwc(x32, b32.w, b32.bias, pad=1, relu=True),
                "f32", 1 * 9 * 9 * 16 * 3 * 3 * 8, (1, 9, 9, 8, 16, 3, 1, 1)))
    # conv2d_nhwc, f16x3: 3x3 / pad 1, 32 -> 48 channels on 13 x 17, S32 input
    x16, b16 = s32(1, 13, 17, 32), _bank(g, 48, 3, 32)
    out.append(("conv2d_nhwc f16x3", lambda: ops.conv2d_nhwc(x16, b16.w, b16.bias, pad=1, relu=True, w16=b16.w16),
                "f16x3", 1 * 13 * 17 * 48 * 3 * 3 * 32, (1, 13, 17, 32, 48, 3, 1, 1)))
    # conv2d_nhwc_multi: 1x1 256 -> 128 beside the 1x1 / stride-2 downsample 256 -> 512 on 44 x 44 (output 22 x 22): the
    # second member is the larger one (by input pixels x Cin x Cout x R^2), so the record carries its shape
    items = _multi_items(g, s32)
    out.append(("conv2d_nhwc_multi", lambda: ops.conv2d_nhwc_multi(items),
                "f16x3", 44 * 44 * 128 * 256 + 22 * 22 * 512 * 256, (1, 44, 44, 256, 512, 1, 2, 1)))
    # conv2d_nhwc_grouped: one 3x3 bank 64 -> 128 on three maps of batch 2
    sizes = [(20, 28), (10, 14), (5, 7)]
    gx, gb = [s32(2, h, w, 64) for h, w in sizes], _bank(g, 128, 3, 64)
    rows = _pixels(2, sizes)
    out.append(("conv2d_nhwc_grouped", lambda: ops.conv2d_nhwc_grouped(gx, [gb] * 3, pad=1),
                "f16x3", rows * 128 * 9 * 64, (1, rows, 1, 64, 128, 3, 1, 1)))
    # conv3x3_thin_levels: 256 -> 8 channels on three maps of batch 3, inputs the first half of a 512-channel stack
    sizes = [(33, 47), (16, 16), (1, 1)]
    tx, tb = [s32(3, h, w, 512)[:, :, :, :8] for h, w in sizes], _bank(g, 8, 3, 256)
    trows = _pixels(3, sizes)
    out.append(("conv3x3_thin_levels", lambda: ops.conv3x3_thin_levels(tx, tb, relu_cols=3),
                "f16x3", trows * 8 * 9 * 256, (1, trows, 1, 256, 8, 3, 1, 1)))
    # conv3x3_thin_levels_group: a 5- and an 8-channel member on the two halves of one stack; the record's shape counts the
    # pixels of member 0 and the output channels of all members
    sizes = [(13, 17), (1, 2), (7, 300)]
    stacks = [s32(2, h, w, 512) for h, w in sizes]
    members = [([s[:, :, :, :8] for s in stacks], _bank(g, 5, 3, 256), 0), ([s[:, :, :, 8:] for s in stacks], _bank(g, 8, 3, 256), 4)]
    px = _pixels(2, sizes)
    out.append(("conv3x3_thin_levels_group", lambda: ops.conv3x3_thin_levels_group(members),
                "f16x3", px * (5 + 8) * 9 * 256, (1, px, 1, 256, 13, 3, 1, 1)))
    # conv3x3_thin_affine_levels: the second 256 of 512 raw tower channels -> 5, two small maps of batch 300 (the smallest
    # problem of test_conv_gpu that the fused kernel takes)
    sizes = [(13, 17), (7, 9)]
    gg = torch.Generator(device="cuda").manual_seed(2025)
    ts = [torch.randn((300, h, w, 512), generator=gg, device="cuda") * 3 for h, w in sizes]
    aff = [(torch.rand((300, 512), generator=gg, device="cuda") + 0.5, torch.randn((300, 512), generator=gg, device="cuda")) for _ in sizes]
    ab = _bank(g, 5, 3, 256)
    assert ops.thin_affine_applies(ts, ab)
    arows = _pixels(300, sizes)
    out.append(("conv3x3_thin_affine_levels", lambda: ops.conv3x3_thin_affine_levels(ts, aff, 256, ab, relu_cols=4),
                "f16x3", arows * 5 * 9 * 256, (1, arows, 1, 256, 5, 3, 1, 1)))
    # the stem forms: an 8 x 10 image with its 3-pixel border, 7x7 / stride 2 -> 4 x 5; the MACs count the 3 real channels
    img = torch.zeros((2, 1, 14, 16, 4), device="cuda", dtype=torch.float16)
    w7, bias = torch.zeros((64, 7, 2, 32), device="cuda", dtype=torch.float16), torch.zeros((128,), device="cuda")
    stem = (1 * 4 * 5 * 64 * 7 * 7 * 3, (1, 8, 10, 4, 64, 7, 2, 1))
    out.append(("conv_stem_split", lambda: ops.conv_stem_split(img, w7, bias, 64), "f16x3") + stem)
    out.append(("conv_stem_pool_split", lambda: ops.conv_stem_pool_split(img, w7, bias), "f16x3") + stem)
    return out


def _multi_items(g, s32):
    """Two members of different shape (test_conv_gpu.py, "bottleneck_ds")"""
    return [(s32(1, 44, 44, 256), _bank(g, 128, 1, 256), dict(relu=True)),
            (s32(1, 44, 44, 256), _bank(g, 512, 1, 256, stride=2), dict(relu=False))]


def test_every_front_end_leaves_one_profile_record(launches):
    from hn_amd import ops
    old = ops.CONV_PROFILE, ops.PROFILE_STAGE
    try:
        for name, call, precision, macs, shape in launches:
            ops.CONV_PROFILE, ops.PROFILE_STAGE = [], "t"
            call()
            torch.cuda.synchronize()
            assert len(ops.CONV_PROFILE) == 1, name
            record = ops.CONV_PROFILE[0]
            assert isinstance(record, tuple) and len(record) == 5, name
            kind, got_macs, timer, got_shape, stage = record
            assert kind[0] == precision, (name, kind)
            assert got_macs == macs, (name, got_macs, macs)
            assert got_shape == shape, (name, got_shape, shape)
            assert stage == "t", name
            assert timer.elapsed_ms() > 0, name
            label = ops.tile_name(kind[1])
            assert isinstance(label, str) and label, (name, kind)
            if name == "conv2d_nhwc_multi":
                assert kind[1] & ops.TILE_MULTI
    finally:
        ops.CONV_PROFILE, ops.PROFILE_STAGE = old


def test_an_unprofiled_call_creates_no_timer_and_asks_the_library_nothing(launches, monkeypatch):
    from hn_amd import _lib, ops

    class NoTimer:
        def __init__(self):
            raise AssertionError("an unprofiled launch created a HipTimer")

    def no_query(*a):
        raise AssertionError("an unprofiled launch made a query that only the profile record needs")

    assert ops.CONV_PROFILE is None
    monkeypatch.setattr(ops, "HipTimer", NoTimer)
    lib = _lib.load()
    for query in ("hn_conv2d_f16x3_pick_tile", "hn_conv2d_pick_tile", "hn_conv2d_f16x3_uses_halo", "hn_conv2d_f16x3_uses_stream",
                  "hn_conv2d_f16x3_uses_rs", "hn_conv3x3_thin_uses_flat"):
        monkeypatch.setattr(lib, query, no_query)
    ops.clear_plan_caches()      # the conv2d_nhwc / multi launches below go the whole way, not through a stored plan
    for name, call, *_ in launches:
        assert call() is not None, name
        assert ops.CONV_PROFILE is None, name
    torch.cuda.synchronize()


def test_plan_store_of_conv2d_nhwc():
    """S32 input, split bank, out=None: the call that stores a plan and the call that replays it.  1x1 1024 -> 256 on
    11 x 11 with the 32x64 tile, the shape that test_conv_gpu.py runs with force_splits=2."""
    from hn_amd import ops
    g = torch.Generator().manual_seed(7)
    x = ops.to_split(torch.randn((1, 11, 11, 1024), generator=g).cuda())
    cw = _bank(g, 256, 1, 1024)

    def call(**kw):
        return ops.conv2d_nhwc(x, cw.w, cw.bias, relu=True, tile=7, w16=cw.w16, **kw)
    ops.clear_plan_caches()
    assert len(ops._PLANS) == 0
    first = call()
    assert len(ops._PLANS) == 1
    again = call()
    assert len(ops._PLANS) == 1 and torch.equal(first, again)
    call(force_splits=2)                                    # a sweep's call is never stored
    assert len(ops._PLANS) == 1
    with ops.f16_terms(1):                                  # another term count: a plan of its own, not the 3-term one
        one_term = call()
    assert len(ops._PLANS) == 2 and not torch.equal(one_term, first)
    assert torch.equal(call(), first)
    ops.clear_plan_caches()
    assert len(ops._PLANS) == 0 and len(ops._DESC_TEMPLATES) == 0
    with ops.f16_terms(1):
        fresh = call()
    assert torch.equal(one_term, fresh)
    ops.clear_plan_caches()


def test_plan_store_of_conv2d_nhwc_multi():
    from hn_amd import ops
    g = torch.Generator().manual_seed(8)
    items = _multi_items(g, lambda n, h, w, c: ops.to_split(torch.randn((n, h, w, c), generator=g).cuda()))
    ops.clear_plan_caches()
    first = ops.conv2d_nhwc_multi(items)
    assert len(ops._PLANS) == 1
    again = ops.conv2d_nhwc_multi(items)
    assert len(ops._PLANS) == 1 and all(torch.equal(a, b) for a, b in zip(first, again))
    fused = []
    asked = ops.conv2d_nhwc_multi(items, fused=fused)       # goes the whole way, and adds no entry
    assert len(fused) == 1 and len(ops._PLANS) == 1 and all(torch.equal(a, b) for a, b in zip(first, asked))
    with ops.f16_terms(1):
        one_term = ops.conv2d_nhwc_multi(items)
    assert len(ops._PLANS) == 2 and not torch.equal(one_term[0], first[0])
    ops.clear_plan_caches()
    assert len(ops._PLANS) == 0
    with ops.f16_terms(1):
        fresh = ops.conv2d_nhwc_multi(items)
    assert all(torch.equal(a, b) for a, b in zip(one_term, fresh))
    ops.clear_plan_caches()
