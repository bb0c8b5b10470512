"""GPU tests: the GroupNorm apply pass carried in the tail of a grouped tower convolution
(hn_conv2d_nhwc_f16x3_grouped_carry, ops.conv2d_nhwc_grouped(carry=...)) and the tower schedule built on it
(FCOSEngine.heads_grouped).  Everything is an equality of bits: the convolution is the plain kernel's body, the carried pass
the stand-alone pass's arithmetic.

Two shapes differ from the first sketch of these tests, because the library refuses them with or without a carried pass:
a 3 x 4 level cannot be a member of the row-shared launch (a 128-pixel tile crosses more row ends than the wide tile has gap
slots: W >= 5) and cannot emit GroupNorm partial sums (OH * OW >= 32).  The convolution's third level is 4 x 8 instead (the
smallest map that can do both), the refusal of the 3 x 4 member is a test of its own, and 3 x 4 stays a level of the CARRIED
tensor, where nothing restricts it."""
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

CONV_LEVELS = ((9, 13), (5, 7), (4, 8))
TILE_128x128 = 1
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def conv():
    """The small carrying convolution: 256 -> 256, 3 x 3, n = 2, three levels, written at channel offset 256 of 512-wide
    outputs with GroupNorm partial sums -- and its result without a carried pass, computed once."""
    from hn_amd import ops
    from hn_amd.weights import split_f16x3
    g = torch.Generator().manual_seed(4401)
    n = 2
    wide = [ops.to_split(torch.randn((n, h, w, 512), generator=g).cuda()) for h, w in CONV_LEVELS]
    wt = torch.randn((256, 3, 3, 256), generator=g) * (2.0 / (9 * 256)) ** 0.5
    cw = NS(w=wt.cuda(), bias=torch.randn((256,), generator=g).cuda(), w16=split_f16x3(wt).cuda())
    c = NS(n=n, xs=[x[:, :, :, 8:] for x in wide], cw=cw, wide=wide)

    def run(carry=None, terms=3, query=False):
        outs = [torch.full((n, h, w, 512), -7.0, device="cuda") for h, w in CONV_LEVELS]
        parts = [torch.full((ops.gn_rows32_scratch_floats(n * h * w, 512),), -3.0, device="cuda") for h, w in CONV_LEVELS]
        with ops.f16_terms(terms):
            r = ops.conv2d_nhwc_grouped(c.xs, [cw] * 3, pad=1, outs=outs, out_channel_offsets=[256] * 3,
                                        gn=[(p, 32) for p in parts], gn_units=64, tile=TILE_128x128, carry=carry, carry_query=query)
        return r if query else (outs, parts)
    c.run = run
    c.plain = {3: run(), 1: run(terms=1)}
    return c


def _carried(n, levels, seed, half=0, plant=None):
    """A [n,h,w,512] fp32 tensor per level, its tables, and the stand-alone pass on one channel half (the reference)."""
    g = torch.Generator().manual_seed(seed)
    xs = [(torch.randn((n, h, w, 512), generator=g) * 3.0).cuda() for h, w in levels]
    if plant is not None:
        lvl, idx, value = plant
        xs[lvl].view(-1)[idx] = value
    aff = [((torch.rand((n, 512), generator=g) + 0.5).cuda(), torch.randn((n, 512), generator=g).cuda()) for _ in levels]
    sl = slice(256 * half, 256 * (half + 1))
    return NS(xs=xs, aff=aff, half=[x[..., sl] for x in xs], tabs=[(sc[:, sl], sh[:, sl]) for sc, sh in aff], k=half)


def _dest(job):
    outs = [torch.full(tuple(x.shape[:3]) + (16, 2, 32), 0, device="cuda", dtype=torch.int16) for x in job.xs]
    for o in outs:
        o.fill_(SENTINEL)
    return [o.view(torch.float16) for o in outs]


def _check(conv, job, relu=True, terms=3):
    """One carrying launch against (plain launch, stand-alone pass): conv outputs and partial sums equal, the carried half
    equal as int16, the other half of the destination untouched."""
    from hn_amd import ops
    dst = _dest(job)
    blocks = [d[:, :, :, 8 * job.k:8 * (job.k + 1)] for d in dst]
    outs, parts = conv.run(carry=(job.half, job.tabs, blocks, relu), terms=terms)
    ref_outs, ref_parts = conv.plain[terms]
    for a, b in zip(outs + parts, ref_outs + ref_parts):
        assert torch.equal(a, b)
    ref = ops.to_split_levels(job.half, job.tabs, relu=relu)
    other = slice(8 * (1 - job.k), 8 * (2 - job.k))
    for d, r in zip(dst, ref):
        assert torch.equal(d[:, :, :, 8 * job.k:8 * (job.k + 1)].view(torch.int16), r.view(torch.int16))
        assert bool((d[:, :, :, other].view(torch.int16) == SENTINEL).all())


def test_launch_takes_the_row_shared_form_and_refuses_others(conv):
    """The small convolution carries (plain row-shared 128 x 128 form, forced tile); with a 3 x 4 member, or with the tile the
    heuristic picks at this size, the call is refused before anything is launched."""
    from hn_amd import ops
    assert conv.run(query=True) is True
    job = _carried(2, ((3, 4),), 1)
    dst = _dest(job)
    small = [ops.to_split(torch.randn((2, h, w, 256)).cuda()) for h, w in ((9, 13), (3, 4))]
    for kw in (dict(tile=TILE_128x128), dict()):
        xs = small if kw else conv.xs
        assert ops.conv2d_nhwc_grouped(xs, [conv.cw] * len(xs), pad=1, carry_query=True, **kw) is False
        with pytest.raises(RuntimeError, match="row-shared 128x128"):
            ops.conv2d_nhwc_grouped(xs, [conv.cw] * len(xs), pad=1, carry=(job.half, job.tabs, [d[:, :, :, :8] for d in dst], True), **kw)
    torch.cuda.synchronize()
    assert bool((dst[0].view(torch.int16) == SENTINEL).all())


def test_carried_pass_equals_stand_alone_pass_and_conv_is_unchanged(conv):
    _check(conv, _carried(2, CONV_LEVELS, 2))


@pytest.mark.parametrize("n,levels", [
    (2, ((40, 52), (20, 26), (10, 13))),     # 90 chunks on 12 workgroups: the grid-stride wrap; 2080 pixels = 32.5 chunks
    (2, ((3, 4),)),                          # fewer chunks than workgroups, a level smaller than one chunk
    (1, ((9, 13), (3, 4), (8, 8))),          # n = 1; 117 pixels = 1 chunk + 53; a whole chunk exactly (64)
    (3, ((5, 7), (11, 6))),                  # n = 3; 35 and 66 pixels
])
def test_chunk_coverage(conv, n, levels):
    _check(conv, _carried(n, levels, 3))


@pytest.mark.parametrize("relu,half", [(False, 0), (True, 1), (False, 1)])
def test_relu_off_and_the_other_half(conv, relu, half):
    _check(conv, _carried(2, CONV_LEVELS, 4, half=half), relu=relu)


@pytest.mark.parametrize("value,want", [(float("inf"), 1), (float("nan"), 1), (None, 0)])
def test_range_contract(conv, value, want):
    """One inf / NaN planted in the carried input sets the range flag exactly as the stand-alone pass does; clean input: 0."""
    from hn_amd import ops
    plant = None if value is None else (1, 5 * 512 + 17, value)        # level 1, pixel 5, channel 17 (cls half)
    job = _carried(2, CONV_LEVELS, 5, plant=plant)
    got = []
    for carried in (True, False):
        block = torch.zeros((4,), device="cuda", dtype=torch.int32)
        with ops.range_scope(block):
            if carried:
                dst = _dest(job)
                conv.run(carry=(job.half, job.tabs, [d[:, :, :, :8] for d in dst], True))
            else:
                ops.to_split_levels(job.half, job.tabs, relu=True)
        got.append(block.cpu().tolist())
    assert got[0] == got[1] and (got[0][0] != 0) == bool(want), got


def test_f16x1_terms(conv):
    _check(conv, _carried(2, CONV_LEVELS, 2), terms=1)


def test_engine_schedule_equals_lock_step_schedule(fcos_sd):
    """FCOSEngine.heads_grouped with the carried schedule (forced on at this size, tower launches on the 128 x 128 tile) and
    with tower_carry off (HN_TOWER_CARRY=0): every returned tensor equal; then the carried schedule under hipGraph capture,
    two replays."""
    from hn_amd import ops
    from hn_amd.fcos_engine import FCOSEngine
    eng = FCOSEngine(fcos_sd, 3, device="cuda")
    eng.tower_tile = TILE_128x128
    g = torch.Generator().manual_seed(6)
    feats = [ops.to_split(torch.randn((2, h, w, 256), generator=g).cuda()) for h, w in ((12, 16), (6, 8), (4, 8))]

    def run(carry):
        eng.tower_carry, eng.tower_carry_force = carry, carry
        with ops.f16_terms(eng.terms):
            return [t for lvl in eng.heads_grouped(feats) for t in lvl if t is not None]
    calls = []
    orig = ops.conv2d_nhwc_grouped
    ops.conv2d_nhwc_grouped = lambda *a, **kw: (calls.append(kw.get("carry") is not None), orig(*a, **kw))[1]
    try:
        on = run(True)
    finally:
        ops.conv2d_nhwc_grouped = orig
    assert sum(calls) == 5                                   # C1 R1 C2 R2 C3 carry; R3 does not
    off = run(False)
    assert len(on) == len(off) == 6
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    graph, outs = ops.capture_step(lambda: run(True))
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, off):
            assert torch.equal(a, b)
