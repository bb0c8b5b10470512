"""CPU tests: the resource usage the build recorded for the carrying tower kernel (conv_igemm_f16x3_carry_kernel) and for the
plain implicit-GEMM kernels beside it, and the host-side parts of the carried apply pass that need no GPU."""
import re

from hn_amd import _lib, build

# conv_igemm_f16x3_kernel<BM, BN, WM, WN, NBUF, BUF, RS, TERMS> -> (VGPRs, AGPRs, SGPRs, static LDS bytes per block) as the commit
# before the carried pass compiled them (the row-shared forms take their LDS dynamically: 0 here).  The carrying kernel lives in a
# translation unit of its own and includes the kernel header unchanged, so none of these may move.
PLAIN_BEFORE = {
    (128, 128, 2, 2, 2, 1, 1, 1): (128, 124, 88, 0),
    (128, 128, 2, 2, 2, 1, 0, 1): (128, 128, 87, 65536),
    (128, 128, 2, 2, 2, 1, 1, 3): (128, 126, 88, 0),
    (128, 128, 2, 2, 2, 1, 0, 3): (128, 128, 87, 65536),
    (128, 128, 2, 2, 2, 0, 0, 3): (128, 128, 87, 65536),
    (128, 64, 2, 2, 2, 1, 1, 1): (122, 32, 94, 0),
    (128, 64, 2, 2, 2, 1, 0, 1): (122, 32, 95, 49152),
    (128, 64, 2, 2, 2, 1, 1, 3): (128, 37, 94, 0),
    (128, 64, 2, 2, 2, 1, 0, 3): (122, 32, 95, 49152),
    (64, 64, 2, 2, 3, 1, 0, 1): (86, 16, 90, 49152),
    (64, 64, 2, 2, 3, 1, 0, 3): (102, 16, 103, 49152),
    (128, 32, 4, 1, 2, 1, 1, 1): (88, 16, 89, 0),
    (128, 32, 4, 1, 2, 1, 0, 1): (88, 16, 89, 40960),
    (128, 32, 4, 1, 2, 1, 1, 3): (89, 16, 89, 0),
    (128, 32, 4, 1, 2, 1, 0, 3): (88, 16, 89, 40960),
    (128, 32, 4, 1, 3, 1, 0, 1): (88, 16, 89, 61440),
    (128, 32, 4, 1, 3, 1, 0, 3): (88, 16, 89, 61440),
    (64, 128, 2, 2, 3, 1, 0, 1): (126, 32, 82, 73728),
    (64, 128, 2, 2, 3, 1, 0, 3): (128, 32, 94, 73728),
    (32, 64, 1, 2, 4, 1, 0, 1): (86, 16, 91, 49152),
    (32, 64, 1, 2, 4, 1, 0, 3): (102, 16, 104, 49152),
    (256, 64, 4, 1, 2, 1, 0, 1): (128, 126, 90, 81920),
    (256, 64, 4, 1, 2, 1, 0, 3): (128, 126, 90, 81920),
}


def _rows(stem):
    build.build_library()
    out = {}
    for line in (build.CSRC / "build" / (stem + ".resources.txt")).read_text().splitlines():
        name, rest = line.split(":", 1)
        f = rest.split()
        out[name] = {f[i]: f[i + 1] for i in range(0, len(f) - 1, 2)}
    return out


def _plain_key(name):
    m = re.search(r"23conv_igemm_f16x3_kernelI(.*?)EEvNS", name)
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1) + "E")) if m else None


def test_plain_kernels_compile_to_what_they_were():
    got = {}
    for name, r in _rows("conv_igemm_f16x3").items():
        key = _plain_key(name)
        if key is not None:
            got[key] = (int(r["VGPRs"]), int(r["AGPRs"]), int(r["SGPRs"]), int(r["lds"]))
    assert got == PLAIN_BEFORE


def test_carry_kernel_runs_from_registers_with_the_plain_kernels_lds():
    rows = {n: r for n, r in _rows("conv_igemm_f16x3_carry").items() if "conv_igemm_f16x3_carry_kernel" in n}
    assert len(rows) == 2                                        # TERMS = 3 and 1
    assert any(k in "conv_igemm_f16x3_carry_kernel" for k in build.NO_SPILL_KERNELS)   # the build's no-scratch rule covers the name
    for name, r in rows.items():
        terms = int(re.search(r"carry_kernelILi(\d)E", name).group(1))
        assert r["scratch"] == "0" and r["vgpr_spill"] == "0" and r["sgpr_spill"] == "0", (name, r)
        assert int(r["VGPRs"]) + int(r["AGPRs"]) <= 256, (name, r)
        assert r["occupancy"] == "2", (name, r)                   # two workgroups per CU, as the plain kernel
        assert int(r["lds"]) == PLAIN_BEFORE[(128, 128, 2, 2, 2, 1, 1, terms)][3], (name, r)


def test_entries_are_bound_and_refuse_bad_jobs_without_a_gpu():
    """The new entries are additive (no struct touched: the ABI version stays); argument errors of the carried job come back
    before any launch."""
    import ctypes as C
    lib = _lib.load()
    assert lib.hn_abi_version() == _lib.ABI_VERSION
    hw = (C.c_int32 * 3)(13600, 3400, 850)
    assert lib.hn_affine_split_f32_levels_streams(hw, 3, 32, 512) == 1      # batch 32: level 0 is 891 MB of fp32
    assert lib.hn_affine_split_f32_levels_streams(hw, 3, 4, 512) == 0       # 111 MB
    assert lib.hn_affine_split_f32_levels_streams(hw, 3, 5, 512) == 1       # 139 MB
    d = _lib.ConvDesc(n=2, h=9, w=13, cin=256, cout=256, r=3, s=3, stride=1, pad=1, dil=1, oh=9, ow=13, tile=1, splitk=-1)
    grp = _lib.ConvGroup()
    grp.count = 2
    for g, (h, w) in enumerate(((9, 13), (5, 7))):
        grp.x16[g], grp.w16[g], grp.y[g], grp.h[g], grp.w[g] = 4096, 8192, 65536 * (g + 1), h, w
    assert lib.hn_conv2d_f16x3_grouped_carry_applies(C.byref(d), C.byref(grp)) == 1
    grp.w[1] = 4                                                            # too narrow for the row-shared form
    assert lib.hn_conv2d_f16x3_grouped_carry_applies(C.byref(d), C.byref(grp)) == 0
    grp.w[1], d.tile = 7, 0                                                 # the heuristic's tile at this size is not 128 x 128
    assert lib.hn_conv2d_f16x3_grouped_carry_applies(C.byref(d), C.byref(grp)) == 0
    d.tile = 1
    lv = _lib.SplitLevels()
    lv.count = 1
    lv.hw[0], lv.x[0], lv.scale[0], lv.shift[0], lv.y16[0] = 12, 1 << 20, 2 << 20, 3 << 20, 4 << 20
    for kw, text in ((dict(c=96), b"power of two"), (dict(c=256, ys=500), b"bad strides"), (dict(c=256, x=(1 << 20) + 4), b"aligned"),
                     (dict(c=256, y=65536), b"must not touch")):
        lv.x[0], lv.y16[0] = kw.get("x", 1 << 20), kw.get("y", 4 << 20)
        st = lib.hn_conv2d_nhwc_f16x3_grouped_carry(C.byref(d), C.byref(grp), C.byref(lv), 1, 2, kw["c"], 512, 512, kw.get("ys", 1024), None)
        assert st == 1 and text in lib.hn_last_error(), (kw, lib.hn_last_error())


def test_engine_form_switch():
    from hn_amd import forms
    assert forms.ENGINE_DEFAULTS["tower_carry"] is True
    saved = dict(forms.ACTIVE)
    try:
        forms.apply_env({"HN_TOWER_CARRY": "0"})
        assert forms.engine_forms()["tower_carry"] is False
    finally:
        forms.ACTIVE.clear()
        forms.ACTIVE.update(saved)
