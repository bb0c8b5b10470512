"""Mirror mode (left=) and per-slot handedness (handed=, left_side=) of the live chain: the surface, the buffer layouts, the new
entry points of the C ABI, and the numpy statement of the un-mirror rules (tests/handed_ref.py) against the oracle's lifter
input.  No GPU."""
import inspect

import numpy as np
import pytest

import handed_ref as hr


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items()}


def test_the_five_callables_carry_handed_and_left_side():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd.live import LiveHandsEngine
    from hn_amd.pipeline import HandNetEngine
    for fn in (HandNetEngine.forward_hands, HandNetEngine.graphed_hands, HandNet.forward_hands, HandNet.live_hands,
               LiveHandsEngine.__init__):
        d = _defaults(fn)
        assert d.get("handed") is False and d.get("left_side") == 0 and type(d["left_side"]) is int, fn.__qualname__


def test_left_is_on_both_live_entries_and_both_engines():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd.live import LiveHandEngine, LiveHandsEngine, _LiveStep
    for fn in (HandNet.live, HandNet.live_hands, LiveHandEngine.__init__, LiveHandsEngine.__init__, _LiveStep.__init__):
        assert _defaults(fn).get("left") is False, fn.__qualname__
    # next to faces and labels on the shared step
    names = list(inspect.signature(_LiveStep.__init__).parameters)
    assert names.index("left") == names.index("labels") + 1 == names.index("faces") + 2


def test_ops_surface():
    from hn_amd import ops
    assert _defaults(ops.ingest_raw).get("flip_w") is False
    assert callable(ops.flip_w)
    assert _defaults(ops.crop_resize_hands).get("handed") is False and _defaults(ops.crop_resize_hands).get("left_side") == 0
    assert _defaults(ops.lifter_input_gated).get("mirror", 0) is None and _defaults(ops.mesh_finish).get("mirror", 0) is None


def test_left_with_handed_is_refused():
    """Before anything touches a device: the engine's constructor and the drop-in's live_hands."""
    import types
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd.live import LiveHandsEngine
    fake = types.SimpleNamespace(device="cuda:0")
    with pytest.raises(ValueError, match="left"):
        LiveHandsEngine(fake, fake, (1.0, 1.0, 0.0, 0.0), 2, left=True, handed=True)
    with pytest.raises(ValueError, match="left"):
        HandNet.live_hands(object.__new__(HandNet), None, (1.0, 1.0, 0.0, 0.0), left=True, handed=True)


@pytest.mark.parametrize("slots,frames", [(2, 1), (64, 32), (7, 7), (48, 3)])
def test_layouts(slots, frames):
    """handed=False: today's numbers (restated here from the record format); handed=True: exactly 4 bytes per slot more, the
    sides behind the score and rank rows and everything behind them moved up by as much."""
    from hn_amd.live import LiveLayout
    from hn_amd.pipeline import hands_record_rows, record_bytes
    v, h, w = 778, 480, 640
    rb = record_bytes(3)
    assert rb == 800
    rows = slots + 1 + (8 * slots + rb - 1) // rb
    assert hands_record_rows(slots, rb) == hands_record_rows(slots, rb, False) == rows
    today = (rows, rb, rows * rb, rows * rb + 4 * slots, rows * rb + 4 * slots + slots * v * 12)
    k = slots // frames
    named = lambda a: (a.record_rows, a.record_bytes, a.lifted_at, a.mesh_at, a.nbytes)
    behind = ("lifted_at", "mesh_at", "overlay_at", "box_label_at", "pose_label_at", "nbytes")
    plain = LiveLayout(frames, k, v)
    assert named(plain) == named(LiveLayout(frames, k, v, handed=False)) == today and plain.side_at is None
    got = LiveLayout(frames, k, v, handed=True)
    assert named(got)[:2] == today[:2] and tuple(g - t for g, t in zip(named(got)[2:], today[2:])) == (4 * slots,) * 3
    assert got.side_at == rows * rb
    for overlay in (False, True):
        for labels in (False, True):
            a = LiveLayout(frames, k, v, (h, w), overlay, labels)
            assert a == LiveLayout(frames, k, v, (h, w), overlay, labels, False) and a.side_at is None
            b = LiveLayout(frames, k, v, (h, w), overlay, labels, True)
            assert b.side_at == rows * rb and (b.record_rows, b.record_bytes) == (a.record_rows, a.record_bytes)
            for f in behind:            # `lifted` and everything behind it: 4 bytes per slot further, or not there in both
                x, y = getattr(a, f), getattr(b, f)
                assert (x is None and y is None) or y - x == 4 * slots, f
            assert (a.overlay_at is not None) == overlay and (a.box_label_at is not None) == labels == (a.pose_label_at is not None)
    # the engine's own to_host record: whole rows, the sides behind the scores and ranks
    assert hands_record_rows(slots, rb, True) == slots + 1 + (12 * slots + rb - 1) // rb


def test_new_symbols_and_version():
    from hn_amd import _lib
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION
    for name in ("hn_ingest_u8bgr_u16mm_flip", "hn_flip_w_f32", "hn_crop_resize_hands_sided", "hn_a2j_aggregate_convert_mirror_f32",
                 "hn_lifter_input_gated_mirror_f32", "hn_mesh_finish_mirror_f32"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    fake = 1 << 20
    # argument checks come before any launch: null pointers and bad sizes are refused on a machine without a GPU
    assert lib.hn_flip_w_f32(None, fake, 4, None, None, 0, 8, None) == 1 and b"null pointer" in lib.hn_last_error()
    assert lib.hn_flip_w_f32(fake, fake, 4, None, None, 0, 8, None) == 1 and b"in place" in lib.hn_last_error()
    assert lib.hn_flip_w_f32(fake, 2 * fake, 0, None, None, 0, 8, None) == 1
    assert lib.hn_lifter_input_gated_mirror_f32(fake, fake, None, 2, 21, fake, fake, None) == 1
    assert lib.hn_lifter_input_gated_mirror_f32(fake, fake, fake, 0, 21, fake, fake, None) == 0      # nothing to do: no launch
    assert lib.hn_mesh_finish_mirror_f32(fake, None, fake, None, fake, 1, 8, 8, 21, fake, None) == 1   # perm and xyz_mm go together
    assert lib.hn_mesh_finish_mirror_f32(fake, None, None, None, fake, 1, 8, 4, 21, fake, None) == 1   # no perm: v == v0
    assert lib.hn_mesh_finish_mirror_f32(fake, fake, fake, None, None, 1, 8, 8, 21, fake, None) == 1
    assert lib.hn_ingest_u8bgr_u16mm_flip(None, None, 0, fake, None, None, 1, 4, 4, 1, None) == 1
    assert b"hn_ingest_u8bgr_u16mm_flip" in lib.hn_last_error()
    args = [fake] * 5 + [8, 2, 0, 2, fake, 1, 1, 0, 480, 640, 176, 4] + [fake] * 4
    assert lib.hn_crop_resize_hands_sided(*args, None, fake, fake, None) == 1 and b"null pointer" in lib.hn_last_error()
    assert lib.hn_a2j_aggregate_convert_mirror_f32(fake, fake, fake, None, None, 1, 11, 11, 21, 16, fake, 176.0, 176.0, None, None,
                                                   fake, fake, None, None) == 1


# ---------------------------------------------------------------------------------------------------------------------
# rules 3-5 against the oracle's lifter input
# ---------------------------------------------------------------------------------------------------------------------
# The oracle (oracle/pose2mesh_ref.py:lifter_input) walks the caller's chain in float32: bounding box, centre and scale, an
# affine map and the standardisation, each rounded at the magnitude of the pixel coordinates it sees.  Mirroring moves every
# x to another magnitude (u -> c - u), so the roundings of the mirrored chain are other roundings: the identity "oracle of the
# mirrored joints == the oracle's plain output with column 0 negated" holds to the chain's own float32 noise, not to the bit.
# Largest difference over the golden joint sets that pass the gate, c = 640 (the frame) and c = 176 (a crop): 2.861023e-06
# (set 2, c = 640); the bound is 4x that.
ORACLE_F32_WORST = 2.861023e-06
ORACLE_F32_BOUND = 4 * ORACLE_F32_WORST
# In float64 the same identity, on the rule the kernel evaluates ((x - mean) / std in float64): the mean of the mirrored
# joints is c - mean up to the rounding of a 21-term float64 sum of values below 2^10 (21 * 2^10 * 2^-53 = 2.4e-12 at worst),
# over a std of at least a pixel for a set that passes the gate.
F64_BOUND = 2.4e-12


@pytest.mark.parametrize("c", [640.0, 176.0])
def test_mirror_rule_against_the_oracle(golden_dir, c):
    from oracle import pose2mesh_ref
    g = np.load(golden_dir / "lifter_input.npz")
    uv, ok = g["joints"].astype(np.float32), g["ok"].astype(bool)
    assert uv.shape[0] == 24 and int(ok.sum()) == 22
    worst32 = worst64 = 0.0
    for i in range(uv.shape[0]):
        mirrored = hr.mirror_joints(uv[i], np.float32(c))
        plain, mir = pose2mesh_ref.lifter_input(uv[i]), pose2mesh_ref.lifter_input(mirrored)
        # the gate flag is the same for the mirrored and the plain joints
        assert (plain is not None) == (mir is not None) == bool(ok[i]), i
        if not ok[i]:
            continue
        want = hr.lifter_input_mirrored(plain[None], [1])[0]
        assert np.array_equal(want[:, 1], plain[:, 1]) and np.array_equal(want[:, 0], -plain[:, 0])
        worst32 = max(worst32, float(np.abs(mir - want).max()))
        u64 = uv[i].astype(np.float64)
        a = hr.standardize64(u64)
        a[:, 0] = -a[:, 0]
        worst64 = max(worst64, float(np.abs(hr.standardize64(hr.mirror_joints(u64, c)) - a).max()))
        # ... and the rule is the oracle's own output to the float32 noise of its chain (as the gate kernel's test bounds it)
        assert float(np.abs(a.astype(np.float32) - mir).max()) < 3e-5, i
    print(f"c = {c}: oracle(mirrored) vs -column 0 of oracle(plain): float32 chain {worst32:.6e}, float64 rule {worst64:.3e}")
    assert worst32 <= ORACLE_F32_BOUND
    assert worst64 <= F64_BOUND


def test_unmirror_and_final_mesh_rules_are_involutions():
    """Rule 3 twice is the identity up to one rounding; rule 5 reflects the final mesh's x about the root joint's x."""
    rng = np.random.default_rng(3)
    kp = rng.uniform(0, 176, size=(4, 21, 3)).astype(np.float32)
    once = hr.unmirror_keypoints(kp, [1, 0, 1, 0])
    assert np.array_equal(once[1], kp[1]) and np.array_equal(once[0, :, 0], np.float32(176) - kp[0, :, 0])
    assert np.array_equal(once[..., 1:], kp[..., 1:])
    assert np.abs(hr.unmirror_keypoints(once, [1, 0, 1, 0]) - kp).max() <= 176 * 2.0 ** -24
    raw = rng.normal(0, 0.04, size=(12, 3)).astype(np.float32)
    perm, xyz0 = rng.permutation(12)[:9], np.array([31.5, -12.25, 640.0], np.float32)
    plain, mirrored = hr.final_mesh_mirrored(raw, perm, xyz0, 0), hr.final_mesh_mirrored(raw, perm, xyz0, 1)
    assert np.array_equal(plain[:, 1:], mirrored[:, 1:])
    root_x = xyz0[0] / np.float32(1000.)
    assert np.abs((plain[:, 0] - root_x) + (mirrored[:, 0] - root_x)).max() < 1e-6
    assert np.array_equal(hr.final_mesh_mirrored(raw, None, None, 1), raw * np.array([-1, 1, 1], np.float32))


def test_resource_report_shows_no_spill_and_no_scratch():
    """The build guards of the neighbouring kernels hold for every kernel this feature adds or changes: no scratch, no VGPR
    or SGPR spill, in every instantiation (the build also refuses packed-fp32 op_sel in all of them)."""
    from hn_amd import _lib, build
    _lib.load()
    want = {"ingest.resources.txt": {"ingest_kernel": 4, "flip_w_kernel": 2},
            "crop_stage.resources.txt": {"hand_slots_kernel": 2, "hand_crop_gather_kernel": 2},
            "a2j_ops.resources.txt": {"a2j_aggregate_kernel": 1, "lifter_input_gated_kernel": 1},
            "graph_ops.resources.txt": {"mesh_finish_kernel": 1}}
    for name, kernels in want.items():
        rows = (build.CSRC / "build" / name).read_text().strip().splitlines()
        for kernel, count in kernels.items():
            mine = [r for r in rows if kernel in r.split(":")[0]]
            assert len(mine) == count, (kernel, len(mine))
            for r in mine:
                assert " scratch 0 " in r and "vgpr_spill 0" in r and "sgpr_spill 0" in r, r
    # results compared bit for bit: contraction off for the crop stage's file, and inside mesh_finish_kernel
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["crop_stage.hip"]
    assert "fp contract(off)" in (build.CSRC / "graph_ops.hip").read_text().split("void mesh_finish_kernel")[1].split("}")[0]
