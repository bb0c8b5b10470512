"""The smoothed live step (smooth=) without a GPU: the filter's numpy statement (tests/smooth_ref.py) --
its behaviour, its fp32 arithmetic against the float64 twin, the four rules against tables written out by hand --, the buffer
layouts, the new options and the C entry's argument checks, and the resource report."""
import inspect
import itertools
import math

import numpy as np
import pytest

import smooth_ref as sr

F = np.float32
DT = F(1 / 30)
PAPER = dict(min_cutoff=1.0, beta=0.007, d_cutoff=1.0)


def _run(xs, dt=DT, dtype=np.float32, **par):
    """A scalar signal through the filter (the first value initialises) -> the outputs.  float32: the reference, stepped on
    its own fp32 state; float64: the twin on a double state."""
    par = {**PAPER, **par}
    xh, dxh, out = dtype(F(xs[0])), dtype(0), [dtype(F(xs[0]))]
    for x in xs[1:]:
        if dtype is np.float32:
            xh, dxh = sr.one_euro(x, xh, dxh, dt, par["min_cutoff"], par["beta"], par["d_cutoff"])
        else:
            xh, dxh = _twin(x, xh, dxh, dt, **par)
        out.append(xh)
    return np.array(out, dtype)


def _twin(x, xp, dxp, dt, min_cutoff, beta, d_cutoff):
    """The float64 twin on a float64 state (one_euro rounds its state operands to fp32: right for stepping from an fp32 state,
    not for carrying a double one)."""
    two_pi, dt = np.float64(sr.TWO_PI), np.float64(F(dt))
    mc, b, dc, x = np.float64(F(min_cutoff)), np.float64(F(beta)), np.float64(F(d_cutoff)), np.float64(F(x))
    rd = (two_pi * dc) * dt
    ad = rd / (rd + 1)
    dx = (x - xp) / dt
    edx = dxp + ad * (dx - dxp)
    r = (two_pi * (mc + b * abs(edx))) * dt
    return xp + (r / (r + 1)) * (x - xp), edx


# ---------------------------------------------------------------------------------------------------------------------
# the filter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.0, 1.0, -312.4199, 0.4567, 1234.5])
def test_a_constant_input_gives_that_constant(c):
    out = _run([c] * 12)
    assert np.array_equal(out.view(np.int32), np.full(12, F(c)).view(np.int32))


def test_with_beta_zero_the_twin_is_the_fixed_alpha_ema():
    """beta = 0: fc = min_cutoff whatever the speed, so xh_n = xh_0 + sum of a (1 - a)^(n-k) (x_k - ...) -- the closed form of an
    exponential moving average with a = r / (r + 1), r = 2 pi min_cutoff dt."""
    rng = np.random.default_rng(0)
    xs = (100 * rng.standard_normal(40)).astype(F)
    got = _run(xs, dtype=np.float64, beta=0.0, min_cutoff=1.5)
    r = np.float64(sr.TWO_PI) * np.float64(F(1.5)) * np.float64(DT)
    a = r / (r + 1)
    for n in range(len(xs)):
        want = (1 - a) ** n * np.float64(xs[0]) + sum(a * (1 - a) ** (n - k) * np.float64(xs[k]) for k in range(1, n + 1))
        assert abs(got[n] - want) <= 1e-12 * 100 * (n + 1), n


@pytest.mark.parametrize("lo,hi", [(0.0, 10.0), (250.0, 180.0), (-0.3, 0.05)])
def test_a_step_input_rises_monotonically_between_old_and_new(lo, hi):
    out = _run([lo] * 3 + [hi] * 40).astype(np.float64)
    sign = 1 if hi > lo else -1
    assert np.all(sign * np.diff(out) >= 0)
    assert np.all(sign * (out - F(lo)) >= 0) and np.all(sign * (F(hi) - out) >= 0)
    assert sign * (out[-1] - out[3]) > 0.5 * abs(hi - lo)            # ... and it does move


def test_a_larger_beta_brings_the_output_closer_to_the_raw_value():
    """On a ramp (600 mm/s: the output lags below the input) any beta > 0 is at least as close as beta = 0 on every step --
    its cutoff is never lower, and xp + a (x - xp) grows with a and with xp while x >= xp --, and over the ramp and over a noisy
    walk the summed distance shrinks from each beta to the next."""
    rng = np.random.default_rng(1)
    ramp = (300 + 20 * np.arange(60)).astype(F)
    walk = (np.cumsum(20 * rng.standard_normal(60)) + 300).astype(F)
    betas = (0.0, 0.007, 0.07, 0.7)
    for xs in (ramp, walk):
        err = [np.abs(_run(xs, beta=b).astype(np.float64) - xs)[1:] for b in betas]
        for small, large in zip(err, err[1:]):
            assert large.sum() < small.sum()
        if xs is ramp:
            for e in err[1:]:
                assert np.all(e <= err[0])


def test_the_fp32_arithmetic_stays_close_to_the_float64_twin():
    """Stepped from the same fp32 state, over signals of the model's range (joints in camera millimetres: +-600 mm, metres
    for the mesh: +-0.6; per-step noise of a few units in 1e3; a jump now and then; dt between 1/120 and 1/10 s; states the
    filter itself produced): |fp32 - twin| <= 16 * 2**-24 * max(|x|, |xp|).  Each of the handful of rounded operations costs at
    most one ulp of the larger operand, and x - xp is exact when the two are close (Sterbenz)."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for scale, beta in ((600.0, 0.007), (0.6, 7.0)):
        for dt in (F(1 / 120), DT, F(0.1)):
            n = 4096
            x = (scale * rng.uniform(-1, 1, n)).astype(F)
            xh, dxh = x.copy(), np.zeros(n, F)
            for t in range(30):
                move = scale * 4e-3 * rng.standard_normal(n) + (rng.random(n) < 0.05) * scale * 0.2 * rng.standard_normal(n)
                x = (x + move).astype(F)
                got, edx = sr.one_euro(x, xh, dxh, dt, 1.0, beta, 1.0)
                twin, _ = sr.one_euro(x, xh, dxh, dt, 1.0, beta, 1.0, np.float64)
                assert got.dtype == np.float32 and twin.dtype == np.float64
                bound = 16 * 2.0 ** -24 * np.maximum(np.abs(x), np.abs(xh)).astype(np.float64)
                ratio = np.abs(got.astype(np.float64) - twin) / np.maximum(bound, 1e-300)
                worst = max(worst, float(ratio.max()))
                assert np.all(np.abs(got.astype(np.float64) - twin) <= bound), (scale, float(dt), t, float(ratio.max()))
                xh, dxh = got, edx
    print(f"worst |fp32 - twin| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# the rule, against tables written out by hand
# ---------------------------------------------------------------------------------------------------------------------
# dt = 0.5, min_cutoff = d_cutoff = 0.5 / (2 pi) as fp32, beta = 0: rd = r = (2 pi * cutoff) * dt, a = ad = r / (r + 1).  With
# these the table's numbers follow by hand from the rule: r = 0.25, a = 0.2 up to rounding -- computed below as the rule says.
T_DT = F(0.5)
T_CUT = F(0.5) / sr.TWO_PI


def _alpha():
    r = (sr.TWO_PI * T_CUT) * T_DT
    return r / (r + F(1))


def _rec(xh=0.0, dxh=0.0, tid=0):
    return [int(F(xh).view(np.int32)), int(F(dxh).view(np.int32)), tid, 0]


def _one(state, x, gate, tid):
    out, new = sr.step(np.array([state], np.int32), np.array([x], F), gate, tid, T_DT, T_CUT, 0.0, T_CUT)
    return out[0], new[0].tolist()


def test_table_initialise_then_filter():
    a = _alpha()
    assert abs(float(a) - 0.2) < 1e-6
    y, st = _one(_rec(), 10.0, True, 7)                          # rule 3: an empty record
    assert y == F(10) and st == _rec(10.0, 0.0, 7)
    y, st = _one(st, 20.0, True, 7)                              # rule 4: dx = 10 / 0.5 = 20, edx = a * 20, xh = 10 + a * 10
    edx = F(0) + a * (F(20) - F(0))
    xh = F(10) + a * (F(20) - F(10))
    assert y == xh and st == _rec(xh, edx, 7) and abs(float(xh) - 12.0) < 1e-5 and abs(float(edx) - 4.0) < 1e-5


def test_table_an_id_change_and_t_zero_initialise():
    st = _rec(10.0, 3.0, 7)
    y, new = _one(st, 20.0, True, 8)                             # another track in the slot: the output is x
    assert y == F(20) and new == _rec(20.0, 0.0, 8)
    y, new = _one(st, 20.0, True, 0)                             # t = 0: never filtered, and the record's id stays 0 ...
    assert y == F(20) and new == _rec(20.0, 0.0, 0)
    y, new = _one(new, 30.0, True, 0)                            # ... so the next step initialises again
    assert y == F(30) and new == _rec(30.0, 0.0, 0)
    y, new = _one(_rec(10.0, 3.0, 0), 20.0, True, 7)             # a record with id 0 is empty whatever else it holds
    assert y == F(20) and new == _rec(20.0, 0.0, 7)


def test_table_gate_off_and_on_again_restarts():
    st = _rec(10.0, 3.0, 7)
    y, new = _one(st, 20.0, False, 7)                            # rule 1 (a held slot keeps its id): 0, the record zeroed
    assert y == F(0) and not np.signbit(y) and new == [0, 0, 0, 0]
    y, new = _one(new, 25.0, True, 7)                            # back with the same id: the raw value, a fresh record
    assert y == F(25) and new == _rec(25.0, 0.0, 7)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_table_a_non_finite_x_passes_and_empties_the_record(bad):
    y, new = _one(_rec(10.0, 3.0, 7), bad, True, 7)              # rule 2
    assert (np.isnan(y) if np.isnan(bad) else y == bad) and new == [0, 0, 0, 0]
    y, new = _one(new, 11.0, True, 7)
    assert y == F(11) and new == _rec(11.0, 0.0, 7)
    y, new = _one(_rec(10.0, 3.0, 7), bad, False, 7)             # rule 1 comes first
    assert y == F(0) and new == [0, 0, 0, 0]


@pytest.mark.parametrize("word", [0, 1])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_table_a_non_finite_state_initialises(word, bad):
    st = _rec(10.0, 3.0, 7)
    st[word] = int(F(bad).view(np.int32))
    y, new = _one(st, 20.0, True, 7)                             # rule 3
    assert y == F(20) and new == _rec(20.0, 0.0, 7)


def test_step_slots_gates_and_betas():
    """xyz_mm follows has_hand, the mesh follows lifted, both the slot's track id; the vertices' beta is float32(1000 beta)."""
    rng = np.random.default_rng(3)
    slots, j, v = 3, 21, 5
    state = sr.empty_state(slots, j, v)
    xyz, mesh = (300 * rng.standard_normal((slots, j, 3))).astype(F), (0.3 * rng.standard_normal((slots, v, 3))).astype(F)
    has, lifted, tid = np.array([1, 1, 0]), np.array([1, 0, 0]), np.array([4, 5, 6])
    sx, sm, state = sr.step_slots(state, xyz, mesh, has, lifted, tid, DT)
    assert np.array_equal(sx[:2], xyz[:2]) and not sx[2].any() and np.array_equal(sm[0], mesh[0]) and not sm[1:].any()
    assert state.shape == (slots, j + v, 3, 4) and not state[2].any() and not state[1, j:].any() and not state[..., 3].any()
    assert (state[0, :, :, 2] == 4).all() and (state[1, :j, :, 2] == 5).all()
    xyz2, mesh2 = xyz + F(2.0), mesh + F(0.002)
    sx2, sm2, state2 = sr.step_slots(state, xyz2, mesh2, has, lifted, tid, DT)
    want_x, _ = sr.one_euro(xyz2[0], xyz[0], 0 * xyz[0], DT, 1.0, 0.007, 1.0)
    want_m, _ = sr.one_euro(mesh2[0], mesh[0], 0 * mesh[0], DT, 1.0, F(0.007 * 1000.0), 1.0)
    assert np.array_equal(sx2[0], want_x) and np.array_equal(sm2[0], want_m)
    assert np.all(np.abs(sx2[0] - xyz[0]) < 2.0) and np.all(sx2[0] != xyz2[0])
    # the same motion in the two units gives the same filter: (sm2 - mesh) * 1000 ~ sx2 - xyz
    assert np.allclose((sm2[0] - mesh[0]) * 1000, (sx2[0] - xyz[0])[:v], rtol=0, atol=5e-2)


# ---------------------------------------------------------------------------------------------------------------------
# layouts, surface, refusals
# ---------------------------------------------------------------------------------------------------------------------
def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items()}


@pytest.mark.parametrize("slots,frames", [(2, 1), (64, 32), (7, 7), (48, 3)])
def test_layouts(slots, frames):
    """smoothed=False is today's layout field for field, for every combination of the other options; smoothed=True adds only
    the two trailing parts, each on a dword."""
    import torch
    from hn_amd.live import LiveLayout, LiveSmoothedViews, LiveTrackedViews, LiveViews
    v, k = 778, slots // frames
    assert LiveSmoothedViews._fields == LiveTrackedViews._fields + ("smooth_xyz", "smooth_mesh")
    assert LiveTrackedViews._fields == LiveViews._fields + ("track_id", "track_age")
    old = ("frames", "hands", "vertices", "hw", "overlay", "labels", "handed", "tracked", "record_rows", "record_bytes", "side_at",
           "track_id_at", "track_age_at", "lifted_at", "mesh_at", "overlay_at", "box_label_at", "pose_label_at", "nbytes")
    for hw in ((480, 640), (5, 7)):                # (5 x 7 frames: the overlay ends off a dword)
        for overlay, labels, handed, tracked in itertools.product((False, True), repeat=4):
            a = LiveLayout(frames, k, v, hw, overlay, labels, handed, tracked)
            assert a == LiveLayout(frames, k, v, hw, overlay, labels, handed, tracked, False) and not a.smoothed
            assert a.smooth_xyz_at is None and a.smooth_mesh_at is None
            assert type(a.views(torch.zeros((a.nbytes,), dtype=torch.uint8))) is (LiveTrackedViews if tracked else LiveViews)
            if not tracked:
                with pytest.raises(ValueError):
                    LiveLayout(frames, k, v, hw, overlay, labels, handed, False, True)
                continue
            b = LiveLayout(frames, k, v, hw, overlay, labels, handed, True, True)
            for f in old[:-1]:
                assert getattr(a, f) == getattr(b, f), f
            assert b.smooth_xyz_at == (a.nbytes + 3) // 4 * 4 and b.smooth_mesh_at == b.smooth_xyz_at + slots * 21 * 12
            assert b.nbytes == b.smooth_mesh_at + slots * v * 12
            buf = torch.zeros((b.nbytes,), dtype=torch.uint8)
            bv = b.views(buf)
            assert type(bv) is LiveSmoothedViews
            for t, at, shape in ((bv.smooth_xyz, b.smooth_xyz_at, (slots, 21, 3)), (bv.smooth_mesh, b.smooth_mesh_at, (slots, v, 3))):
                assert t.data_ptr() - buf.data_ptr() == at and at % 4 == 0 and t.dtype == torch.float32 and tuple(t.shape) == shape
            av = a.views(buf[:a.nbytes])
            for name in LiveTrackedViews._fields:
                x, y = getattr(av, name), getattr(bv, name)
                assert (x is None and y is None) or (x.data_ptr() == y.data_ptr() and x.shape == y.shape and x.dtype == y.dtype), name
    with pytest.raises(ValueError):
        LiveLayout(frames, None, v, smoothed=True)


def test_read_types():
    from hn_amd.live import _HANDS_FIELDS, LiveHandsRead, _read_type
    assert _read_type("LiveHands", _HANDS_FIELDS, False, False, False) is LiveHandsRead
    tracked = _read_type("LiveHands", _HANDS_FIELDS, True, False, True, True)
    assert tracked._fields == _HANDS_FIELDS + ("overlay", "side", "track_age", "track_id")
    assert _read_type("LiveHands", _HANDS_FIELDS, True, False, True, True, False) is not None
    t = _read_type("LiveHands", _HANDS_FIELDS, True, False, True, True, True)
    assert t._fields == tracked._fields + ("smooth_xyz", "smooth_mesh") and t.box_label is None and t.pose_label is None
    assert t.__name__ == "LiveHandsOverlaySidedTrackedSmoothedRead"
    assert _read_type("LiveHands", _HANDS_FIELDS, False, False, False, True, True)._fields[-3:] == ("track_id", "smooth_xyz", "smooth_mesh")


def test_surface():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import ops
    from hn_amd.live import LiveHandsEngine, LiveHandsOutput
    for fn in (HandNet.live_hands, LiveHandsEngine.__init__):
        d = _defaults(fn)
        assert d.get("smooth") is False and d.get("smooth_min_cutoff") == 1.0 and d.get("smooth_beta") == 0.007, fn.__qualname__
        assert d.get("smooth_d_cutoff") == 1.0 and d.get("smooth_rate") == 30.0, fn.__qualname__
        assert list(d)[-5:] == ["smooth", "smooth_min_cutoff", "smooth_beta", "smooth_d_cutoff", "smooth_rate"]
    assert "smooth" not in _defaults(HandNet.live)
    for name in ("smooth_reset", "smooth_dt", "track_reset"):
        assert callable(getattr(LiveHandsEngine, name))
    assert [f for f in LiveHandsOutput.__dataclass_fields__][-2:] == ["smooth_xyz", "smooth_mesh"]
    d = _defaults(ops.mesh_finish_smooth)
    assert (d["min_cutoff"], d["beta"], d["d_cutoff"], d["mirror"]) == (1.0, 0.007, 1.0, None)
    assert ops.check_smooth_options() == (1.0, 0.007, 1.0, 30.0) == ops.check_smooth_options(1, 0.007, 1, 30)
    assert ops.check_smooth_options(0.5, 0, 2.0, 120) == (0.5, 0.0, 2.0, 120.0)
    for bad in ((0, .007, 1, 30), (-1, .007, 1, 30), (math.nan, .007, 1, 30), (math.inf, .007, 1, 30), (1, -1e-3, 1, 30),
                (1, math.nan, 1, 30), (1, math.inf, 1, 30), (1, 1e36, 1, 30), (1, .007, 0, 30), (1, .007, math.inf, 30),
                (1, .007, 1, 0), (1, .007, 1, -30), (1, .007, 1, math.inf), (1, .007, 1, math.nan), (1e-60, .007, 1, 30),
                ("x", .007, 1, 30), (1, .007, 1, 1e-50)):
        with pytest.raises(ValueError):
            ops.check_smooth_options(*bad)
    st = ops.smooth_state(3, 21, 7, "cpu")
    assert tuple(st.shape) == (3, 28, 3, 4) and st.dtype.is_floating_point is False and st.element_size() == 4 and not st.any()
    with pytest.raises(ValueError):
        ops.smooth_state(0, 21, 7, "cpu")


class _Part:
    device = "cpu"

    def set_convert(self, **_kw):
        return self


def test_smooth_needs_track_and_perm_reverse():
    """Refused in the constructor, before anything touches a device."""
    from hn_amd.live import LiveHandsEngine
    with pytest.raises(ValueError, match="track=True"):
        LiveHandsEngine(_Part(), _Part(), (1, 1, 0, 0), 2, smooth=True)
    with pytest.raises(ValueError, match="perm_reverse"):
        LiveHandsEngine(_Part(), _Part(), (1, 1, 0, 0), 2, track=True, smooth=True)
    with pytest.raises(ValueError, match="smooth_beta"):
        LiveHandsEngine(_Part(), _Part(), (1, 1, 0, 0), 2, perm_reverse=[0], track=True, smooth=True, smooth_beta=-1)
    with pytest.raises(ValueError, match="smooth_rate"):
        LiveHandsEngine(_Part(), _Part(), (1, 1, 0, 0), 2, perm_reverse=[0], track=True, smooth=True, smooth_rate=0)


def test_c_entry_refuses_bad_arguments_without_a_gpu():
    from hn_amd import _lib
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION
    for name in ("hn_mesh_finish_smooth_f32", "hn_smooth_state_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.hn_smooth_state_bytes(3, 21, 7) == 3 * 28 * 3 * 16 and lib.hn_smooth_state_bytes(32, 21, 778) == 32 * 799 * 48
    assert lib.hn_smooth_state_bytes(1 << 20, 21, 778) == (1 << 20) * 799 * 48          # (beyond 2^31 bytes)
    for bad in ((0, 21, 7), (3, 0, 7), (3, 21, 0), (-1, 21, 7)):
        assert lib.hn_smooth_state_bytes(*bad) == 0
    fake = 1 << 20
    names = ("mesh", "perm", "xyz_mm", "lifted", "has_hand", "mirror", "track_id", "dt", "state", "out", "smooth_xyz", "smooth_mesh")

    def call(dims=(2, 12, 7, 21), par=(1.0, 0.007, 7.0, 1.0), **ptrs):
        p = {n: fake for n in names}
        p.update(ptrs)
        return lib.hn_mesh_finish_smooth_f32(p["mesh"], p["perm"], p["xyz_mm"], p["lifted"], p["has_hand"], p["mirror"],
                                             p["track_id"], p["dt"], p["state"], *dims, *par, p["out"], p["smooth_xyz"],
                                             p["smooth_mesh"], None)
    err = lib.hn_last_error
    for n in names:
        if n != "mirror":                                       # (mirror may be NULL: the unsided step)
            assert call(**{n: None}) == 1 and b"hn_mesh_finish_smooth_f32: null pointer" in err(), n
    for off in (4, 8, 12):
        assert call(state=fake + off) == 1 and b"16-byte aligned" in err()
    for i in range(4):
        for bad in (0, -3):
            dims = [2, 12, 7, 21]
            dims[i] = bad
            assert call(dims=tuple(dims)) == 1 and b"bad dims" in err()
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(par=(bad, 0.007, 7.0, 1.0)) == 1 and b"min_cutoff and d_cutoff must be finite and > 0" in err()
        assert call(par=(1.0, 0.007, 7.0, bad)) == 1 and b"min_cutoff and d_cutoff must be finite and > 0" in err()
    for bad in (-1e-6, math.nan, math.inf, -math.inf):
        assert call(par=(1.0, bad, 7.0, 1.0)) == 1 and b"beta must be finite and >= 0" in err()
        assert call(par=(1.0, 0.007, bad, 1.0)) == 1 and b"beta must be finite and >= 0" in err()


def test_python_wrapper_refuses_before_a_device_is_touched():
    import torch
    from hn_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError, match="min_cutoff"):
        ops.mesh_finish_smooth(z((1, 4, 3)), z((4,), dtype=torch.int64), z((1, 21, 3)), None, None, None, None, None, min_cutoff=0)
    with pytest.raises(ValueError, match="beta"):
        ops.mesh_finish_smooth(z((1, 4, 3)), z((4,), dtype=torch.int64), z((1, 21, 3)), None, None, None, None, None, beta=-1.0)


def test_resource_report_shows_no_spill_no_scratch_no_lds():
    """The new kernel runs from registers (no scratch, no VGPR or SGPR spill), holds no LDS and no atomic, keeps contraction off
    inside itself and in the filter's function, and moves its state as one 16-byte vector per element; mesh_finish_kernel's own
    row is still there, once."""
    from hn_amd import _lib, build
    _lib.load()
    rows = (build.CSRC / "build" / "graph_ops.resources.txt").read_text().strip().splitlines()
    mine = [r for r in rows if "mesh_finish_smooth_kernel" in r.split(":")[0]]
    assert len(mine) == 1 and len([r for r in rows if "mesh_finish_kernel" in r.split(":")[0]]) == 1
    assert " scratch 0 " in mine[0] and "vgpr_spill 0" in mine[0] and "sgpr_spill 0" in mine[0], mine[0]
    src = (build.CSRC / "graph_ops.hip").read_text()
    kernel = src.split("void mesh_finish_smooth_kernel")[1].split("\n}\n")[0]
    helper = src.split("float one_euro(")[1].split("\n}\n")[0]
    for body in (kernel, helper):
        assert "fp contract(off)" in body and "__shared__" not in body and "atomic" not in body.lower()
    assert "u32x4* rec" in helper and helper.count("*rec") == 2           # one 16-byte load, one 16-byte store
