"""The smoothed live step on the GPU (smooth=): the kernel against tests/smooth_ref.py byte for byte, step
by step, into canary-framed views; then the engine -- against the tracked step, against the reference run on the host over
what read() hands out, eager against captured, and the state's handling (captures, smooth_dt, smooth_reset)."""
import numpy as np
import pytest
import torch

import smooth_ref as sr
from test_track_gpu import PARAS, _frames, _same, _step, gate, parts  # noqa: F401  (the tracker tests' fixtures)

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
J = 21
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: ops.mesh_finish_smooth
# ---------------------------------------------------------------------------------------------------------------------
def _views(slots, v):
    """out, smooth_xyz, smooth_mesh and the state as views into one canary-filled buffer, four canary words between neighbours
    (every view starts on 16 bytes)."""
    sizes = [("out", slots * v * 3), ("smooth_xyz", slots * J * 3), ("state", slots * (J + v) * 3 * 4), ("smooth_mesh", slots * v * 3)]
    spans, end = {}, 4
    for name, words in sizes:
        spans[name] = (end, end + words)
        end = (end + words + 3) // 4 * 4 + 4
    buf = torch.full((end,), CANARY, dtype=torch.int32, device="cuda")
    cut = {name: buf[a:b] for name, (a, b) in spans.items()}
    views = dict(out=cut["out"].view(torch.float32).view(slots, v, 3), smooth_xyz=cut["smooth_xyz"].view(torch.float32).view(slots, J, 3),
                 smooth_mesh=cut["smooth_mesh"].view(torch.float32).view(slots, v, 3), state=cut["state"].view(slots, J + v, 3, 4))
    outside = torch.ones((end,), dtype=torch.bool)
    for a, b in spans.values():
        outside[a:b] = False
    return buf, views, outside.cuda()


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


def _check_step(t, v, outside, buf, want_out, ref):
    sx, sm, state = ref
    assert bool((buf[outside] == CANARY).all()), f"step {t}: a word outside the outputs was written"
    assert torch.equal(v["out"].view(torch.int32), want_out.view(torch.int32)), f"step {t}: out is not mesh_finish's"
    for name, want in (("smooth_xyz", sx), ("smooth_mesh", sm), ("state", state)):
        got = _bits(v[name])
        bad = np.argwhere(got != want.view(np.int32))
        assert bad.size == 0, (t, name, len(bad), bad[:4].tolist())


# per step: track id, has_hand, lifted, mirror per slot, and dt -- every rule fires:
#   slot 0: the id changes at step 3 (rule 3); lifted goes off at step 4 while has_hand stays on (the mesh restarts, the joints go on)
#   slot 1: t = 0 on steps 0 and 1 (never filtered), then track 3; its mirror flag flips at steps 4 and 6
#   slot 2: gated off at steps 2, 3 and 6 (has_hand 0 and 2: anything but 1) and back with the same id (rule 1, then 3)
SCRIPT = [  # ids,        has_hand,    lifted,      mirror,      dt
    ((1, 0, 5), (1, 1, 1), (1, 1, 1), (0, 1, 0), 1 / 30),
    ((1, 0, 5), (1, 1, 1), (1, 1, 1), (0, 1, 1), 1 / 30),
    ((1, 3, 5), (1, 1, 0), (1, 1, 0), (0, 1, 0), 1 / 15),
    ((2, 3, 5), (1, 1, 0), (1, 1, 0), (0, 1, 0), 1 / 30),
    ((2, 3, 5), (1, 1, 1), (0, 1, 1), (0, 0, 0), 0.01),
    ((2, 3, 5), (1, 1, 1), (1, 1, 1), (0, 0, 1), 1 / 30),
    ((2, 3, 5), (1, 1, 2), (1, 1, 0), (0, 1, 0), 1 / 30),
    ((2, 3, 5), (1, 1, 1), (1, 1, 1), (0, 1, 0), 1 / 60),
]


@pytest.mark.parametrize("sided", [True, False])
def test_kernel_step_by_step(sided):
    """slots = 3, v0 = 12, v = 7 with a shuffled perm, 21 joints, 8 scripted steps; a NaN and an inf in x (rule 2) at step 5 and a
    NaN root joint at step 6, a NaN and an inf poked into the state (rule 3) before step 7.  `out` is ops.mesh_finish's; the two
    filtered signals and the whole state are the fp32 reference's, byte for byte, after every step."""
    from hn_amd import ops
    slots, v0, v = 3, 12, 7
    rng = np.random.default_rng(11)
    perm = torch.from_numpy(rng.permutation(v0)[:v].astype(np.int64)).cuda()
    buf, views, outside = _views(slots, v)
    views["state"].zero_()
    dt = torch.zeros((1,), dtype=torch.float32, device="cuda")
    ref_state = sr.empty_state(slots, J, v)
    raw0 = (0.08 * rng.standard_normal((slots, v0, 3))).astype(F)
    xyz0 = (rng.uniform(-300, 300, (slots, J, 3)) + np.array([0, 0, 600])).astype(F)
    filtered = 0
    for t, (ids, has, lifted, mirror, step_dt) in enumerate(SCRIPT):
        raw = (raw0 + 2e-3 * t + 1e-3 * rng.standard_normal(raw0.shape)).astype(F)
        xyz = (xyz0 + 3.0 * t + 2.0 * rng.standard_normal(xyz0.shape)).astype(F)
        if t == 5:
            xyz[1, 4, 2] = np.nan                      # a joint that is not the root: that coordinate of smooth_xyz only
            raw[1, int(perm[2]), 1] = np.inf           # one vertex coordinate of the mesh
        if t == 6:
            xyz[0, 0, 0] = np.nan                      # the root joint: x of every vertex of slot 0
        if t == 7:                                     # a broken record: the element starts over
            for (s, e, c, w), bad in (((2, 3, 1, 0), np.nan), ((0, J + 4, 0, 1), np.inf), ((1, 2, 2, 1), np.nan)):
                ref_state[s, e, c, w] = F(bad).view(np.int32)
            views["state"].copy_(torch.from_numpy(ref_state))
        d = lambda a, dtype=torch.int32: torch.tensor(a, dtype=dtype, device="cuda")
        raw_d, xyz_d, dt_f = torch.from_numpy(raw).cuda(), torch.from_numpy(xyz).cuda(), F(step_dt)
        dt.fill_(float(dt_f))
        mir = d(mirror) if sided else None
        res = ops.mesh_finish_smooth(raw_d, perm, xyz_d, d(lifted), d(has), d(ids), dt, views["state"], mirror=mir,
                                     out=views["out"], smooth_xyz=views["smooth_xyz"], smooth_mesh=views["smooth_mesh"])
        assert res[0] is views["out"] and res[1] is views["smooth_xyz"] and res[2] is views["smooth_mesh"]
        want_out = ops.mesh_finish(raw_d, perm, xyz_d, valid=d(lifted), mirror=mir)
        before = ref_state
        ref = sr.step_slots(ref_state, xyz, want_out.cpu().numpy(), np.array(has), np.array(lifted), np.array(ids), dt_f)
        ref_state = ref[2]
        _check_step(t, views, outside, buf, want_out, ref)
        filtered += int(((before[..., 2] != 0) & (ref_state[..., 2] == before[..., 2]) & (ref_state[..., 1] != 0)).sum())
    assert filtered > 5 * slots * v          # (most steps did filter: the script is not all restarts)


def test_kernel_more_elements_than_one_pass_of_the_grid():
    """900 slots of 778 vertices: 2 157 300 elements for a grid of 8192 x 256 threads, so some threads take a second element;
    first step initialises, the second and third filter."""
    from hn_amd import ops
    slots, v0, v = 900, 800, 778
    assert slots * (v + J) * 3 > 8192 * 256
    rng = np.random.default_rng(12)
    perm = torch.from_numpy(rng.permutation(v0)[:v].astype(np.int64)).cuda()
    buf, views, outside = _views(slots, v)
    views["state"].zero_()
    dt = torch.full((1,), 1 / 30, dtype=torch.float32, device="cuda")
    ref_state = sr.empty_state(slots, J, v)
    ids = np.arange(1, slots + 1, dtype=np.int32)
    has = (rng.random(slots) < 0.9).astype(np.int32)
    lifted = has * (rng.random(slots) < 0.9).astype(np.int32)
    mirror = (rng.random(slots) < 0.5).astype(np.int32)
    raw0 = (0.08 * rng.standard_normal((slots, v0, 3))).astype(F)
    xyz0 = (rng.uniform(-300, 300, (slots, J, 3)) + np.array([0, 0, 600])).astype(F)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for t in range(3):
        raw, xyz = (raw0 + F(1.5e-3 * t)).astype(F), (xyz0 + F(2.5 * t)).astype(F)
        ops.mesh_finish_smooth(d(raw), perm, d(xyz), d(lifted), d(has), d(ids), dt, views["state"], mirror=d(mirror),
                               out=views["out"], smooth_xyz=views["smooth_xyz"], smooth_mesh=views["smooth_mesh"])
        want_out = ops.mesh_finish(d(raw), perm, d(xyz), valid=d(lifted), mirror=d(mirror))
        ref = sr.step_slots(ref_state, xyz, want_out.cpu().numpy(), has, lifted, ids, F(1 / 30))
        ref_state = ref[2]
        _check_step(t, views, outside, buf, want_out, ref)
    assert bool((views["smooth_mesh"] != views["out"]).any())


def test_wrapper_refusals_on_the_device():
    from hn_amd import ops
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device="cuda")
    i = lambda n: z(n, dtype=torch.int32)
    args = lambda state=None, dt=None, ids=None: (z(2, 12, 3), z(7, dtype=torch.int64), z(2, J, 3), i(2), i(2),
                                                 i(2) if ids is None else ids, z(1) if dt is None else dt,
                                                 ops.smooth_state(2, J, 7, "cuda") if state is None else state)
    with pytest.raises(ValueError, match="smooth_state"):
        ops.mesh_finish_smooth(*args(state=ops.smooth_state(2, J, 8, "cuda")))
    with pytest.raises(ValueError, match="one fp32 word"):
        ops.mesh_finish_smooth(*args(dt=z(2)))
    with pytest.raises(ValueError, match="track_id"):
        ops.mesh_finish_smooth(*args(ids=i(3)))
    with pytest.raises(TypeError):
        ops.mesh_finish_smooth(*args(state=ops.smooth_state(2, J, 7, "cuda").float()))


# ---------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------
def _engine(parts, **kw):  # noqa: F811
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm = parts
    return LiveHandsEngine(hand, lifter, PARAS, 2, True, perm, track=True, **kw)


def _nudged(frames):
    """The same frames with the depth map 1 % farther: the detections (and so the track ids) stay, every camera coordinate moves
    by millimetres -- a step on which the filter has something to filter."""
    return frames[0], (frames[1] * 1.01).contiguous()


def _follow(state, r, dt, **par):
    """One step of the reference on the host over what read() hands out -> (smooth_xyz, smooth_mesh, the new state)."""
    n, k = r.track_id.shape
    s = n * k
    return sr.step_slots(state, r.xyz_mm.numpy().reshape(s, J, 3), r.mesh.numpy().reshape(s, -1, 3), r.has_hand.numpy().reshape(s),
                         r.lifted.numpy().reshape(s), r.track_id.numpy().reshape(s), F(dt), **par)


def _is_ref(r, ref):
    for name, want in (("smooth_xyz", ref[0]), ("smooth_mesh", ref[1])):
        got = getattr(r, name).numpy()
        assert np.array_equal(got.view(np.int32).reshape(want.shape), want.view(np.int32)), name


def _is_raw(r):
    """The filter passes the raw values: zeros where the gate is off."""
    has, lifted = (r.has_hand == 1)[..., None, None], r.lifted[..., None, None]
    assert torch.equal(r.smooth_xyz, torch.where(has, r.xyz_mm, torch.zeros(()))), "smooth_xyz"
    assert torch.equal(r.smooth_mesh, torch.where(lifted, r.mesh, torch.zeros(()))), "smooth_mesh"


@pytest.mark.parametrize("n", [1, 2])
def test_the_same_frame_replayed_is_the_tracked_step(parts, n):  # noqa: F811
    """Five steps on frame A: every byte the smoothed buffer shares with the tracked step's is that step's, on every step, and
    the filtered signals are the raw ones bit for bit (x - xp = 0)."""
    a = _frames(n, "A")
    tracked, eng = _engine(parts), _engine(parts, smooth=True)
    la, lb = tracked._layout(n), eng._layout(n)
    assert lb.smoothed and not la.smoothed and lb.smooth_xyz_at == la.nbytes
    tracked.track_reset()
    want = [(o.host.clone(), r) for o, r in (_step(tracked, a) for _ in range(5))]
    eng.track_reset()
    for t in range(5):
        out, r = _step(eng, a)
        assert torch.equal(out.host[:la.nbytes], want[t][0]), t
        assert r._fields == want[t][1]._fields + ("smooth_xyz", "smooth_mesh")
        _same(want[t][1], r, want[t][1]._fields)
        assert bool(r.lifted.any()) and tuple(r.smooth_xyz.shape) == (n, 2, J, 3) and r.smooth_mesh.shape == r.mesh.shape
        _is_raw(r)
        assert torch.equal(out.smooth_mesh.cpu(), r.smooth_mesh) and torch.equal(out.smooth_xyz.cpu(), r.smooth_xyz)


def test_changing_frames_follow_the_reference_and_the_overlay_shows_the_filtered_mesh(parts):  # noqa: F811
    """A, B, A, B with faces= (and then A and A with its depth nudged, a step that filters whatever the tracker made of B):
    read().smooth_* are the fp32 reference run on the host over the raw read() values, ids and gates; the overlay is
    ops.mesh_render of smooth_mesh; mesh and the rest are the tracked step's."""
    from hn_amd import ops
    from scipy.spatial import Delaunay
    faces = Delaunay(np.random.default_rng(7).random((778, 2))).simplices.astype(np.int64)
    n = 1
    seq = [_frames(n, w) for w in "ABABA"]
    seq.append(_nudged(seq[-1]))
    tracked = _engine(parts, faces=faces)
    tracked.track_reset()
    want = [_step(tracked, f)[1] for f in seq]
    eng = _engine(parts, faces=faces, smooth=True)
    eng.track_reset()
    state, moved = sr.empty_state(n * 2, J, 778), 0
    for t, f in enumerate(seq):
        out, r = _step(eng, f)
        _same(want[t], r, [x for x in want[t]._fields if x != "overlay"])
        ref = _follow(state, r, 1 / 30)
        state = ref[2]
        _is_ref(r, ref)
        moved += int((r.smooth_mesh != r.mesh).sum())
        drawn = ops.mesh_render(out.smooth_mesh, eng.faces, PARAS, f[0], lifted=out.lifted.view(-1), k=2)
        assert torch.equal(drawn.cpu(), r.overlay), t
        if t == 0:
            assert torch.equal(r.overlay, want[t].overlay)
    assert torch.equal(r.track_id, want[-2].track_id) and bool(r.lifted.any())
    assert moved > 500                       # (the last step kept its ids and moved every vertex: the filter did filter)


def test_sequence_eager_captured_and_camera_feed(parts, gate):  # noqa: F811
    """A, a frame without a hand, A, A with its depth nudged: on the hand's return the filter restarts (the output is the raw value); the sequence is
    the same bytes through eager steps, through graphed() -- captured in the MIDDLE of a sequence, which changes nothing -- and
    through forward_raw's capture."""
    n = 1
    seq = [(_frames(n, w), w != "C") for w in ("A", "C", "A")]
    seq.append((_nudged(seq[0][0]), True))
    eager = _engine(parts, smooth=True)
    eager.track_reset()
    want = [_step(eager, f, gate, hands)[1] for f, hands in seq]
    assert bool(want[0].lifted.any()) and not bool(want[1].has_hand.any()) and torch.equal(want[1].track_id, want[0].track_id)
    assert not want[1].smooth_mesh.any() and not want[1].smooth_xyz.any()
    _is_raw(want[0])
    _is_raw(want[2])                                         # back after a held step: the raw value
    assert bool((want[3].smooth_mesh != want[3].mesh).any())  # ... and then it filters again
    state = sr.empty_state(2 * n, J, 778)
    for r in want:
        ref = _follow(state, r, 1 / 30)
        state = ref[2]
        _is_ref(r, ref)
    # captured after the first step of the sequence: the capture's warm-up steps leave tracker and filters as they were
    eng = _engine(parts, smooth=True)
    eng.track_reset()
    _same(want[0], _step(eng, seq[0][0], gate, True)[1])
    saved = eng._smooth_state(n)[0].clone()
    gate.fill_(1)
    run, s_img, s_dep, out = eng.graphed(*seq[3][0])
    assert torch.equal(eng._smooth_state(n)[0], saved) and bool(saved.any())
    for t in (1, 2, 3):
        f, hands = seq[t]
        s_img.copy_(f[0])
        s_dep.copy_(f[1])
        gate.fill_(1 if hands else 0)
        run()
        torch.cuda.synchronize()
        _same(want[t], out.read())
    eng.track_reset()
    for t, (f, hands) in enumerate(seq):                     # ... and the whole sequence through the capture
        s_img.copy_(f[0])
        s_dep.copy_(f[1])
        gate.fill_(1 if hands else 0)
        run()
        torch.cuda.synchronize()
        _same(want[t], out.read())
    # the camera feed: uint8 frames through the ingest kernel into forward_raw's capture, against eager steps on the same
    # frames converted on the host
    rng = np.random.default_rng(3)
    raw = [(rng.integers(0, 256, size=(n, 480, 640, 3), dtype=np.uint8), rng.integers(300, 1500, size=(n, 480, 640)).astype(np.uint16),
            t != 1) for t in range(3)]
    feed = lambda bgr, mm: (torch.from_numpy(bgr[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) / 255.0).cuda(),
                            torch.from_numpy(mm.astype(np.float32) / 1000.0).unsqueeze(1).cuda())
    eager.track_reset()
    want = [_step(eager, feed(bgr, mm), gate, hands)[1] for bgr, mm, hands in raw]
    eng.track_reset()
    for (bgr, mm, hands), w in zip(raw, want):
        gate.fill_(1 if hands else 0)
        o = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(mm))
        torch.cuda.synchronize()
        _same(w, o.read())


def test_smooth_dt_and_smooth_reset_between_replays(parts):  # noqa: F811
    """One capture: A, then A with its depth nudged (B) at the engine's dt; smooth_dt(0.1) and A -- the reference with dt = 0.1,
    and not the one with 1/60; smooth_reset() and B -- the raw values, the track ids kept; other parameters give another result, as the reference says."""
    n = 1
    a = _frames(n, "A")
    b = _nudged(a)
    eng = _engine(parts, smooth=True, smooth_min_cutoff=0.5, smooth_beta=0.02, smooth_d_cutoff=2.0, smooth_rate=60.0)
    par = dict(min_cutoff=0.5, beta=0.02, d_cutoff=2.0)
    eng.track_reset()
    run, s_img, s_dep, out = eng.graphed(*a)
    assert not bool(eng._smooth_state(n)[0].any())

    def replay(f):
        s_img.copy_(f[0])
        s_dep.copy_(f[1])
        run()
        torch.cuda.synchronize()
        return out.read()
    state = sr.empty_state(2 * n, J, 778)
    for f, dt in ((a, 1 / 60), (b, 1 / 60)):
        r = replay(f)
        ref = _follow(state, r, dt, **par)
        state = ref[2]
        _is_ref(r, ref)
    assert eng.smooth_dt(0.1) is eng
    r = replay(a)
    ref, other = _follow(state, r, 0.1, **par), _follow(state, r, 1 / 60, **par)
    _is_ref(r, ref)
    assert not np.array_equal(ref[1], other[1]) and not np.array_equal(ref[1], _follow(state, r, 0.1)[1])
    ids = r.track_id.clone()
    assert eng.smooth_reset() is eng and not bool(eng._smooth_state(n)[0].any())
    r = replay(b)
    assert torch.equal(r.track_id, ids) and bool(ids.any())
    _is_raw(r)
    for bad in (0, -1.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError):
            eng.smooth_dt(bad)
    with pytest.raises(ValueError):
        _engine(parts).smooth_reset()
