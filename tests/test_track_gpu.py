"""Tracked hand slots on the GPU (track=): the slot kernel against tests/track_ref.py byte for byte, step by
step, on hand-built detections; then the engines -- the tracked live step against the untracked one, eager against captured."""
import numpy as np
import pytest
import torch

import track_ref as tr
from test_track_cpu import SCENARIOS

pytestmark = pytest.mark.gpu

H, W, OUT = 48, 64, 8
CANARY = 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: ops.crop_resize_hands(track=) on hand-built detections
# ---------------------------------------------------------------------------------------------------------------------
def _spread(dets, t):
    """The same detections with 63 / 64 detections of another label in between: the hands lie on both sides of entry 64 (the
    kernel walks the list 64 entries at a time)."""
    filler = [([1, 30, 9, 40], 0.01, t % 2, 0)] * (64 if t % 2 else 63)
    return list(dets[:t % 2]) + filler + list(dets[t % 2:]) if dets else filler[:3]


def _views(n, k, sided, device="cuda"):
    """The outputs as views into one canary-filled buffer, four canary words between neighbours (16-byte steps)."""
    slots = n * k
    sizes = [("crop_box", slots * 8), ("has_hand", slots), ("score", slots), ("det_index", slots), ("track_id", slots),
             ("track_age", slots), ("crops", slots * OUT * OUT * 4)] + ([("side", slots), ("mirror", slots)] if sided else [])
    spans, end = {}, 4
    for name, words in sizes:
        spans[name] = (end, end + words)
        end = (end + words + 3) // 4 * 4 + 4
    buf = torch.full((end,), CANARY, dtype=torch.int32, device=device)
    cut = {name: buf[a:b] for name, (a, b) in spans.items()}
    views = dict(crop_box=cut["crop_box"].view(torch.int64).view(n, k, 4), score=cut["score"].view(torch.float32).view(n, k),
                 crops=cut["crops"].view(torch.float32).view(slots, OUT, OUT, 4))
    for name in cut:
        if name not in views:
            views[name] = cut[name].view(n, k)
    outside = torch.ones((end,), dtype=torch.bool)
    for a, b in spans.values():
        outside[a:b] = False
    return buf, views, outside


def _compare_run(streams, k, thr, hold, sided, cap, seed=0):
    """streams[i][t] = the detection list of batch row i at step t.  Every step through the device (state carried on the device)
    and through track_ref (state carried on the host): all outputs, the crops and the state must be equal bytes."""
    from hn_amd import ops
    n, steps = len(streams), len(streams[0])
    packed = [[tr.pack(streams[i][t], cap) for i in range(n)] for t in range(steps)]
    stack = lambda j, dt: torch.from_numpy(np.stack([np.stack([packed[t][i][j] for i in range(n)]) for t in range(steps)])).to(dt).cuda()
    boxes, scores, labels, sides = stack(0, torch.float32), stack(1, torch.float32), stack(2, torch.int32), stack(3, torch.int32)
    count = torch.tensor([[packed[t][i][4] for i in range(n)] for t in range(steps)], dtype=torch.int32).cuda()
    depth = torch.rand((n, 1, H, W), generator=torch.Generator().manual_seed(seed))
    depth_dev = depth.cuda()
    state = ops.track_state(n, k, "cuda")
    buf, v, outside = _views(n, k, sided)
    base = ops.alloc_detections(n, cap, "cuda")
    got = []
    for t in range(steps):
        det = ops.Detections(boxes[t], scores[t], labels[t], sides[t], base.level, base.keep, count[t])
        res = ops.crop_resize_hands(det, 2, depth_dev, k, OUT, 4, crop_box=v["crop_box"], has_hand=v["has_hand"], score=v["score"],
                                    det_index=v["det_index"], crops=v["crops"], handed=sided, left_side=0, side=v.get("side"),
                                    mirror=v.get("mirror"), track=state, track_iou=thr / 1000.0, track_hold=hold,
                                    track_id=v["track_id"], track_age=v["track_age"])
        assert len(res) == (9 if sided else 7) and res[-2] is v["track_id"] and res[-1] is v["track_age"]
        got.append((buf.clone(), state.clone()))
    torch.cuda.synchronize()
    ref_state = tr.empty_state(n, k)
    for t, (b, st) in enumerate(got):
        p = packed[t]
        want = tr.step(ref_state, [x[0] for x in p], [x[1] for x in p], [x[2] for x in p], [x[3] for x in p] if sided else None,
                       [x[4] for x in p], 2, k, H, W, thr, hold, 0)
        ref_state = want["state"]
        b = b.cpu()
        assert bool((b[outside] == CANARY).all()), f"step {t}: a word outside the outputs was written"
        buf.copy_(b)                       # (the views cut this step's bytes)
        for name in ("crop_box", "has_hand", "det_index", "track_id", "track_age") + (("side", "mirror") if sided else ()):
            assert np.array_equal(v[name].cpu().numpy(), want[name]), (t, name, v[name].cpu().numpy(), want[name])
        assert np.array_equal(v["score"].cpu().numpy().view(np.int32), want["score"].view(np.int32)), (t, "score")
        assert np.array_equal(st.cpu().numpy(), want["state"]), (t, "state", st.cpu().numpy(), want["state"])
        crops = tr.crops(depth.numpy(), want["crop_box"], want["has_hand"], want["mirror"], OUT)
        assert np.array_equal(v["crops"].cpu().numpy().view(np.int32), crops.view(np.int32)), (t, "crops")
    return got


@pytest.mark.parametrize("sided", [True, False])
@pytest.mark.parametrize("n", [1, 3])
def test_scenarios_step_by_step(n, sided):
    """Every scenario of tests/test_track_cpu.py, compact (cap 8) and spread over a list of 80; batch 3 runs the scenario in
    rows 0 and 2 around another stream, and the two rows' state must be equal: a frame does not depend on its neighbours."""
    rng = np.random.default_rng(2)
    for name, (k, thr, hold, steps, _want) in SCENARIOS.items():
        for cap in (8, 80):
            mine = [_spread(d, t) for t, d in enumerate(steps)] if cap == 80 else steps
            other = tr.random_stream(rng, len(steps), hands=3, cap=cap)
            got = _compare_run([mine, other, mine][:n] if n == 3 else [mine], k, thr, hold, sided, cap)
            if n == 3:
                for _buf, st in got:
                    assert torch.equal(st[0], st[2]), name


@pytest.mark.parametrize("k", [1, 2, 3, 16])
def test_more_hands_than_candidates(k):
    """About 24 hands in a list of 80 on both sides of entry 64: the candidates are the first 16 whatever K; K = 16 has four
    pairs on every lane, K = 3 a ragged pair count."""
    rng = np.random.default_rng(k)
    streams = [[(_spread(d, t) if t % 3 else d)[:80] for t, d in enumerate(tr.random_stream(rng, 8, hands=24, cap=80))]
               for _ in range(3)]
    assert max(sum(1 for d in frame if d[2] == 2) for s in streams for frame in s) > 16
    _compare_run(streams, k, 300, 2, k != 2, 80, seed=k)


def test_random_walk():
    rng = np.random.default_rng(7)
    streams = [tr.random_stream(rng, 200, hands=5, cap=12) for _ in range(4)]
    got = _compare_run(streams, 4, 300, 1, True, 12, seed=1)
    assert int(got[-1][1][:, 0, 0].min()) > 8          # every stream lost and re-admitted hands


def test_wrapper_refusals_on_the_device():
    from hn_amd import ops
    det = ops.alloc_detections(1, 8, "cuda")
    depth = torch.zeros((1, 1, H, W), device="cuda")
    with pytest.raises(ValueError, match="track_state"):
        ops.crop_resize_hands(det, 2, depth, 2, OUT, track=ops.track_state(1, 3, "cuda"))
    res = ops.crop_resize_hands(det, 2, depth, 2, OUT, track=ops.track_state(1, 2, "cuda"))
    assert len(res) == 7 and res[-1].dtype == torch.int32 and tuple(res[-1].shape) == (1, 2)
    assert len(ops.crop_resize_hands(det, 2, depth, 2, OUT)) == 5          # without the option: today's tuple


# ---------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------
PARAS = (617.343, 617.343, 312.42, 241.42)


@pytest.fixture(scope="module")
def parts(golden_dir, fcos_sd, a2j_sd):
    """The live fixture's engines, as tests/test_live_hands_gpu.py builds them, + the triangle list for the overlay."""
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    g = np.load(golden_dir / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    p2m_sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    hand = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    return hand, Pose2MeshEngine(p2m_sd, graphs, device="cuda"), g["perm_reverse"][:778]


def _frames(n, which):
    """Frame A, frame B and frame C (noise frames of the live fixture's kind)."""
    import parity_cases as pc
    seed = {"A": 0, "B": 1, "C": 2}[which]
    return pc.noise_frames(n, seed=3000 + seed).cuda(), pc.depth_noise(n, seed=4000 + seed).cuda()


@pytest.fixture
def gate(monkeypatch):
    """The fixture's detector finds hands on every frame, a black one included.  A frame WITHOUT a hand is made on the device:
    the detections' count is multiplied by gate[0] (int32, 1 or 0) in front of the crop stage, by an op that a captured step
    replays like any other -- so eager steps, captures and the camera feed all see the same empty detection list."""
    from hn_amd import pipeline
    g = torch.ones((1,), dtype=torch.int32, device="cuda")
    real = pipeline.ops.crop_resize_hands

    def crop(det, *a, **kw):
        det.count.mul_(g)
        return real(det, *a, **kw)
    monkeypatch.setattr(pipeline.ops, "crop_resize_hands", crop)
    return g


def _step(eng, frames, gate=None, hands=True):
    if gate is not None:
        gate.fill_(1 if hands else 0)
    out = eng.forward_device(*frames)
    torch.cuda.synchronize()
    return out, out.read()


def _same(a, b, fields=None):
    for f in fields or a._fields:
        x, y = getattr(a, f), getattr(b, f)
        if f in ("words", "more"):
            assert x == y, f
        else:
            assert torch.equal(x, y), f


def _hand_count(det, i):
    cnt = min(int(det.count[i]), det.labels.shape[1])
    return int((det.labels[i, :cnt] == 2).sum())


@pytest.mark.parametrize("n", [1, 2])
def test_first_step_is_the_untracked_step_and_a_repeat_keeps_the_slots(parts, n):
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm = parts
    plain = LiveHandsEngine(hand, lifter, PARAS, 2, True, perm)
    a = _frames(n, "A")
    out0, want = _step(plain, a)
    # the precondition of "a first tracked step is the untracked step": every candidate of the frames has a non-empty slice
    wide = hand.forward_hands(a[0], a[1], 16)
    for i in range(n):
        nh = min(16, _hand_count(wide.detections, i))
        assert nh >= 1 and bool((wide.has_hand[i, :nh] == 1).all()) and not bool(wide.has_hand[i, nh:].any())
    eng = LiveHandsEngine(hand, lifter, PARAS, 2, True, perm, track=True)
    eng.track_reset()
    out1, first = _step(eng, a)
    assert first._fields[:len(want._fields)] == want._fields and first._fields[-2:] == ("track_age", "track_id")
    _same(want, first, want._fields)
    la, lb = plain._layout(n), eng._layout(n)
    assert lb.tracked and not la.tracked and lb.nbytes == la.nbytes + 16 * n
    assert torch.equal(out0.host[:la.lifted_at], out1.host[:la.lifted_at])          # the records, byte for byte
    assert torch.equal(out0.host[la.lifted_at:], out1.host[lb.lifted_at:])          # lifted + mesh, 8 bytes per slot further on
    filled = first.has_hand != 0
    assert torch.equal(first.track_id, torch.where(filled, torch.tensor([[1, 2]] * n, dtype=torch.int32), 0))
    assert not first.track_age.any() and torch.equal(out1.track_id.cpu(), first.track_id)
    _o, second = _step(eng, a)
    _same(first, second, [f for f in first._fields if f != "track_age"])
    assert torch.equal(second.track_age, filled.to(torch.int32))


def test_a_different_frame_follows_the_reference(parts):
    """Frame A, then frame B: the assignment track_ref makes from the untracked step's detections of B and the state after A
    is the tracked step's, exactly; and every filled slot's keypoints and mesh are those of the untracked slot with the same
    detection, to the suite's bounds for another batch position (1e-4 keypoints, 2e-3 mesh: DESIGN.md 9d)."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm = parts
    n, k = 2, 2
    eng = LiveHandsEngine(hand, lifter, PARAS, k, True, perm, handed=True, track=True)
    wide = LiveHandsEngine(hand, lifter, PARAS, 16, True, perm, handed=True)
    eng.track_reset()
    a, b = _frames(n, "A"), _frames(n, "B")
    _step(eng, a)
    state = hand._track_state(n, k).cpu().numpy()
    out_w, ref = _step(wide, b)
    det = out_w.hands.detections
    want = tr.step(state, det.boxes.cpu().numpy(), det.scores.cpu().numpy(), det.labels.cpu().numpy(), det.sides.cpu().numpy(),
                   det.count.cpu().numpy(), 2, k, 480, 640, 300, 5, 0)
    out, got = _step(eng, b)
    for name, mine in (("crop_box", out.hands.crop_box), ("det_index", got.det_index), ("side", got.side),
                       ("track_id", got.track_id), ("track_age", got.track_age), ("has_hand", out.hands.has_hand)):
        assert np.array_equal(mine.cpu().numpy(), want[name]), name
    assert np.array_equal(got.score.numpy().view(np.int32), want["score"].view(np.int32))
    assert np.array_equal(hand._track_state(n, k).cpu().numpy(), want["state"])
    assert bool(got.has_hand.any())
    for i in range(n):
        for s in range(k):
            if not got.has_hand[i, s]:
                continue
            j = ref.det_index[i].tolist().index(int(got.det_index[i, s]))
            assert torch.equal(ref.crop_box[i, j], got.crop_box[i, s]) and bool(ref.lifted[i, j]) == bool(got.lifted[i, s])
            assert (ref.keypoints[i, j] - got.keypoints[i, s]).abs().max().item() < 1e-4
            assert (ref.mesh[i, j] - got.mesh[i, s]).abs().max().item() < 2e-3


@pytest.mark.parametrize("n", [1, 2])
def test_graphed_sequence_equals_eager(parts, gate, n):
    """A, B, a frame without a hand, A: eagerly on one engine; through graphed() and through forward_raw's capture on another
    -- read() is the same bytes step for step, and a reset followed by A is the first step again."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm = parts
    seq = [(_frames(n, w), w != "C") for w in ("A", "B", "C", "A")]
    gate.zero_()
    assert not bool(hand.forward_hands(seq[2][0][0], seq[2][0][1], 2).has_hand.any())      # the gated frame: no hand
    eager = LiveHandsEngine(hand, lifter, PARAS, 2, True, perm, track=True)
    eager.track_reset()
    want = [_step(eager, f, gate, hands)[1] for f, hands in seq]
    assert bool(want[0].track_id.any()) and not bool(want[2].has_hand.any())
    assert torch.equal(want[2].track_id, want[1].track_id)                            # every live slot is held over the gap
    eng = LiveHandsEngine(hand, lifter, PARAS, 2, True, perm, track=True)
    eng.track_reset()
    gate.fill_(1)
    run, s_img, s_dep, out = eng.graphed(*seq[1][0])         # (captured on B: the capture leaves the tracker as it was)
    assert not bool(hand._track_state(n, 2).any())
    for t, (f, hands) in enumerate(seq + seq[:1]):
        if t == len(seq):
            eng.track_reset()
        s_img.copy_(f[0])
        s_dep.copy_(f[1])
        gate.fill_(1 if hands else 0)
        run()
        torch.cuda.synchronize()
        _same(want[t % len(seq)], out.read())
    # the camera feed: uint8 frames through the ingest kernel into forward_raw's capture, against eager steps on the same
    # frames converted on the host
    rng = np.random.default_rng(3)
    raw = [(rng.integers(0, 256, size=(n, 480, 640, 3), dtype=np.uint8), rng.integers(300, 1500, size=(n, 480, 640)).astype(np.uint16),
            t != 1) for t in range(3)]
    feed = lambda bgr, mm: (torch.from_numpy(bgr[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) / 255.0).cuda(),
                            torch.from_numpy(mm.astype(np.float32) / 1000.0).unsqueeze(1).cuda())
    eager.track_reset()
    want = [_step(eager, feed(bgr, mm), gate, hands)[1] for bgr, mm, hands in raw]
    assert bool(want[0].track_id.any()) and torch.equal(want[1].track_id, want[0].track_id)
    eng.track_reset()
    for (bgr, mm, hands), w in zip(raw, want):
        gate.fill_(1 if hands else 0)
        out = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(mm))
        torch.cuda.synchronize()
        _same(w, out.read())


@pytest.mark.parametrize("option", ["handed", "left", "faces+labels"])
def test_options(parts, gate, option):
    """track with handed, with left, and with faces + labels: the first step is that option's untracked step; over a frame
    without a hand the slots are held -- ids kept, nothing lifted, nothing drawn, zero pose_label; track_id is read()'s last
    field."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm = parts
    kw = dict(handed=dict(handed=True), left=dict(left=True), **{"faces+labels": dict(labels=True)})[option]
    if option == "faces+labels":
        from scipy.spatial import Delaunay
        kw["faces"] = Delaunay(np.random.default_rng(7).random((778, 2))).simplices.astype(np.int64)
    n = 1
    a, c = _frames(n, "A"), _frames(n, "C")
    plain = LiveHandsEngine(hand, lifter, PARAS, 2, True, perm, **kw)
    _o, want = _step(plain, a, gate)
    _o, want_none = _step(plain, c, gate, hands=False)
    assert bool(want.lifted.any()) and not want_none.has_hand.any()
    eng = LiveHandsEngine(hand, lifter, PARAS, 2, True, perm, track=True, track_hold=3, **kw)
    eng.track_reset()
    _o, first = _step(eng, a, gate)
    assert first._fields == want._fields + ("track_age", "track_id")
    _same(want, first, want._fields)
    out, held = _step(eng, c, gate, hands=False)
    assert torch.equal(held.track_id, first.track_id) and bool(held.track_id.any())
    assert not held.has_hand.any() and not held.lifted.any() and not held.mesh.any()
    _same(want_none, held, want_none._fields)
    if option == "handed":
        assert bool((held.side == -1).all())
    if option == "faces+labels":
        assert not held.pose_label.any()
        assert torch.equal(held.overlay, want_none.overlay) and torch.equal(held.box_label, want_none.box_label)
