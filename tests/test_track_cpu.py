"""Tracked hand slots (track=) without a GPU: the rule's plain-Python statement (tests/track_ref.py)
against tables written out by hand, the new C entries' argument checks, the buffer layouts and the resource report."""
import inspect
import itertools

import numpy as np
import pytest

import track_ref as tr

H, W = 48, 64
# 10 x 10 detection boxes (label 2 = hand): the padding adds 4 pixels on every side
A = [10, 10, 20, 20]            # padded (6, 6, 24, 24)
A6 = [16, 10, 26, 20]           # A moved 6 to the right: padded (12, 6, 30, 24), I = 216, U = 432 against A: IoU = 1/2 exactly
A18 = [28, 10, 38, 20]          # padded (24, 6, 42, 24): touches A's padded box along x = 24, I = 0
B = [40, 10, 50, 20]            # padded (36, 6, 54, 24)
F = [25, 30, 35, 40]            # padded (21, 26, 39, 44): overlaps neither A nor B
T = [24, 10, 34, 20]            # padded (20, 6, 38, 24); L and R lie 4 to its left and right: I = 252, U = 396 both
L = [20, 10, 30, 20]            # padded (16, 6, 34, 24)
R = [28, 10, 38, 20]            # padded (24, 6, 42, 24)
E = [10, 60, 20, 70]            # below the 48-row frame: the padded slice is empty (ok = 0)
OTHER = [2, 30, 12, 40]         # a detection with another label


def hand(box, score, side=1):
    return (box, score, 2, side)


# name -> (K, thr_milli, hold, steps, expected); a step is the frame's detection list in score order, and its expectation is
# (det_index per slot, track_id per slot, track_age per slot) -- written by hand from the rule's text.
SCENARIOS = {
    "score order flips every step": (2, 300, 5, [
        [hand(A, .9), hand(B, .8)], [hand(B, .9), hand(A, .8)], [hand(A, .9), hand(B, .8)], [hand(B, .9, 0), hand(A, .8)]],
        [([0, 1], [1, 2], [0, 0]), ([1, 0], [1, 2], [1, 1]), ([0, 1], [1, 2], [2, 2]), ([1, 0], [1, 2], [3, 3])]),
    "missing for track_hold steps: back in its slot, id and age continued": (2, 300, 2, [
        [hand(A, .9), hand(B, .8)], [hand(A, .9)], [hand(A, .9)], [hand(A, .9), hand(B, .8)]],
        [([0, 1], [1, 2], [0, 0]), ([0, -1], [1, 2], [1, 0]), ([0, -1], [1, 2], [2, 0]), ([0, 1], [1, 2], [3, 1])]),
    "missing for track_hold + 1 steps: freed, back with a new id": (2, 300, 2, [
        [hand(A, .9), hand(B, .8)], [hand(A, .9)], [hand(A, .9)], [hand(A, .9)], [hand(A, .9), hand(B, .8)]],
        [([0, 1], [1, 2], [0, 0]), ([0, -1], [1, 2], [1, 0]), ([0, -1], [1, 2], [2, 0]), ([0, -1], [1, 0], [3, 0]),
         ([0, 1], [1, 3], [4, 0])]),
    # step 1: slot 1 is held for B, so F is dropped; step 2: B has been missing for hold + 1 steps, the slot is freed (rule 4)
    # and F, still without a slot, takes it in the same step (rule 5 comes after rule 4) with the next id
    "third hand: dropped while every slot is held or taken, admitted once one frees": (2, 300, 1, [
        [hand(A, .9), hand(B, .8), hand(F, .7)], [hand(A, .9), hand(F, .7)], [hand(A, .9), hand(F, .7)]],
        [([0, 1], [1, 2], [0, 0]), ([0, -1], [1, 2], [1, 0]), ([0, 1], [1, 3], [2, 0])]),
    "exact tie: the lower candidate": (2, 300, 5, [[hand(T, .9)], [hand(L, .9), hand(R, .8)]],
                                       [([0, -1], [1, 0], [0, 0]), ([0, 1], [1, 2], [1, 0])]),
    "exact tie, candidates the other way round": (2, 300, 5, [[hand(T, .9)], [hand(R, .9), hand(L, .8)]],
                                                  [([0, -1], [1, 0], [0, 0]), ([0, 1], [1, 2], [1, 0])]),
    "1000 I == thr_milli U is a match": (2, 500, 5, [[hand(A, .9)], [hand(A6, .9)]],
                                         [([0, -1], [1, 0], [0, 0]), ([0, -1], [1, 0], [1, 0])]),
    "one unit below is not": (2, 501, 5, [[hand(A, .9)], [hand(A6, .9)]],
                              [([0, -1], [1, 0], [0, 0]), ([-1, 0], [1, 2], [0, 0])]),
    "I == 0 never matches": (2, 1, 5, [[hand(A, .9)], [hand(A18, .9)]],
                             [([0, -1], [1, 0], [0, 0]), ([-1, 0], [1, 2], [0, 0])]),
    "K = 1 follows its hand": (1, 300, 5, [
        [hand(A, .9)], [hand(B, .95), hand(A, .8)], [(OTHER, .99, 0, 0), hand(B, .95), hand(A, .7)]],
        [([0], [1], [0]), ([1], [1], [1]), ([2], [1], [2])]),
    "empty padded slice is skipped": (2, 300, 5, [[hand(E, .9), hand(A, .8)]], [([1, -1], [1, 0], [0, 0])]),
}
# the slot-0 box after the tie: whichever of L and R came first in the list
TIE_BOXES = {"exact tie: the lower candidate": [16, 6, 34, 24], "exact tie, candidates the other way round": [24, 6, 42, 24]}


def run(k, thr, hold, steps, sided=True, cap=8):
    """A scenario through the reference, one frame: the per-step outputs."""
    state, outs = tr.empty_state(1, k), []
    for dets in steps:
        b, s, l, sd, cnt = tr.pack(dets, cap)
        o = tr.step(state, b[None], s[None], l[None], sd[None] if sided else None, [cnt], 2, k, H, W, thr, hold, 0)
        state = o["state"]
        outs.append(o)
    return outs


def test_the_boxes_are_what_the_tables_assume():
    pad = lambda b: tuple(tr.pad_box(np.array(b, np.float32), H, W)[1])
    assert pad(A) == (6, 6, 24, 24) and pad(A6) == (12, 6, 30, 24) and pad(A18) == (24, 6, 42, 24) == pad(R)
    assert pad(B) == (36, 6, 54, 24) and pad(F) == (21, 26, 39, 44) and pad(T) == (20, 6, 38, 24) and pad(L) == (16, 6, 34, 24)
    assert tr.pad_box(np.array(E, np.float32), H, W) == (0, [0, 0, 0, 0])
    assert tr.inter_union(pad(A), pad(A6)) == (216, 432) and 1000 * 216 == 500 * 432 and 1000 * 216 < 501 * 432
    assert tr.inter_union(pad(A), pad(A18))[0] == 0
    assert tr.inter_union(pad(T), pad(L)) == tr.inter_union(pad(T), pad(R)) == (252, 396)
    for x, y in itertools.combinations((A, B, F), 2):
        assert tr.inter_union(pad(x), pad(y))[0] == 0


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_reference_against_hand_written_tables(name):
    k, thr, hold, steps, want = SCENARIOS[name]
    outs = run(k, thr, hold, steps)
    for t, (o, (idx, ids, ages)) in enumerate(zip(outs, want)):
        assert o["det_index"][0].tolist() == idx, (name, t)
        assert o["track_id"][0].tolist() == ids and o["track_age"][0].tolist() == ages, (name, t)
        # what follows from the index: a filled slot carries its detection's box, score and side, an empty one nothing
        for s, j in enumerate(idx):
            if j < 0:
                assert not o["crop_box"][0, s].any() and o["has_hand"][0, s] == 0 and o["score"][0, s] == 0
                assert o["side"][0, s] == -1 and o["mirror"][0, s] == 0
            else:
                box, sc, _lab, sd = steps[t][j]
                assert o["crop_box"][0, s].tolist() == tr.pad_box(np.array(box, np.float32), H, W)[1]
                assert o["has_hand"][0, s] == 1 and o["score"][0, s] == np.float32(sc)
                assert o["side"][0, s] == sd and o["mirror"][0, s] == (sd == 0)
    if name in TIE_BOXES:
        assert outs[-1]["crop_box"][0, 0].tolist() == TIE_BOXES[name]
    # a held slot keeps its box in the state; a free slot's row is zero
    last = outs[-1]["state"][0]
    for s, tid in enumerate(want[-1][1]):
        assert int(last[1 + s, 8]) == tid and (tid != 0 or not last[1 + s].any())
    assert int(last[0, 0]) == max(max(ids) for _, ids, _ in want) and not last[0, 1:].any()


def test_held_slot_keeps_box_and_counts_missed():
    k, thr, hold, steps, _ = SCENARIOS["missing for track_hold steps: back in its slot, id and age continued"]
    outs = run(k, thr, hold, steps)
    row = outs[2]["state"][0, 2]
    assert row[:8].copy().view(np.int64).tolist() == [36, 6, 54, 24] and row[8:].tolist() == [2, 0, 2, 0]
    assert outs[3]["state"][0, 2, 8:].tolist() == [2, 1, 0, 0]


def test_from_an_empty_state_the_slots_are_the_untracked_rule():
    """All candidates ok: slot k is the k-th hand detection in score order, ids 1.. in that order."""
    rng = np.random.default_rng(5)
    for steps in (tr.random_stream(rng, 1, hands=h) for h in (1, 2, 3, 5) for _ in range(10)):
        dets = steps[0]
        hands = [j for j, d in enumerate(dets) if d[2] == 2]
        if not all(tr.pad_box(np.array(dets[j][0], np.float32), H, W)[0] for j in hands):
            continue
        for k in (1, 2, 4, 16):
            o = run(k, 300, 5, [dets], cap=12)[0]
            want = (hands + [-1] * k)[:k]
            assert o["det_index"][0].tolist() == want
            assert o["track_id"][0].tolist() == [s + 1 if j >= 0 else 0 for s, j in enumerate(want)]


def test_ids_are_unique_and_issued_in_order():
    rng = np.random.default_rng(11)
    steps = tr.random_stream(rng, 120, hands=4)
    seen, last = {}, 0
    for t, o in enumerate(run(3, 300, 2, steps, cap=12)):
        ids = [i for i in o["track_id"][0].tolist() if i]
        assert len(set(ids)) == len(ids)
        fresh = sorted(i for i in ids if i not in seen)
        assert fresh == list(range(last + 1, last + 1 + len(fresh))), t      # no id twice, none left out
        for i, age in zip(o["track_id"][0].tolist(), o["track_age"][0].tolist()):
            if i:
                assert age >= seen.get(i, 0)
                seen[i] = age
        last = max([last] + ids)
        assert int(o["state"][0, 0, 0]) == last
    assert last > 6      # the walk did lose and re-admit hands


# ---------------------------------------------------------------------------------------------------------------------
# bindings and layouts
# ---------------------------------------------------------------------------------------------------------------------
def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items()}


def test_surface():
    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd import ops
    from hn_amd.live import LiveHandsEngine
    from hn_amd.pipeline import HandNetEngine, HandsOutput
    for fn in (HandNetEngine.forward_hands, HandNetEngine.graphed_hands, HandNet.forward_hands, HandNet.live_hands,
               LiveHandsEngine.__init__):
        d = _defaults(fn)
        assert d.get("track") is False and d.get("track_iou") == 0.3 and d.get("track_hold") == 5, fn.__qualname__
    d = _defaults(ops.crop_resize_hands)
    assert d.get("track", 0) is None and d.get("track_iou") == 0.3 and d.get("track_hold") == 5
    assert callable(HandNetEngine.track_reset) and callable(LiveHandsEngine.track_reset)
    assert [f for f in HandsOutput.__dataclass_fields__][-2:] == ["track_id", "track_age"]
    assert ops.check_track_options(0.3, 5) == (300, 5) and ops.check_track_options(1, 0) == (1000, 0)
    for iou, hold in ((0.0, 5), (1.2, 5), (0.3, -1), (0.3, 1000001), (0.3, 1.5)):
        with pytest.raises(ValueError):
            ops.check_track_options(iou, hold)


def test_c_entry_refuses_bad_arguments_without_a_gpu():
    from hn_amd import _lib
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION
    for name in ("hn_crop_resize_hands_tracked", "hn_track_state_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.hn_track_state_bytes(3, 2) == 3 * 3 * 48 and lib.hn_track_state_bytes(1, 16) == 17 * 48
    assert lib.hn_track_state_bytes(0, 2) == 0 and lib.hn_track_state_bytes(1, 17) == 0
    fake = 1 << 20

    def call(k=2, h=480, w=640, side=(fake, fake, fake), state=fake, thr=300, hold=5, ids=(fake, fake)):
        return lib.hn_crop_resize_hands_tracked(fake, fake, fake, side[0], fake, 8, 2, 0, k, fake, 1, 1, 0, h, w, 176, 4, fake,
                                                fake, fake, fake, side[1], side[2], fake, state, thr, hold, ids[0], ids[1], None)
    err = lib.hn_last_error
    assert call(state=None) == 1 and b"hn_crop_resize_hands_tracked: null pointer" in err()
    assert call(ids=(None, fake)) == 1 and b"null pointer" in err()
    assert call(ids=(fake, None)) == 1 and b"null pointer" in err()
    assert call(side=(fake, None, fake)) == 1 and b"go together" in err()       # all three, or none of them
    assert call(side=(None, fake, fake)) == 1 and b"go together" in err()
    assert call(state=fake + 8) == 1 and b"16-byte aligned" in err()
    for thr in (0, 1001, -5):
        assert call(thr=thr) == 1 and b"thr_milli must be 1..1000" in err()
    for hold in (-1, 1000001):
        assert call(hold=hold) == 1 and b"hold must be 0..1000000" in err()
    assert call(h=32768) == 1 and b"32767" in err()
    assert call(w=40000) == 1 and b"32767" in err()
    for k in (0, 17):
        assert call(k=k) == 1 and b"max_hands must be 1..16" in err()


def test_python_wrapper_refuses_large_frames_and_bad_options():
    """Before anything touches a device."""
    import torch
    from hn_amd import ops
    state = torch.zeros((1, 3, 12), dtype=torch.int32)
    with pytest.raises(ValueError, match="32767"):
        ops.crop_resize_hands(None, 2, torch.empty((1, 1, 2, 32768)), 2, track=state)
    with pytest.raises(ValueError, match="track_iou"):
        ops.crop_resize_hands(None, 2, torch.empty((1, 1, 48, 64)), 2, track=state, track_iou=0.0)
    with pytest.raises(ValueError, match="track_hold"):
        ops.crop_resize_hands(None, 2, torch.empty((1, 1, 48, 64)), 2, track=state, track_hold=-1)


@pytest.mark.parametrize("slots,frames", [(2, 1), (64, 32), (7, 7), (48, 3)])
def test_layouts(slots, frames):
    """tracked=False is today's layout field for field, for every combination of the other options; tracked=True adds 8 bytes
    per slot behind `side` and moves only what lies behind it."""
    import torch
    from hn_amd.live import LiveLayout, LiveTrackedViews, LiveViews
    from hn_amd.pipeline import hands_record_rows, record_bytes
    v, hw, k = 778, (480, 640), slots // frames
    rb = record_bytes(3)
    rows = slots + 1 + (8 * slots + rb - 1) // rb
    front = ("record_rows", "record_bytes", "side_at")
    behind = ("lifted_at", "mesh_at", "overlay_at", "box_label_at", "pose_label_at", "nbytes")
    # views(): an untracked step's are today's seven; a tracked step's are those seven and the tracker's two rows at the end
    assert LiveViews._fields == ("records", "side", "lifted", "mesh", "overlay", "box_label", "pose_label")
    assert LiveTrackedViews._fields == LiveViews._fields + ("track_id", "track_age")
    lay = LiveLayout(frames, k, 5, tracked=True)
    buf = torch.zeros((lay.nbytes,), dtype=torch.uint8)
    tv = lay.views(buf)
    assert type(tv) is LiveTrackedViews and type(LiveLayout(frames, k, 5).views(buf[:LiveLayout(frames, k, 5).nbytes])) is LiveViews
    for t, at in ((tv.track_id, lay.track_id_at), (tv.track_age, lay.track_age_at)):
        assert t.data_ptr() - buf.data_ptr() == at and t.dtype == torch.int32 and tuple(t.shape) == (slots,)
    for overlay, labels, handed in itertools.product((False, True), repeat=3):
        a = LiveLayout(frames, k, v, hw, overlay, labels, handed)
        assert a == LiveLayout(frames, k, v, hw, overlay, labels, handed, False) and not a.tracked
        assert a.track_id_at is None and a.track_age_at is None
        # today's numbers, restated: records, [side], lifted, mesh, [overlay], [labels, dword aligned]
        at = rows * rb
        assert (a.record_rows, a.record_bytes) == (rows, rb) and a.side_at == (at if handed else None)
        at += 4 * slots * handed
        assert a.lifted_at == at and a.mesh_at == at + 4 * slots
        at += 4 * slots + slots * v * 12
        if overlay:
            assert a.overlay_at == at
            at += frames * 480 * 640 * 3
        if labels:
            assert a.box_label_at == at
            at += frames * 480 * 640 * 3
            assert a.pose_label_at == at
            at += slots * 176 * 176 * 3
        assert a.nbytes == at
        b = LiveLayout(frames, k, v, hw, overlay, labels, handed, True)
        for f in front:
            assert getattr(a, f) == getattr(b, f), f
        assert b.track_id_at == rows * rb + 4 * slots * handed and b.track_age_at == b.track_id_at + 4 * slots
        assert b.lifted_at == b.track_age_at + 4 * slots
        for f in behind:
            x, y = getattr(a, f), getattr(b, f)
            assert (x is None and y is None) or y - x == 8 * slots, f
    with pytest.raises(ValueError):
        LiveLayout(frames, None, v, tracked=True)
    # the engine's own to_host record: the existing layouts do not move, the ids and ages come last
    assert hands_record_rows(slots, rb) == hands_record_rows(slots, rb, False, False) == rows
    assert hands_record_rows(slots, rb, True) == hands_record_rows(slots, rb, True, False) == slots + 1 + (12 * slots + rb - 1) // rb
    assert hands_record_rows(slots, rb, False, True) == slots + 1 + (16 * slots + rb - 1) // rb
    assert hands_record_rows(slots, rb, True, True) == slots + 1 + (20 * slots + rb - 1) // rb


def test_record_tail_and_read_types():
    import torch
    from hn_amd.live import _read_type, LiveHandsRead, _HANDS_FIELDS
    from hn_amd.pipeline import hands_record_rows, read_hands_tail, record_bytes
    slots, rb = 6, record_bytes(3)
    rec = torch.zeros((hands_record_rows(slots, rb, True, True), rb), dtype=torch.uint8)
    words = rec.view(-1)[(slots + 1) * rb:].view(torch.int32)
    words[:5 * slots] = torch.arange(5 * slots, dtype=torch.int32)
    plain, sided, both = read_hands_tail(rec, slots), read_hands_tail(rec, slots, True), read_hands_tail(rec, slots, True, True)
    assert len(plain) == 2 and len(sided) == 3 and len(both) == 5
    for a, b in zip(plain + sided, both[:2] + both[:3]):
        assert torch.equal(a, b)
    assert both[3].tolist() == list(range(3 * slots, 4 * slots)) and both[4].tolist() == list(range(4 * slots, 5 * slots))
    unsided = read_hands_tail(rec, slots, False, True)
    assert unsided[2].tolist() == list(range(2 * slots, 3 * slots)) and len(unsided) == 4
    # read(): the existing positional forms give the existing classes; the tracked flag appends track_age, track_id
    assert _read_type("LiveHands", _HANDS_FIELDS, False, False, False) is LiveHandsRead
    t = _read_type("LiveHands", _HANDS_FIELDS, True, False, True, True)
    assert t._fields == _HANDS_FIELDS + ("overlay", "side", "track_age", "track_id") and t.box_label is None
    assert _read_type("LiveHands", _HANDS_FIELDS, False, False, False, True)._fields[-1] == "track_id"


def test_resource_report_shows_no_spill_and_no_scratch():
    """The tracked slot kernel runs from registers, like the plain one: no scratch, no VGPR or SGPR spill, both instantiations."""
    from hn_amd import _lib, build
    _lib.load()
    rows = (build.CSRC / "build" / "crop_stage.resources.txt").read_text().strip().splitlines()
    for kernel in ("hand_slots_tracked_kernel", "hand_slots_kernel"):
        mine = [r for r in rows if kernel in r.split(":")[0]]
        assert len(mine) == 2, (kernel, len(mine))
        for r in mine:
            assert " scratch 0 " in r and "vgpr_spill 0" in r and "sgpr_spill 0" in r, r


def test_crop_stage_kernels_live_in_one_file_once():
    """crop_stage.hip holds the stage's three kernels, two instantiations each, all from registers -- and no kernel of the
    top-1 copies they replaced; fcos_post.hip holds none of the five."""
    from hn_amd import _lib, build
    _lib.load()
    names = lambda f: [r.split(":")[0] for r in (build.CSRC / "build" / f).read_text().strip().splitlines()]
    rows = (build.CSRC / "build" / "crop_stage.resources.txt").read_text().strip().splitlines()
    assert len(rows) == 6
    for kernel in ("hand_slots_kernel", "hand_slots_tracked_kernel", "hand_crop_gather_kernel"):
        mine = [r for r in rows if kernel in r.split(":")[0]]
        assert len(mine) == 2, (kernel, len(mine))
        for r in mine:
            assert " scratch 0 " in r and "vgpr_spill 0" in r and "sgpr_spill 0" in r, r
    gone = ("15crop_box_kernel", "18crop_gather_kernel")      # (mangled with their lengths: the second ends the gather's name)
    assert not [n for n in names("crop_stage.resources.txt") if any(g in n for g in gone)]
    assert not [n for n in names("fcos_post.resources.txt")
                if any(k in n for k in gone + ("hand_slots_kernel", "hand_slots_tracked_kernel", "hand_crop_gather_kernel"))]
    assert build.EXTRA_FLAGS["crop_stage.hip"] == build.EXTRA_FLAGS["fcos_post.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]


def test_abi_and_bindings_are_unchanged():
    """The move changes no entry point: ABI 36 and the 136 bound signatures, every one of them exported by the built library."""
    from hn_amd import _lib
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES) == 136
    for name in ("hn_crop_resize", "hn_crop_resize_hands", "hn_crop_resize_hands_sided", "hn_crop_resize_hands_tracked",
                 "hn_track_state_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
