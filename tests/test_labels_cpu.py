"""The label images without a GPU: the entry point's surface and argument checks, the numpy statement of the rule
(tests/draw_ref.py) against itself, and the layout of the live steps' buffer."""
import ctypes as C
import re

import numpy as np
import pytest

import draw_ref as dr


def test_entry_point_is_declared_bound_and_exported():
    import subprocess
    from hn_amd import _lib, build
    text = (build.REPO_ROOT / "include" / "handnet_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+hn_draw_labels_u8\s*\(([^)]*)\)\s*;", text)
    assert proto
    params = [p.strip() for p in proto.group(1).split(",")]
    res, args = _lib.SIGNATURES["hn_draw_labels_u8"]
    assert res is C.c_int and len(params) == len(args) == 13
    for p, a in zip(params, args):
        assert (a is C.c_void_p) if "*" in p else (p.startswith("int ") and a is C.c_int), p
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T hn_draw_labels_u8\b", out)
    assert _lib.load().hn_abi_version() == 36 and _lib.ABI_VERSION == 36
    assert "typedef struct" not in proto.group(0)


def test_argument_errors_do_not_need_a_gpu():
    """Every argument check comes before the first launch: HN_ERR_ARG and a message, no device touched (the pointers are
    never dereferenced)."""
    from hn_amd import _lib
    lib = _lib.load()
    P = 4096        # stands for a device address

    def call(kp=P, box=P, drawn=None, s=2, k=2, frame=P, fmt=0, h=480, w=640, clamp=1, out_box=P, out_pose=P):
        return lib.hn_draw_labels_u8(kp, box, drawn, s, k, frame, fmt, h, w, clamp, out_box, out_pose, None)
    cases = ((dict(h=0), b"frame size"), (dict(w=0), b"frame size"), (dict(h=16385), b"frame size"), (dict(w=16385), b"frame size"),
             (dict(h=-1), b"frame size"), (dict(k=0), b"at least 1"), (dict(k=-2), b"at least 1"), (dict(s=3, k=2), b"multiple"),
             (dict(kp=None), b"keypoints is NULL"), (dict(box=None), b"crop_box is NULL"),
             (dict(out_box=None, out_pose=None), b"both NULL"), (dict(fmt=2), b"format"), (dict(frame=None), b"frame is NULL"))
    for kw, word in cases:
        assert call(**kw) == 1, kw
        assert word in lib.hn_last_error(), (kw, lib.hn_last_error())


def test_resource_report_shows_no_spill_and_no_scratch():
    from hn_amd import _lib, build
    _lib.load()
    rows = (build.CSRC / "build" / "label_draw.resources.txt").read_text().strip().splitlines()
    assert sum("label_box_kernel" in r for r in rows) == 4 and sum("label_pose_kernel" in r for r in rows) == 2
    for r in rows:
        assert " scratch 0 " in r and "vgpr_spill 0" in r and "sgpr_spill 0" in r, r
    assert build.EXTRA_FLAGS["label_draw.hip"] == ["-ffp-contract=off"]


def _grid_segments(n=12):
    pts = [(x, y) for x in range(n) for y in range(n)]
    return ((a, b) for a in pts for b in pts)


def test_stepping_bresenham_equals_the_closed_form():
    count = 0
    for (x0, y0), (x1, y1) in _grid_segments():
        a, b = dr.line_points(x0, y0, x1, y1), dr.line_points_stepping(x0, y0, x1, y1)
        assert a == b, ((x0, y0), (x1, y1))
        assert a[0] == (x0, y0) and a[-1] == (x1, y1) and len(a) == max(abs(x1 - x0), abs(y1 - y0)) + 1
        count += 1
    assert count == 144 * 144
    assert dr.line_points(3, 4, 3, 4) == [(3, 4)]
    # a tie stays on the start point's side: (0,0) -> (2,1) passes (1,0); the other way round it passes (1,1)
    assert dr.line_points(0, 0, 2, 1) == [(0, 0), (1, 0), (2, 1)]
    assert dr.line_points(2, 1, 0, 0) == [(2, 1), (1, 1), (0, 0)]


def test_disc_has_13_pixels():
    pts = dr.disc_points(10, 20)
    assert len(pts) == len(set(pts)) == 13 and (12, 20) in pts and (10, 18) in pts and (12, 21) not in pts


def test_resize_identity_mean_and_constant():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(176, 176, 3), dtype=np.uint8)
    assert np.array_equal(dr.resize176(img), img)
    big = rng.integers(0, 256, size=(352, 352, 3), dtype=np.uint8)
    b = big.astype(np.int64)
    mean = (b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2
    assert np.array_equal(dr.resize176(big), mean.astype(np.uint8))
    for s in range(1, 401):
        i0, i1, w0, w1 = dr.resize_taps(s)
        assert np.all(w0 + w1 == 2048) and i0.min() >= 0 and i1.max() <= s - 1 and np.all((i1 == i0) | (i1 == i0 + 1))
        for value in (0, 1, 77, 254, 255):
            crop = np.full((1 if s % 7 else s, s, 3), value, np.uint8)        # (the full square now and then, a single row else)
            assert np.all(dr.resize176(crop) == value), (s, value)
    for s in (1, 2, 175, 176, 177, 352, 400):
        assert np.all(dr.resize176(np.full((s, 3, 3), 200, np.uint8)) == 200)


def test_draw_order_and_colours():
    """The skeleton's layers follow VisualUtil('dexycb'): per finger discs then lines; finger 4 also draws joint 0; the
    last layer wins on a shared pixel."""
    kp = np.zeros((21, 3), np.float32)
    kp[:, 0] = np.arange(21) * 8 + 4.9
    kp[:, 1] = 50.2
    layers = dr.skeleton_layers(kp, True)
    assert [k for k, _, _ in layers] == (["disc"] * 4 + ["line"] * 4) * 4 + ["disc"] * 5 + ["line"] * 4
    assert len(layers) == 41
    img = dr.draw_skeleton(np.zeros((176, 176, 3), np.uint8), kp, True)
    assert tuple(img[50, 4]) == (255, 153, 153)          # joint 0: drawn last, by finger 4
    # (the joints lie on one row, so finger 4's first bone runs over all of them: look at the discs' rims)
    assert tuple(img[52, 12]) == (102, 0, 0) and tuple(img[52, 8 * 9 + 4]) == (255, 0, 0) and tuple(img[50, 12]) == (255, 153, 153)
    # all joints on one pixel: 13 disc pixels of the last finger's colour, nothing else
    one = dr.draw_skeleton(np.zeros((176, 176, 3), np.uint8), np.full((21, 3), 88.7, np.float32), True)
    assert int((one.sum(axis=2) > 0).sum()) == 13 and tuple(one[88, 88]) == (255, 153, 153)
    assert dr.joint_pixel(175.9999, True) == 175 and dr.joint_pixel(300.0, True) == 176 and dr.joint_pixel(-3.5, True) == 0
    assert dr.joint_pixel(-3.5, False) == -3 and dr.joint_pixel(float("nan"), True) == 0


def test_rectangle_and_box_rule():
    img = np.zeros((10, 12, 3), np.uint8)
    dr.rectangle(img, 2, 3, 12, 8)           # x2 == W: the right edge is invisible
    on = img[:, :, 1] == 255
    assert on[3, 2:12].all() and on[8, 2:12].all() and on[3:9, 2].all() and int(on.sum()) == 10 + 10 + 4
    # the clamp quirk: x1 is clamped to H, not W
    (x1, y1, x2, y2), (cx, cy), (sw, sh), drawn = dr.slot_box([500, 10, 600, 200], 1, 480, 640, True)
    assert (x1, x2, cx, sw, sh, drawn) == (480, 600, 480, 120, 190, True)
    assert dr.slot_box([500, 10, 600, 200], 1, 480, 640, False)[0][0] == 500
    assert not dr.slot_box([5, 5, 5, 50], 1, 480, 640, True)[3] and not dr.slot_box([5, 5, 50, 50], 0, 480, 640, True)[3]
    assert not dr.slot_box([5, 5, 50, 50], 2, 480, 640, True)[3] and dr.slot_box([5, 5, 50, 50], None, 480, 640, True)[3]


def test_layouts_without_labels_are_the_parents():
    from hn_amd.live import LiveLayout
    front = lambda a: (a.record_rows, a.record_bytes, a.side_at, a.lifted_at, a.mesh_at)       # what every step has
    for n, v, h, w in ((1, 778, 480, 640), (3, 778, 37, 53), (32, 1538, 480, 640)):
        for k in (None, 1, 2):
            s = n * (k or 1)
            # labels off: the step with an overlay and the bare step as they were, and no offset for what is not there
            bare, shown = LiveLayout(n, k, v), LiveLayout(n, k, v, (h, w), overlay=True)
            assert LiveLayout(n, k, v, (h, w), overlay=True, labels=False) == shown
            assert LiveLayout(n, k, v, (h, w), overlay=False, labels=False).nbytes == bare.nbytes
            assert front(LiveLayout(n, k, v, (h, w))) == front(bare) == front(shown)
            assert bare.overlay_at is None and shown.overlay_at == bare.nbytes and shown.nbytes == bare.nbytes + n * h * w * 3
            for a in (bare, shown):
                assert a.box_label_at is None and a.pose_label_at is None
            # labels on: both images behind what the parent step has, each on a dword, nothing in front of them moved
            for parent in (bare, shown):
                got = LiveLayout(n, k, v, (h, w), overlay=parent.overlay, labels=True)
                end, bo, po = parent.nbytes, got.box_label_at, got.pose_label_at
                assert front(got) == front(parent) and got.overlay_at == parent.overlay_at
                assert end <= bo < end + 4 and bo % 4 == 0 and po % 4 == 0
                assert bo + n * h * w * 3 <= po < bo + n * h * w * 3 + 4 and got.nbytes == po + s * 92928
    # the camera's frame needs no padding: the growth is exactly N H W 3 + N K 92928
    a = LiveLayout(32, 2, 778, (480, 640), overlay=True, labels=False).nbytes
    b = LiveLayout(32, 2, 778, (480, 640), overlay=True, labels=True).nbytes
    assert b - a == 32 * 480 * 640 * 3 + 64 * 92928


def test_read_results_carry_absent_images_as_none():
    from hn_amd import live
    assert live.LiveRead.overlay is None and live.LiveRead.box_label is None and live.LiveRead.pose_label is None
    assert live.LiveOverlayRead.box_label is None and live.LiveHandsOverlayRead.pose_label is None
    assert live.LiveLabelsRead.overlay is None and live.LiveHandsLabelsRead.overlay is None
    assert live.LiveRead._fields == ("keypoints", "has_hand", "crop_box", "words", "more", "mesh")
    assert live.LiveOverlayRead._fields == live.LiveRead._fields + ("overlay",)
    assert live.LiveHandsLabelsRead._fields == live.LiveHandsRead._fields + ("box_label", "pose_label")
    assert live.LiveHandsOverlayLabelsRead._fields == live.LiveHandsRead._fields + ("overlay", "box_label", "pose_label")
    r = live.LiveRead(1, 2, 3, 4, 5, 6)
    assert tuple(r) == (1, 2, 3, 4, 5, 6) and r.mesh == 6 and r.box_label is None
