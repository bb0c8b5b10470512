"""hn_amd.live.LiveLayout against the byte offsets of the layout functions it replaced."""
import json

import pytest
import torch


def test_layout_reproduces_the_replaced_functions(golden_dir):
    """tests/golden/live_layout.json holds what commit 01c37630d31f's six layout functions in hn_amd/live.py
    (live_overlay_layout, live_labels_layout, live_hands_layout, live_hands_overlay_layout, live_hands_labels_layout -- the
    narrower ones cross-checked against the widest --, and _labels_behind through them) return over frames 1, 2, 3, 32 x hands
    None, 1, 2, 3, 16 x vertices 778 (and 5 at one frame) x frames of 5x7, 48x64, 480x640 x overlay x labels x handed (K-hand
    steps): inputs, record rows and bytes, every offset (null: the step has no such part) and the total.  LiveLayout gives
    every row exactly -- the 5x7 frames in odd numbers included, whose images end off a dword, so that the label images are
    padded."""
    table = json.loads((golden_dir / "live_layout.json").read_text())
    from hn_amd.live import LiveLayout
    cols = table["columns"]
    assert len(table["rows"]) == 540
    padded = 0
    for row in table["rows"]:
        r = dict(zip(cols, row))
        got = LiveLayout(r["frames"], r["hands"], r["vertices"], (r["h"], r["w"]), bool(r["overlay"]), bool(r["labels"]),
                         bool(r["handed"]))
        assert [getattr(got, c) for c in cols[8:]] == row[8:], r
        if not (r["overlay"] or r["labels"]):        # a step that draws nothing has no frame size to give
            bare = LiveLayout(r["frames"], r["hands"], r["vertices"], handed=bool(r["handed"]))
            assert [getattr(bare, c) for c in cols[8:]] == row[8:], r
        if r["labels"]:
            before = r["mesh_at"] + got.slots * r["vertices"] * 12 + (r["frames"] * r["h"] * r["w"] * 3 if r["overlay"] else 0)
            padded += (r["box_label_at"] != before) + (r["pose_label_at"] != r["box_label_at"] + r["frames"] * r["h"] * r["w"] * 3)
    assert padded > 0
    # spot values, as the parent's functions gave them
    a = LiveLayout(1, None, 778, (480, 640), True, True)
    assert (a.mesh_at, a.overlay_at, a.box_label_at, a.pose_label_at, a.nbytes) == (1600, 10936, 932536, 1854136, 1947064)
    b = LiveLayout(2, None, 778, (5, 7), False, True)
    assert (b.mesh_at, b.overlay_at, b.box_label_at, b.pose_label_at, b.nbytes) == (2400, None, 21072, 21284, 207140)
    c, d = LiveLayout(1, 2, 778), LiveLayout(1, 2, 778, handed=True)
    assert (c.record_rows, c.record_bytes, c.side_at, c.lifted_at, c.mesh_at, c.nbytes) == (4, 800, None, 3200, 3208, 21880)
    assert (d.record_rows, d.record_bytes, d.side_at, d.lifted_at, d.mesh_at, d.nbytes) == (4, 800, 3200, 3208, 3216, 21888)


def test_views_cut_the_buffer_where_the_layout_says():
    """views(): every part typed and shaped, starting at its offset, None where the step has none; the parts do not overlap and
    end at nbytes."""
    from hn_amd.live import LiveLayout
    lay = LiveLayout(3, 2, 5, (5, 7), True, True, True)
    buf = torch.zeros((lay.nbytes,), dtype=torch.uint8)
    v = lay.views(buf)
    want = {"records": (0, torch.uint8, (lay.record_rows, lay.record_bytes)), "side": (lay.side_at, torch.int32, (6,)),
            "lifted": (lay.lifted_at, torch.int32, (6,)), "mesh": (lay.mesh_at, torch.float32, (6, 5, 3)),
            "overlay": (lay.overlay_at, torch.uint8, (3, 5, 7, 3)), "box_label": (lay.box_label_at, torch.uint8, (3, 5, 7, 3)),
            "pose_label": (lay.pose_label_at, torch.uint8, (6, 176, 176, 3))}
    assert v._fields == tuple(want)
    end = 0
    for name, (at, dtype, shape) in want.items():
        t = getattr(v, name)
        assert t.data_ptr() - buf.data_ptr() == at >= end and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()
        end = at + t.numel() * t.element_size()
    assert end == lay.nbytes
    bare = LiveLayout(3, None, 5).views(torch.zeros((LiveLayout(3, None, 5).nbytes,), dtype=torch.uint8))
    assert [f for f in bare._fields if getattr(bare, f) is None] == ["side", "lifted", "overlay", "box_label", "pose_label"]
    with pytest.raises(ValueError):
        LiveLayout(1, 2, 778, None, overlay=True)
    with pytest.raises(ValueError):
        LiveLayout(1, None, 778, handed=True)
