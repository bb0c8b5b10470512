"""The FCOS criterion's rule (tests/fcos_loss_ref.py) without a GPU: the rule against the imported reference's compute_loss
(tests/golden/fcos_loss.npz: the float32 matching bit for bit, the float64 terms for the batch and image by image), the reference's
own float32 result and the fp32 emulation of the kernels inside the derived bound, every mutant of the emulation outside it on a
golden configuration, the target packing and its refusals, the C entries' bindings, and the drop-in's paths that keep raising."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import fcos_loss_cases as lc
import fcos_loss_ref as fr


def _image_losses(name, want):
    c = lc.BY_NAME[name]
    return np.stack([fr._losses(want["terms"][i:i + 1], want["fg"][i:i + 1], lc.points(c)) for i in range(c.n)])


@pytest.mark.parametrize("tag", list(lc.GOLDEN))
def test_rule_is_the_references_criterion(golden_dir, tag):
    g = np.load(golden_dir / "fcos_loss.npz")
    name = lc.GOLDEN[tag]
    assert int(g[f"{tag}_seed"]) == lc.BY_NAME[name].seed
    want, b = lc.reference(name)
    assert np.array_equal(want["matched"], g[f"{tag}_matched"]) and want["matched"].dtype == np.int32
    rel = lambda got, ref: (np.abs(got - ref) <= 1e-12 * np.abs(ref)).all()
    assert rel(want["losses"], g[f"{tag}_f64_losses"]), (want["losses"], g[f"{tag}_f64_losses"])
    assert rel(_image_losses(name, want), g[f"{tag}_f64_image_losses"])
    # the reference's own all-float32 run lies inside the bound
    err = np.abs(g[f"{tag}_f32_losses"] - want["losses"])
    ratio = np.where(err == 0, 0.0, err / np.where(b["losses"] > 0, b["losses"], 1.0))
    print(f"golden {tag}: the reference's float32 run, |err| / bound = {np.round(ratio, 4).tolist()}")
    assert (err <= b["losses"]).all()
    # image by image == the batch of one
    for i in range(lc.BY_NAME[name].n):
        one = fr.rule(*lc.image(name, i))
        assert np.array_equal(one["terms"][0], want["terms"][i]) and np.array_equal(one["matched"][0], want["matched"][i])


def test_the_cases_meet_their_conditions():
    assert lc.NAMES == ("golden-1", "golden-2", "1pt", "edge", "chunks", "chunks-ext", "nofg", "sat")
    m = lc.reference("golden-1")[0]["matched"][0]
    at = lambda x, y, lvl=0: int(m[[0, 1360, 1700][lvl] + (y // (8 << lvl)) * [34, 17, 9][lvl] + x // (8 << lvl)])
    assert at(120, 120) == 0                          # nested: the larger box has the larger key
    assert at(216, 56) == 2                           # keys tie in float32: the first index
    assert at(56, 216) == -1 and at(64, 216) == 4     # an edge on the anchor centre is not inside
    assert at(152, 248) == 5 and at(144, 248) == -1   # distance exactly 8 * size on level 0
    assert at(144, 240, 1) == -1 and at(160, 256, 1) == -1       # ... and exactly 4 * size on level 1
    gt = lc.make("golden-1")[3]
    keys = np.float32(1e8) - (gt[0][0, :, 1] - gt[0][0, :, 0]) * (gt[0][0, :, 3] - gt[0][0, :, 1])
    assert keys[2] == keys[3] and keys[0] > keys[1]
    assert lc.points(lc.BY_NAME["chunks"]) == 1790 and lc.make("chunks")[3][3].tolist() == [64, 1, 0]
    assert lc.make("chunks-ext")[3][3].tolist() == [64, 1, 2]
    for name in ("golden-1", "edge"):                 # foreground on every level
        c = lc.BY_NAME[name]
        lvl = np.searchsorted(fr.cr.starts_of(c.sizes)[1:], np.nonzero(lc.reference(name)[0]["matched"] >= 0)[1], side="right")
        assert set(lvl.tolist()) == set(range(len(c.sizes))), name
    want, b = lc.reference("nofg")
    assert not want["fg"].any() and not want["terms"][:, 1:3].any() and not b["terms"][:, 1:3].any()
    assert lc.reference("1pt")[0]["fg"].tolist() == [1]
    assert all(np.abs(t).max() == 80.0 for t in lc.make("sat")[0]) and np.isfinite(lc.reference("sat")[0]["losses"]).all()


@pytest.mark.parametrize("name", lc.NAMES)
def test_emulation_is_inside_the_bound(name):
    detail = {}
    ratio = fr.check(fr.emulate(*lc.args(name)), lc.reference(name), detail=detail)
    print(f"fcos loss emulate {name}: max |err| / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in detail.items()))
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", fr.MUTANTS)
def test_every_mutant_fails_on_a_golden_configuration(mutant):
    """on the whole batch or on one of its images as a batch of one, the runs the golden holds"""
    failed = []
    for name in lc.GOLDEN.values():
        for a in [lc.args(name)] + [lc.image(name, i) for i in range(lc.BY_NAME[name].n)]:
            try:
                fr.check(fr.mutants()[mutant](*a), (fr.rule(*a), fr.bound(*a)))
            except AssertionError as e:
                assert "bound" in str(e)
                failed.append(name)
    assert failed, mutant


def test_pack_fcos_targets(monkeypatch):
    from hn_amd import ops
    from oracle import fcos_ref
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)        # (no device here: keep the tables on the host)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    boxes = torch.tensor([[10.0, 20.0, 110.5, 220.25], [3.0, 4.0, 5.0, 6.0]])
    t = {"boxes": boxes, "labels": torch.tensor([1, 0]), "box_info": torch.tensor([[1.0, 0.0, 0.5, 0.1, 0.0], [-1.0, -1.0, 0.0, 0.0, 0.0]])}
    ratios = ops.fcos_target_ratios([(480, 640)], [(800, 1067)])
    packed = ops.pack_fcos_targets([t], ratios, num_classes=3, ext=True)
    want = fcos_ref.resize_boxes(boxes, (480, 640), (800, 1067))
    assert torch.equal(packed.boxes[0], want) and packed.count.tolist() == [2] and packed.labels.dtype == torch.int32
    assert ops.pack_fcos_targets([t], ratios, G=7).boxes.shape == (1, 7, 4)
    for bad, err in (({"boxes": torch.tensor([[5.0, 5.0, 5.0, 9.0]])}, ValueError), ({"boxes": torch.tensor([[5.0, 9.0, 6.0, 9.0]])}, ValueError),
                     ({"labels": torch.tensor([3, 0])}, ValueError), ({"labels": torch.tensor([-1, 0])}, ValueError)):
        d = dict(t, **bad)
        if "boxes" in bad:
            d["labels"], d["box_info"] = t["labels"][:1], t["box_info"][:1]
        with pytest.raises(err):
            ops.pack_fcos_targets([d], ratios, num_classes=3)
    many = {"boxes": boxes[:1].repeat(65, 1), "labels": torch.zeros(65, dtype=torch.int64), "box_info": torch.zeros(65, 5)}
    with pytest.raises(ValueError, match="more than 64"):
        ops.pack_fcos_targets([many], ratios)
    with pytest.raises(ValueError, match="G = 65"):
        ops.pack_fcos_targets([t], ratios, G=65)
    empty = {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64), "box_info": torch.zeros(0, 5)}
    with pytest.raises(KeyError, match="hand_contact_state"):
        ops.pack_fcos_targets([t, empty], ratios * 2, ext=True)
    assert ops.pack_fcos_targets([t, empty], ratios * 2, ext=False).count.tolist() == [2, 0]


def test_padding_rows_never_change_the_rule():
    a = lc.args("golden-2")
    want = lc.reference("golden-2")[0]
    c = lc.BY_NAME["golden-2"]
    for fill in (0.0, 1e6, -3.0):
        wide = lc.pad_targets(c.targets, g=9, fill=fill)
        got = fr.rule(*a[:5], *wide)
        assert all(np.array_equal(got[k], want[k]) for k in want)


def test_entry_points_are_bound():
    from hn_amd import _lib
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION
    assert {"hn_fcos_loss_f32", "hn_fcos_loss_ws_bytes"} <= set(_lib.SIGNATURES)
    assert lib.hn_fcos_loss_ws_bytes(3, 1790) == 3 * (2 + 1) * 64 and lib.hn_fcos_loss_ws_bytes(0, 5) == 0
    # refused on the host, before any launch: null pointers, G and num_classes out of range
    lv = _lib.FcosLevels()
    lv.num_levels = 1
    lv.h[0], lv.w[0], lv.stride[0] = 1, 1, 8
    lv.cls_lr[0] = lv.reg_ctr[0] = 64                      # (never dereferenced on the host)
    p = 64
    call = lambda **k: lib.hn_fcos_loss_f32(C.byref(lv), None, 1, k.get("c", 3), k.get("boxes", p), p, p, p, k.get("g", 4), 1.5,
                                            p, p, p, None, k.get("ws", p), 64 * 2, None)
    for kw, word in ((dict(boxes=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(g=0), b"outside 1..64"),
                     (dict(g=65), b"outside 1..64"), (dict(c=0), b"outside 1..8"), (dict(c=9), b"outside 1..8")):
        assert call(**kw) != 0 and word in lib.hn_last_error(), kw


def test_the_drop_in_is_opt_in():
    from fcos_utils.fcos import FCOS
    net = FCOS(num_classes=3)
    assert net._device_loss is False
    with pytest.raises(NotImplementedError):
        net.train()(images=[], targets=[{}])
    with pytest.raises(NotImplementedError):
        net.train()(images=[])
    with pytest.raises(NotImplementedError):
        net.eval()(images=[], targets=[{}])
    assert net.device_loss() is net and net._device_loss is True
    with pytest.raises(NotImplementedError):                 # on, in eval mode: targets are still refused
        net.eval()(images=[], targets=[{}])
    with pytest.raises(ValueError, match="targets should be passed"):
        net.train()(images=[])
    assert net.device_loss(False)._device_loss is False
    assert "out of scope" not in sys.modules[FCOS.__module__].__doc__
