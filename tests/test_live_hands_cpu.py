"""The K-hand live step (hn_amd.live.LiveHandsEngine, HandNet.live_hands, hn_lifter_input_gated_f32): argument contracts, the
host buffer's layout and the skip rule's boundary cases, checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

PARAS = (617.343, 617.343, 312.42, 241.42)


def _spread(n, lo, hi, seed):
    """n float32 values from lo to hi, both ends included, in a shuffled joint order."""
    v = np.linspace(lo, hi, n, dtype=np.float64).astype(np.float32)
    v[0], v[-1] = np.float32(lo), np.float32(hi)
    return np.random.default_rng(seed).permutation(v)


def gate_cases():
    """(name, uv [21,2] float32, valid flag) around process_bbox(get_bbox(uv))'s boundary (coord_utils.py:21-49): the rule
    holds iff the fp32 box has w * h > 0, x + (w - 1) >= x and y + (h - 1) >= y."""
    below1 = np.nextafter(np.float32(1.0), np.float32(0.0))                # one fp32 ulp below 1
    cases = []

    def add(name, xs, ys, valid=1):
        cases.append((name, np.stack([np.asarray(xs, np.float32), np.asarray(ys, np.float32)], axis=1), valid))
    ys = _spread(21, 50.0, 80.0, 1)
    add("width exactly 1 px", _spread(21, 100.0, 101.0, 2), ys)
    add("width 1 px at x = 0", _spread(21, 0.0, 1.0, 3), ys)
    add("width one ulp below 1 px, small x", _spread(21, 0.0, below1, 4), ys)
    big = np.float32(1000.0)
    add("width one ulp below 1 px, large x", _spread(21, big, np.nextafter(big + np.float32(1.0), big), 5), ys)
    # a negative power of two: the joints span less than 1 px, get_bbox's roundings give a box of 1 px, which is kept
    add("width two ulps below 1 px at x = -2", _spread(21, -2.0, np.nextafter(np.float32(-1.0), np.float32(-2.0)), 6), ys)
    # 1 px wide at 1e7 (fp32 ulp 1): get_bbox's centre rounds to even and the box collapses to width 0
    add("width 1 px at x = 1e7, even start", _spread(21, 1e7, 1e7 + 1.0, 7), ys)
    add("width 1 px at x = 1e7, odd start", _spread(21, 1e7 + 1.0, 1e7 + 2.0, 8), ys)
    add("width 2 px at x = 1e7", _spread(21, 1e7, 1e7 + 2.0, 9), ys)
    add("zero height", _spread(21, 40.0, 90.0, 10), np.full(21, 60.0))
    add("height one ulp below 1 px", _spread(21, 40.0, 90.0, 11), _spread(21, 0.0, below1, 12))
    add("all joints equal", np.full(21, 88.5), np.full(21, 88.5))
    add("all joints at the crop edge", np.full(21, 640.0), np.full(21, 480.0))
    add("ordinary hand", _spread(21, 210.0, 290.0, 13), _spread(21, 120.0, 230.0, 14))
    add("ordinary hand, valid 0", _spread(21, 210.0, 290.0, 13), _spread(21, 120.0, 230.0, 14), 0)
    add("ordinary hand, valid 2", _spread(21, 210.0, 290.0, 13), _spread(21, 120.0, 230.0, 14), 2)
    return cases


def oracle_lifted(uv, valid):
    from oracle import pose2mesh_ref
    return valid == 1 and pose2mesh_ref.process_bbox(pose2mesh_ref.get_bbox(uv).copy()) is not None


def test_gate_cases_straddle_the_rule():
    """The boundary cases decide both ways under the reference's rule (numpy float32, one rounding per operation), and the
    ones named for it are decided by the rounding itself."""
    got = {name: oracle_lifted(uv, valid) for name, uv, valid in gate_cases()}
    assert got["width exactly 1 px"] and got["width 1 px at x = 0"] and got["ordinary hand"]
    # the same joint spread decides differently by position: at x = 1000 (fp32 ulp 2^-14) get_bbox's centre and half-width
    # round the box back to 1 px; at x = 0 the box keeps its width 1 - 2^-24 and x + (w - 1) < x
    assert not got["width one ulp below 1 px, small x"] and got["width one ulp below 1 px, large x"]
    assert got["width two ulps below 1 px at x = -2"]
    assert not got["width 1 px at x = 1e7, even start"] and not got["width 1 px at x = 1e7, odd start"]
    assert got["width 2 px at x = 1e7"]
    assert not got["zero height"] and not got["height one ulp below 1 px"] and not got["all joints equal"]
    assert not got["all joints at the crop edge"]
    assert not got["ordinary hand, valid 0"] and not got["ordinary hand, valid 2"]


@pytest.mark.parametrize("k", [0, 17, -1, 2.5, None])
def test_live_hands_refuses_out_of_range_counts(k):
    """max_hands outside 1..16 is refused before any engine or device is touched."""
    import types

    from handnet_pipeline.handnet_pipeline import HandNet
    from hn_amd.live import LiveHandsEngine
    with pytest.raises(ValueError, match="max_hands"):
        LiveHandsEngine(None, None, PARAS, max_hands=k)
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    with pytest.raises(ValueError, match="max_hands"):
        net.live_hands(None, PARAS, max_hands=k)


def test_gated_entry_refuses_bad_arguments_without_a_gpu():
    from hn_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(256)     # never dereferenced: the argument checks run before any launch
    for args in ((None, None, 4, 21, fake, fake), (fake, None, 4, 21, None, fake), (fake, None, 4, 21, fake, None)):
        assert lib.hn_lifter_input_gated_f32(*args, None) == 1 and b"null pointer" in lib.hn_last_error()
    for n, j in ((4, 1), (4, 0), (-1, 21)):
        assert lib.hn_lifter_input_gated_f32(fake, fake, n, j, fake, fake, None) == 1
        assert b"bad dims" in lib.hn_last_error()
    assert lib.hn_lifter_input_gated_f32(fake, fake, 0, 21, fake, fake, None) == 0     # nothing to do: no launch


@pytest.mark.parametrize("n,k,v", [(1, 1, 778), (1, 2, 778), (32, 2, 1152), (32, 16, 778)])
def test_host_buffer_layout_and_read(n, k, v):
    """The buffer's offsets follow from hands_record_rows, and LiveHandsOutput.read() takes every field from its place."""
    import torch
    from hn_amd import pipeline
    from hn_amd.live import LiveHandsOutput, LiveLayout
    s = n * k
    layout = LiveLayout(n, k, v)
    rows, rb, lo, mo, nbytes = layout.record_rows, layout.record_bytes, layout.lifted_at, layout.mesh_at, layout.nbytes
    assert layout.side_at is None and layout.overlay_at is None and layout.box_label_at is None and layout.pose_label_at is None
    assert rb == pipeline.record_bytes(3) and rows == pipeline.hands_record_rows(s, rb)
    assert lo == rows * rb and mo == lo + 4 * s and nbytes == mo + s * v * 12 and lo % 8 == 0 and mo % 4 == 0
    g = torch.Generator().manual_seed(s)
    kp, img, xyz = (torch.randn((s, 21, 3), generator=g) for _ in range(3))
    box = torch.randint(0, 640, (s, 4), generator=g, dtype=torch.int64)
    has = torch.randint(0, 3, (s,), generator=g, dtype=torch.int32)
    score, index = torch.rand((s,), generator=g), torch.randint(-1, 50, (s,), generator=g, dtype=torch.int32)
    lifted = torch.randint(0, 2, (s,), generator=g, dtype=torch.int32)
    mesh = torch.randn((s, v, 3), generator=g)
    host = torch.zeros((nbytes,), dtype=torch.uint8)
    rec = host[:lo].view(rows, rb)
    rec[:s, :32] = box.view(torch.uint8).view(s, 32)
    rec[:s, 32:36] = has.view(torch.uint8).view(s, 4)
    for f, t in enumerate((kp, img, xyz)):
        rec[:s, 40 + 252 * f:40 + 252 * (f + 1)] = t.view(torch.uint8).view(s, 252)
    rec[s, :16] = torch.tensor([0, 0, 0, 7], dtype=torch.int32).view(torch.uint8)
    sc, ix = pipeline._hands_tail(rec, s)
    sc.copy_(score)
    ix.copy_(index)
    host[lo:mo] = lifted.view(torch.uint8)
    host[mo:] = mesh.view(-1).view(torch.uint8)
    r = LiveHandsOutput(None, None, None, torch.empty((n, k, v, 3)), None, host, n, k, layout=layout).read()
    per = lambda t: t.reshape((n, k) + tuple(t.shape[1:]))
    assert torch.equal(r.keypoints, per(kp)) and torch.equal(r.image_uvd, per(img)) and torch.equal(r.xyz_mm, per(xyz))
    assert torch.equal(r.crop_box, per(box)) and torch.equal(r.has_hand, per(has))
    assert torch.equal(r.score, per(score)) and torch.equal(r.det_index, per(index))
    assert r.lifted.dtype == torch.bool and torch.equal(r.lifted, per(lifted) != 0)
    assert torch.equal(r.mesh, per(mesh)) and r.words == [0, 0, 0, 7]
    host.zero_()            # fresh tensors: the pinned buffer is the next step's
    assert r.mesh.abs().sum() > 0 and r.keypoints.abs().sum() > 0 and bool(r.lifted.any() == per(lifted).bool().any())
