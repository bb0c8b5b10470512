"""Up to K hands per frame: the argument contract of every layer, checked without a GPU."""
import ctypes as C

import pytest


def test_abi_version_is_36():
    from hn_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 36 and lib.hn_abi_version() == 36


@pytest.mark.parametrize("k", [0, 17, -1])
def test_crop_resize_hands_refuses_out_of_range_counts(k):
    from hn_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(256)     # never dereferenced: the argument checks run before any launch
    st = lib.hn_crop_resize_hands(fake, fake, fake, fake, 8, 2, k, fake, 1, 1, 0, 480, 640, 176, 4, fake, fake, fake, fake,
                                  fake, None)
    assert st == 1 and b"max_hands must be 1..16" in lib.hn_last_error()


def test_top1_entry_wants_aligned_crops_and_takes_an_8_byte_aligned_box():
    """hn_crop_resize stores the crops as 16-byte vectors, like its siblings, and refuses a pointer that would split one; its
    crop_box is the C caller's own int64 array and needs no more than that.  No launch is reached: the entry checks the
    addresses before the channel count, so the refusal of five channels tells that the addresses before it were accepted."""
    from hn_amd import _lib
    lib = _lib.load()
    fake = 1 << 20

    def call(crop_box=fake, crops=fake, in_ch=5):
        return lib.hn_crop_resize(fake, fake, fake, 8, 2, fake, 1, in_ch, 0, 480, 640, 176, 4, crop_box, fake, crops, None)
    assert call(crops=fake + 8) == 1 and b"16-byte aligned" in lib.hn_last_error()
    assert call(crops=fake + 4) == 1 and b"16-byte aligned" in lib.hn_last_error()
    assert call(crop_box=fake + 8) == 1 and b"depth image must have 1..4 channels" in lib.hn_last_error()
    assert call() == 1 and b"depth image must have 1..4 channels" in lib.hn_last_error()
    # its siblings still want both at 16 bytes
    st = lib.hn_crop_resize_hands(fake, fake, fake, fake, 8, 2, 1, fake, 1, 5, 0, 480, 640, 176, 4, fake + 8, fake, fake, fake, fake,
                                  None)
    assert st == 1 and b"16-byte aligned" in lib.hn_last_error()


@pytest.mark.parametrize("k", [0, 17, 2.5, "2", None])
def test_python_layers_refuse_out_of_range_counts(k):
    from hn_amd import ops
    with pytest.raises(ValueError, match="max_hands"):
        ops.check_max_hands(k)
    with pytest.raises(ValueError, match="max_hands"):
        ops.crop_resize_hands(None, 2, None, k)


def test_dropin_forward_hands_refuses_out_of_range_counts():
    import types

    import torch
    from handnet_pipeline.handnet_pipeline import HandNet
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    img, dep = torch.zeros((1, 3, 64, 64)), torch.zeros((1, 1, 64, 64))
    for k in (0, 17):
        with pytest.raises(ValueError, match="max_hands"):
            net.forward_hands(img, dep, max_hands=k)
    assert net.forward_hands(img, dep, max_hands=2, is_detect=True) is None


def test_hands_record_layout():
    import torch
    from hn_amd import pipeline
    rb = pipeline.record_bytes(1)
    for slots in (1, 2, 37, 64, 512):
        rows = pipeline.hands_record_rows(slots, rb)
        rec = torch.zeros((rows, rb), dtype=torch.uint8)
        score, index = pipeline._hands_tail(rec, slots)
        score.copy_(torch.arange(slots, dtype=torch.float32) + 0.5)
        index.copy_(torch.arange(slots, dtype=torch.int32) - 1)
        # the tail starts behind the range-word row and fits the record
        assert rec[:slots + 1].abs().sum() == 0
        s, i = pipeline.read_hands_tail(rec, slots)
        assert torch.equal(s, torch.arange(slots, dtype=torch.float32) + 0.5)
        assert torch.equal(i, torch.arange(slots, dtype=torch.int32) - 1)
