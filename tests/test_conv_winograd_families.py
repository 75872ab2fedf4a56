"""CPU-only checks of the Winograd predicate's pixel floors (mvdetr_amd/ops/conv_winograd.py): the layer1/2 families
(NARROW_FAMILIES) need one unit per CU, 512 / K times the pixels of the first table's families; the first table's floor is
what it was; both setters lower their own.  No kernel is launched: meta tensors stand in for device ones."""
import pytest
import torch
from torch import nn

from mvdetr_amd.ops import conv_winograd as cw


@pytest.fixture
def on_device(monkeypatch):
    monkeypatch.setattr(cw, "_on_device", lambda t: t.device.type == "meta")
    monkeypatch.setattr(cw, "_enabled", True)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)


def _x(C, pixels):
    """1 x C x 1 x pixels"""
    return torch.empty(1, C, 1, pixels, dtype=torch.float32, device="meta").contiguous(memory_format=torch.channels_last)


def _conv(C, K, d=1):
    return nn.Conv2d(C, K, 3, 1, d, d, bias=False, device="meta").requires_grad_(False).eval()


def _every_family():
    return [(C, K, d) for table in (cw.FAMILIES, cw.NARROW_FAMILIES) for (C, K), ds in table.items() for d in ds]


def test_the_tables():
    assert cw.FAMILIES == {(128, 256): (1,), (256, 256): (1, 2), (256, 512): (2,), (512, 512): (1, 4)}
    assert cw.NARROW_FAMILIES == {(64, 64): (1,), (128, 128): (1,)}
    assert cw.MIN_PIXELS == 8192
    assert cw.min_pixels(64, 64, 1) == 65536 and cw.min_pixels(128, 128, 1) == 32768
    assert cw.min_pixels(512, 512, 4) == 8192 and cw.min_pixels(64, 64, 2) is None and cw.min_pixels(64, 128, 1) is None


@pytest.mark.parametrize("C,K,floor", [(64, 64, 65536), (128, 128, 32768)])
def test_new_families_floor(on_device, C, K, floor):
    ok = cw.winograd_conv3x3_available
    with torch.no_grad():
        assert not ok(_x(C, floor - 1), _conv(C, K))                           # one pixel below
        assert ok(_x(C, floor), _conv(C, K))                                   # at it
        assert not ok(_x(C, floor), _conv(C, K, 2))                            # a dilation outside the family


def test_old_families_floor_is_unchanged(on_device):
    ok = cw.winograd_conv3x3_available
    with torch.no_grad():
        for (C, K), ds in cw.FAMILIES.items():
            for d in ds:
                assert not ok(_x(C, 8191), _conv(C, K, d)) and ok(_x(C, 8192), _conv(C, K, d))


def test_everything_is_accepted_at_floor_zero(on_device):
    ok = cw.winograd_conv3x3_available
    with torch.no_grad():
        prev = cw.set_winograd_min_pixels(0)
        narrow = cw.set_winograd_narrow_min_pixels(0)
        try:
            assert prev == cw.MIN_PIXELS and narrow == cw.MIN_PIXELS
            for C, K, d in _every_family():
                assert ok(_x(C, 1), _conv(C, K, d)), (C, K, d)
            # each setter moves its own table only
            assert cw.set_winograd_narrow_min_pixels(narrow) == 0
            assert not ok(_x(64, 65535), _conv(64, 64)) and ok(_x(512, 1), _conv(512, 512))
        finally:
            cw.set_winograd_narrow_min_pixels(narrow)
            cw.set_winograd_min_pixels(prev)
        for C, K, d in _every_family():
            assert not ok(_x(C, 8191), _conv(C, K, d))


def test_a_family_moved_into_the_first_table_has_its_floor(on_device, monkeypatch):
    monkeypatch.setattr(cw, "FAMILIES", {**cw.FAMILIES, (64, 64): (1,)})
    with torch.no_grad():
        assert cw.winograd_conv3x3_available(_x(64, 8192), _conv(64, 64))
        assert not cw.winograd_conv3x3_available(_x(64, 8191), _conv(64, 64))
