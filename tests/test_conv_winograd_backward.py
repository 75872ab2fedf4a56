"""The Winograd convolution's backward without a GPU (mvdetr_amd/ops/conv_winograd.py, csrc/conv_winograd_backward.hip):
the two identities it rests on, restated in numpy and held to torch.nn.grad in fp64 with no tolerance on integer data; the
conditions that make the GPU tests' integer cases exact; the training predicate on meta tensors; the weight gradient's
split without a device; and the C entries' refusals that need no device."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import conv_winograd_backward_oracle as oracle
import conv_winograd_oracle as fwd
from mvdetr_amd.ops import conv_winograd as cw

SIZES = (1, 2, 3, 4, 5, 9)
INVALID, NOT_SUPPORTED = 1, 801


@pytest.mark.parametrize("d", [1, 2, 4])
def test_both_identities_hold_exactly_on_integer_data(d):
    for H in SIZES:
        for W in SIZES:
            x, gy, w = oracle.integer_backward_case(2, 8, 16, H, W, d)
            gx, gw = oracle.reference_fp64(x, gy, w, d)
            assert torch.equal(oracle.input_grad_flipped(gy, w, d), gx), (H, W, d)
            got = torch.from_numpy(oracle.weight_grad_winograd(x.numpy(), gy.numpy(), d))
            assert torch.equal(got, gw), f"{H}x{W} d {d}: " + oracle.first_mismatch_w(got, gw)


def test_dgrad_is_the_forward_emulation_on_the_transformed_flipped_weights():
    """Ut fed to the forward's float32 emulation (C and K exchanged) is the data gradient, bit for bit on integer data."""
    for H, W, d in ((5, 9, 1), (9, 4, 2), (3, 9, 4)):
        x, gy, w = oracle.integer_backward_case(2, 8, 16, H, W, d)
        flipped = np.ascontiguousarray(w.numpy()[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
        assert np.array_equal(oracle.dgrad_weights(w.numpy()), fwd.transformed_weights(flipped))
        got = torch.from_numpy(fwd.emulate_f32(gy.numpy(), flipped, d))
        assert torch.equal(got.double(), oracle.reference_fp64(x, gy, w, d)[0])


@pytest.mark.parametrize("grid", ["GEOMETRY_GRID", "CHANNEL_GRID", "BOUNDARY_GRID"])
def test_the_gpu_grids_are_exact_cases_with_references_that_are_not_empty(grid):
    """integer_backward_case asserts its bounds for every case of the GPU grids, and 90 % of every reference is non-zero
    where it can be (the weight gradient of a tap that no pixel pair reaches is zero by geometry)."""
    cases = getattr(oracle, grid)
    if grid == "CHANNEL_GRID":
        cases = [c for c in cases if c[5] == 2 and max(c[1], c[2]) <= 128]     # the wide ones take seconds each in fp64
    for N, C, K, H, W, d in cases:
        x, gy, w = oracle.integer_backward_case(N, C, K, H, W, d)
        sx, sw = oracle.check_sanity(*oracle.reference_fp64(x, gy, w, d), H, W, d)
        assert sx >= 0.90 and sw >= 0.90, (N, C, K, H, W, d, sx, sw)


# ---- the predicate, on meta tensors -------------------------------------------------------------------------------------------------
@pytest.fixture()
def on_device(monkeypatch):
    monkeypatch.setattr(cw, "_on_device", lambda t: t.device.type == "meta")
    monkeypatch.setattr(cw, "TRAIN_FAMILIES", {(64, 128): {1: ("dgrad", "wgrad"), 2: ("wgrad",)}})
    monkeypatch.setattr(cw, "FAMILIES", {(64, 128): (1, 2)})
    monkeypatch.setattr(cw, "_enabled", True)
    monkeypatch.setattr(cw, "_train_enabled", True)
    monkeypatch.setattr(cw, "_train_min_pixels", None)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)


def _x(C=64, H=64, W=128, N=1, dtype=torch.float32, grad=False):
    return torch.empty(N, C, H, W, dtype=dtype, device="meta").contiguous(memory_format=torch.channels_last).requires_grad_(grad)


def _conv(C=64, K=128, d=1, grad=True, **kw):
    kw.setdefault("bias", False)
    return nn.Conv2d(C, K, 3, 1, d, d, device="meta", **kw).requires_grad_(grad)


def test_predicate_is_true_under_autograd_for_a_family_that_is_on(on_device, monkeypatch):
    ok = cw.winograd_conv3x3_train_available
    assert ok(_x(), _conv()) and ok(_x(), _conv(d=2))
    assert ok(_x(grad=True), _conv(grad=False))                                 # only the input needs a gradient
    assert not cw.winograd_conv3x3_available(_x(), _conv())                     # the inference entry stays out of autograd
    assert not ok(_x(), _conv(grad=False))                                      # nothing needs autograd: the inference route's
    with torch.no_grad():
        assert not ok(_x(), _conv()) and cw.winograd_conv3x3_available(_x(), _conv())
    assert not ok(_x(), _conv(d=4))                                             # not in the table
    assert not ok(_x(C=128), _conv(C=128, K=128))
    monkeypatch.setattr(cw, "TRAIN_FAMILIES", {(128, 128): {1: ("wgrad",)}, (64, 128): {1: ()}})
    # the table patched ((128, 128, 1) has the narrow families' floor: 32,768 pixels); a family with no piece on
    assert ok(_x(C=128, H=256), _conv(C=128, K=128)) and not ok(_x(C=128), _conv(C=128, K=128)) and not ok(_x(), _conv())


def test_predicate_is_false_where_the_issue_says_so(on_device, monkeypatch):
    ok = cw.winograd_conv3x3_train_available
    assert ok(_x(), _conv())
    monkeypatch.setattr(cw, "_train_enabled", False)
    assert not ok(_x(), _conv()) and not cw.trunk_winograd_training_enabled()
    monkeypatch.setattr(cw, "_train_enabled", True)
    prev = cw.set_trunk_winograd(False)                                         # the inference switch takes training with it
    try:
        assert not ok(_x(), _conv()) and not cw.trunk_winograd_training_enabled()
    finally:
        cw.set_trunk_winograd(prev)
    assert cw.set_trunk_winograd_training(False) is True and not ok(_x(), _conv())
    assert cw.set_trunk_winograd_training(True) is False and ok(_x(), _conv())
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    assert not ok(_x(), _conv())
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    # C or K not a multiple of 64, with the table saying yes
    monkeypatch.setattr(cw, "TRAIN_FAMILIES", {(72, 128): {1: cw.PIECES}, (64, 128): {1: cw.PIECES}, (64, 96): {1: cw.PIECES}})
    assert not ok(_x(C=72), _conv(C=72)) and not ok(_x(), _conv(K=96))
    for dtype in (torch.float16, torch.bfloat16):                               # 16-bit never takes the route
        assert not ok(_x(dtype=dtype), _conv(dtype=dtype)) and not ok(_x(dtype=dtype), _conv())
    assert not ok(_x(), _conv(bias=True)) and not ok(_x().contiguous(), _conv())
    # the floor: the inference floor of the shape by default, a setting of its own otherwise
    assert cw.train_min_pixels(64, 128, 1) == cw.min_pixels(64, 128, 1) == 8192
    assert ok(_x(H=64, W=128), _conv()) and not ok(_x(H=64, W=127), _conv())
    assert cw.set_winograd_train_min_pixels(100) is None
    try:
        assert ok(_x(H=10, W=10), _conv()) and not ok(_x(H=9, W=11), _conv())
    finally:
        assert cw.set_winograd_train_min_pixels(None) == 100
    assert cw.train_min_pixels(64, 64, 2) == 8192 * 8                           # in neither inference table: MIN_PIXELS 512 / K


def test_train_entry_raises_instead_of_falling_back(on_device):
    with pytest.raises(RuntimeError, match="do not take the kernel"):
        cw.winograd_conv3x3_train(_x(), _conv(d=4))                             # not in the table
    with pytest.raises(RuntimeError, match="do not take the kernel"):
        cw.winograd_conv3x3_train(_x(C=72), _conv(C=72), force=True)            # force does not make the kernel take C = 72


def test_the_environment_variable_starts_with_training_off():
    import os
    import subprocess
    import sys
    code = ("from mvdetr_amd.ops import conv_winograd as cw; "
            "print(int(cw.trunk_winograd_training_enabled()), int(cw.trunk_winograd_enabled()))")
    env = dict(os.environ, MVDETR_TRUNK_WINOGRAD_TRAIN="0")
    env.pop("MVDETR_TRUNK_WINOGRAD", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["0", "1"]


# ---- the split, without a device ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def settings():
    prev = cw.set_winograd_wgrad_splits(0), cw.set_winograd_max_workgroups(0)
    yield
    cw.set_winograd_wgrad_splits(prev[0])
    cw.set_winograd_max_workgroups(prev[1])


def _check_partition(p, tiles, C, K):
    assert p["units"] == (C // 64) * (K // 64) and p["chunks"] == -(-tiles // 8)
    S, per, last = p["S"], p["per_split"], p["last_split"]
    assert 1 <= S <= p["chunks"] and per >= 1 and 1 <= last <= per
    # split s runs the chunks [s per, min((s + 1) per, chunks)): contiguous, in order, none empty, all of them
    ranges = [range(s * per, min((s + 1) * per, p["chunks"])) for s in range(S)]
    assert all(len(r) for r in ranges) and len(ranges[-1]) == last
    assert [c for r in ranges for c in r] == list(range(p["chunks"]))


def test_wgrad_plan_partitions_the_chunks(settings):
    import random
    rng = random.Random(20261)
    for _ in range(300):
        N, H, W = rng.randint(1, 9), rng.randint(1, 40), rng.randint(1, 40)
        C, K, d = 64 * rng.randint(1, 4), 64 * rng.randint(1, 4), rng.choice((1, 2, 4))
        cus, forced, cap = rng.randint(1, 300), rng.choice((0, 0, 1, 2, 3, 7, 1 << 20)), rng.choice((0, 0, 1, 3))
        cw.set_winograd_wgrad_splits(forced)
        cw.set_winograd_max_workgroups(cap)
        p = cw.wgrad_plan(N, H, W, C, K, d, cus)
        tiles = oracle.tile_count(N, H, W, d)
        _check_partition(p, tiles, C, K)
        want = forced if forced else max(1, (min(cus, cap) if cap else cus) // p["units"])
        want = min(want, p["chunks"])
        assert p["per_split"] == -(-p["chunks"] // want) and p["S"] == -(-p["chunks"] // p["per_split"]), (p, want)
        assert p == cw.wgrad_plan(N, H, W, C, K, d, cus)                        # a function of the arguments alone


def test_wgrad_plan_on_the_workloads_shapes(settings):
    for C, K, d, units in ((64, 64, 1, 1), (128, 128, 1, 4), (256, 256, 2, 16), (256, 512, 2, 32), (512, 512, 4, 64)):
        N, H, W = (7, 180, 320) if C == 64 else (7, 90, 160)
        p = cw.wgrad_plan(N, H, W, C, K, d, 256)
        assert p["units"] == units and p["S"] * units <= 256 and p["S"] * units > 128, p
    cw.set_winograd_wgrad_splits(1 << 20)                                       # more than there are chunks: clamped
    p = cw.wgrad_plan(1, 8, 8, 64, 64, 1, 256)
    assert (p["chunks"], p["S"], p["per_split"], p["last_split"]) == (2, 2, 1, 1)
    assert cw.set_winograd_wgrad_splits(0) == 1 << 20 and cw.set_winograd_wgrad_splits(-5) == 0 and cw.set_winograd_wgrad_splits(0) == 0


# ---- the C entries' refusals that need no device ------------------------------------------------------------------------------------
def test_the_c_entries_refuse_without_a_device(settings):
    from mvdetr_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    x, gy, gw, ws = base, base + 1024, base + 2048, base + 4096               # never dereferenced: every call below is refused
    wgrad = lib.mvdetr_conv3x3_winograd_wgrad_f32
    args = (1, 2, 2, 64, 64, 1)
    big = 1 << 30
    assert wgrad(None, gy, gw, *args, ws, big, None) == INVALID
    assert wgrad(x, None, gw, *args, ws, big, None) == INVALID
    assert wgrad(x, gy, None, *args, ws, big, None) == INVALID
    assert wgrad(x, gy, x, *args, ws, big, None) == INVALID                     # gw is x
    assert wgrad(x, gy, gy, *args, ws, big, None) == INVALID
    assert wgrad(x, gy, x + 512, *args, base + (1 << 20), 64, None) == INVALID  # gw inside x's bytes
    assert wgrad(x, gy, gw, *args, gw, big, None) == INVALID                    # the workspace over gw
    assert wgrad(x, gy, gw, 1, 0, 2, 64, 64, 1, ws, big, None) == INVALID
    assert wgrad(x, gy, gw, -1, 2, 2, 64, 64, 1, ws, big, None) == INVALID
    far = base + (1 << 40)                                                      # apart from everything
    assert wgrad(x, gy, far, 1, 2, 2, 72, 64, 1, far + (1 << 20), 64, None) == NOT_SUPPORTED       # C = 72
    assert wgrad(x, gy, far, 1, 2, 2, 64, 96, 1, far + (1 << 20), 64, None) == NOT_SUPPORTED
    assert wgrad(x, gy, far, 1, 2, 2, 64, 64, 3, far + (1 << 20), 64, None) == NOT_SUPPORTED       # dilation
    assert wgrad(x + 4, gy, far, *args, far + (1 << 20), big, None) == NOT_SUPPORTED               # misaligned
    assert wgrad(x, gy + 8, far, *args, far + (1 << 20), big, None) == NOT_SUPPORTED
    assert wgrad(x, gy, far + 4, *args, far + (1 << 20), big, None) == NOT_SUPPORTED
    assert wgrad(x, gy, far, *args, far + (1 << 20) + 4, big, None) == NOT_SUPPORTED
    assert wgrad(x, gy, far, 1, 40000, 40000, 64, 64, 1, far + (1 << 20), big, None) == NOT_SUPPORTED   # 32-bit offsets
    need = lib.mvdetr_winograd_wgrad_workspace_bytes(*args, 256)
    assert need == 64 * 64 * 36                                                 # one chunk: one split
    assert wgrad(x, gy, far, *args, far + (1 << 20), need - 4, None) == NOT_SUPPORTED              # a short workspace
    assert wgrad(x, gy, far, *args, None, 0, None) == NOT_SUPPORTED
    assert lib.mvdetr_winograd_wgrad_workspace_bytes(1, 2, 2, 72, 64, 1, 256) == -1

    dgrad = lib.mvdetr_winograd_weights_dgrad_f32
    assert dgrad(None, 64, 64, gw, None) == INVALID and dgrad(x, 64, 64, None, None) == INVALID
    assert dgrad(x, 0, 64, gw, None) == INVALID
    assert dgrad(x, 72, 64, gw, None) == NOT_SUPPORTED and dgrad(x, 64, 12, gw, None) == NOT_SUPPORTED
    assert dgrad(x, 64, 64, gw + 4, None) == NOT_SUPPORTED

    out = (ctypes.c_int64 * 5)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    plan = lib.mvdetr_winograd_wgrad_plan
    assert plan(1, 8, 8, 64, 64, 1, 4, ptr) == 0
    assert plan(1, 8, 8, 72, 64, 1, 4, ptr) == NOT_SUPPORTED and plan(1, 8, 8, 64, 32, 1, 4, ptr) == NOT_SUPPORTED
    assert plan(1, 8, 8, 64, 64, 3, 4, ptr) == NOT_SUPPORTED
    assert plan(1, 8, 8, 64, 64, 1, 0, ptr) == INVALID and plan(1, 8, 8, 64, 64, 1, 4, None) == INVALID


# ---- the caches, with the launches replaced by counters (host code) ----------------------------------------------------------------
def test_both_caches_follow_the_weight_tensor(monkeypatch):
    built = []

    class Lib:
        @staticmethod
        def mvdetr_winograd_weights_f32(w_ptr, C, K, U_ptr, stream):
            built.append("U")
            return 0

        @staticmethod
        def mvdetr_winograd_weights_dgrad_f32(w_ptr, C, K, U_ptr, stream):
            built.append("Ut")
            return 0

    class NoDevice:
        def __init__(self, device):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(cw._lib, "lib", lambda: Lib)
    monkeypatch.setattr(cw._lib, "current_stream_ptr", lambda device: 0)
    monkeypatch.setattr(torch.cuda, "device", NoDevice)
    conv = nn.Conv2d(64, 128, 3, 1, 1, bias=False)
    n0, n1 = cw.cached_weight_count(), cw.cached_dgrad_weight_count()
    U, Ut = cw._transformed_weights(conv.weight), cw._transformed_weights_dgrad(conv.weight)
    assert U.shape == (16, 64, 128) and Ut.shape == (16, 128, 64) and built == ["U", "Ut"]
    assert cw._transformed_weights(conv.weight) is U and cw._transformed_weights_dgrad(conv.weight) is Ut and len(built) == 2
    opt = torch.optim.SGD(conv.parameters(), lr=0.1)
    conv.weight.grad = torch.ones_like(conv.weight)
    opt.step()                                                                  # an in-place update: both are stale
    assert cw._transformed_weights(conv.weight) is not U and cw._transformed_weights_dgrad(conv.weight) is not Ut
    assert built == ["U", "Ut", "U", "Ut"]
    assert (cw.cached_weight_count(), cw.cached_dgrad_weight_count()) == (n0 + 1, n1 + 1)
    del conv, opt
    import gc
    gc.collect()
    assert (cw.cached_weight_count(), cw.cached_dgrad_weight_count()) == (n0, n1)   # the entries go with the tensor
