"""CPU-only checks of the Winograd convolution's Python face (mvdetr_amd/ops/conv_winograd.py): the predicate's truth
table, the transformed-weights cache, the F(2x2,3x3) matrices, and the oracle of the GPU tests (conv_winograd_oracle.py: the
float32 emulation at every geometry, exact on integer data).  No kernel is launched: the predicate is asked about meta
tensors standing in for device ones, and the cache is exercised with the weight transform's launch replaced by a
counter."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import conv_winograd_oracle as oracle
from mvdetr_amd.ops import conv_winograd as cw


@pytest.fixture
def on_device(monkeypatch):
    """Meta tensors count as device tensors; one family on, cudnn.deterministic off, the switch on."""
    monkeypatch.setattr(cw, "_on_device", lambda t: t.device.type == "meta")
    monkeypatch.setattr(cw, "FAMILIES", {(64, 128): (1, 2)})
    monkeypatch.setattr(cw, "_enabled", True)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)


def _x(C=64, H=64, W=128, N=1, dtype=torch.float32):
    return torch.empty(N, C, H, W, dtype=dtype, device="meta").contiguous(memory_format=torch.channels_last)


def _conv(C=64, K=128, k=3, stride=1, d=1, padding=None, **kw):
    kw.setdefault("bias", False)
    return nn.Conv2d(C, K, k, stride, d if padding is None else padding, d, device="meta", **kw).requires_grad_(False).eval()


def test_predicate_truth_table(on_device):
    ok = cw.winograd_conv3x3_available
    with torch.no_grad():
        assert ok(_x(), _conv()) and ok(_x(), _conv(d=2))
        assert not ok(_x(), _conv(d=4))                                        # a dilation outside the family
        assert not ok(_x(128), _conv(128, 128))                                # a shape outside every family
        assert not ok(_x().contiguous(), _conv())                              # NCHW
        assert not ok(_x(W=256)[..., ::2], _conv())                            # a strided view
        assert not ok(_x(dtype=torch.float64), _conv()) and not ok(_x(dtype=torch.float16), _conv())
        assert not ok(_x(), _conv(stride=2))
        assert not ok(_x(), _conv(bias=True))
        assert not ok(_x(), _conv(groups=2))
        assert not ok(_x(), _conv(k=1, padding=0))
        assert not ok(_x(), _conv(padding=0)) and not ok(_x(), _conv(d=2, padding=1))     # padding != dilation
        assert not ok(_x(), _conv(padding_mode="reflect"))
        assert not ok(_x(), _conv(padding="same"))
        assert not ok(_x(128), _conv())                                        # channel mismatch
        assert not ok(_x(H=64, W=127), _conv())                                # 8,128 pixels: below the floor
        assert ok(_x(H=64, W=128), _conv()) and cw.MIN_PIXELS == 8192          # 8,192: at it
        assert not ok(torch.empty(1, 64, 64, 128).contiguous(memory_format=torch.channels_last), nn.Conv2d(64, 128, 3, 1, 1, bias=False))  # CPU

        class Sub(nn.Conv2d):
            pass
        assert not ok(_x(), Sub(64, 128, 3, 1, 1, bias=False, device="meta").requires_grad_(False))


def test_predicate_switches(on_device):
    ok = cw.winograd_conv3x3_available
    x, conv = _x(), _conv()
    with torch.no_grad():
        assert ok(x, conv)
        prev = cw.set_trunk_winograd(False)
        assert prev is True and not ok(x, conv) and not cw.trunk_winograd_enabled()
        assert cw.set_trunk_winograd(prev) is False and ok(x, conv)
        torch.backends.cudnn.deterministic = True                              # (the fixture restores it)
        assert not ok(x, conv)
        torch.backends.cudnn.deterministic = False
        small = _x(H=8, W=8)
        assert not ok(small, conv)
        prev = cw.set_winograd_min_pixels(0)
        assert prev == cw.MIN_PIXELS and ok(small, conv)
        assert cw.set_winograd_min_pixels(prev) == 0 and not ok(small, conv)


def test_predicate_refuses_what_needs_autograd(on_device):
    ok = cw.winograd_conv3x3_available
    x = _x()
    with torch.enable_grad():
        assert ok(x, _conv())                                                  # nothing requires grad
        assert not ok(x, _conv().requires_grad_(True))                         # the weight does
        assert not ok(_x().requires_grad_(True), _conv())
        assert not ok(x, _conv().requires_grad_(True).train())
    with torch.no_grad():
        assert ok(x, _conv().requires_grad_(True))                             # inference over trainable weights


def _numpy_weights(w):
    G = np.array(cw.G)
    return np.einsum("ij,kcjl,ml->imck", G, w.detach().double().numpy(), G).reshape(16, w.shape[1], w.shape[0]).astype(np.float32)


@pytest.fixture
def host_transform(monkeypatch):
    """_transformed_weights() with the kernel launch replaced by a counter of the builds (the cache logic is host code)."""
    built = []

    class Lib:
        @staticmethod
        def mvdetr_winograd_weights_f32(w_ptr, C, K, U_ptr, stream):
            built.append((w_ptr, C, K))
            return 0
    monkeypatch.setattr(cw._lib, "lib", lambda: Lib)
    monkeypatch.setattr(cw._lib, "current_stream_ptr", lambda device: 0)

    class NoDevice:
        def __init__(self, device):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False
    monkeypatch.setattr(torch.cuda, "device", NoDevice)
    return built


def test_cache_follows_the_weight_tensor(host_transform):
    built = host_transform
    conv = nn.Conv2d(8, 64, 3, 1, 1, bias=False)
    n0 = cw.cached_weight_count()
    U = cw._transformed_weights(conv.weight)
    assert U.shape == (16, 8, 64) and len(built) == 1 and cw.cached_weight_count() == n0 + 1
    assert cw._transformed_weights(conv.weight) is U and len(built) == 1      # unchanged weights: the same U
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight))                       # an in-place edit
    U2 = cw._transformed_weights(conv.weight)
    assert U2 is not U and len(built) == 2 and cw.cached_weight_count() == n0 + 1
    conv.load_state_dict({"weight": torch.randn_like(conv.weight)})
    U3 = cw._transformed_weights(conv.weight)
    assert U3 is not U2 and len(built) == 3
    conv.double().float()                                                      # .to(): new storage behind the same Parameter
    U4 = cw._transformed_weights(conv.weight)
    assert U4 is not U3 and len(built) == 4
    twin = copy.deepcopy(conv)                                                 # a copy has an entry of its own
    Ut = cw._transformed_weights(twin.weight)
    assert Ut is not U4 and len(built) == 5 and cw.cached_weight_count() == n0 + 2
    assert cw._transformed_weights(conv.weight) is U4 and cw._transformed_weights(twin.weight) is Ut and len(built) == 5
    del twin, Ut
    del conv, U, U2, U3, U4                                                    # entries go with their tensors
    assert cw.cached_weight_count() == n0


def test_the_matrices_are_f2x2_3x3():
    """Y = A^T [ (G g G^T) .* (B^T d B) ] A on one 6 x 6 image and one filter equals the direct 3 x 3 correlation with zero
    padding -- with the matrices the module documents and the kernels hard-code (conv_winograd.hip: winograd_weights_f32,
    transform_row, the epilogue)."""
    G, BT, AT = np.array(cw.G), np.array(cw.BT), np.array(cw.AT)
    assert G.shape == (4, 3) and BT.shape == (4, 4) and AT.shape == (2, 4)
    rng = np.random.default_rng(0)
    img, g = rng.standard_normal((6, 6)), rng.standard_normal((3, 3))
    pad = np.zeros((8, 8))
    pad[1:7, 1:7] = img
    want = np.array([[(pad[y:y + 3, x:x + 3] * g).sum() for x in range(6)] for y in range(6)])
    U = G @ g @ G.T
    got = np.zeros((6, 6))
    for ty in range(3):
        for tx in range(3):
            d = pad[2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]
            got[2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = AT @ (U * (BT @ d @ BT.T)) @ AT.T
    assert np.abs(got - want).max() < 1e-13
    # the layout of U the kernel reads: [16 = 4 xi + nu][C][K]
    w = torch.from_numpy(rng.standard_normal((2, 3, 3, 3)).astype(np.float32))
    Uk = _numpy_weights(w)
    assert Uk.shape == (16, 3, 2)
    assert np.allclose(Uk[4 * 1 + 2, 1, 0], (G @ w[0, 1].double().numpy() @ G.T)[1, 2], rtol=1e-7)


def test_float32_f2x2_3x3_is_within_a_few_ulp_of_fp64():
    """The arithmetic the kernel does, emulated in float32 on the CPU at one small trunk-like shape: its deviation from fp64 is
    a handful of output ulps (DESIGN 4.9b has the GPU figures; tests/test_conv_winograd_gpu.py holds the kernel against
    the same emulation)."""
    rng = np.random.default_rng(1)
    C, K, H, W = 64, 8, 6, 6
    x = np.maximum(rng.standard_normal((C, H, W)), 0).astype(np.float32)
    w = (rng.standard_normal((K, C, 3, 3)) * (2.0 / (K * 9)) ** 0.5).astype(np.float32)
    G, BT, AT = np.array(cw.G), np.array(cw.BT, dtype=np.float32), np.array(cw.AT, dtype=np.float32)
    U = np.einsum("ij,kcjl,ml->kcim", G, w.astype(np.float64), G).astype(np.float32)
    pad = np.zeros((C, H + 2, W + 2), np.float32)
    pad[:, 1:-1, 1:-1] = x
    want = np.zeros((K, H, W))
    got = np.zeros((K, H, W), np.float32)
    for y in range(H):
        for xx in range(W):
            want[:, y, xx] = np.einsum("kcij,cij->k", w.astype(np.float64), pad[:, y:y + 3, xx:xx + 3].astype(np.float64))
    for ty in range(H // 2):
        for tx in range(W // 2):
            d = pad[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]
            V = np.einsum("ij,cjl,ml->cim", BT, d, BT).astype(np.float32)
            M = np.zeros((K, 4, 4), np.float32)
            for c in range(C):
                M = (M.astype(np.float64) + U[:, c].astype(np.float64) * V[c].astype(np.float64)).astype(np.float32)   # fma chain
            got[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = np.einsum("ij,kjl,ml->kim", AT, M, AT)
    err = np.abs(got - want).max()
    assert np.abs(want).max() > 1 and err < 16 * np.spacing(np.float32(np.abs(want).max()))


# ---- the oracle of the GPU tests (tests/conv_winograd_oracle.py), validated without a GPU ------------------------------------------

def test_oracle_weights_have_the_kernels_layout():
    w = torch.randn(64, 8, 3, 3, generator=torch.Generator().manual_seed(2))
    assert np.array_equal(oracle.transformed_weights(w.numpy()), _numpy_weights(w))


@pytest.mark.parametrize("N,C,K,H,W,d", [(3, 24, 64, 5, 7, 4), (3, 24, 64, 9, 13, 2), (3, 8, 64, 3, 2, 4), (3, 256, 64, 10, 16, 1),
                                         (3, 8, 64, 2, 2, 1), (3, 24, 64, 6, 4, 1), (2, 72, 64, 1, 9, 2)])
def test_generalised_emulation_is_exact_on_integer_cases(N, C, K, H, W, d):
    """Integer activations in [-3, 3], weights 4 * [-2, 2]: every intermediate of float32 F(2x2,3x3) is an integer below 2^24
    (integer_case asserts the bound), so the emulation equals the fp64 direct convolution bit for bit -- dilated, odd, smaller
    than the dilation."""
    x, w = oracle.integer_case(N, C, K, H, W, d)
    assert x.is_contiguous(memory_format=torch.channels_last) and x.min() == -3 and x.max() == 3
    assert set(w.unique().tolist()) == {-8.0, -4.0, 0.0, 4.0, 8.0}
    want = oracle.direct_fp64(x, w, d)
    got = torch.from_numpy(oracle.emulate_f32(x.numpy(), w.numpy(), d))
    oracle.check_sanity(want, C)
    assert torch.equal(got.double(), want), oracle.first_mismatch(got, want, d)


@pytest.mark.parametrize("H,W,d", [(10, 16, 1), (5, 7, 1), (9, 13, 2), (5, 7, 4), (3, 2, 4), (18, 17, 2)])
def test_generalised_emulation_on_random_data_is_within_a_few_ulp_of_fp64(H, W, d):
    """Kaiming weights, post-ReLU N(0,1) activations as in the trunk: the bar of
    test_float32_f2x2_3x3_is_within_a_few_ulp_of_fp64."""
    g = torch.Generator().manual_seed(17 * H + W + 101 * d)
    C, K = 64, 64
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (K * 9)) ** 0.5
    x = torch.randn(2, C, H, W, generator=g).relu_()
    want = oracle.direct_fp64(x, w, d).numpy()
    got = oracle.emulate_f32(x.numpy(), w.numpy(), d)
    err = np.abs(got - want).max()
    assert np.abs(want).max() > 1 and err < 16 * np.spacing(np.float32(np.abs(want).max()))
    assert err > 0                                                             # (float32 arithmetic, not fp64 in disguise)


def test_every_exact_case_has_a_reference_worth_comparing_with():
    """The sanity condition of tests/test_conv_winograd_exact_gpu.py on its three grids: at least 90 % of the reference outputs
    non-zero, max |want| > 50 from C = 24 on."""
    assert len(oracle.GEOMETRY_GRID) == 108 and len(oracle.CHANNEL_GRID) == 54 and len(oracle.BOUNDARY_GRID) == 9
    for N, C, K, H, W, d in oracle.GEOMETRY_GRID + oracle.CHANNEL_GRID + oracle.BOUNDARY_GRID:
        x, w = oracle.integer_case(N, C, K, H, W, d)
        oracle.check_sanity(oracle.direct_fp64(x, w, d), C)


def test_the_span_guard_of_the_predicate(on_device):
    """(256 + 2 H W) * max(C, K) < 2^30: the last shape below the limit takes the kernel, the first above does not (the C entry's
    own guard is in tests/test_conv_winograd_gpu.py; nothing this large is ever launched)."""
    with torch.no_grad():
        for C, K, H, W, W_over in ((64, 64, 2896, 2896, 2897), (128, 64, 2048, 2047, 2048), (64, 128, 2048, 2047, 2048)):
            assert (256 + 2 * H * W) * max(C, K) < 1 << 30 <= (256 + 2 * H * W_over) * max(C, K)
            assert cw._structure_ok(_x(C, H, W), _conv(C, K))
            assert not cw._structure_ok(_x(C, H, W_over), _conv(C, K))
