"""CPU oracle of the Winograd convolution's backward (mvdetr_amd/csrc/conv_winograd_backward.hip): numpy/torch only.

input_grad_flipped      the data gradient as the issue states it: the SAME convolution of grad_y with the weights flipped in
                        both spatial axes and transposed in (C, K).
weight_grad_winograd    the weight gradient in the Winograd domain: dM = A dY A^T per 2x2 tile of grad_y,
                        dU[p][c][k] = sum over the tiles of V[p][tile][c] dM[p][tile][k] with V = B^T d B as the forward
                        forms it (conv_winograd_oracle._input_tiles), dw = G^T dU G.  The tile rule is the forward's:
                        sub-lattices x[..., sy::d, sx::d], grad_y zero-extended to even extents.
dgrad_weights           Ut[16][K][C], the forward transform of the flipped, transposed weights, in fp64 rounded once.
integer_backward_case   inputs on which both kernels are EXACT in float32 in any summation order and any split; the bounds
                        that make it so are asserted from the arrays themselves.
The grids of tests/test_conv_winograd_backward_gpu.py live here so that the CPU suite can check their sanity condition."""
import numpy as np
import torch
import torch.nn.functional as F

import conv_winograd_oracle as fwd
from conv_winograd_oracle import G, _input_tiles, _sublattices

AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def input_grad_flipped(gy, w, d):
    """gy [N, K, H, W], w [K, C, 3, 3] torch tensors -> fp64 [N, C, H, W]."""
    return F.conv2d(gy.double(), w.double().flip(2, 3).transpose(0, 1), None, 1, d, d)


def dgrad_weights(w):
    """Ut[4 xi + nu][k][c] of w [K, C, 3, 3] (numpy): conv_winograd_oracle.transformed_weights of the flipped, transposed
    weights, whose 'input channels' are K and 'output channels' C."""
    w = np.asarray(w, dtype=np.float64)
    return fwd.transformed_weights(np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)))


def _output_tiles(sub):
    """A dY A^T of every 2x2 tile of one undilated image batch [N, K, h, w], zero-extended to even extents: [4 xi][4 nu] arrays
    of shape [N, K, th, tw], in the array's own precision."""
    N, K, h, w = sub.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    pad = np.zeros((N, K, 2 * th, 2 * tw), sub.dtype)
    pad[:, :, :h, :w] = sub
    dY = [[pad[:, :, i::2, j::2] for j in range(2)] for i in range(2)]
    rows = [[sum(AT[i][xi] * dY[i][j] for i in range(2)) for j in range(2)] for xi in range(4)]
    return [[sum(AT[j][nu] * rows[xi][j] for j in range(2)) for nu in range(4)] for xi in range(4)]


def tile_count(N, H, W, d):
    return N * sum(((len(range(sy, H, d)) + 1) // 2) * ((len(range(sx, W, d)) + 1) // 2) for sy in range(d) for sx in range(d))


def weight_grad_winograd(x, gy, d):
    """x [N, C, H, W], gy [N, K, H, W] numpy arrays -> fp64 [K, C, 3, 3] by the Winograd-domain expression."""
    x, gy = np.asarray(x, dtype=np.float32), np.asarray(gy, dtype=np.float64)
    C, K = x.shape[1], gy.shape[1]
    dU = np.zeros((4, 4, C, K))
    for (sy, sx, sub), (_, _, gsub) in zip(_sublattices(x, d), _sublattices(gy, d)):
        V, dM = _input_tiles(sub), _output_tiles(gsub)
        for xi in range(4):
            for nu in range(4):
                dU[xi, nu] += np.einsum("ncyx,nkyx->ck", V[xi][nu].astype(np.float64), dM[xi][nu])
    return np.einsum("xi,xnck,nj->kcij", G, dU, G)


def integer_backward_case(N, C, K, H, W, d, seed=0):
    """(x, gy, w): x int-valued in [-3, 3] channels-last [N, C, H, W], gy int-valued in [-2, 2] channels-last [N, K, H, W],
    w = 4 * randint(-2, 3) [K, C, 3, 3] as integer_case makes it.

    Weight gradient: every V and dM is an integer, so every product and every partial sum of dU over ANY subset of the T tiles
    is an integer of magnitude <= T max|V| max|dM| = B.  A G^T dU G entry is sum G[xi][i] G[nu][j] dU[xi][nu]: a multiple of
    1/4 of magnitude <= 4 B (the columns of |G| sum to at most 2), as is every intermediate of it, so 16 B < 2^24 would do;
    the bound asserted is the wider 36 B < 2^24.  All of it is then exact in float32, in any order and any split.
    Data gradient: the forward's bound on (gy, Ut): integers throughout, 9 K max|V(gy)| max|Ut| < 2^24."""
    g = torch.Generator().manual_seed(7 + 100003 * seed + 7919 * N + 31 * C + 3 * K + 1009 * H + 11 * W + 13 * d)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).float().contiguous(memory_format=torch.channels_last)
    gy = torch.randint(-2, 3, (N, K, H, W), generator=g).float().contiguous(memory_format=torch.channels_last)
    w = (4 * torch.randint(-2, 3, (K, C, 3, 3), generator=g)).float()
    v_max = max(float(np.abs(v).max()) for _, _, sub in _sublattices(x.numpy(), d) for row in _input_tiles(sub) for v in row)
    m_max = max(float(np.abs(m).max()) for _, _, sub in _sublattices(gy.numpy(), d) for row in _output_tiles(sub) for m in row)
    T = tile_count(N, H, W, d)
    assert 36 * T * v_max * m_max < 2 ** 24, (T, v_max, m_max)
    Ut = dgrad_weights(w.numpy())
    assert np.array_equal(Ut, np.round(Ut))
    g_max = max(float(np.abs(v).max()) for _, _, sub in _sublattices(gy.numpy(), d) for row in _input_tiles(sub) for v in row)
    assert 9 * K * g_max * float(np.abs(Ut).max()) < 2 ** 24, (K, g_max)
    return x, gy, w


def reference_fp64(x, gy, w, d):
    """(grad_x, grad_w) of F.conv2d(x, w, stride 1, padding d, dilation d) for grad_y = gy, by torch.nn.grad in fp64."""
    gx = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), 1, d, d)
    gw = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), 1, d, d)
    return gx, gw


def reachable_taps(H, W, d):
    """[3, 3] bool: the taps (i, j) that pair at least one pixel of the image with one of the image: |i - 1| d < H and
    |j - 1| d < W.  The weight gradient of every other tap is zero whatever the data."""
    return torch.tensor([[abs(i - 1) * d < H and abs(j - 1) * d < W for j in range(3)] for i in range(3)])


def check_sanity(gx, gw, H, W, d):
    """A trivially small or all-zero reference must not make an exact comparison empty: the share of non-zero elements of
    grad_x, and of grad_w among the taps that can be non-zero at all (at 1 x 1 eight of the nine taps of EVERY weight gradient
    are zero by geometry).  Returns the two shares; the callers assert 0.90 of each."""
    taps = reachable_taps(H, W, d)
    assert taps[1, 1] and not gw[:, :, ~taps].any()
    return (gx != 0).double().mean().item(), (gw[:, :, taps] != 0).double().mean().item()


def first_mismatch_w(got, want):
    idx = (got.double() != want).nonzero()
    if idx.numel() == 0:
        return "equal"
    k, c, i, j = idx[0].tolist()
    return (f"{idx.shape[0]} of {want.numel()} differ; first at (k {k}, c {c}, tap {i}, {j}): got {got[k, c, i, j].item()!r} want "
            f"{want[k, c, i, j].item()!r}; unit (k block {k // 64}, c block {c // 64}), wave block ({k % 64 // 32}, {c % 64 // 32})")


# ---- the grids of the exact GPU tests: (N, C, K, H, W, d) ------------------------------------------------------------------------
GEOMETRY_GRID = [(N, 64, 64, H, W, d) for N, _, _, H, W, d in fwd.GEOMETRY_GRID]
CHANNEL_GRID = [(2, C, K, 9, 13, d) for d in (1, 2, 4) for C in (64, 128, 192) for K in (64, 128, 192)]
BOUNDARY_GRID = [(N, 64, 64, H, W, d) for N, _, _, H, W, d in fwd.BOUNDARY_GRID]
SPLITS = (1, 2, 3, 7, 1 << 20)               # forced S; the last one is more than there are chunks
