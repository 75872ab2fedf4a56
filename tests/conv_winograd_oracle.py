"""CPU oracle of the fp32 Winograd F(2x2,3x3) convolution (mvdetr_amd/csrc/conv_winograd.hip): numpy/torch only.

emulate_f32     the algorithm in float32 in the kernel's own terms and order of operations, at any geometry: dilation d is
                d x d undilated problems on the sub-lattices x[..., sy::d, sx::d]; an odd extent is zero-extended to even and
                the result cropped (in the kernel pixels outside the image read as zero and are never stored); U = G g G^T
                in fp64 rounded once; B^T d B rows first; one fused multiply-add per input channel, channels in order;
                A^T M A rows first.
integer_case    inputs on which F(2x2,3x3) in float32 is EXACT: integer activations in [-3, 3], weights that are integer
                multiples of 4 in [-8, 8].  G g G^T (two factors of 1/2) stays integral, and every intermediate -- B^T d B,
                each product, each running sum over the channels, A^T M A -- is an integer below 2^24, so the float32 kernel
                must equal the fp64 direct convolution bit for bit at any geometry.  The helper asserts the bound that makes
                this a property of the inputs.
direct_fp64     F.conv2d in fp64 on the CPU.
The grids of tests/test_conv_winograd_exact_gpu.py live here so that the CPU suite can check their sanity condition."""
import numpy as np
import torch
import torch.nn.functional as F

G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])


def transformed_weights(w):
    """U[4 xi + nu][c][k] = (G g G^T)[xi][nu] of w [K, C, 3, 3], in fp64, rounded once: the layout the kernel reads."""
    w = np.asarray(w, dtype=np.float64)
    return np.einsum("ij,kcjl,ml->imck", G, w, G).reshape(16, w.shape[1], w.shape[0]).astype(np.float32)


def _input_tiles(sub):
    """B^T d B of every 4x4 input tile of one undilated float32 image batch [N, C, h, w] (zero padding 1, odd extents
    zero-extended to even), rows first: [4 xi][4 nu] arrays of shape [N, C, th, tw]."""
    N, C, h, w = sub.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    pad = np.zeros((N, C, 2 * th + 2, 2 * tw + 2), np.float32)
    pad[:, :, 1:1 + h, 1:1 + w] = sub
    d = [[pad[:, :, i:i + 2 * th:2, j:j + 2 * tw:2] for j in range(4)] for i in range(4)]
    V = []
    for xi in range(4):
        if xi == 0:
            t = [d[0][j] - d[2][j] for j in range(4)]
        elif xi == 1:
            t = [d[1][j] + d[2][j] for j in range(4)]
        elif xi == 2:
            t = [d[2][j] - d[1][j] for j in range(4)]
        else:
            t = [d[1][j] - d[3][j] for j in range(4)]
        V.append([t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]])
    return V


def _sublattices(x, d):
    for sy in range(d):
        for sx in range(d):
            sub = x[:, :, sy::d, sx::d]
            if sub.size:                                                       # H or W smaller than d: nothing there
                yield sy, sx, sub


def _emulate_undilated(sub, U):
    N, C, h, w = sub.shape
    K = U.shape[2]
    th, tw = (h + 1) // 2, (w + 1) // 2
    V = _input_tiles(sub)
    V = np.stack([np.stack(row, -1) for row in V], -2).astype(np.float64)      # [N, C, th, tw, xi, nu]
    U64 = U.reshape(4, 4, C, K).transpose(2, 3, 0, 1).astype(np.float64)       # [C, K, xi, nu]
    M = np.zeros((N, K, th, tw, 4, 4), np.float32)
    for c in range(C):            # the product of two floats is exact in fp64, so this is fmaf up to a rare double rounding
        M = (M.astype(np.float64) + V[:, c, None] * U64[c][None, :, None, None]).astype(np.float32)
    s0 = M[..., 0, :] + M[..., 1, :] + M[..., 2, :]
    s1 = M[..., 1, :] - M[..., 2, :] - M[..., 3, :]
    y = np.zeros((N, K, 2 * th, 2 * tw), np.float32)
    y[:, :, 0::2, 0::2], y[:, :, 0::2, 1::2] = s0[..., 0] + s0[..., 1] + s0[..., 2], s0[..., 1] - s0[..., 2] - s0[..., 3]
    y[:, :, 1::2, 0::2], y[:, :, 1::2, 1::2] = s1[..., 0] + s1[..., 1] + s1[..., 2], s1[..., 1] - s1[..., 2] - s1[..., 3]
    return y[:, :, :h, :w]


def emulate_f32(x, w, d=1):
    """F(2x2,3x3) in float32 on the host: x [N, C, H, W] and w [K, C, 3, 3] float32 numpy arrays, stride 1, padding =
    dilation = d.  Returns y [N, K, H, W] float32."""
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    N, C, H, W = x.shape
    U = transformed_weights(w)
    y = np.zeros((N, w.shape[0], H, W), np.float32)
    for sy, sx, sub in _sublattices(x, d):
        y[:, :, sy::d, sx::d] = _emulate_undilated(sub, U)
    return y


def integer_case(N, C, K, H, W, d, seed=0):
    """(x, w) on which float32 F(2x2,3x3) is exact: x int-valued float32 in [-3, 3] (both signs), channels-last
    [N, C, H, W]; w = 4 * randint(-2, 3) float32 [K, C, 3, 3]."""
    g = torch.Generator().manual_seed(100003 * seed + 7919 * N + 31 * C + 3 * K + 1009 * H + 11 * W + 13 * d)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).float().contiguous(memory_format=torch.channels_last)
    w = (4 * torch.randint(-2, 3, (K, C, 3, 3), generator=g)).float()
    # the a-priori bound, from the arrays themselves: an output is a signed sum of nine Winograd-domain sums over C
    # products |V| |U|, and everything on the way is an integer
    U = transformed_weights(w.numpy())
    assert np.array_equal(U, np.round(U))
    v_max = max(float(np.abs(v).max()) for _, _, sub in _sublattices(x.numpy(), d) for row in _input_tiles(sub) for v in row)
    assert 9 * C * v_max * float(np.abs(U).max()) < 2 ** 24, (C, v_max, float(np.abs(U).max()))
    return x, w


def direct_fp64(x, w, d):
    return F.conv2d(x.double(), w.double(), None, 1, d, d)


def check_sanity(want, C):
    """A trivially small or all-zero reference must not make an exact comparison empty."""
    share = (want != 0).double().mean().item()
    assert share >= 0.90, share
    if C >= 24:
        assert want.abs().max().item() > 50, want.abs().max().item()
    return share


def first_mismatch(got, want, d):
    """Where got [N, K, H, W] first differs from want, in the kernel's coordinates."""
    idx = (got.double() != want).nonzero()
    if idx.numel() == 0:
        return "equal"
    n, k, y, x = idx[0].tolist()
    return (f"{idx.shape[0]} of {want.numel()} differ; first at (n {n}, k {k}, y {y}, x {x}): got {got[n, k, y, x].item()!r} want "
            f"{want[n, k, y, x].item()!r}; sub-lattice ({y % d}, {x % d}), tile (row {y // d // 2}, column {x // d // 2}), "
            f"position in tile ({y // d % 2}, {x // d % 2})")


# ---- the grids of the exact GPU tests: (N, C, K, H, W, d) ------------------------------------------------------------------------
SIZES = (1, 2, 3, 4, 5, 9)
GEOMETRY_GRID = [(3, 24, 64, H, W, d) for d in (1, 2, 4) for H in SIZES for W in SIZES]
CHANNEL_GRID = [(2, C, K, 9, 13, d) for d in (1, 2, 4) for C in (8, 16, 24, 40, 72, 256) for K in (64, 128, 192)]
BOUNDARY_GRID = [
    (70, 8, 64, 1, 1, 1),         # one workgroup's 64 tiles span 64 images; the next one starts at image 64
    (4, 8, 64, 8, 8, 1),          # exactly 64 tiles
    (5, 8, 64, 2, 26, 1),         # 65 tiles
    (1, 8, 64, 16, 16, 1),
    (17, 8, 64, 1, 1, 4),         # 272 tiles, 17 of them real
    (3, 8, 64, 10, 9, 4),         # a tile row wholly outside the image on the short sub-lattices
    (2, 8, 64, 18, 17, 1), (2, 8, 64, 18, 17, 2), (2, 8, 64, 18, 17, 4),
]
