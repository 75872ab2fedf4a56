"""ops.ingest_frames on the library's host path against the fp64 oracle (tests/ingest_oracle.py), the C-ABI symbols, and
mvdetr_amd/augment.py against the reference's own random_affine (golden).  Runs without a GPU.

Bar per element (ingest_oracle.bar): 32 u 255 a_c + 2 u |ref|, u = 2^-24, no element excluded.  Where the result must be one
normalised pixel exactly (equal sizes, a constant image, an integer translation) the bar is 2 u 255 a_c: the roundings of a_c and
of b_c (|b_c| < 255 a_c since mean < 1) and the one FMA are half an ulp each of a number no larger than 255 a_c."""
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import ingest_cases as cases
import ingest_oracle as oracle
from conftest import load_golden
from mvdetr_amd import _lib, augment
from mvdetr_amd.ops import ingest_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = oracle.U
A = [1.0 / (255.0 * s) for s in oracle.STD]
DTYPES = [torch.float32, torch.float64]


def exact_pixels(fr):
    """(p / 255 - mean) / std in fp64, [K, 3, H, W]"""
    x = fr.permute(0, 3, 1, 2).double() / 255.0
    return (x - torch.tensor(oracle.MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(oracle.STD, dtype=torch.float64).view(1, 3, 1, 1)


def exact_bar():
    return 2 * U * 255 * torch.tensor(A, dtype=torch.float64).view(1, 3, 1, 1)


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("src,dst", cases.IDENTITY_SHAPES)
def test_identity_matches_oracle(src, dst, K, dtype, channels_last):
    fr = cases.frames(K, *src)
    out = ingest_frames(fr, None, dst, dtype=dtype, channels_last=channels_last)
    assert out.shape == (K, 3) + dst and out.dtype == dtype
    assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    w = oracle.worst(out, cases.identity_ref(K, src, dst), torch.float32)
    print(f"identity {src}->{dst} K={K} {dtype} err/bar {w:.3f}")
    assert w <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_five_dimensional_form(dtype):
    src, dst = cases.IDENTITY_SHAPES[1]
    fr = cases.frames(3, *src)
    M = cases.translation_matrix(2, -1)[None].repeat(3, 1, 1)
    for m4, m5 in ((None, None), (M, M.view(1, 3, 3, 3))):
        flat = ingest_frames(fr, m4, dst, dtype=dtype)
        five = ingest_frames(fr.view(1, 3, *src, 3), m5, dst, dtype=dtype)
        assert five.shape == (1, 3, 3) + dst and torch.equal(five.view(3, 3, *dst), flat)
        assert five.view(3, 3, *dst).is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_size_is_the_normalised_pixels(dtype):
    fr = cases.frames(3, 8, 8)
    out = ingest_frames(fr, None, (8, 8), dtype=dtype)
    assert bool(((out.double() - exact_pixels(fr)).abs() <= exact_bar()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_image(dtype):
    for p in (0, 37, 255):
        fr = torch.full((2, 20, 31, 3), p, dtype=torch.uint8)
        out = ingest_frames(fr, None, (33, 47), dtype=dtype)
        want = torch.tensor([a * p - m / s for a, m, s in zip(A, oracle.MEAN, oracle.STD)], dtype=torch.float64).view(1, 3, 1, 1)
        assert bool(((out.double() - want).abs() <= exact_bar()).all())


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cropped_view_is_read_in_place(dtype, with_M):
    fr = cases.frames(3, 37, 53)
    view = fr[:, 2:-3, 5:-7]
    assert not view.is_contiguous()
    M = cases.GENERAL_WARPS["scale0.8_hflip"][None].repeat(3, 1, 1) if with_M else None
    a = ingest_frames(view, M, (24, 35), dtype=dtype)
    b = ingest_frames(view.contiguous(), M, (24, 35), dtype=dtype)
    assert torch.equal(a, b)
    assert oracle.worst(a, oracle.ingest_oracle(view, M, (24, 35)), torch.float32) <= 1.0
    # a layout the kernels do not read in place (channels first in memory) is copied, not misread
    planar = fr.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert torch.equal(ingest_frames(planar, None, (24, 35), dtype=dtype), ingest_frames(fr, None, (24, 35), dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_translation_is_exact(dtype):
    Hs, Ws, tx, ty = 12, 20, 3, -2
    fr = cases.frames(2, Hs, Ws)
    M = cases.translation_matrix(tx, ty)[None].repeat(2, 1, 1)
    out = ingest_frames(fr, M, (Hs, Ws), dtype=dtype).double()
    grey = torch.full((2, Hs, Ws, 3), 128, dtype=torch.uint8)
    grey[:, : Hs + ty, tx:] = fr[:, -ty:, : Ws - tx]                         # destination (x, y) <- source (x - tx, y - ty)
    assert bool(((out - exact_pixels(grey)).abs() <= exact_bar()).all())
    assert oracle.worst(out, oracle.ingest_oracle(fr, M, (Hs, Ws)), torch.float32) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_hflip_keeps_its_off_by_one(dtype):
    """[[-1, 0, Ws], [0, 1, 0], [0, 0, 1]]: destination column x shows source column Ws - x, so column 0 is the border colour and
    source column 0 is lost -- the reference's own matrix (image_utils.py:19-23), kept."""
    Hs, Ws = 12, 20
    fr = cases.frames(2, Hs, Ws)
    M = cases.hflip_matrix(Ws)[None].repeat(2, 1, 1)
    out = ingest_frames(fr, M, (Hs, Ws), dtype=dtype).double()
    grey = torch.full((2, Hs, Ws, 3), 128, dtype=torch.uint8)
    grey[:, :, 1:] = fr.flip(2)[:, :, : Ws - 1]
    assert bool(((out - exact_pixels(grey)).abs() <= exact_bar()).all())
    assert oracle.worst(out, oracle.ingest_oracle(fr, M, (Hs, Ws)), torch.float32) <= 1.0


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases.GENERAL_WARPS))
def test_general_warps_match_oracle(name, dtype, channels_last):
    share = cases.border_fraction(name)
    assert 0.05 <= share <= 0.60, f"{name}: {share:.3f} of the pixels are pure border -- both regimes must be present"
    src, dst = cases.WARP_SHAPE
    M = cases.GENERAL_WARPS[name][None].repeat(2, 1, 1)
    out = ingest_frames(cases.frames(2, *src), M, dst, dtype=dtype, channels_last=channels_last)
    w = oracle.worst(out, cases.warp_ref(name), torch.float32)
    print(f"warp {name} {dtype} border share {share:.3f} err/bar {w:.3f}")
    assert w <= 1.0


def test_float32_matrices_and_identity_matrix():
    src, dst = cases.WARP_SHAPE
    fr = cases.frames(2, *src)
    eye = torch.eye(3)[None].repeat(2, 1, 1)                                   # float32, as a dataloader hands it over
    assert oracle.worst(ingest_frames(fr, eye, dst), cases.identity_ref(2, src, dst)) <= 1.0
    bad = torch.zeros(2, 3, 3)                                                 # singular: every pixel is the border colour
    out = ingest_frames(fr, bad, dst).double()
    want = torch.tensor([a * 128 - m / s for a, m, s in zip(A, oracle.MEAN, oracle.STD)], dtype=torch.float64).view(1, 3, 1, 1)
    assert bool(((out - want).abs() <= exact_bar()).all())


def test_teeth_a_wrong_contract_fails_the_bar():
    """Each wrong reading of the contract, evaluated by the oracle itself, is at least 10 bars away from the right one on some
    case; and torch's own float32 composition (positions formed in float32) fails the bar on the ragged downscale."""
    src, dst = cases.IDENTITY_SHAPES[0]
    ref = cases.identity_ref(3, src, dst)
    fr = cases.frames(3, *src)
    assert oracle.worst(oracle.ingest_oracle(fr, None, dst, align_corners=True), ref, torch.float32) >= 10
    assert oracle.worst(oracle.ingest_oracle(fr, None, dst, antialias=True), ref, torch.float32) >= 10
    name = "scale0.8_hflip"
    M = cases.GENERAL_WARPS[name][None].repeat(2, 1, 1)
    fw = cases.frames(2, *cases.WARP_SHAPE[0])
    assert oracle.worst(oracle.ingest_oracle(fw, M, cases.WARP_SHAPE[1], border=0), cases.warp_ref(name), torch.float32) >= 10
    f2 = cases.frames(2, 12, 20)
    right = oracle.ingest_oracle(f2, cases.hflip_matrix(20)[None].repeat(2, 1, 1), (12, 20))
    wrong = oracle.ingest_oracle(f2, cases.hflip_matrix(20, plus_width=False)[None].repeat(2, 1, 1), (12, 20))
    assert oracle.worst(wrong, right, torch.float32) >= 10
    src, dst = cases.IDENTITY_SHAPES[1]
    w = oracle.worst(oracle.torch_fp32_composition(cases.frames(3, *src), dst), cases.identity_ref(3, src, dst))
    print(f"torch float32 composition on {src}->{dst}: err/bar {w:.3f}")
    assert w > 1.0


def test_symbols_are_declared_bound_and_exported():
    names = ["mvdetr_ingest_frames_f32", "mvdetr_ingest_frames_f16", "mvdetr_ingest_frames_bf16", "mvdetr_ingest_last_kernel",
             "mvdetr_ingest_frames_host_f32", "mvdetr_ingest_frames_host_f64"]
    hdr = open(os.path.join(ROOT, "include", "mvdetr_ops.h")).read()
    declared = set(re.findall(r"\b(mvdetr_[a-z0-9_]+)\s*\(", hdr))
    _lib.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (mvdetr_[a-z0-9_]+)", nm))
    for n in names:
        assert n in declared and n in _lib.SIGNATURES and n in exported, n
    assert re.search(r"#define MVDETR_OPS_ABI_VERSION 18\b", hdr)
    assert _lib.ABI_VERSION == 18 and _lib.lib().mvdetr_ops_abi_version() == 18
    import mvdetr_amd.ops as ops
    assert ops.ingest_frames is ingest_frames


def test_augment_matches_the_reference():
    """20 seeded draws of the reference's random_affine (tests/golden/make_golden_affine.py): the matrix, the surviving boxes
    (clipped ones among them) and their pids; rejected boxes and an empty set included."""
    g = load_golden("affine_boxes.npz")
    n_in = n_out = clipped = empty = 0
    for i in range(int(g["draws"])):
        k, seed, hw = g[f"{i}_kw"], int(g[f"{i}_seed"]), tuple(int(v) for v in g[f"{i}_hw"])
        np.random.seed(seed)
        random.seed(seed)
        boxes, pids, M = augment.random_affine(hw, g[f"{i}_boxes"], g[f"{i}_pids"], hflip=k[0], degrees=(k[1], k[2]),
                                               translate=(k[3], k[4]), scale=(k[5], k[6]), shear=(k[7], k[8]))
        want = g[f"{i}_out_boxes"]
        assert M.shape == (3, 3) and np.abs(M - g[f"{i}_M"]).max() <= 1e-12
        assert boxes.shape == want.shape and (len(want) == 0 or np.abs(boxes - want).max() <= 1e-12)
        assert np.array_equal(pids, g[f"{i}_out_pids"])
        n_in, n_out, empty = n_in + len(g[f"{i}_boxes"]), n_out + len(want), empty + (len(g[f"{i}_boxes"]) == 0)
        clipped += int(((want[:, [0, 1]] == 0) | (want[:, [2]] == hw[1] - 1) | (want[:, [3]] == hw[0] - 1)).any(1).sum())
    assert n_out < n_in and clipped > 0 and empty > 0


def test_affine_matrix_parts():
    M = augment.affine_matrix((1080, 1920), hflip=True)
    assert np.array_equal(M, np.array([[-1.0, 0, 1920], [0, 1, 0], [0, 0, 1]]))
    M = augment.affine_matrix((100, 200), angle=90.0, scale=2.0)              # the centre stays where it is
    assert np.allclose(M @ np.array([100.0, 50.0, 1.0]), [100.0, 50.0, 1.0], atol=1e-12)
    assert np.allclose(M[:2, :2], [[0, 2], [-2, 0]], atol=1e-12)


def test_misuse_raises():
    fr = cases.frames(2, 8, 8)
    with pytest.raises(TypeError, match="uint8"):
        ingest_frames(fr.float(), None, (8, 8))
    with pytest.raises(ValueError, match="frames must be"):
        ingest_frames(torch.zeros(2, 8, 8, 4, dtype=torch.uint8), None, (8, 8))
    with pytest.raises(ValueError, match="one 3x3 matrix per frame"):
        ingest_frames(fr, torch.eye(3)[None].repeat(3, 1, 1), (8, 8))
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="GPU only"):
            ingest_frames(fr, None, (8, 8), dtype=dt)
    with pytest.raises(ValueError, match="out must be"):
        ingest_frames(fr, None, (8, 8), out=torch.empty(2, 3, 8, 9))
    with pytest.raises(ValueError, match="dense in channels_last"):
        ingest_frames(fr, None, (8, 8), out=torch.empty(2, 3, 8, 8))
