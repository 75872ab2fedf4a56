"""Cases shared by tests/test_ingest.py (host path) and tests/test_ingest_gpu.py (device): seeded frames, the matrices of the warp
cases and the fp64 oracle of each case, computed once per process and never modified."""
import functools

import torch

import ingest_oracle as oracle

# (Hs, Ws) -> (Ho, Wo): the exact-ratio downscale; a ragged downscale with a 159-byte row pitch; an upscale (both clamps);
# equal size (the result is the normalised pixels); one pixel blown up
IDENTITY_SHAPES = [((216, 384), (144, 256)), ((37, 53), (24, 35)), ((20, 31), (33, 47)), ((8, 8), (8, 8)), ((1, 1), (3, 5))]
WARP_SHAPE = ((216, 384), (144, 256))


@functools.lru_cache(maxsize=None)
def frames(K, Hs, Ws, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * Hs + Ws + K)
    return torch.randint(0, 256, (K, Hs, Ws, 3), dtype=torch.uint8, generator=g)


def _affine(hw, scale, hflip, tx, ty):
    """scale about the image centre, optional reference hflip (x -> Ws - x), translation: T @ R @ F"""
    Hs, Ws = hw
    F = torch.eye(3, dtype=torch.float64)
    if hflip:
        F[0, 0], F[0, 2] = -1.0, float(Ws)
    R = torch.eye(3, dtype=torch.float64)
    R[0, 0] = R[1, 1] = scale
    R[0, 2], R[1, 2] = (1 - scale) * Ws / 2, (1 - scale) * Hs / 2
    T = torch.eye(3, dtype=torch.float64)
    T[0, 2], T[1, 2] = tx, ty
    return T @ R @ F


def hflip_matrix(Ws, plus_width=True):
    """the reference's flip (image_utils.py:19-23); without the + width it is the wrong contract of the teeth test"""
    M = torch.eye(3, dtype=torch.float64)
    M[0, 0] = -1.0
    M[0, 2] = float(Ws) if plus_width else 0.0
    return M


def translation_matrix(tx, ty):
    M = torch.eye(3, dtype=torch.float64)
    M[0, 2], M[1, 2] = float(tx), float(ty)
    return M


def _perspective():
    # w of the pre-image, 1 - x / 330 + y / 2600, changes sign inside the 384-wide image
    M = torch.eye(3, dtype=torch.float64)
    M[2, 0], M[2, 1] = 1.0 / 330.0, -1.0 / 2600.0
    return M @ _affine(WARP_SHAPE[0], 1.8, False, 0.0, 0.0)


GENERAL_WARPS = {
    "scale0.8_hflip": _affine(WARP_SHAPE[0], 0.8, True, 10.3, -7.6),
    "scale1.3": _affine(WARP_SHAPE[0], 1.3, False, 100.5, 45.25),
    "perspective": _perspective(),
}


@functools.lru_cache(maxsize=None)
def identity_ref(K, src, dst):
    return oracle.ingest_oracle(frames(K, *src), None, dst)


@functools.lru_cache(maxsize=None)
def warp_ref(name, K=2):
    M = GENERAL_WARPS[name][None].repeat(K, 1, 1)
    return oracle.ingest_oracle(frames(K, *WARP_SHAPE[0]), M, WARP_SHAPE[1])


@functools.lru_cache(maxsize=None)
def border_fraction(name):
    """share of output pixels all of whose 16 taps are border: the oracle of a black frame with border 255, unnormalised"""
    black = torch.zeros((1,) + WARP_SHAPE[0] + (3,), dtype=torch.uint8)
    r = oracle.ingest_oracle(black, GENERAL_WARPS[name][None], WARP_SHAPE[1], mean=(0, 0, 0), std=(1, 1, 1), border=255)
    return float((r[0, 0] > 1 - 1e-9).double().mean())
