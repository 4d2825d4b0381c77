"""Shapes and inputs shared by the CPU selfcheck of the preprocessing oracle (test_oracle_selfchecks.py) and the GPU
tests of preprocess.hip (test_preprocess_gpu.py): the selfcheck pins the oracle and resample_coeffs against PIL on exactly
the images the kernel is later judged on."""
from functools import lru_cache

import numpy as np

# ((H, W), (OH, OW), clips): `clips` marks the shapes that upscale at least one dimension of more than one pixel, where a
# random binary image must come out of the resize with 0, 255 and values in between.
SHAPES = [
    ((480, 640), (322, 322), False),      # two column blocks; the workload's size
    ((1080, 1920), (322, 322), False),    # two column blocks, large downscale
    ((300, 400), (322, 322), True),       # height up, width down
    ((322, 322), (322, 322), False),      # identity tables in both passes
    ((480, 640), (196, 196), False),
    ((480, 640), (168, 168), False),
    ((50, 70), (257, 513), True),         # three column blocks, the last one partial (1 column); both dimensions up
    ((96, 130), (40, 600), True),         # non-square
    ((130, 96), (600, 40), True),
    ((17, 4000), (20, 20), False),        # ksize 401 (bilinear) / 801 (bicubic) in the width pass
    ((3, 5), (16, 16), True),
    ((1, 1), (8, 8), False),              # one pixel: every output byte is a copy of it
]
KINDS = ("uniform", "binary", "checker")
FILTERS = ("bilinear", "bicubic")
NORMS = (((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
B = 2


def case_id(shape) -> str:
    (H, W), (OH, OW), _ = shape
    return f"{H}x{W}-{OH}x{OW}"


@lru_cache(maxsize=None)
def images(H: int, W: int, kind: str) -> np.ndarray:
    """[B, H, W, 3] u8, two different images.  uniform: random bytes; binary: every byte 0 or 255 (bicubic overshoots past
    both ends of the range around each edge, so the [0, 255] clamp fires on both sides); checker: a one-pixel checkerboard,
    its inverse as the second image, the green channel in opposite phase."""
    rng = np.random.default_rng(1000 * H + W)
    if kind == "uniform":
        out = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    elif kind == "binary":
        out = (rng.integers(0, 2, (B, H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)
    elif kind == "checker":
        y, x = np.mgrid[0:H, 0:W]
        base = (((x + y) & 1) * 255).astype(np.uint8)
        img = np.stack([base, 255 - base, base], axis=-1)
        out = np.stack([img, 255 - img])
    else:
        raise ValueError(kind)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def pil_reference(H: int, W: int, OH: int, OW: int, kind: str, filt: str) -> np.ndarray:
    """[B, OH, OW, 3] u8: PIL.Image.resize of images(H, W, kind)."""
    from PIL import Image
    pf = Image.BILINEAR if filt == "bilinear" else Image.BICUBIC
    out = np.stack([np.asarray(Image.fromarray(im).resize((OW, OH), pf)) for im in images(H, W, kind)])
    out.setflags(write=False)
    return out


def assert_reference_clips(ref_u8: np.ndarray, what) -> None:
    """Both ends of the byte range and values strictly inside it occur in the reference."""
    assert (ref_u8 == 0).any() and (ref_u8 == 255).any(), what
    assert ((ref_u8 > 0) & (ref_u8 < 255)).any(), what
