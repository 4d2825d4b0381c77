"""GPU: vpr_preprocess_resize_normalize against PIL (bytes, exact) and ToTensor+Normalize (f32)."""
import ctypes

import numpy as np
import pytest
import torch

import preprocess_cases as pc
from oracle import preprocess as opre

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W,filt,mean,std", [
    (480, 640, "bilinear", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),           # dinov2salad_validation.py:18-22
    (1080, 1920, "bilinear", (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),   # dinov2salad_finetuning.py:45-50
    (600, 800, "bicubic", (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),      # HF Swin processor
    (224, 224, "bilinear", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    (150, 199, "bicubic", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),            # upscaling
])
def test_resize_normalize_matches_pil(dev, H, W, filt, mean, std):
    from PIL import Image
    from vpr_amd.preprocess import ResizeNormalize
    rng = np.random.default_rng(H + W)
    imgs = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    pf = Image.BILINEAR if filt == "bilinear" else Image.BICUBIC
    ref_u8 = np.stack([np.asarray(Image.fromarray(im).resize((224, 224), pf)) for im in imgs])
    ref_f = np.stack([opre.to_tensor_normalize(u, mean, std) for u in ref_u8])
    pp = ResizeNormalize(224, filt, mean, std, torch.float32)
    out, out_u8 = pp(torch.from_numpy(imgs).to(dev), return_bytes=True)
    assert np.array_equal(out_u8.cpu().numpy(), ref_u8)
    assert np.abs(out.cpu().numpy() - ref_f).max() < 1e-6
    out16 = ResizeNormalize(224, filt, mean, std, torch.bfloat16)(torch.from_numpy(imgs).to(dev))
    assert torch.equal(out16.cpu(), torch.from_numpy(ref_f).to(torch.bfloat16))


# ------------------------------------------------------------------ away from 224 px: shapes, inputs, state, refusals
INVALID_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3      # include/vpr_amd.h


def _ref_float(ref_u8, mean, std):
    return np.stack([opre.to_tensor_normalize(u, mean, std) for u in ref_u8])


def _assert_exact(pp_args, x, ref_u8):
    """One (out size, filter, mean, std) on the device tensor x: bytes equal PIL's, f32 bit-identical to ToTensor +
    Normalize of them, bf16 equal to that rounded to nearest even, and the same without the byte output."""
    from vpr_amd.preprocess import ResizeNormalize
    size, filt, mean, std = pp_args
    ref_f = _ref_float(ref_u8, mean, std)
    pp = ResizeNormalize(size, filt, mean, std, torch.float32)
    out, out_u8 = pp(x, return_bytes=True)
    assert np.array_equal(out_u8.cpu().numpy(), ref_u8)
    got = out.cpu().numpy()
    assert got.shape == ref_f.shape
    assert np.array_equal(got.view(np.uint32), ref_f.view(np.uint32))
    assert torch.equal(pp(x), out)                                   # null out_u8
    pp16 = ResizeNormalize(size, filt, mean, std, torch.bfloat16)
    out16, out16_u8 = pp16(x, return_bytes=True)
    assert np.array_equal(out16_u8.cpu().numpy(), ref_u8)
    assert torch.equal(out16.cpu(), torch.from_numpy(ref_f).to(torch.bfloat16))
    assert torch.equal(pp16(x), out16)


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("filt", pc.FILTERS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.case_id)
def test_resize_normalize_shapes_and_inputs(dev, shape, filt, kind):
    """More than one column block (OW > 256), OH != OW, up- and downscaling, very wide kernels and tiny inputs, on random
    bytes, random binary images (bicubic overshoot clamped at both ends) and a checkerboard.  PIL is the reference for the
    bytes; the float stage must reproduce u8/255 then (x - mean)/std in IEEE f32 bit for bit (no step of it can contract)."""
    (H, W), (OH, OW), clips = shape
    ref_u8 = pc.pil_reference(H, W, OH, OW, kind, filt)
    if clips and kind == "binary":
        pc.assert_reference_clips(ref_u8, (shape, filt))
    x = torch.from_numpy(pc.images(H, W, kind).copy()).to(dev)
    size = OH if OH == OW else (OH, OW)
    for mean, std in pc.NORMS:
        _assert_exact((size, filt, mean, std), x, ref_u8)


@pytest.mark.parametrize("filt", pc.FILTERS)
def test_float_stage_on_every_byte_value(dev, filt):
    """Identity-size 16 x 16 images whose every channel holds each byte value once: the float stage on all 768
    (value, channel) pairs, both normalisations, f32 and bf16."""
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([ramp, ramp[::-1, ::-1], ramp + np.uint8(85)], axis=-1)
    imgs = np.stack([img, img[:, ::-1]]).copy()
    for c in range(3):
        assert len(np.unique(imgs[0, :, :, c])) == 256
    x = torch.from_numpy(imgs).to(dev)
    for mean, std in pc.NORMS:
        _assert_exact((16, filt, mean, std), x, imgs)                  # identity tables: the resized bytes are the input


def test_one_object_across_sizes_streams_and_offsets(dev):
    """One ResizeNormalize object on inputs of sizes A, B, A (B needs a smaller workspace than A), then a third size on a
    non-default stream, then a view at a 1-byte storage offset: neither the table cache nor the per-stream workspace leaks
    between calls, and the kernel needs no alignment of its input."""
    from vpr_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD, ResizeNormalize
    pp = ResizeNormalize(322, "bicubic", IMAGENET_MEAN, IMAGENET_STD, torch.float32)

    def case(H, W, kind):
        ref_u8 = pc.pil_reference(H, W, 322, 322, kind, "bicubic")
        return torch.from_numpy(pc.images(H, W, kind).copy()).to(dev), ref_u8, _ref_float(ref_u8, IMAGENET_MEAN, IMAGENET_STD)

    def check(res, ref_u8, ref_f):
        out, out_u8 = res
        assert np.array_equal(out_u8.cpu().numpy(), ref_u8)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref_f.view(np.uint32))

    a, b, c = case(480, 640, "uniform"), case(300, 400, "binary"), case(322, 322, "checker")
    for x, ref_u8, ref_f in (a, b, a):
        check(pp(x, return_bytes=True), ref_u8, ref_f)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        res = pp(c[0], return_bytes=True)
    side.synchronize()
    check(res, c[1], c[2])
    check(pp(b[0], return_bytes=True), b[1], b[2])                   # back on the first stream, the smaller size again
    store = torch.zeros(1 + a[0].numel(), dtype=torch.uint8, device=dev)
    view = store[1:].view(a[0].shape)
    view.copy_(a[0])
    assert view.is_contiguous() and view.data_ptr() % 2 == 1
    check(pp(view, return_bytes=True), a[1], a[2])
    # (OH, OW) form == the square form
    sq = ResizeNormalize((322, 322), "bicubic", IMAGENET_MEAN, IMAGENET_STD, torch.float32)(a[0])
    assert np.array_equal(sq.cpu().numpy().view(np.uint32), a[2].view(np.uint32))


def test_refusals_leave_the_outputs_alone(dev):
    """vpr_preprocess_resize_normalize returns its documented status for a null input or workspace, B = 0, ksize_x = 0,
    B = 65536 and a workspace one byte short, and writes neither output."""
    from vpr_amd import _lib, ops
    from vpr_amd.preprocess import resample_coeffs
    B, H, W, OH, OW = 1, 4, 6, 8, 8
    kx, xb, ksx = resample_coeffs(W, OW, "bilinear")
    ky, yb, ksy = resample_coeffs(H, OH, "bilinear")
    t = lambda a: torch.from_numpy(a.copy()).to(dev)
    kx, xb, ky, yb = t(kx), t(xb), t(ky), t(yb)
    x = torch.full((B, H, W, 3), 200, dtype=torch.uint8, device=dev)
    out = torch.empty((B, 3, OH, OW), dtype=torch.float32, device=dev)
    out_u8 = torch.empty((B, OH, OW, 3), dtype=torch.uint8, device=dev)
    need = B * H * OW * 3
    ws = torch.empty(int(_lib.lib().vpr_preprocess_workspace_bytes(B, H, OW)), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def call(inp=x, B=B, ksx=ksx, wsp=ws, ws_bytes=need):
        return _lib.lib().vpr_preprocess_resize_normalize(
            ops._ptr(inp), B, H, W, OH, OW, ops._ptr(kx), ops._ptr(xb), ksx, ops._ptr(ky), ops._ptr(yb), ksy, mean, std,
            ops._ptr(out), 0, ops._ptr(out_u8), ops._ptr(wsp), ws_bytes, ops._stream())

    for kwargs, status in (({"inp": None}, INVALID_ARG), ({"wsp": None}, INVALID_ARG), ({"B": 0}, INVALID_ARG),
                           ({"ksx": 0}, INVALID_ARG), ({"B": 65536}, UNSUPPORTED), ({"ws_bytes": need - 1}, WORKSPACE)):
        out.fill_(-77.0)
        out_u8.fill_(0xA5)
        assert call(**kwargs) == status, kwargs
        torch.cuda.synchronize()
        assert bool((out == -77.0).all()) and bool((out_u8 == 0xA5).all()), kwargs
    assert call() == 0                                               # the same arguments, none of them wrong: it runs
    torch.cuda.synchronize()
    assert bool((out_u8 == 200).all()) and bool((out == (np.float32(200) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)).all())
