"""GPU: vpr_patchify_bf16 at its edges.  The kernel is a pure copy, so every comparison is on the int16 view of the
bf16 data (NaN payloads, infinities, denormals and -0 count): arbitrary bit patterns, the 48 KiB LDS limit from both
sides, work loops longer than one pass, block index -> image past 64, alignment, and every refusal leaving `out` alone.
The output always sits in the middle of a larger sentinel buffer whose margins are checked."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2      # include/vpr_amd.h
POISON = 0x7FFF                               # a NaN as bf16; never what the kernel writes into padding (zero bits)
MARGIN = 4096                                 # int16 elements on either side of `out` (8 KiB: keeps `out` 16-byte aligned)
SPECIALS = (0x7F80, 0xFF80, 0x7FC1, 0xFFFF, 0x8000, 0x0001, 0x807F)     # +Inf, -Inf, two NaNs, -0, two denormals


def _i16(v: int) -> int:
    return v - 65536 if v >= 32768 else v


def _random_bits(B, Cin, H, W, seed):
    """[B, Cin, H, W] int16, uniformly random bit patterns with every special value planted at a random place."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(-32768, 32768, (B, Cin, H, W), generator=g, dtype=torch.int16)
    flat = img.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:len(SPECIALS)]
    flat[where] = torch.tensor([_i16(s) for s in SPECIALS], dtype=torch.int16)
    f = img.view(torch.bfloat16)
    assert f.isnan().any() and f.isposinf().any() and f.isneginf().any()
    assert (img == _i16(0x8000)).any()                                                  # -0
    assert (((img & 0x7F80) == 0) & ((img & 0x007F) != 0)).any()                        # denormals
    return img


def _reference(img16, P, kpad, lead):
    """[B, lead + n, kpad] int16 by plain indexing: out[b, lead + py*G + px, c*P*P + i*P + j] = img[b, c, py*P + i, px*P + j]."""
    B, Cin, H, W = img16.shape
    GH, G, K = H // P, W // P, Cin * P * P
    ref = torch.zeros((B, lead + GH * G, kpad), dtype=torch.int16)
    ref[:, lead:, :K] = img16.view(B, Cin, GH, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B, GH * G, K)
    return ref


class _Out:
    """`numel` int16 elements in the middle of a poisoned buffer, `shift` elements past the 16-byte-aligned position."""

    def __init__(self, dev, numel, shift=0):
        self.big = torch.full((2 * MARGIN + numel + shift,), POISON, dtype=torch.int16, device=dev)
        self.lo, self.hi = MARGIN + shift, MARGIN + shift + numel
        assert (self.big.data_ptr() + 2 * MARGIN) % 16 == 0
        self.ptr = self.big.data_ptr() + 2 * self.lo

    def body(self):
        return self.big[self.lo:self.hi].cpu()

    def margins_intact(self):
        return bool((self.big[:self.lo] == POISON).all()) and bool((self.big[self.hi:] == POISON).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.big == POISON).all())


def _raw(images_ptr, B, Cin, H, W, P, kpad, lead, out_ptr):
    from vpr_amd import _lib, ops
    return _lib.lib().vpr_patchify_bf16(ctypes.c_void_p(images_ptr), B, Cin, H, W, P, kpad, lead, ctypes.c_void_p(out_ptr),
                                        ops._stream())


def _check_exact(dev, img16, P, kpad, lead):
    """The raw entry on a poisoned `out`: patches bit-identical, lead rows and columns K..kpad zero bits, margins intact."""
    B, Cin, H, W = img16.shape
    n = (H // P) * (W // P)
    x = img16.to(dev)
    out = _Out(dev, B * (lead + n) * kpad)
    assert _raw(x.data_ptr(), B, Cin, H, W, P, kpad, lead, out.ptr) == OK
    torch.cuda.synchronize()
    got = out.body().view(B, lead + n, kpad)
    assert torch.equal(got, _reference(img16, P, kpad, lead))
    assert out.margins_intact()
    return x, got


@pytest.mark.parametrize("B,Cin,H,W,P,kpad,lead", [(2, 3, 168, 168, 14, 640, 0), (2, 3, 28, 56, 14, 592, 3),
                                                    (1, 3, 7, 56, 7, 152, 1)])
def test_arbitrary_bit_patterns_and_poisoned_output(dev, B, Cin, H, W, P, kpad, lead):
    from vpr_amd import ops
    img16 = _random_bits(B, Cin, H, W, seed=H + W + P)
    x, got = _check_exact(dev, img16, P, kpad, lead)
    # the wrapper (a fresh torch.empty output) gives the same bits, and F.unfold agrees with the indexing reference
    wrapped = ops.patchify_bf16(x.view(torch.bfloat16), P, kpad, lead).cpu().view(torch.int16)
    assert torch.equal(wrapped.view(got.shape), got)
    unf = torch.nn.functional.unfold(img16.double(), P, stride=P).transpose(1, 2).to(torch.int16)      # int16 is exact in f64
    assert torch.equal(got[:, lead:, :Cin * P * P], unf)


@pytest.mark.parametrize("B,Cin,H,W,P,kpad,lead", [
    (1, 3, 16, 512, 16, 768, 1),      # LDS exactly 49 152 B, kpad == K
    (1, 3, 14, 560, 14, 640, 0),      # 47 040 B
    (1, 1, 8, 2048, 8, 64, 0),        # G = 256, 2048 output chunks: eight passes of the store loop, 8 of the load loop
])
def test_lds_limit_and_long_work_loops(dev, B, Cin, H, W, P, kpad, lead):
    _check_exact(dev, _random_bits(B, Cin, H, W, seed=W), P, kpad, lead)


@pytest.mark.parametrize("Cin,H,W,P,kpad,lead", [(3, 16, 528, 16, 768, 1),      # 50 688 B of LDS
                                                  (3, 14, 616, 14, 640, 0)])     # 51 744 B
def test_past_the_lds_limit_is_refused(dev, Cin, H, W, P, kpad, lead):
    from vpr_amd import ops
    assert Cin * P * W * 2 > 48 * 1024
    x = torch.zeros((1, Cin, H, W), dtype=torch.int16, device=dev)
    out = _Out(dev, (lead + (H // P) * (W // P)) * kpad)
    assert _raw(x.data_ptr(), 1, Cin, H, W, P, kpad, lead, out.ptr) == UNSUPPORTED
    assert out.untouched()
    with pytest.raises(RuntimeError):
        ops.patchify_bf16(x.view(torch.bfloat16), P, kpad, lead)


def test_batch_of_zero_and_of_seventy(dev):
    from vpr_amd import ops
    x = torch.zeros((1, 3, 14, 56), dtype=torch.int16, device=dev)
    out = _Out(dev, 5 * 592)
    assert _raw(x.data_ptr(), 0, 3, 14, 56, 14, 592, 1, out.ptr) == OK
    assert out.untouched()
    empty = ops.patchify_bf16(torch.empty((0, 3, 14, 56), dtype=torch.bfloat16, device=dev), 14, 592, 1)
    assert empty.shape == (0, 592)
    _check_exact(dev, _random_bits(70, 3, 14, 56, seed=70), 14, 592, 1)      # block index -> image past 64


def test_alignment(dev):
    """Both pointers must be 16-byte aligned (the kernel moves 16-byte chunks): an image view 2 bytes into its storage
    and an output 8 bytes off are refused; an image view 16 bytes in is accepted and exact."""
    from vpr_amd import ops
    B, Cin, H, W, P, kpad, lead = 2, 3, 28, 56, 14, 592, 1
    img16 = _random_bits(B, Cin, H, W, seed=9)
    n, N = (H // P) * (W // P), img16.numel()
    store = torch.zeros(N + 8, dtype=torch.int16, device=dev)
    off1 = store[1:1 + N].view(img16.shape)
    off1.copy_(img16)
    assert off1.is_contiguous() and off1.data_ptr() % 16 == 2
    out = _Out(dev, B * (lead + n) * kpad)
    assert _raw(off1.data_ptr(), B, Cin, H, W, P, kpad, lead, out.ptr) == UNSUPPORTED
    assert out.untouched()
    with pytest.raises(RuntimeError):
        ops.patchify_bf16(off1.view(torch.bfloat16), P, kpad, lead)
    off8 = store[8:8 + N].view(img16.shape)
    off8.copy_(img16)
    assert off8.data_ptr() % 16 == 0 and off8.storage_offset() == 8
    assert _raw(off8.data_ptr(), B, Cin, H, W, P, kpad, lead, out.ptr) == OK
    torch.cuda.synchronize()
    assert torch.equal(out.body().view(B, lead + n, kpad), _reference(img16, P, kpad, lead)) and out.margins_intact()
    got = ops.patchify_bf16(off8.view(torch.bfloat16), P, kpad, lead).cpu().view(torch.int16)
    assert torch.equal(got.view(B, lead + n, kpad), _reference(img16, P, kpad, lead))
    shifted = _Out(dev, B * (lead + n) * kpad, shift=4)              # out 8 bytes off
    assert shifted.ptr % 16 == 8
    assert _raw(off8.data_ptr(), B, Cin, H, W, P, kpad, lead, shifted.ptr) == UNSUPPORTED
    assert shifted.untouched()


@pytest.mark.parametrize("what,Cin,H,W,P,kpad,lead,status", [
    ("W % 8", 3, 14, 196, 14, 592, 0, UNSUPPORTED),
    ("H % P", 3, 15, 56, 14, 592, 0, UNSUPPORTED),
    ("W % P", 3, 14, 64, 14, 592, 0, UNSUPPORTED),
    ("kpad < K", 3, 14, 56, 14, 584, 0, UNSUPPORTED),
    ("kpad % 8", 3, 14, 56, 14, 590, 0, UNSUPPORTED),
    ("Cin = 0", 0, 14, 56, 14, 592, 0, INVALID_ARG),
    ("lead_rows = -1", 3, 14, 56, 14, 592, -1, INVALID_ARG),
    ("null images", 3, 14, 56, 14, 592, 1, INVALID_ARG),
    ("null out", 3, 14, 56, 14, 592, 1, INVALID_ARG),
])
def test_other_refusals_leave_the_output_alone(dev, what, Cin, H, W, P, kpad, lead, status):
    x = torch.zeros((2, 3, 16, 256), dtype=torch.int16, device=dev)      # larger than any of the shapes claimed below
    out = _Out(dev, 2 * 64 * 640)
    img_ptr = 0 if what == "null images" else x.data_ptr()
    out_ptr = 0 if what == "null out" else out.ptr
    assert _raw(img_ptr, 2, Cin, H, W, P, kpad, lead, out_ptr) == status
    assert out.untouched()
