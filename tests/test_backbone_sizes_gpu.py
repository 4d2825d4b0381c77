"""GPU: the ViT backbone away from 224 px (vit_small, patch 14), against the plain block loop.
  168 px: n = 144, T = 145 — the split HIP path (own patchify shape, embedding offsets, zero rows, cls side chain, a
          144-row ragged tiling);
  196 px: W % 8 != 0 — the cls-first HIP path with the HIP attention at T = 197;
  322 px: T = 530 > 288 — the cls-first HIP path with scaled_dot_product_attention.
The criterion is the one of test_heads_gpu.py::test_backbone_hip_path_matches_block_loop (same constants), applied to
all tokens, to the cls row alone and to the patch rows alone; LayerScale and the cls token are randomised so that a wrong
cls offset or position row is as large as the tokens themselves.  Each case also asserts which route ran."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B = 3
C = 384
CASES = [(168, "split_side"), (168, "split"), (168, "split_unfused"), (196, "resid_gemm"), (196, "add_ln"), (322, "resid_gemm")]


def _model(dev, img_size, mode="split_side", seed=0):
    from vpr_amd.backbone import DinoV2
    torch.manual_seed(seed)
    m = DinoV2("vit_small", img_size=img_size).to(dev).to(torch.bfloat16).eval()
    # hip_split stays on (the default): at 196 and 322 px the image shape alone must send forward() down the cls-first path
    m.cls_side_chain = mode == "split_side"
    m.fuse_ln_cls = mode == "split"
    m.residual_in_gemm = mode != "add_ln"
    for b in m.blocks:
        torch.nn.init.normal_(b.ls1, std=0.3)
        torch.nn.init.normal_(b.ls2, std=0.3)
    torch.nn.init.normal_(m.cls_token, std=0.5)        # the default 1e-6 would hide a wrong cls offset
    m.fold_layerscale()
    return m


def _block_loop(model, inp):
    t = model.patch_embed(inp).flatten(2).transpose(1, 2)
    t = torch.cat([model.cls_token.expand(inp.shape[0], -1, -1), t], dim=1) + model.pos_embed
    for blk in model.blocks:
        t = blk(t)
    return F.layer_norm(t.float(), (C,), model.norm.weight.float(), model.norm.bias.float(), 1e-6)


class _Counter:
    """Counting wrappers around the three attention routes and the two LayerNorm forms of the cls-first path."""
    NAMES = ("attention_qkv_split_bf16", "attention_qkv_bf16", "bias_layernorm_bf16", "add_layernorm_bf16")

    def __init__(self, monkeypatch):
        from vpr_amd import ops
        self.n = {name: 0 for name in self.NAMES + ("sdpa",)}
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        monkeypatch.setattr(F, "scaled_dot_product_attention", self._wrap("sdpa", F.scaled_dot_product_attention))

    def _wrap(self, name, fn):
        def counted(*args, **kwargs):
            self.n[name] += 1
            return fn(*args, **kwargs)
        return counted

    def reset(self):
        for k in self.n:
            self.n[k] = 0


def _run_and_compare(m, x, count, label):
    """forward() against the bf16 and the f32 block loop on the same weights -> the calls forward() made.  The criterion
    of test_backbone_hip_path_matches_block_loop, on all rows, on the cls row alone (1/T of the RMS over all rows: a wrong
    cls row would pass there) and on the patch rows alone."""
    m32 = copy.deepcopy(m).float()                     # same (bf16-rounded, LayerScale-folded) weights, f32 math
    with torch.no_grad():
        count.reset()
        fast = m(x)
        calls = dict(count.n)
        slow = _block_loop(m, x)                       # bf16 activations, PyTorch ops only
        ref = _block_loop(m32, x.float())              # f32 activations
    assert fast.shape == (x.shape[0], 1 + m.num_patches, C)
    # two bf16 pipelines differ from each other by up to the sum of their errors; judge each against f32:
    # the HIP path must not be worse than the plain bf16 block loop
    rms = lambda d: d.float().pow(2).mean().sqrt().item()
    for what, rows in (("all", slice(0, None)), ("cls", slice(0, 1)), ("patch", slice(1, None))):
        f, s, r = fast[:, rows].float(), slow[:, rows], ref[:, rows]
        err_fast, err_slow = rms(f - r), rms(s - r)
        max_fast, max_slow = (f - r).abs().max().item(), (s - r).abs().max().item()
        print(f"{label} {what}: rms fast/slow {err_fast / err_slow:.3f}, fast/rms(ref) {err_fast / rms(r):.4f}, "
              f"max fast/slow {max_fast / max_slow:.3f}")
        assert err_fast < 1.15 * err_slow and err_fast < 0.02 * rms(r), (what, err_fast, err_slow, rms(r))
        assert max_fast < 2.0 * max_slow, (what, max_fast, max_slow)
    return calls


@pytest.mark.parametrize("img_size,mode", CASES)
def test_tokens_match_block_loop_away_from_224(dev, monkeypatch, img_size, mode):
    m = _model(dev, img_size, mode)
    x = torch.randn(B, 3, img_size, img_size, device=dev, dtype=torch.bfloat16)
    assert m.num_patches == (img_size // 14) ** 2
    assert m.hip_split and m._hip_split_ok(x) == (img_size == 168)     # 196: W % 8 != 0; 322: that and T = 530 > 288
    calls = _run_and_compare(m, x, _Counter(monkeypatch), f"{img_size} {mode}")
    # the route: 12 HIP attentions at 168 (split layout) and 196 (cls-first), none at 322; never the PyTorch block loop,
    # which would show as 12 sdpa calls at 168 / 196 and as no bias / add LayerNorm launch at any size
    want = {"attention_qkv_split_bf16": 12 if img_size == 168 else 0, "attention_qkv_bf16": 12 if img_size == 196 else 0,
            "sdpa": 12 if img_size == 322 else 0}
    assert {k: calls[k] for k in want} == want, calls
    if mode == "resid_gemm":
        assert calls["bias_layernorm_bf16"] == 24 and calls["add_layernorm_bf16"] == 0, calls
    if mode == "add_ln":
        assert calls["add_layernorm_bf16"] == 24 and calls["bias_layernorm_bf16"] == 0, calls


@pytest.mark.parametrize("W,split", [(560, True), (616, False)])
def test_patchify_lds_limit_decides_the_route(dev, monkeypatch, W, split):
    """A 56 x W image, 4 patch rows: three channels of one patch row are 47 040 B of LDS at W = 560 (the split path, with
    patchify) and 51 744 B at W = 616, which vpr_patchify_bf16 refuses — there forward() must take the cls-first path by
    itself (_hip_split_ok agrees with the kernel's limit), and either way the tokens match the block loop."""
    from vpr_amd.backbone import DinoV2
    n = 4 * (W // 14)
    assert 1 + n <= 288 and (3 * 14 * W * 2 <= 48 * 1024) == split
    torch.manual_seed(5)
    m = DinoV2("vit_small")
    m.num_patches = n
    m.pos_embed = torch.nn.Parameter(torch.nn.init.trunc_normal_(torch.zeros(1, 1 + n, C), std=0.02))
    m = m.to(dev).to(torch.bfloat16).eval()
    for b in m.blocks:
        torch.nn.init.normal_(b.ls1, std=0.3)
        torch.nn.init.normal_(b.ls2, std=0.3)
    torch.nn.init.normal_(m.cls_token, std=0.5)
    m.fold_layerscale()
    x = torch.randn(2, 3, 56, W, device=dev, dtype=torch.bfloat16)
    assert m._hip_split_ok(x) == split
    calls = _run_and_compare(m, x, _Counter(monkeypatch), f"56x{W}")
    assert calls["attention_qkv_split_bf16"] == (12 if split else 0) and calls["attention_qkv_bf16"] == (0 if split else 12)
    assert calls["sdpa"] == 0


def test_patch_embed_hip_matches_conv_at_168(dev):
    """patchify + GEMM + static offsets == conv + cls cat + position add at n = 144, with position rows so far apart that
    a token row off by one exceeds the tolerance.  (Each row of pos_embed is a random +-1 code plus noise: the tolerance
    is relative to the largest value, so rows whose mean merely grows with the row number, 145 of them, would sit
    closer together than the tolerance.)"""
    from vpr_amd import ops
    m = _model(dev, 168, seed=1)
    n = 144
    with torch.no_grad():
        g = torch.Generator().manual_seed(2)
        code = (torch.randint(0, 2, (1 + n, C), generator=g) * 2 - 1).float() + 0.02 * torch.randn(1 + n, C, generator=g)
        m.pos_embed.copy_(code.unsqueeze(0).to(dev))
    x = torch.randn(2, 3, 168, 168, device=dev, dtype=torch.bfloat16)
    assert m._hip_split_ok(x)
    with torch.no_grad():
        w, off = m._embed_consts(x)
        assert off.shape == (2 * n + 2, C)
        raw = ops.patchify_bf16(x, 14, w.shape[1], 0) @ w.t()                       # [2*144, 384]
        body = (raw.float() + off[:2 * n].float()).view(2, n, C)
        cls = off[2 * n:].float()
        m32 = m.float()

        def reference(pos):
            t = m32.patch_embed(x.float()).flatten(2).transpose(1, 2)
            return torch.cat([m32.cls_token.expand(2, -1, -1), t], dim=1) + pos

        ref = reference(m32.pos_embed)
        tol = 0.02 * max(1.0, ref.abs().max().item())
        # the reference itself tells rows apart: position rows moved by one change it by more than the tolerance, in the
        # patch rows and in the cls row
        moved = reference(torch.roll(m32.pos_embed, 1, dims=1))
        assert (moved[:, 1:] - ref[:, 1:]).abs().amax(dim=2).min().item() > tol
        assert (moved[:, 0] - ref[:, 0]).abs().max().item() > tol
    err_body, err_cls = (body - ref[:, 1:]).abs().max().item(), (cls - ref[:, 0]).abs().max().item()
    print(f"patch embed at 168: body {err_body:.4f} cls {err_cls:.4f} tol {tol:.4f}")
    assert err_body < tol and err_cls < tol


@pytest.mark.parametrize("batch", [3, 1])
def test_cls_side_chain_is_bit_identical_at_168(dev, batch):
    """The cls rows on their own stream against the single-stream path at n = 144: same kernels on the same data."""
    m = _model(dev, 168, seed=3)
    x = torch.randn(batch, 3, 168, 168, device=dev, dtype=torch.bfloat16)
    assert m._hip_split_ok(x)
    m.cls_side_chain = False
    ref = m(x, split=True)
    assert ref.patch.shape == (batch, 144, C) and ref.cls.shape == (batch, C)
    m.cls_side_chain = True
    for _ in range(3):
        got = m(x, split=True)
        assert torch.equal(got.patch, ref.patch) and torch.equal(got.cls, ref.cls)


@pytest.mark.parametrize("img_size", [168, 196, 322])
def test_split_and_joined_layouts_agree(dev, img_size):
    """168: forward(split=True) joined == forward(); 196 / 322: the SplitTokens built from the cls-first result == slicing it."""
    m = _model(dev, img_size, seed=4)
    n = (img_size // 14) ** 2
    x = torch.randn(B, 3, img_size, img_size, device=dev, dtype=torch.bfloat16)
    assert m._hip_split_ok(x) == (img_size == 168)
    st = m(x, split=True)
    full = m(x)
    assert st.patch.shape == (B, n, C) and st.cls.shape == (B, C) and full.shape == (B, 1 + n, C)
    assert st.patch.is_contiguous() and st.cls.is_contiguous() and full.is_contiguous()
    assert torch.equal(st.joined(), full)
    assert torch.equal(st.patch, full[:, 1:]) and torch.equal(st.cls, full[:, 0])
