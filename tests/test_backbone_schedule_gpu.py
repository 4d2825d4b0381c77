"""GPU: the launch schedule of the backbone's HIP paths, written out.  One forward of each mode is recorded as the
sequence of (call, rows of its activation operand, "main" | "side" by the current stream) and compared with the expected
sequence below, which doubles as the documentation of the schedule: what is launched, in which order, on which rows and
on which stream.  vit_small cut to its first 3 blocks (a first, an inner and a last block), B = 2 (the smallest batch at
which the cls-row kernels see more than one row); 224 px for the split row layout [B*256 patch rows | B cls rows], 196 px
(W % 8 != 0) for the cls-first layout [B, 197, C].  Recorded: the `ops` entry points the backbone calls, the library GEMM
calls (torch.mm / addmm / _addmm_activation, Tensor.addmm_, F.linear), fork / join of the side chain and the cls tail hook
(the recorder: tests/backbone_trace.py).
A cls-row linear carries its mode (0 bias, 1 bias + tanh-GELU, 2 accumulate into the residual stream) and "+stats" where
it also leaves LayerNorm statistics partials."""
import pytest

from backbone_trace import MAIN, SIDE, _on, _record

pytestmark = pytest.mark.gpu

B, L = 2, 3
MP, M = B * 256, B * 257            # split row layout at 224 px: patch rows, all rows
BT = B * 197                        # cls-first layout at 196 px


# patch embedding: patchify, one GEMM into the patch rows of the zero-row buffer, add + LayerNorm (block 0's norm1) on all rows
EMBED = _on(MAIN, ("patchify_bf16", MP), ("mm", MP), ("add_layernorm_bf16", M))
ATTENTION = _on(MAIN, ("attention_qkv_split_bf16", M))


def test_split_side_chain_schedule(dev, monkeypatch):
    """The default: after each attention the six cls-row launches go to the side stream (issued first), the six patch-row
    launches stay on the main stream; one fork after the attention, one join before the next.  Block 0's qkv precedes
    the loop, both parts on the main stream; the last block has no next qkv and ends its side chain with the hook."""
    calls, out = _record(dev, monkeypatch, 224)
    want = EMBED + _on(MAIN, ("addmm", MP), ("skinny:0", B))
    for i in range(L):
        last = i == L - 1
        want += ATTENTION + _on(MAIN, ("fork", None))
        want += _on(SIDE, ("skinny:2", B), ("bias_layernorm_bf16", B), ("skinny:1", B), ("skinny:2", B), ("bias_layernorm_bf16", B),
                    ("cls_tail_hook", B) if last else ("skinny:0", B))
        want += _on(MAIN, ("addmm_", MP), ("bias_layernorm_bf16", MP), ("_addmm_activation", MP), ("addmm_", MP),
                    ("bias_layernorm_bf16", MP), *(() if last else (("addmm", MP),)))
        want += _on(MAIN, ("join", None))
    assert calls == want
    assert [c[0] for c in calls].count("fork") == L and [c[0] for c in calls].count("join") == L
    assert [c for c in calls if c[0] == "cls_tail_hook"] == [("cls_tail_hook", B, SIDE)] and out.token_ready


@pytest.mark.parametrize("cls_after_gemm", [True, False])
def test_split_in_stream_unfused_schedule(dev, monkeypatch, cls_after_gemm):
    """One stream: each LayerNorm one launch over all rows, each GEMM stage its patch-row library GEMM and its cls-row
    launch, cls after (default) or before; each block issues its own qkv at the top.  No fork, no hook."""
    calls, out = _record(dev, monkeypatch, 224, cls_side_chain=False, cls_after_gemm=cls_after_gemm)

    def pair(gemm, cls):
        return [gemm, cls] if cls_after_gemm else [cls, gemm]

    block = (pair(("addmm", MP), ("skinny:0", B)) + [("attention_qkv_split_bf16", M)] + pair(("addmm_", MP), ("skinny:2", B))
             + [("bias_layernorm_bf16", M)] + pair(("_addmm_activation", MP), ("skinny:1", B)) + pair(("addmm_", MP), ("skinny:2", B))
             + [("bias_layernorm_bf16", M)])
    assert calls == EMBED + _on(MAIN, *block) * L
    assert not out.token_ready


def test_split_in_stream_fused_schedule(dev, monkeypatch):
    """fuse_ln_cls: the cls-row fc1 and (from block 1 on) qkv ride in the LayerNorm launch before them, so those stages
    issue only their patch-row GEMM; the cls-row proj and fc2 leave the statistics partials that LayerNorm reads (not the
    last fc2: the final norm is a plain launch)."""
    calls, out = _record(dev, monkeypatch, 224, cls_side_chain=False, fuse_ln_cls=True)
    want = list(EMBED)
    for i in range(L):
        last = i == L - 1
        want += _on(MAIN, ("addmm", MP), *((("skinny:0", B),) if i == 0 else ()))
        want += ATTENTION + _on(MAIN, ("addmm_", MP), ("skinny:2+stats", B), ("bias_layernorm_cls_linear_bf16", M), ("_addmm_activation", MP),
                                ("addmm_", MP), ("skinny:2", B) if last else ("skinny:2+stats", B),
                                ("bias_layernorm_bf16", M) if last else ("bias_layernorm_cls_linear_bf16", M))
    assert calls == want
    assert not out.token_ready


def test_cls_first_residual_in_gemm_schedule(dev, monkeypatch):
    """196 px: all B*197 rows as one range, library GEMMs only; qkv through the block's nn.Linear."""
    calls, _ = _record(dev, monkeypatch, 196)
    block = _on(MAIN, ("linear", BT), ("attention_qkv_bf16", BT), ("addmm_", BT), ("bias_layernorm_bf16", BT), ("_addmm_activation", BT),
                ("addmm_", BT), ("bias_layernorm_bf16", BT))
    assert calls == _on(MAIN, ("layernorm_bf16", BT)) + block * L


def test_cls_first_add_layernorm_schedule(dev, monkeypatch):
    """196 px, residual_in_gemm off: biased proj / fc2 through nn.Linear, each residual add inside the next LayerNorm."""
    calls, _ = _record(dev, monkeypatch, 196, residual_in_gemm=False)
    block = _on(MAIN, ("linear", BT), ("attention_qkv_bf16", BT), ("linear", BT), ("add_layernorm_bf16", BT), ("_addmm_activation", BT),
                ("linear", BT), ("add_layernorm_bf16", BT))
    assert calls == _on(MAIN, ("layernorm_bf16", BT)) + block * L
