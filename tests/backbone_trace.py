"""The recorder of the backbone's launches, once: what tests/test_backbone_schedule_gpu.py compares with its written-out
schedules, and, in capturing mode, the operands and results of every launch for tests/test_backbone_stages_gpu.py.

Recorded: the `ops` entry points the backbone calls, the library GEMM calls (torch.mm / addmm / _addmm_activation,
Tensor.addmm_, F.linear), fork / join of the side chain and the cls tail hook; capturing adds the in-place erf-GELU and
F.scaled_dot_product_attention (the attention beyond 288 tokens).  A cls-row linear carries its mode and "+stats".

Capturing: for every recorded call, clones of its tensor operands taken BEFORE the call and of its results taken AFTER
it (Tensor.addmm_ and skinny mode 2 write in place), each made on the stream that is current at the call, which orders
it with the launch; parameters and weights are kept by reference, scalars as they are.  Where a launch writes a row
range of a larger buffer, the whole buffer is cloned before and after too — except next to the cls side chain, whose
two streams write their row ranges of one buffer at the same time.  Read nothing before torch.cuda.synchronize().

`stage_records` turns a captured call list into oracle.backbone.Stage records by checking it against `schedule(mode)`,
the expected launch list of the mode annotated with (block, stage, part), and fails at the first differing position.
"""
import torch
import torch.nn.functional as F

from oracle import backbone as ob

MAIN, SIDE = "main", "side"
PATCH, CLS, ALL = ob.PATCH, ob.CLS, ob.ALL


class Call:
    """One captured call: before / after are lists parallel to (args, sorted kwargs) / the results."""
    def __init__(self, label, rows, stream, args, kwargs, result, after_args, whole):
        self.label, self.rows, self.stream, self.args, self.kwargs = label, rows, stream, args, kwargs
        self.result, self.after_args, self.whole = result, after_args, whole


def _is_parameter(t: torch.Tensor) -> bool:
    return isinstance(t, torch.nn.Parameter) or (t._is_view() and isinstance(t._base, torch.nn.Parameter))


class _Recorder:
    OPS = ("patchify_bf16", "layernorm_bf16", "add_layernorm_bf16", "bias_layernorm_bf16", "bias_layernorm_cls_linear_bf16",
           "skinny_linear_bf16", "attention_qkv_split_bf16", "attention_qkv_bf16")
    LIBRARY = ((torch, "mm", 0), (torch, "addmm", 1), (torch, "_addmm_activation", 1), (torch.Tensor, "addmm_", 1), (F, "linear", 0))
    CAPTURE_ONLY = ((torch._C._nn, "gelu_", 0), (F, "scaled_dot_product_attention", 0))

    def __init__(self, monkeypatch, dev, capture=False, capture_whole=True):
        from vpr_amd import _streams, ops
        self.dev, self.main, self.calls = dev, torch.cuda.current_stream(dev), []
        self.capture, self.capture_whole, self.captured, self.hooked = capture, capture_whole, [], None
        for name in self.OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name), 0))
        for owner, name, operand in self.LIBRARY + (self.CAPTURE_ONLY if capture else ()):
            monkeypatch.setattr(owner, name, self._wrap(name, getattr(owner, name), operand))
        for name in ("fork", "join"):                   # side_sync = "events": _TorchEvents does both
            monkeypatch.setattr(_streams._TorchEvents, name, self._wrap(name, getattr(_streams._TorchEvents, name), None))

    def note(self, name, rows):
        self.calls.append((name, rows, MAIN if torch.cuda.current_stream(self.dev) == self.main else SIDE))

    def _keep(self, v):
        if isinstance(v, torch.Tensor) and v.is_cuda and not _is_parameter(v):
            return v.detach().clone()
        return v

    def _whole(self, t):
        """The buffer `t` is a row range of, and its first row there; None when `t` is no row range of a matrix of its width."""
        base = t._base if t._is_view() else t
        if base is None or base.dtype != t.dtype or base.shape[-1] != t.shape[-1] or not base.is_contiguous() or not t.is_contiguous():
            return None
        return base.reshape(-1, t.shape[-1]), (t.storage_offset() - base.storage_offset()) // t.shape[-1]

    def _wrap(self, name, fn, operand):
        def recorded(*args, **kwargs):
            grab = self.capture and operand is not None
            if grab:
                before = [self._keep(a) for a in args], {k: self._keep(v) for k, v in kwargs.items()}
                target = kwargs.get("out")
                if name == "addmm_":
                    target = args[0]
                elif name == "skinny_linear_bf16":
                    target = args[3]
                elif name == "bias_layernorm_cls_linear_bf16":
                    target = args[8]
                whole = self._whole(target) if (target is not None and self.capture_whole) else None
                whole_before = whole[0].clone() if whole is not None else None
            out = fn(*args, **kwargs)                   # the call still runs; nothing below launches anything
            label, rows = name, None
            if name == "patchify_bf16":
                rows = out.shape[0]                     # the rows it makes (its input is the image batch)
            elif operand is not None:
                rows = args[operand].numel() // args[operand].shape[-1]
            if name == "skinny_linear_bf16":
                mode = args[4] if len(args) > 4 else kwargs.get("mode", 0)
                stats = args[6] if len(args) > 6 else kwargs.get("row_stats")
                label = f"skinny:{mode}" + ("+stats" if stats is not None else "")
            self.note(label, rows)
            if grab:
                result = [self._keep(t) for t in (out if isinstance(out, tuple) else (out,))]
                after_args = [self._keep(a) for a in args]      # operands a launch wrote besides its result (row_stats, out)
                self.captured.append(Call(label, rows, self.calls[-1][2], before[0], before[1], result, after_args,
                                          None if whole is None else (whole_before, whole[0].clone(), whole[1])))
            elif self.capture:
                self.captured.append(Call(label, rows, self.calls[-1][2], (), {}, [], [], None))
            return out
        return recorded

    def hook(self, cls_rows, main_raw, n):
        self.note("cls_tail_hook", cls_rows.shape[0])
        if self.capture:
            self.hooked = cls_rows.detach().clone()
            self.captured.append(Call("cls_tail_hook", cls_rows.shape[0], self.calls[-1][2], (), {}, [], [], None))


def _record(dev, monkeypatch, img_size, B=2, L=3, **switches):
    """-> (calls of one forward(split=True) after a warm-up forward, its SplitTokens)."""
    from vpr_amd.backbone import DinoV2
    torch.manual_seed(0)
    m = DinoV2("vit_small", img_size=img_size).to(dev).to(torch.bfloat16).eval()
    m.blocks = torch.nn.ModuleList(list(m.blocks)[:L])
    m.fold_layerscale()
    for name, value in switches.items():
        assert hasattr(m, name)
        setattr(m, name, value)
    x = torch.randn(B, 3, img_size, img_size, device=dev, dtype=torch.bfloat16)
    assert m._hip_split_ok(x) == (img_size == 224)
    rec = _Recorder(monkeypatch, dev)
    m.cls_tail_hook = rec.hook
    m(x, split=True)                                    # builds the cached constants
    rec.calls.clear()
    out = m(x, split=True)
    torch.cuda.synchronize()
    return rec.calls, out


def _on(stream, *calls):
    return [(name, rows, stream) for name, rows in calls]


# ---------------------------------------------------------------------------------------------- the annotated schedules
SWITCHES = {"split_side": {}, "split_after": {"cls_side_chain": False, "cls_after_gemm": True},
            "split_before": {"cls_side_chain": False, "cls_after_gemm": False},
            "fused": {"cls_side_chain": False, "fuse_ln_cls": True}, "cf_resid": {}, "cf_add": {"residual_in_gemm": False}}


def schedule(mode, B, n, L, gelu="tanh", hip_attention=True, fusable=True):
    """The launches of one forward as (label, rows, stream, block, stage, part), in issue order.  The same lists as the
    written-out expectations of tests/test_backbone_schedule_gpu.py, annotated."""
    Mp, M = B * n, B * n + B
    erf = gelu == "erf"
    out = []

    def add(stream, label, rows, block, stage, part):
        out.append((label, rows, stream, block, stage, part))

    def fc1(stream, i, part, rows):
        if part == CLS:
            add(stream, "skinny:4" if erf else "skinny:1", rows, i, "fc1", CLS)
        elif erf:
            add(stream, "addmm", rows, i, "fc1", part)
            add(stream, "gelu_", rows, i, "fc1", part)
        else:
            add(stream, "_addmm_activation", rows, i, "fc1", part)

    if mode in ob.CLS_FIRST_MODES:
        add(MAIN, "layernorm_bf16", M, -1, "ln_first", ALL)
        for i in range(L):
            add(MAIN, "linear", M, i, "qkv", ALL)
            if hip_attention:
                add(MAIN, "attention_qkv_bf16", M, i, "attention", ALL)
            else:
                add(MAIN, "scaled_dot_product_attention", None, i, "attention", ALL)
            for half, (a, ln) in enumerate((("proj_add", "ln2"), ("fc2_add", "ln_next"))):
                if mode == "cf_resid":
                    add(MAIN, "addmm_", M, i, a, ALL)
                    add(MAIN, "bias_layernorm_bf16", M, i, ln, ALL)
                else:
                    add(MAIN, "linear", M, i, a, ALL)
                    add(MAIN, "add_layernorm_bf16", M, i, ln, ALL)
                if half == 0:
                    fc1(MAIN, i, ALL, M)
        return out

    add(MAIN, "patchify_bf16", Mp, -1, "embed_patchify", ALL)
    add(MAIN, "mm", Mp, -1, "embed_gemm", PATCH)
    add(MAIN, "add_layernorm_bf16", M, -1, "embed_add_ln", ALL)
    gemm = {"qkv": ("addmm", "skinny:0"), "proj_add": ("addmm_", "skinny:2"), "fc2_add": ("addmm_", "skinny:2")}

    def one(stream, i, stage, part, stats=False):
        label = gemm[stage][part == CLS] + ("+stats" if stats else "")
        add(stream, label, Mp if part == PATCH else B, i, stage, part)

    if mode == "split_side":
        one(MAIN, 0, "qkv", PATCH)
        one(MAIN, 0, "qkv", CLS)
        for i in range(L):
            last = i == L - 1
            add(MAIN, "attention_qkv_split_bf16", M, i, "attention", ALL)
            add(MAIN, "fork", None, i, None, None)
            for stream, part, rows in ((SIDE, CLS, B), (MAIN, PATCH, Mp)):
                one(stream, i, "proj_add", part)
                add(stream, "bias_layernorm_bf16", rows, i, "ln2", part)
                fc1(stream, i, part, rows)
                one(stream, i, "fc2_add", part)
                add(stream, "bias_layernorm_bf16", rows, i, "ln_next", part)
                if not last:
                    one(stream, i + 1, "qkv", part)
                elif part == CLS:
                    add(SIDE, "cls_tail_hook", B, i, None, None)
            add(MAIN, "join", None, i, None, None)
        return out

    fuse = mode == "fused" and not erf and fusable
    order = (CLS, PATCH) if mode == "split_before" else (PATCH, CLS)
    for i in range(L):
        last = i == L - 1
        for part in order:
            if not (fuse and part == CLS and i > 0):
                one(MAIN, i, "qkv", part)
        add(MAIN, "attention_qkv_split_bf16", M, i, "attention", ALL)
        for part in order:
            one(MAIN, i, "proj_add", part, stats=fuse and part == CLS)
        add(MAIN, "bias_layernorm_cls_linear_bf16" if fuse else "bias_layernorm_bf16", M, i, "ln2", ALL)
        for part in order:
            if not (fuse and part == CLS):
                fc1(MAIN, i, part, Mp if part == PATCH else B)
        for part in order:
            one(MAIN, i, "fc2_add", part, stats=fuse and part == CLS and not last)
        add(MAIN, "bias_layernorm_cls_linear_bf16" if fuse and not last else "bias_layernorm_bf16", M, i, "ln_next", ALL)
    return out


def _cpu(t):
    return t.cpu() if isinstance(t, torch.Tensor) else t


def _stage(call, block, stage, part):
    """The oracle's record of one captured call: its operands by name."""
    a, kw, res, lab = call.args, call.kwargs, call.result, call.label
    scalars, ref, inp, out = {}, {}, {}, {}
    if lab == "patchify_bf16":
        inp, out, scalars = {"img": a[0]}, {"a": res[0]}, {"patch": a[1], "kpad": a[2], "lead_rows": a[3]}
    elif lab == "mm":
        inp, out, ref = {"a": a[0]}, {"y": res[0]}, {"w": a[1]}
    elif lab == "add_layernorm_bf16":
        inp, out, ref, scalars = {"x": a[0], "res": a[1]}, {"x": res[0], "h": res[1]}, {"gamma": a[2], "beta": a[3]}, {"eps": a[4]}
        if stage == "embed_add_ln":
            inp = {"raw": a[0], "off": a[1]}
    elif lab == "layernorm_bf16":
        inp, out, ref, scalars = {"x": a[0]}, {"h": res[0]}, {"gamma": a[1], "beta": a[2]}, {"eps": a[3]}
    elif lab in ("addmm", "_addmm_activation"):
        inp, out, ref, scalars = {"h": a[1]}, {"y": res[0]}, {"b": a[0], "w": a[2]}, {"gelu": kw.get("use_gelu", False)}
    elif lab == "linear":
        inp, out, ref = {"h" if stage == "qkv" else "a": a[0]}, {"y": res[0]}, {"w": a[1], "b": a[2]}
    elif lab == "gelu_":
        inp, out = {"y": a[0]}, {"y": res[0]}
    elif lab == "addmm_":
        inp, out, ref = {"x": a[0], "a": a[1]}, {"x": res[0]}, {"w": a[2]}
    elif lab.startswith("skinny:"):
        mode = int(lab[7])
        scalars, ref = {"mode": mode}, {"w": a[1], "b": a[2]}
        if mode == 2:
            inp, out = {"a": a[0], "x": a[3]}, {"x": res[0]}
            if lab.endswith("+stats"):
                inp["c"], out["row_stats"] = a[5], call.after_args[6]
        else:
            inp, out = {"h": a[0]}, {"y": res[0]}
    elif lab in ("attention_qkv_split_bf16", "attention_qkv_bf16"):
        inp, out = {"qkv": a[0]}, {"att": res[0]}
        scalars = dict(zip(("B", "T", "body_tokens", "heads"), a[1:])) if "split" in lab else {"heads": a[1]}
        lab = "attention"
    elif lab == "scaled_dot_product_attention":
        inp, out, lab = {"q": a[0], "k": a[1], "v": a[2]}, {"att": res[0]}, "sdpa"
    elif lab == "bias_layernorm_bf16":
        inp, out, ref, scalars = {"x": a[0], "c": a[1]}, {"h": res[0]}, {"gamma": a[2], "beta": a[3]}, {"eps": a[4]}
    elif lab == "bias_layernorm_cls_linear_bf16":
        inp, out = {"x": a[0], "c": a[1], "row_stats": a[6]}, {"h": res[0], "lin": call.after_args[8]}
        ref, scalars = {"gamma": a[2], "beta": a[3], "consts": a[7]}, {"eps": a[4], "cls_row0": a[5], "gelu": kw.get("gelu", False)}
    else:
        raise AssertionError(f"no stage form for {lab}")
    whole = None if call.whole is None else (call.whole[0].cpu(), call.whole[1].cpu(), call.whole[2])
    return ob.Stage(block, stage, part, lab, {k: _cpu(v) for k, v in inp.items()}, {k: _cpu(v) for k, v in out.items()},
                    scalars, ref, whole, call.stream)


def stage_records(captured, want):
    """Captured calls -> stage records, after checking them against the annotated schedule `want`."""
    got = [(c.label, c.rows, c.stream) for c in captured]
    for pos, (g, w) in enumerate(zip(got, want)):
        rows_ok = w[1] is None or g[1] == w[1]
        assert g[0] == w[0] and rows_ok and g[2] == w[2], f"launch {pos}: recorded {g}, the schedule has {w[:3]} ({w[3:]})"
    assert len(got) == len(want), f"{len(got)} launches recorded, the schedule has {len(want)}"
    return [_stage(c, *w[3:]) for c, w in zip(captured, want) if w[4] is not None]


# ------------------------------------------------------------------------------------------------------------ the model
def make_model(arch, img_size, L, seed=0, fold=True):
    """DinoV2 cut to its first L blocks (CPU, bf16, eval, LayerScale folded unless fold=False) with every parameter away from its init value
    and no two blocks, norms or bias rows alike: norm weights 1 + 0.3 N, norm / Linear / conv biases 0.5 N, LayerScale
    N(0, 0.3) before the fold, cls token 0.5 N, pos_embed a +-1 code plus noise, fc1 weights scaled to pre-activation
    std >= 1 (0.9 / sqrt(C) per weight on LayerNorm outputs of mean square ~ 1.3, plus the 0.5 N bias: a larger scale
    widens the f32 accumulation term of the fc1 bound until it hides the difference between the two GELU forms)."""
    from vpr_amd.backbone import DinoV2
    torch.manual_seed(seed)
    m = DinoV2(arch, img_size=img_size)
    m.blocks = torch.nn.ModuleList(list(m.blocks)[:L])
    g = torch.Generator().manual_seed(1000 + seed)
    C = m.embed_dim
    rn = lambda *s: torch.randn(*s, generator=g)
    with torch.no_grad():
        for norm in [b.norm1 for b in m.blocks] + [b.norm2 for b in m.blocks] + [m.norm]:
            norm.weight.copy_(1 + 0.3 * rn(C))
            norm.bias.copy_(0.5 * rn(C))
        for b in m.blocks:
            for lin in (b.qkv, b.proj, b.fc1, b.fc2):
                lin.bias.copy_(0.5 * rn(lin.bias.shape[0]))
            b.fc1.weight.copy_(0.9 * C ** -0.5 * rn(*b.fc1.weight.shape))
            b.ls1.copy_(0.3 * rn(C))
            b.ls2.copy_(0.3 * rn(C))
        m.patch_embed.bias.copy_(0.5 * rn(C))
        m.cls_token.copy_(0.5 * rn(1, 1, C))
        T = 1 + m.num_patches
        m.pos_embed.copy_(((torch.randint(0, 2, (T, C), generator=g) * 2 - 1).float() + 0.02 * rn(T, C)).unsqueeze(0))
    m = m.to(torch.bfloat16).eval()
    if fold:
        m.fold_layerscale()
    return m


def make_image(B, img_size, seed=0):
    return torch.randn(B, 3, img_size, img_size, generator=torch.Generator().manual_seed(77 + seed)).to(torch.bfloat16)


def trace(m, x, mode, monkeypatch, gelu="tanh"):
    """One captured forward of GPU model `m` on images `x` in `mode` (after whatever forwards the caller already ran) ->
    oracle.backbone.Trace, everything on the CPU."""
    from vpr_amd.backbone import _hip_attention_ok
    dev = x.device
    for name, value in {"cls_side_chain": True, "cls_after_gemm": True, "fuse_ln_cls": False, "residual_in_gemm": True,
                        **SWITCHES[mode]}.items():
        assert hasattr(m, name)
        setattr(m, name, value)
    m.gelu = gelu
    split = mode in ob.SPLIT_MODES
    assert m._hip_split_ok(x) == split
    B, n, C = x.shape[0], m.num_patches, m.embed_dim
    with monkeypatch.context() as mp:
        rec = _Recorder(mp, dev, capture=True, capture_whole=mode != "split_side")
        m.cls_tail_hook = rec.hook
        try:
            out = m(x, split=split)
            torch.cuda.synchronize()
        finally:
            m.cls_tail_hook = None
    want = schedule(mode, B, n, len(m.blocks), gelu, _hip_attention_ok(C // m.blocks[0].heads, 1 + n), C % 32 == 0)
    stages = stage_records(rec.captured, want)
    tr = ob.Trace(stages, B, n)
    with torch.no_grad():
        if mode != "cf_add":
            tr.cum = m._cumulative_bias(dev).cpu()
        if split:
            tr.embed = tuple(t.cpu() for t in m._embed_consts(x))
            tr.result = (out.patch.reshape(B * n, C).cpu(), out.cls.cpu())
            assert out.token_ready == (mode == "split_side")
        else:
            tr.result = out.reshape(-1, C).cpu()
        if mode == "fused" and gelu == "tanh" and C % 32 == 0:
            tr.fused = [None if k is None else tuple(t.cpu() for t in k) for k in m._cls_fused_consts(dev)]
    tr.hook = None if rec.hooked is None else rec.hooked.cpu()
    torch.cuda.synchronize()
    return tr
