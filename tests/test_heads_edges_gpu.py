"""Pose heads (vpr_pose_head, vpr_pose_head_split, vpr_pose_head_fused in both its forms, the linear head) and
vpr_ln_meanpool_head against the f64 oracle at the shapes where csrc/pose_head.hip changes behaviour.

Every comparison is per element: |out - f64| <= oracle.heads.mlp_head_bound / ln_meanpool_bound (derived there from
u = 2^-24 and the split forms' documented 2^-16 per product), never one max-abs number over the output; on
oracle.heads.exact_head_operands every form must return the f64 result bit for bit.  The CPU self-checks
(tests/test_oracle_selfchecks.py) show that the same bounds, on the same inputs, reject a dead lo plane, a dropped K-step,
a bias applied after the ReLU and a slab added twice.

Forms: "counters" VPR_POSE_VARIANT=1 + fused=True (one launch, arrival counters); "frag" fused=True (fragment-order planes
+ epilogue launch); "split" the default; "split8" the split form with eight waves (VPR_POSE_VARIANT=8); "f32" split=False
(exact-f32 MFMA, hidden % 32 == 0 only)."""
import pytest
import torch

from oracle import heads as oheads

pytestmark = pytest.mark.gpu

SPLIT_FORMS = ("counters", "frag", "split")
EPS = 1e-5


def _set_form(tune, form):
    tune("VPR_POSE_VARIANT", {"counters": 1, "split8": 8}.get(form))


def _run(dev, tune, form, ops_args, off=-1):
    from vpr_amd import ops
    _set_form(tune, form)
    return ops.pose_head(*ops_args, off, split=form != "f32", fused=form in ("counters", "frag"))


def _slices(form, B, D, hidden):
    """Upper bound of the slab count of a form at this shape (exact when B * hidden * 4 is a multiple of 256), read from the
    library's own workspace queries under the switches that are set now."""
    from vpr_amd import _lib
    L = _lib.lib()
    nbytes = L.vpr_pose_head_workspace_bytes(B, D, hidden, 1) if form == "f32" else L.vpr_pose_head_split_workspace_bytes(B, D, hidden)
    return -(-nbytes // (B * hidden * 4))


def _to(dev, ts):
    return [None if t is None else t.to(dev) for t in ts]


def _check(out, ops_cpu, form, off, slices, what):
    """Per-element bound; prints and returns the worst err / bound."""
    x, W1, b1, W2, b2 = ops_cpu
    ref = oheads.mlp_head(x, W1, b1, W2, b2, off)
    bound = oheads.mlp_head_bound(x, W1, b1, W2, b2, form != "f32", off, slices)
    assert torch.isfinite(bound).all(), what
    err = (out.cpu().double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"pose head {form:8s} {what}: worst err/bound {ratio:.4f} (max err {err.max().item():.2e})")
    assert ratio <= 1.0, f"{form} {what}: worst err/bound {ratio:.3f}, max err {err.max().item():.3e}"
    return ratio


# ------------------------------------------------------------------------------------------------ split-form K edges
@pytest.mark.parametrize("case", oheads.SPLIT_K_EDGE_CASES, ids=lambda c: f"B{c[0]}-D{c[1]}-ks{c[5]}")
def test_split_forms_at_k_edges(dev, tune, case):
    """hidden = 16.  D = 32: one K-step, three of four waves idle; D = 96; D = 224: seven steps (the single-step tail loop);
    D = 544: 17 steps in two uneven slices; D = 128 with VPR_POSE_KS=3: the third slice is empty.  The eight-wave kernel
    (VPR_POSE_VARIANT=8) at D = 32 and D = 224."""
    B, D, hidden, n_out, off, ks = case
    cpu = oheads.head_case_inputs(B, D, hidden, n_out, 1000 + D, off)
    args = _to(dev, cpu)
    tune("VPR_POSE_KS", ks)
    forms = SPLIT_FORMS + (("split8",) if D in (32, 224) else ())
    for form in forms:
        _set_form(tune, form)
        slices = _slices(form, B, D, hidden)
        assert slices >= oheads.split_case_slices(D, ks)
        _check(_run(dev, tune, form, args, off), cpu, form, off, oheads.split_case_slices(D, ks), f"D={D} ks={ks}")


@pytest.mark.parametrize("ks", [17, 33])
def test_split_forms_with_more_than_16_slabs(dev, tune, ks):
    """D = 1056 (33 K-steps) forced into 17 slices (16 of two steps + one of one) and 33 (one step each): the epilogue
    kernels request slabs in groups of 16 and the counter form in groups of 8, with a clamped ragged last group."""
    B, D, hidden, n_out, off = 2, 1056, 16, 4, 2
    cpu = oheads.head_case_inputs(B, D, hidden, n_out, 2000 + ks, off)
    args = _to(dev, cpu)
    tune("VPR_POSE_KS", ks)
    for form in SPLIT_FORMS + ("split8",):
        _check(_run(dev, tune, form, args, off), cpu, form, off, ks, f"D={D} ks={ks}")


# ------------------------------------------------------------------------------------------------ exact-f32 path
@pytest.mark.parametrize("D", [16, 208, 400])
@pytest.mark.parametrize("hidden", [32, 96])
def test_exact_f32_path_at_load_ahead_edges(dev, tune, D, hidden):
    """D / 16 = 1, 13 and 25 K-steps against the PH_CH = 12 load-ahead chunks (ragged tails of 1 step), ragged batch tiles."""
    for B in (3, 66):
        cpu = oheads.head_case_inputs(B, D, hidden, 4, 3000 + D + hidden + B, 1)
        _check(_run(dev, tune, "f32", _to(dev, cpu), 1), cpu, "f32", 1, _slices("f32", B, D, hidden), f"B={B} D={D} hidden={hidden}")


@pytest.mark.parametrize("D,above16", [(1056, False), (2176, True)])
def test_exact_f32_path_epilogue_request_groups(dev, tune, D, above16):
    """The epilogue requests slabs in groups of 16: a slab count that is not a multiple of 16 (D = 1056) and one above 16.
    vpr_pose_head keeps at least 8 K-steps of 16 per slice, so more than 16 slabs need D >= 2176 (B = 2, hidden = 32: 17
    slabs of 139 KB in all); below that the groups above 16 are exercised through the split forms
    (test_split_forms_with_more_than_16_slabs: the same epilogue kernel).  The count is read from the workspace query."""
    B, hidden = 2, 32                       # B * hidden * 4 = 256: the query's rounding to 256 bytes leaves the count exact
    slices = _slices("f32", B, D, hidden)
    assert slices % 16 != 0 and (slices > 16) == above16, slices
    cpu = oheads.head_case_inputs(B, D, hidden, 8, 3100 + D, 6)
    _check(_run(dev, tune, "f32", _to(dev, cpu), 6), cpu, "f32", 6, slices, f"D={D} slices={slices}")


# ------------------------------------------------------------------------------------------------ ragged tiles
@pytest.mark.parametrize("hidden", [16, 48, 80, 208, 32, 96])
def test_ragged_batch_and_hidden_tiles(dev, tune, hidden):
    """B around the 64-row tile with hidden that is no multiple of 64 (split and fragment forms: masked rows and columns of
    the last tiles) and the exact-f32 form at its own widths (hidden % 32 == 0)."""
    D = 96
    forms = ("f32",) + SPLIT_FORMS if hidden % 32 == 0 else SPLIT_FORMS
    for B in (1, 63, 64, 65, 130):
        cpu = oheads.head_case_inputs(B, D, hidden, 3, 4000 + B + hidden, 0)
        args = _to(dev, cpu)
        for form in forms:
            _set_form(tune, form)
            _check(_run(dev, tune, form, args, 0), cpu, form, 0, 1, f"B={B} hidden={hidden}")


def test_split_entry_point_writes_every_slab_it_reads(dev, tune):
    """vpr_pose_head_split called directly on a deliberately oversized workspace filled with NaN: a slab (or a masked row or
    column of one) the first layer leaves unwritten and the epilogue reads would show as NaN in the output."""
    from vpr_amd import _lib, ops
    tune("VPR_POSE_VARIANT", None)
    L = _lib.lib()
    for B, D, hidden, ks in ((65, 96, 48, None), (130, 544, 80, None), (5, 128, 16, 3)):
        tune("VPR_POSE_KS", ks)
        cpu = oheads.head_case_inputs(B, D, hidden, 4, 5000 + B, 2)
        x, W1, b1, W2, b2 = _to(dev, cpu)
        hi, lo = ops._pack_w1_planes(W1, False)
        need = L.vpr_pose_head_split_workspace_bytes(B, D, hidden)
        ws = torch.full((need // 4 + 4096,), float("nan"), dtype=torch.float32, device=dev)
        out = torch.full((B, 4), float("nan"), dtype=torch.float32, device=dev)
        st = L.vpr_pose_head_split(ops._ptr(x), ops._ptr(hi), ops._ptr(lo), ops._ptr(b1), ops._ptr(W2), ops._ptr(b2), ops._ptr(out),
                                   B, D, hidden, 4, 2, ops._ptr(ws), ws.numel() * 4, ops._stream())
        assert st == 0
        _check(out, cpu, "split", 2, oheads.split_case_slices(D, ks), f"direct B={B} D={D} hidden={hidden}")
        assert torch.equal(out, ops.pose_head(x, W1, b1, W2, b2, 2))
        assert bool(torch.isnan(ws[-4096:]).all())                     # nothing written past the slabs


@pytest.mark.parametrize("variant", [None, 1], ids=["frag", "counters"])
def test_fused_entry_point_writes_every_slab_it_reads(dev, tune, variant):
    """The same for vpr_pose_head_fused in both of its forms, on the tile-contiguous slabs: the counter area at the head of
    the workspace zero, everything after it NaN.  One writer (the first-layer kernel) and two readers (the epilogue launch,
    the arrival-counter finisher) have to agree on the tile layout; the counters are left zero and nothing is written past
    the workspace the query asks for."""
    from vpr_amd import _lib, ops
    L = _lib.lib()
    form = "counters" if variant == 1 else "frag"
    for B, D, hidden, ks in ((65, 96, 48, None), (130, 544, 80, None), (5, 128, 16, 3)):
        tune("VPR_POSE_VARIANT", variant)
        tune("VPR_POSE_KS", ks)
        cpu = oheads.head_case_inputs(B, D, hidden, 4, 5000 + B, 2)
        x, W1, b1, W2, b2 = _to(dev, cpu)
        hi, lo = ops._pack_w1_planes(W1, True)
        need, cnt = L.vpr_pose_head_fused_workspace_bytes(B, D, hidden), L.vpr_pose_head_fused_counter_bytes(B, D, hidden)
        assert 0 < cnt < need and cnt % 4 == 0 and need % 4 == 0
        ws = torch.full((need // 4 + 4096,), float("nan"), dtype=torch.float32, device=dev)
        ws[:cnt // 4].view(torch.int32).zero_()
        out = torch.full((B, 4), float("nan"), dtype=torch.float32, device=dev)
        st = L.vpr_pose_head_fused(ops._ptr(x), ops._ptr(hi), ops._ptr(lo), ops._ptr(b1), ops._ptr(W2), ops._ptr(b2), ops._ptr(out),
                                   B, D, hidden, 4, 2, ops._ptr(ws), ws.numel() * 4, ops._stream())
        assert st == 0
        _check(out, cpu, form, 2, oheads.split_case_slices(D, ks), f"direct fused B={B} D={D} hidden={hidden}")
        assert torch.equal(out, ops.pose_head(x, W1, b1, W2, b2, 2, fused=True))
        assert bool(torch.isnan(ws[-4096:]).all())                     # nothing written past the workspace
        assert int(ws[:cnt // 4].view(torch.int32).abs().sum()) == 0   # the counters are zero again


@pytest.mark.parametrize("B,D,hidden,ks", [(65, 544, 80, None), (130, 96, 208, None), (5, 128, 16, 3), (2, 1056, 16, 17)])
def test_fragment_order_form_gives_the_bits_of_the_split_form(dev, tune, B, D, hidden, ks):
    """"frag" and "split" run the same first-layer routine (slice count, per-wave K partition, MFMA order, four-way sum) and
    the same epilogue; they differ in where a weight fragment is read and where a finished block is stored, so their outputs
    are the same bits.  ("split8" and "counters" add in other orders.)"""
    args = _to(dev, oheads.head_case_inputs(B, D, hidden, 4, 5500 + B, 2))
    tune("VPR_POSE_KS", ks)
    assert torch.equal(_run(dev, tune, "frag", args, 2), _run(dev, tune, "split", args, 2))


# ------------------------------------------------------------------------------------------------ outputs and the pair
@pytest.mark.parametrize("n_out", range(1, 9))
def test_n_out_and_pair_offsets(dev, tune, n_out):
    """n_out 1..8 with sincos_offset in {-1, 0, n_out - 2}: the pair within its bound, every other column bit-identical to
    the run without a normalise."""
    for form, hidden in (("counters", 48), ("frag", 48), ("split", 48), ("f32", 32), ("linear", 0)):
        B, D = 5, 96
        offs = [-1] + ([0, n_out - 2] if n_out >= 2 else [])
        cpu = oheads.head_case_inputs(B, D, hidden, n_out, 6000 + n_out, max(offs))
        if max(offs) > 0:
            cpu[4][0], cpu[4][1] = 1.5, -2.0                               # the pair at offset 0 far from the origin as well
        args = _to(dev, cpu)
        run = (lambda off: _run(dev, tune, "split", args, off)) if form == "linear" else (lambda off: _run(dev, tune, form, args, off))
        kform = "f32" if form == "linear" else form
        plain = run(-1)
        _check(plain, cpu, kform, -1, 1, f"{form} n_out={n_out}")
        for off in offs[1:]:
            out = run(off)
            _check(out, cpu, kform, off, 1, f"{form} n_out={n_out} off={off}")
            keep = [c for c in range(n_out) if c not in (off, off + 1)]
            assert torch.equal(out[:, keep], plain[:, keep]), (form, n_out, off)
            assert (out[:, off:off + 2].double().norm(dim=1) - 1).abs().max().item() < 1e-6


def test_pair_offset_without_a_pair_is_refused(dev, tune):
    """sincos_offset >= 0 needs sincos_offset + 2 <= n_out (include/vpr_amd.h): the wrappers raise, the five entry points
    return VPR_ERR_INVALID_ARG and write nothing."""
    from vpr_amd import _lib, ops
    L = _lib.lib()
    B, D, hidden, n_out = 3, 64, 32, 3
    cpu = oheads.head_case_inputs(B, D, hidden, n_out, 1)
    x, W1, b1, W2, b2 = _to(dev, cpu)
    for off in (n_out - 1, n_out, 8):
        for form in SPLIT_FORMS + ("f32",):
            with pytest.raises(RuntimeError):
                _run(dev, tune, form, (x, W1, b1, W2, b2), off)
        with pytest.raises(RuntimeError):
            ops.pose_head(x, None, None, W1[:n_out].contiguous(), b2, off)
        with pytest.raises(RuntimeError):
            ops.ln_meanpool_head(torch.zeros(1, 4, 512, device=dev), torch.ones(512, device=dev), torch.zeros(512, device=dev), EPS,
                                 torch.zeros(n_out, 512, device=dev), b2, off)
    tune("VPR_POSE_VARIANT", None)
    off = n_out - 1
    out = torch.full((B, n_out), 7.0, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    p, s = ops._ptr, ops._stream()
    hi, lo = ops._pack_w1_planes(W1, False)
    fhi, flo = ops._pack_w1_planes(W1, True)
    assert L.vpr_pose_head(p(x), p(W1), p(b1), p(W2), p(b2), p(out), B, D, hidden, n_out, off, p(ws), ws.numel(), s) == -1
    assert L.vpr_pose_head(p(x), None, None, p(W1), p(b2), p(out), B, D, 0, n_out, off, p(ws), ws.numel(), s) == -1
    assert L.vpr_pose_head_split(p(x), p(hi), p(lo), p(b1), p(W2), p(b2), p(out), B, D, hidden, n_out, off, p(ws), ws.numel(), s) == -1
    assert L.vpr_pose_head_fused(p(x), p(fhi), p(flo), p(b1), p(W2), p(b2), p(out), B, D, hidden, n_out, off, p(ws), ws.numel(), s) == -1
    xs, gm = torch.zeros(B, 4, 512, device=dev), torch.ones(512, device=dev)
    Wh = torch.zeros(n_out, 512, device=dev)
    assert L.vpr_ln_meanpool_head(p(xs), 0, B, 4, 512, p(gm), p(gm), EPS, None, p(Wh), p(b2), n_out, off, p(out), s) == -1
    # without a head the offset is not looked at; the last valid offset is accepted
    pooled = torch.empty(B, 512, device=dev)
    assert L.vpr_ln_meanpool_head(p(xs), 0, B, 4, 512, p(gm), p(gm), EPS, p(pooled), None, None, 0, 5, None, s) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert L.vpr_pose_head(p(x), p(W1), p(b1), p(W2), p(b2), p(out), B, D, hidden, n_out, n_out - 2, p(ws), ws.numel(), s) == 0


# ------------------------------------------------------------------------------------------------ exact operands
def _exact_cases():
    return [("kinds", 65, 224, 48, None), ("kinds", 3, 32, 16, None), ("kinds", 4, 128, 16, 3), ("kinds", 2, 1056, 16, 17), ("kinds", 2, 1056, 16, 33),
            ("kinds", 66, 416, 96, None), ("dead", 65, 224, 48, None), ("dead", 3, 224, 32, None),
            ("negzero", 65, 224, 48, None), ("negzero", 3, 224, 32, None)]


@pytest.mark.parametrize("kind,B,D,hidden,ks", _exact_cases())
def test_exact_operands_give_f64_bits_in_every_form(dev, tune, kind, B, D, hidden, ks):
    """On exact operands every form, slab count and wave count returns the f64 result (an f32 value) bit for bit before the
    normalise.  kinds: positive, dead, exactly-zero-in-row-0 and exactly-zero-everywhere hidden units side by side;
    dead: every unit dead, out == b2 exactly; negzero: the zeros of x are -0.0."""
    n_out = 4
    x, W1, b1, W2, b2 = oheads.exact_head_operands(B, D, hidden, n_out, 8000 + D)
    if kind == "dead":
        b1 = -((x.abs().double() @ W1.abs().double().T).amax(0) + 1).float()
    if kind == "negzero":
        assert (x == 0).any()
        x = torch.where(x == 0, torch.tensor(-0.0), x)
        assert torch.signbit(x[x == 0]).all()
    ref = oheads.mlp_head(x, W1, b1, W2, b2)
    assert torch.equal(ref.float().double(), ref)
    if kind == "dead":
        assert torch.equal(ref, b2.double().expand(B, n_out))
    args = _to(dev, (x, W1, b1, W2, b2))
    tune("VPR_POSE_KS", ks)
    forms = SPLIT_FORMS + ("split8",) + (("f32",) if D % 16 == 0 and hidden % 32 == 0 else ())
    for form in forms:
        out = _run(dev, tune, form, args).cpu()
        assert torch.equal(out.double(), ref), (form, (out.double() - ref).abs().max().item())


# ------------------------------------------------------------------------------------------------ isolation
def test_rows_past_b_and_a_shared_workspace_change_no_bits(dev, tune):
    """x is the head of a larger parent buffer whose later rows are NaN (the kernels clamp row indices, never read past B);
    and the same shapes called back to back on the one cached workspace, after a larger shape has filled it, repeat their bits."""
    shapes = ((1, 96, 48), (63, 224, 80), (65, 544, 16), (3, 416, 32))
    first = {}
    for rnd in range(2):
        for B, D, hidden in shapes:
            cpu = oheads.head_case_inputs(B, D, hidden, 4, 9000 + B, 2)
            x, W1, b1, W2, b2 = _to(dev, cpu)
            parent = torch.full((B + 70, D), float("nan"), device=dev)
            parent[:B] = x
            for form in SPLIT_FORMS + (("f32",) if hidden % 32 == 0 else ()):
                out = _run(dev, tune, form, (parent[:B], W1, b1, W2, b2), 2)
                if rnd == 0:
                    first[(B, form)] = out.clone()
                    assert torch.equal(out, _run(dev, tune, form, (x, W1, b1, W2, b2), 2)), (B, form)
                    _check(out, cpu, form, 2, 3, f"isolation B={B}")       # at most 3 slabs at these shapes
                else:
                    assert torch.equal(out, first[(B, form)]), (B, form)
        if rnd == 0:                                   # a larger shape passes through the same workspaces
            big = _to(dev, oheads.head_case_inputs(130, 1056, 192, 4, 9999, 2))
            for form in SPLIT_FORMS + ("f32",):
                assert torch.isfinite(_run(dev, tune, form, big, 2)).all()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ linear head
@pytest.mark.parametrize("D", [1, 255, 256, 257])
def test_linear_head_at_block_stride_edges(dev, D):
    """hidden == 0 with D around the 256-thread block stride, n_out = 8.  D = 1, 255 and 257 are no multiples of 16: the linear
    branch has no such requirement (it returns before the MLP forms' D % 16 check)."""
    from vpr_amd import ops
    B, n_out = 5, 8
    for off in (-1, 6):
        cpu = oheads.head_case_inputs(B, D, 0, n_out, 7000 + D, off)
        out = ops.pose_head(*_to(dev, cpu), off)
        _check(out, cpu, "f32", off, 1, f"linear D={D} off={off}")
    x, _, _, W2, b2 = oheads.exact_head_operands(B, D, 0, n_out, 7100 + D)
    ref = oheads.mlp_head(x, None, None, W2, b2)
    out = ops.pose_head(x.to(dev), None, None, W2.to(dev), b2.to(dev)).cpu()
    assert torch.equal(out.double(), ref)


# ------------------------------------------------------------------------------------------------ vpr_ln_meanpool_head
T_SWEEP = {512: (1, 15, 16, 17, 63, 64, 65, 129), 768: (1, 15, 16, 17, 63, 64, 65, 129), 1024: (1, 15, 16, 17, 63, 64, 65, 129),
           1536: (31, 32, 33)}       # the token loop turns at 16 * TB tokens: 64 for H <= 1024, 32 for H = 1536


def _ln_params(H, g, n_out=4):
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    Wh = (torch.rand(n_out, H, generator=g) * 2 - 1) / H ** 0.5
    bh = (torch.rand(n_out, generator=g) * 2 - 1) / H ** 0.5
    return gamma, beta, Wh, bh


def _ln_check(dev, x, gamma, beta, Wh, bh, off, what):
    """Full call against the bounds + the pooled-only call gives the same bits.  Returns (pooled, out) on the device."""
    from vpr_amd import ops
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    pooled_ref, out_ref = oheads.ln_meanpool_head(x, gamma, beta, EPS, Wh, bh, off)
    pb, ob = oheads.ln_meanpool_bound(x, gamma, beta, EPS, Wh, bh, off)
    pooled, out = ops.ln_meanpool_head(xd, gd, bd, EPS, None if Wh is None else Wh.to(dev), None if bh is None else bh.to(dev), off)
    rp = ((pooled.cpu().double() - pooled_ref).abs() / pb).max().item()
    ro = ((out.cpu().double() - out_ref).abs() / ob).max().item() if Wh is not None else 0.0
    print(f"ln_meanpool {what}: worst err/bound pooled {rp:.4f} head {ro:.4f}")
    assert rp <= 1.0 and ro <= 1.0, (what, rp, ro)
    if Wh is not None:
        # the head stage by itself, on the pooled vector the kernel returned: the bound above carries the pooled bound through
        # sum_j |Wh_oj| in the worst case (H terms of one sign) and is loose for the head; this one has only the head's own
        # 32 roundings (oracle.heads.ln_meanpool_bound) and the pair normalise
        pk, Whd, bhd = pooled.cpu().double(), Wh.double(), bh.double()
        raw = pk @ Whd.T + bhd
        sb = oheads.normalized_pair_bound(raw, 32 * oheads.U * (pk.abs() @ Whd.abs().T + bhd.abs()), off)
        rs = ((out.cpu().double() - oheads._normalize_pair(raw, off)).abs() / sb).max().item()
        print(f"ln_meanpool {what}: head stage on the kernel's pooled vector, worst err/bound {rs:.4f}")
        assert rs <= 1.0, (what, rs)
    pooled_only, none = ops.ln_meanpool_head(xd, gd, bd, EPS)
    assert none is None and torch.equal(pooled_only, pooled), what
    return pooled, out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [512, 768, 1024, 1536])
def test_ln_meanpool_token_counts(dev, H, dtype):
    g = torch.Generator().manual_seed(H)
    gamma, beta, Wh, bh = _ln_params(H, g)
    bh[2], bh[3] = 1.5, -2.0
    for T in T_SWEEP[H]:
        x = oheads.ln_case_rows("unit", 2, T, H, g).to(dtype)
        _ln_check(dev, x, gamma, beta, Wh, bh, 2, f"H={H} T={T} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["offset1000", "alternating", "constant"])
def test_ln_meanpool_edge_rows(dev, kind, dtype):
    """Rows 1000 + N(0, 1) (one-pass statistics lose the variance), one image whose tokens alternate between two scales
    (a mean over the wrong token count shows), and constant rows: var = 0 and, with a bf16-representable beta (its T-fold
    sums are exact), pooled == beta exactly."""
    for H, T in ((512, 17), (1024, 65), (1536, 33)):
        g = torch.Generator().manual_seed(H + T)
        gamma, beta, Wh, bh = _ln_params(H, g)
        bh[2], bh[3] = 1.5, -2.0
        if kind == "constant":
            beta = beta.to(torch.bfloat16).float()
        x = oheads.ln_case_rows(kind, 2, T, H, g).to(dtype)
        pooled, _ = _ln_check(dev, x, gamma, beta, Wh, bh, 2, f"{kind} H={H} T={T} {dtype}")
        if kind == "constant":
            assert torch.equal(pooled.cpu(), beta.expand(2, H)), (H, T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ln_meanpool_nan_image_stays_in_its_image(dev, dtype):
    """Image 0 all NaN: image 1's pooled vector and head output are the bits of image 1 run alone."""
    from vpr_amd import ops
    for H, T in ((768, 17), (1536, 33)):
        g = torch.Generator().manual_seed(T)
        gamma, beta, Wh, bh = (t.to(dev) for t in _ln_params(H, g))
        x = oheads.ln_case_rows("unit", 2, T, H, g).to(dtype)
        x[0] = float("nan")
        pooled, out = ops.ln_meanpool_head(x.to(dev), gamma, beta, EPS, Wh, bh, 2)
        alone_p, alone_o = ops.ln_meanpool_head(x[1:].contiguous().to(dev), gamma, beta, EPS, Wh, bh, 2)
        assert torch.isnan(pooled[0]).all() and torch.isnan(out[0]).all()
        assert torch.equal(pooled[1:], alone_p) and torch.equal(out[1:], alone_o)


@pytest.mark.parametrize("n_out,off", [(0, -1), (1, -1), (8, -1), (8, 0), (8, 6), (2, 0)])
def test_ln_meanpool_head_outputs(dev, n_out, off):
    H, T = 768, 65
    g = torch.Generator().manual_seed(n_out * 10 + off + 1)
    gamma, beta, Wh, bh = _ln_params(H, g, max(n_out, 1))
    if off >= 0:
        bh[off], bh[off + 1] = 1.5, -2.0
    x = oheads.ln_case_rows("unit", 2, T, H, g)
    if n_out == 0:
        _ln_check(dev, x, gamma, beta, None, None, -1, "n_out=0")
        return
    _, out = _ln_check(dev, x, gamma, beta, Wh, bh, off, f"n_out={n_out} off={off}")
    if off >= 0:
        _, plain = _ln_check(dev, x, gamma, beta, Wh, bh, -1, f"n_out={n_out}")
        keep = [c for c in range(n_out) if c not in (off, off + 1)]
        assert torch.equal(out[:, keep], plain[:, keep])
