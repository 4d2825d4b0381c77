"""GPU: what SALAD's MLP stages leave in the workspace — the partial-sum slabs of the cluster scores S and features F
(gemm256_fuse2_kernel, or gemm256 + the grouped second layers on the unfused route), the hidden activations H (unfused
route) and the token features g (skinny_linear_kernel x2) — element by element against the f64 stage oracle
(oracle/salad_stages.py), read through ops.salad_stage_views (include/vpr_amd_salad_stages.h).

The descriptor-level tests cannot see these stages: Sinkhorn and three normalisations sit between them and the 1e-4 bound,
and a per-cluster constant in S — the whole of b2_s — cancels exactly.  Three kinds of check:
  * exact-arithmetic inputs (oracle.salad_stages.exact_inputs; preconditions asserted on the CPU in
    tests/test_oracle_selfchecks.py): f32 arithmetic is exact in any order, so torch.equal with f64, no tolerance;
  * Gaussian inputs: a per-element bound computed from the inputs (stage_error_bounds) and the RMS error against that of a
    plain f32 restatement on the CPU;
  * the views are what stage A consumes: slabs summed + the public Sinkhorn stage = the one-call descriptor.
"""
import functools
import importlib.util
import os

import pytest
import torch

from oracle import salad_stages as ost

pytestmark = pytest.mark.gpu
N, M, L, T, HID = 256, 64, 128, 256, 512
COUNTERS = 4096                # head of the workspace: arrival counters, zero by contract — never poisoned below

_spec = importlib.util.spec_from_file_location("_salad_dropout_cpu", os.path.join(os.path.dirname(__file__), "test_salad_dropout_cpu.py"))
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)
salad_mask = _cpu.salad_mask


@functools.lru_cache(maxsize=None)
def _exact_inputs(C, B):
    return ost.exact_inputs(C, B, seed=100 * C + B)


@functools.lru_cache(maxsize=None)
def _exact(C, B):
    """Exact-arithmetic inputs and their f64 stage outputs, computed once per shape and shared (read-only)."""
    tokens, w = _exact_inputs(C, B)
    return tokens, w, ost.salad_stage_outputs(tokens, w)


def _to_dev(w, dev, dustbin=1.0):
    from vpr_amd.ops import SaladWeights
    return SaladWeights(**{k: v.to(dev) for k, v in w.items()}, dustbin=dustbin)


def _aggregate(td, wd, layout):
    from vpr_amd import ops
    if layout == "hub":                                      # cls first: image stride 257 C, patch rows offset by C
        return ops.salad_aggregate(td, wd, 3)[0]
    return ops.salad_aggregate_split(td[:, 1:].contiguous(), td[:, 0].contiguous(), wd, 3)[0]


def _views(dev, B, wd, poison=False):
    """CPU copies of the stage views of the current stream's SALAD workspace.  poison: fill everything behind the counter
    area with 0xFF bytes (f32 / bf16 NaN) instead — whatever a later run does not write shows."""
    from vpr_amd import ops
    ws = ops.workspace("salad", 256, dev)
    if poison:
        ws[COUNTERS:].fill_(0xFF)
        return None
    v = ops.salad_stage_views(ws, B, N, wd)
    return {k: getattr(v, k).cpu() for k in ("S", "F", "g")} | {"H": None if v.H is None else v.H.cpu()}


def _assert_stage_bits(v, o, fused, what=""):
    """Every element of the views equals the f64 oracle `o` (salad_stage_outputs) exactly."""
    eq = lambda a, b: torch.equal(a.double(), b)
    assert v["S"].shape == ((2 if fused else 1), o["S"].shape[1], M) and v["F"].shape == ((2 if fused else 1), o["F"].shape[1], L)
    if fused:                                                # per-slab contract: slab 0 = b2 + first 256 hidden columns, slab 1 the rest
        assert v["H"] is None
        for key in ("S", "F"):
            for s in (0, 1):
                bad = (v[key][s].double() != o[key][s]).sum().item()
                assert bad == 0, f"{what}{key} slab {s}: {bad} of {o[key][s].numel()} elements differ from f64"
            assert eq(v[key][0] + v[key][1], o[key].sum(0)), f"{what}{key}: slab sum"
    else:
        for key in ("S", "F"):
            bad = (v[key][0].double() != o[key].sum(0)).sum().item()
            assert bad == 0, f"{what}{key}: {bad} of {o[key][0].numel()} elements differ from f64"
        assert v["H"].dtype == torch.bfloat16 and eq(v["H"], o["H"]), f"{what}H != bf16(relu(z))"
    assert eq(v["g"], o["g"]), f"{what}g"


def _run_exact(dev, C, B, layout, fused, o=None, run=None):
    """One exact case with the stability protocol: poisoned workspace -> run -> run again on the same workspace -> a batch of
    another size (its layout differs) -> run again.  All three leave the oracle's bits."""
    tokens, w, ref = _exact(C, B)
    o = ref if o is None else o
    td, wd = tokens.to(dev), _to_dev(w, dev)
    run = run or (lambda: _aggregate(td, wd, layout))
    other_tok, other_w = _exact_inputs(C, B + 1 if B < 8 else B - 2)
    other_td, other_wd = other_tok.to(dev), _to_dev(other_w, dev)
    _views(dev, B, wd, poison=True)
    d1 = run()
    first = _views(dev, B, wd)
    _assert_stage_bits(first, o, fused, "first run: ")
    d2 = run()
    _assert_stage_bits(_views(dev, B, wd), o, fused, "second run: ")
    _aggregate(other_td, other_wd, layout)
    d3 = run()
    _assert_stage_bits(_views(dev, B, wd), o, fused, "after another batch size: ")
    assert torch.isfinite(d1).all() and torch.equal(d1, d2) and torch.equal(d1, d3)
    return first


SHAPES = [(C, B) for C in (128, 192, 320) for B in (1, 3, 9)] + [(128, 33), (1024, 2)]
# tiles = 4 B: 4, 12, 36, 132 — 36 and 132 are no multiple of 8 (the XCD remap's ragged branch) and 9, 33 row tiles leave a
# short last group in the 4-row raster; K-tiles = C / 64: 2 (fewer than the prologue issues), 3 (odd), 5, 16


@pytest.mark.parametrize("layout", ["hub", "split"])
@pytest.mark.parametrize("C,B", SHAPES)
def test_fused_route_leaves_the_f64_bits(dev, C, B, layout):
    _run_exact(dev, C, B, layout, fused=True)


@pytest.mark.parametrize("layout", ["hub", "split"])
@pytest.mark.parametrize("C,B", SHAPES)
def test_fused_route_with_row_major_w2_leaves_the_f64_bits(dev, C, B, layout):
    from vpr_amd import ops
    ops.salad_use_fragments = False                          # null *_frag members: the epilogue reads W2 row-major
    try:
        _run_exact(dev, C, B, layout, fused=True)
    finally:
        ops.salad_use_fragments = True


@pytest.mark.parametrize("layout", ["hub", "split"])
@pytest.mark.parametrize("C,B", SHAPES + [(64, 1), (64, 3), (64, 9)])
def test_unfused_route_leaves_the_f64_bits_and_the_hidden_activations(dev, tune, C, B, layout):
    """VPR_SALAD_VARIANT=1, and C = 64 on its own (salad_slabs sends it there): layer 1 on gemm256 / gemm_nt, H through
    HBM as bf16 — compared bit for bit with bf16(relu(z)), ties to even included — and the grouped second layers."""
    if C != 64:
        tune("VPR_SALAD_VARIANT", 1)
    _run_exact(dev, C, B, layout, fused=False)


@pytest.mark.parametrize("stagger", [1, 2, 3, 4, 5])
def test_k_walk_rotations_leave_the_f64_bits(dev, tune, stagger):
    """VPR_GEMM256_STAGGER at C = 192 (three K-tiles) and B = 9: koff reaches 2 tn + 1 = 7 and tm + tn = 11, so koff % nk wraps
    and the walk starts in the middle of K; the sum is the same exact number."""
    tune("VPR_GEMM256_STAGGER", stagger)
    _run_exact(dev, 192, 9, "split", fused=True)
    tune("VPR_SALAD_VARIANT", 1)
    _run_exact(dev, 192, 9, "hub", fused=False)


@pytest.mark.parametrize("layout", ["hub", "split"])
@pytest.mark.parametrize("C,B,p", [(128, 3, 0.0), (192, 9, 0.0), (128, 3, 0.5), (192, 9, 0.5), (320, 1, 0.5), (1024, 2, 0.5)])
def test_train_form_leaves_the_f64_bits_of_its_mask(dev, C, B, p, layout):
    """vpr_salad_aggregate_train.  p = 0 with a mask requested runs the dropout kernel with threshold 0: the mask is all ones
    and S / F are the eval form's.  p = 0.5: the scale is exactly 2, a power of two, so the arithmetic stays exact; the mask
    is the numpy statement of the header (tests/test_salad_dropout_cpu.py)."""
    from vpr_amd import ops
    tokens, w, ref = _exact(C, B)
    td, wd = tokens.to(dev), _to_dev(w, dev)
    seed, pass_index, base = 0x5EEDFACE12345678, 4, 1000
    keep = salad_mask(B, N, HID, p, seed, pass_index, base)
    o = ref if p == 0.0 else ost.salad_stage_outputs(tokens, w, keep=torch.from_numpy(keep), scale=2.0)
    assert keep.all() if p == 0.0 else 0.45 < keep.mean() < 0.55
    mo = torch.full((B * N, 2 * HID), 7, dtype=torch.uint8, device=dev)
    pair = td if layout == "hub" else (td[:, 1:].contiguous(), td[:, 0].contiguous())
    run = lambda: ops.salad_aggregate_train(pair, wd, p, seed, pass_index, base, 3, True, mask_out=mo)[0]
    _run_exact(dev, C, B, layout, fused=True, o=o, run=run)
    assert torch.equal(mo.cpu(), torch.from_numpy(keep))
    if p > 0:
        assert not torch.equal(o["S"], ref["S"])             # the mask did move the scores


@pytest.mark.parametrize("C", [64, 128, 192, 1024])
@pytest.mark.parametrize("B", [1, 3, 17, 65])
def test_token_mlp_leaves_the_f64_bits(dev, C, B):
    """Stage T alone (vpr_salad_stage_token): launch_skinny_linear blocks 64 rows per workgroup up to M = 16 and 16 rows
    above it; 17 and 65 leave a last row block with one live row."""
    from vpr_amd import ops
    tokens, w = ost.exact_inputs(C, B, seed=7 * C + B, n=0)  # cls rows only
    o = ost.salad_stage_outputs(tokens, w)
    wd, cls = _to_dev(w, dev), tokens[:, 0].contiguous().to(dev)
    raw = torch.cuda.current_stream(dev).cuda_stream
    _views(dev, B, wd, poison=True)
    for attempt in ("first", "second"):
        ops.salad_stage_token(cls, wd, N, raw)
        g = _views(dev, B, wd)["g"]
        bad = (g.double() != o["g"]).sum().item()
        assert bad == 0, f"{attempt} run: {bad} of {g.numel()} token features differ from f64"


def test_mutations_of_the_stage_outputs_are_caught(dev):
    """The comparison above, applied to a workspace corrupted the way a subtly wrong kernel would leave it (the exact
    difference each mistake makes, added to the scores the GPU produced): every one of them fails it.  None of the four
    moves a descriptor entry by the 1e-4 the end-to-end tests allow; dropping b2_s moves none at all."""
    C, B = 128, 3
    tokens, w, o = _exact(C, B)
    good = _run_exact(dev, C, B, "split", fused=True)
    total = o["S"].sum(0)
    for kind in ost.MUTATIONS:
        delta = (ost.mutated_scores(tokens, w, kind) - total).float()
        assert delta.abs().max() > 0
        bad = dict(good, S=torch.stack([good["S"][0] + delta, good["S"][1]]))
        with pytest.raises(AssertionError, match="S slab 0"):
            _assert_stage_bits(bad, o, True)
    swapped = dict(good, F=good["F"][:, torch.arange(B * N).roll(1)])
    with pytest.raises(AssertionError, match="F slab 0"):
        _assert_stage_bits(swapped, o, True)


# ---------------------------------------------------------------------------------------------- random values
@functools.lru_cache(maxsize=None)
def _gaussian(C, B, std):
    tokens, w = ost.gaussian_inputs(C, B, seed=31 * C + B, std=std)
    o = ost.salad_stage_outputs(tokens, w)
    ref = dict(S=o["S"].sum(0), F=o["F"].sum(0), g=o["g"])
    cpu32 = dict(zip(("S", "F", "g"), ost.salad_mlps_f32(tokens, w)))
    bound = dict(zip(("S", "F", "g"), ost.stage_error_bounds(tokens, w)))
    return tokens, w, ref, cpu32, bound


_rms = lambda a: a.double().pow(2).mean().sqrt().item()
GAUSSIAN = [(128, 0.02), (768, 0.02), (768, 0.08)]


def _gaussian_views(dev, tune, C, std, route):
    B = 3
    tokens, w, ref, cpu32, bound = _gaussian(C, B, std)
    td, wd = tokens.to(dev), _to_dev(w, dev, 0.7)
    if route == "unfused":
        tune("VPR_SALAD_VARIANT", 1)
    _views(dev, B, wd, poison=True)
    _aggregate(td, wd, "hub")
    v = _views(dev, B, wd)
    assert v["S"].shape[0] == v["F"].shape[0] == (2 if route == "fused" else 1)
    got = dict(S=v["S"].sum(0), F=v["F"].sum(0), g=v["g"])       # the slabs added in f32, as stage A adds them
    return got, ref, cpu32, bound


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("C,std", GAUSSIAN)
def test_gaussian_values_stay_inside_the_element_bound(dev, tune, C, std, route):
    """|kernel - f64| <= oracle.salad_stages.stage_error_bounds on every element: the worst case of f32 accumulation in both
    layers plus the hidden values that the layer-1 error can push across a bf16 rounding boundary.  Computed from the inputs
    alone (self-checked on the CPU: plain f32 stays inside it; a dropped bias, exchanged rows and a zeroed W2 column exceed it
    16 to 2000 times, unrounded hidden values at C = 128 only — those are what the RMS test below is for)."""
    got, ref, _, bound = _gaussian_views(dev, tune, C, std, route)
    for key in ("S", "F", "g"):
        ratio = ((got[key].double() - ref[key]).abs() / bound[key]).max().item()
        print(f"\n[{route} C={C} std={std}] {key}: max |err| / bound {ratio:.3f} (largest bound {bound[key].max().item():.2e})")
        assert ratio <= 1.0, key


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("C,std", GAUSSIAN)
def test_gaussian_rms_error_is_that_of_plain_f32(dev, tune, C, std, route):
    """rms(kernel - f64) <= 4 rms(torch f32 on the CPU - f64) for S, F and g: both sides round the same hidden values to
    bf16 and accumulate in f32; the 4 is the margin for another summation order (MFMA blocks of 32 against the CPU's).
    Observed on an MI355X: 0.48 ... 1.09 (beside the SALAD error table, with what the ratio is made of)."""
    got, ref, cpu32, _ = _gaussian_views(dev, tune, C, std, route)
    ratios = {}
    for key in ("S", "F", "g"):
        e_gpu, e_cpu = _rms(got[key].double() - ref[key]), _rms(cpu32[key].double() - ref[key])
        ratios[key] = e_gpu / e_cpu
        print(f"\n[{route} C={C} std={std}] {key}: rms err GPU {e_gpu:.3e}, CPU f32 {e_cpu:.3e}, ratio {ratios[key]:.2f}")
    assert all(r <= 4.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("C,std,route", [(768, 0.02, "fused"), (768, 0.02, "unfused"), (64, 0.08, "unfused")])
def test_views_are_what_the_aggregation_stage_consumes(dev, tune, C, std, route):
    """Slabs summed in f32, slab 0 first (what sinkhorn_aggregate_kernel does on loading them), and g, through the public
    Sinkhorn stage = the descriptor of the one-call form, to the Sinkhorn stage's own bound."""
    from vpr_amd import ops
    B = 3
    tokens, w = ost.gaussian_inputs(C, B, seed=5 * C, std=std)
    td, wd = tokens.to(dev), _to_dev(w, dev, 0.7)
    if route == "unfused":
        tune("VPR_SALAD_VARIANT", 1)
    _views(dev, B, wd, poison=True)
    desc = _aggregate(td, wd, "hub")
    ws = ops.workspace("salad", 256, dev)
    v = ops.salad_stage_views(ws, B, N, wd)
    assert v.S.shape[0] == (2 if route == "fused" else 1)
    S = (v.S[0] + v.S[1]) if route == "fused" else v.S[0].clone()
    F = (v.F[0] + v.F[1]) if route == "fused" else v.F[0].clone()
    again, _ = ops.salad_sinkhorn_aggregate(S.view(B, N, M), F.view(B, N, L), v.g.clone(), 0.7, 3)
    err = (again - desc).abs().max().item()
    print(f"\n[{route} C={C}] descriptor from the views vs one call: max abs diff {err:.2e}")
    assert torch.isfinite(desc).all() and err <= 2e-6
