"""GPU: what the f32-accurate SALAD path (vpr_salad_aggregate_f32, _f32_n, _f32_hires) leaves in its workspace — the bf16
planes of tokens, weights and hidden values (split3_kernel, both plane orders), the f32 hidden values H / Ht (gemm256 or the
gemm_nt_group fallback over a K axis of 6 C), the scores S, features F and token features g (one grouped launch over 6 x
hidden) — element by element against the stage oracle (oracle/salad_f32_stages.py), read through ops.salad_f32_stage_views
(include/vpr_amd_salad_f32_stages.h).

The descriptor-level tests cannot see these stages: dropping every low plane moves no descriptor entry by more than 3e-7,
under the 5e-7 they assert, and b2_s cancels exactly (tests/test_oracle_selfchecks.py asserts both on the oracle).  Checks:
  * planes bit for bit, on values chosen for the two roundings;
  * exact families E0 / E1 / E2 (preconditions asserted on the CPU): f32 accumulation is exact in any order, so torch.equal
    with the plane model, no tolerance, on a poisoned workspace, twice, and again after a batch of another size;
  * Gaussian values: RMS error against that of plain torch f32 on the CPU, and a per-element bound computed from the inputs;
  * the views are what stage A consumes; every oracle mutation, applied to the views the GPU produced, fails the checks.
Which layer-1 kernel ran is not something the library reports for this launch; the tests choose it through the one rule that
decides it (launch_gemm256 refuses a bias that is not 16-byte aligned, gemm_nt_group takes it) and assert that alignment.
"""
import functools

import pytest
import torch

from oracle import salad_f32_stages as o32

pytestmark = pytest.mark.gpu
M, L, T, HID = 64, 128, 256, 512
G = 4.0                        # rms(kernel - f64) <= G rms(torch f32 on the CPU - f64); tests/test_oracle_selfchecks.py: F32_STAGE_G
KEYS = ("H", "Ht", "S", "F", "g")
ENTRIES = {"f32": "salad_aggregate_f32", "f32_n": "salad_aggregate_f32_n", "f32_hires": "salad_aggregate_f32_hires"}


def _to_dev(w, dev, dustbin=1.0, route="gemm256"):
    """SaladWeightsF32 on the device.  route "gemm_nt": b1_sc at a 4-byte offset, which launch_gemm256 refuses (it reads the
    bias as float4) and the fallback, launch_gemm_nt_group, takes."""
    from vpr_amd.ops import SaladWeightsF32
    d = {k: v.to(dev) for k, v in w.items()}
    if route == "gemm_nt":
        buf = torch.empty(d["b1_sc"].numel() + 1, dtype=torch.float32, device=dev)
        buf[1:].copy_(d["b1_sc"])
        d["b1_sc"] = buf[1:]
    wd = SaladWeightsF32(**d, dustbin=dustbin)
    assert wd.b1_sc.data_ptr() % 16 == (4 if route == "gemm_nt" else 0)
    return wd


def _aggregate(td, wd, layout, entry="f32"):
    from vpr_amd import ops
    fn = getattr(ops, ENTRIES[entry])
    if layout == "hub":                                      # cls first: image stride (1 + n) C, patch rows offset by C
        return fn(td, wd, 3)[0]
    return fn((td[:, 1:].contiguous(), td[:, 0].contiguous()), wd, 3)[0]


def _workspace(dev, B, n, wd, poison=False):
    from vpr_amd import _lib, ops
    C, hidden, m, l, t = wd.validate()
    ws = ops.workspace("salad_f32", _lib.lib().vpr_salad_f32_workspace_bytes(B, n, C, m, l, t, hidden), dev)
    if poison:
        ws.fill_(0xFF)                                       # f32 / bf16 NaN: whatever a later run does not write shows
    return ws


def _views(dev, B, n, wd, keys=KEYS):
    """CPU copies of the stage views of the current stream's f32 SALAD workspace."""
    from vpr_amd import ops
    v = ops.salad_f32_stage_views(_workspace(dev, B, n, wd), B, n, wd)
    return {k: getattr(v, k).cpu() for k in keys}


def _assert_bits(v, o, judged, what=""):
    """Every element of the judged views equals the plane model `o` (f32_stage_outputs) exactly; the others are finite."""
    for key in KEYS:
        assert v[key].dtype == torch.float32 and v[key].shape == o[key].shape, key
        if key in judged:
            bad = (v[key].double() != o[key].double()).sum().item()
            assert bad == 0, f"{what}{key}: {bad} of {o[key].numel()} elements differ from the plane model"
        else:
            assert torch.isfinite(v[key]).all(), f"{what}{key} not finite"


def _run_exact(dev, family, C, B, layout, n=256, entry="f32", route="gemm256"):
    """One exact case with the stability protocol: poisoned workspace -> run -> run again on the same workspace -> a batch of
    another size (its layout differs) -> run again.  All three leave the plane model's bits."""
    tokens, w, o = o32.exact_case(family, C, B, n)
    judged = o32.FAMILIES[family][1]
    td, wd = tokens.to(dev), _to_dev(w, dev, route=route)
    B2 = B + 1 if B < 8 else B - 2
    other_tok, other_w = o32.FAMILIES[family][0](C, B2, seed=5, n=n)
    other_td, other_wd = other_tok.to(dev), _to_dev(other_w, dev, route=route)
    _workspace(dev, max(B, B2), n, wd, poison=True)
    d1 = _aggregate(td, wd, layout, entry)
    first = _views(dev, B, n, wd)
    _assert_bits(first, o, judged, "first run: ")
    d2 = _aggregate(td, wd, layout, entry)
    _assert_bits(_views(dev, B, n, wd), o, judged, "second run: ")
    _aggregate(other_td, other_wd, layout, entry)
    d3 = _aggregate(td, wd, layout, entry)
    _assert_bits(_views(dev, B, n, wd), o, judged, "after another batch size: ")
    assert torch.isfinite(d1).all() and torch.equal(d1, d2) and torch.equal(d1, d3)
    return first


# ------------------------------------------------------------------------------------------------ planes
def _plane_inputs(C, B):
    """Gaussian tokens and weights with the rounding cases written over the head of every matrix: full magnitude range
    (2^-60 .. 2^60) in the tokens, moderate powers of two in the weights so that H, S, F and g stay finite."""
    tokens, w = o32.gaussian_inputs(C, B, seed=17 * C + B, std=0.05)
    wide, mild = o32.rounding_cases(), o32.rounding_cases(scales=(1.0, 2.0 ** -7, 2.0 ** -20, 4.0))
    tokens.view(-1)[:wide.numel()] = wide                                 # the cls row and the first patch rows of image 0
    tokens[-1, -1, :] = wide[:C]                                          # the last patch row of the batch
    tokens[-1, 0, :] = wide[-C:]                                          # the last cls row
    for k in ("w1_sc", "w1_t", "w2_s", "w2_c", "w2_t"):
        w[k].view(-1)[:mild.numel()] = mild
        w[k][-1, :mild.numel()] = mild[:w[k].shape[1]]
    return tokens, w


@pytest.mark.parametrize("C,B,layout", [(64, 1, "hub"), (128, 3, "hub"), (128, 3, "split"), (192, 2, "split")])
def test_planes_are_split3_of_the_operands_in_the_order_of_their_role(dev, C, B, layout):
    """A1, cls3 (activation order q h m m h h), W1, W1t, W2s, W2c, W2t (weight order h q m h m h) equal the oracle's split3 of
    the inputs bit for bit — ties at both roundings to even, negative residuals, powers of two, zero planes, +-0 — and H2 /
    Ht2 equal split3 of the H / Ht the kernel itself left, the score head's six segments ahead of the cluster head's."""
    tokens, w = _plane_inputs(C, B)
    td, wd = tokens.to(dev), _to_dev(w, dev)
    _workspace(dev, B, 256, wd, poison=True)
    _aggregate(td, wd, layout)
    v = _views(dev, B, 256, wd, ("H", "Ht", "S", "F", "g", "A1", "cls3", "W1", "H2", "W1t", "W2s", "W2c", "W2t", "Ht2"))
    bits = lambda t: t.view(torch.int16)
    x, cls = tokens[:, 1:].reshape(-1, C).contiguous(), tokens[:, 0].contiguous()
    want = dict(A1=(x, o32.ACT_ORDER), cls3=(cls, o32.ACT_ORDER), W1=(w["w1_sc"], o32.WGT_ORDER), W1t=(w["w1_t"], o32.WGT_ORDER),
                W2s=(w["w2_s"], o32.WGT_ORDER), W2c=(w["w2_c"], o32.WGT_ORDER), W2t=(w["w2_t"], o32.WGT_ORDER), Ht2=(v["Ht"], o32.ACT_ORDER))
    for key, (src, order) in want.items():
        exp = o32.planes_in_order(src, order)
        bad = (bits(v[key]) != exp).sum().item()
        assert v[key].shape == exp.shape and bad == 0, f"{key}: {bad} of {exp.numel()} plane elements differ from split3"
    for head in (0, 1):
        exp = o32.planes_in_order(v["H"][:, head * HID:(head + 1) * HID].contiguous(), o32.ACT_ORDER)
        bad = (bits(v["H2"][:, head]) != exp).sum().item()
        assert bad == 0, f"H2 head {head}: {bad} of {exp.numel()} plane elements differ from split3 of the kernel's H"
    for key in KEYS:
        assert torch.isfinite(v[key]).all(), key
    assert (v["H"] > 0).float().mean() > 0.2


# ------------------------------------------------------------------------------------------------ exact families
SHAPES = [(C, B) for C in (64, 128, 192, 320) for B in (1, 3, 9)]
# 256-row tiles: B, 3 B, 9 B of them x 4 column tiles (36 is no multiple of 8); K-tiles of 64: 6 C / 64 = 6, 12, 18, 30
SOME = [(64, 1), (128, 3), (192, 9), (320, 3)]


@pytest.mark.parametrize("layout", ["hub", "split"])
@pytest.mark.parametrize("C,B", SHAPES)
def test_e0_one_plane_leaves_the_plane_model_bits(dev, C, B, layout):
    """E0: the exact inputs of the bf16 stage tests as f32 — only the (h,h) segment of layer 1 is non-zero; addressing, row
    groups, strides, bias, ReLU.  The hidden values stay f32 here (no bf16 rounding), so H itself is compared."""
    _run_exact(dev, "E0", C, B, layout)


@pytest.mark.parametrize("layout", ["hub", "split"])
@pytest.mark.parametrize("C,B", SOME)
@pytest.mark.parametrize("family", ["E1", "E2"])
def test_three_plane_families_leave_the_plane_model_bits(dev, family, C, B, layout):
    """E1 judges H and Ht (all six segments of layer 1 alive), E2 judges S, F and g (all six of layer 2)."""
    _run_exact(dev, family, C, B, layout)


@pytest.mark.parametrize("family", ["E0", "E1", "E2"])
@pytest.mark.parametrize("C,B", [(64, 1), (192, 9)])
def test_fallback_layer_1_route_leaves_the_same_bits(dev, family, C, B):
    """Layer 1 on launch_gemm_nt_group (128-row tiles), chosen by a b1_sc that launch_gemm256 refuses."""
    _run_exact(dev, family, C, B, "hub", route="gemm_nt")


@pytest.mark.parametrize("stagger", [1, 2, 3, 4, 5])
def test_k_walk_rotations_leave_the_plane_model_bits(dev, tune, stagger):
    """VPR_GEMM256_STAGGER at C = 192 (18 K-tiles) and B = 9: the rotated K walk starts in the middle of the six segments;
    the sum is the same exact number."""
    tune("VPR_GEMM256_STAGGER", stagger)
    _run_exact(dev, "E1", 192, 9, "split")
    _run_exact(dev, "E2", 192, 9, "hub")


@pytest.mark.parametrize("family", ["E0", "E1"])
@pytest.mark.parametrize("n,entry", [(65, "f32_n"), (529, "f32_n"), (577, "f32_hires")])
def test_other_token_counts_leave_the_plane_model_bits(dev, family, n, entry):
    """B = 2, C = 128: the workspace has B n rows (130, 1058, 1154 — none a multiple of a tile) and no image bleeds into the
    next; 577 is the smallest count only the high-resolution entry takes."""
    for layout in ("hub", "split"):
        _run_exact(dev, family, 128, 2, layout, n=n, entry=entry)


# ------------------------------------------------------------------------------------------------ random values
@functools.lru_cache(maxsize=None)
def _gaussian(C, B, std):
    tokens, w = o32.gaussian_inputs(C, B, seed=31 * C + B, std=std)
    return tokens, w, o32.true_stage_outputs(tokens, w), o32.mlps_f32_cpu(tokens, w), o32.stage_error_bounds(tokens, w)


_rms = lambda a: a.double().pow(2).mean().sqrt().item()
GAUSSIAN = [(128, 0.02), (768, 0.02), (768, 0.08)]


def _assert_gaussian(got, true, cpu32, bound, tag=""):
    """rms(kernel - f64) <= G rms(torch f32 on the CPU - f64) for H, S, F and g, and |kernel - f64| <= the per-element bound
    (worst-case f32 accumulation over 6 K + 1 terms, the dropped products, the layer-1 error carried through |W2|) for all five."""
    ratios, over = {}, {}
    for key in KEYS:
        err = got[key].double() - true[key]
        over[key] = (err.abs() / bound[key]).max().item()
        if key != "Ht":
            e_gpu, e_cpu = _rms(err), _rms(cpu32[key].double() - true[key])
            ratios[key] = e_gpu / e_cpu
            print(f"\n[{tag}] {key}: rms err GPU {e_gpu:.3e}, CPU f32 {e_cpu:.3e}, ratio {ratios[key]:.2f}; max |err| / bound {over[key]:.4f}")
    assert all(r <= G for r in ratios.values()), f"rms ratio {ratios}"
    assert all(r <= 1.0 for r in over.values()), f"element bound {over}"


@pytest.mark.parametrize("route", ["gemm256", "gemm_nt"])
@pytest.mark.parametrize("C,std", GAUSSIAN)
def test_gaussian_values_have_the_error_of_plain_f32_and_stay_inside_the_element_bound(dev, C, std, route):
    """Observed on an MI355X: ratios 0.32 ... 0.67 on both routes, max |err| / bound 0.002 (beside the SALAD error
    table).  They are below 2, so G = 4, the project's margin for another summation order; the mildest mutation (one
    low-order segment missing) sits at 5.9 (C = 768) and 8.3 (C = 128) on the same inputs (asserted in the self-checks)."""
    B = 3
    tokens, w, true, cpu32, bound = _gaussian(C, B, std)
    td, wd = tokens.to(dev), _to_dev(w, dev, 0.7, route)
    _workspace(dev, B, 256, wd, poison=True)
    desc = _aggregate(td, wd, "hub")
    assert torch.isfinite(desc).all()
    _assert_gaussian(_views(dev, B, 256, wd), true, cpu32, bound, f"{route} C={C} std={std}")


@pytest.mark.parametrize("C,std", [(768, 0.02), (64, 0.08)])
def test_views_are_what_the_aggregation_stage_consumes(dev, C, std):
    """S, F and g from the views through the public Sinkhorn stage = the descriptor of the one-call form."""
    from vpr_amd import ops
    B = 3
    tokens, w = o32.gaussian_inputs(C, B, seed=5 * C, std=std)
    td, wd = tokens.to(dev), _to_dev(w, dev, 0.7)
    _workspace(dev, B, 256, wd, poison=True)
    desc = _aggregate(td, wd, "hub")
    v = ops.salad_f32_stage_views(_workspace(dev, B, 256, wd), B, 256, wd)
    again, _ = ops.salad_sinkhorn_aggregate(v.S.clone().view(B, 256, M), v.F.clone().view(B, 256, L), v.g.clone(), 0.7, 3)
    err = (again - desc).abs().max().item()
    print(f"\n[C={C}] descriptor from the views vs one call: max abs diff {err:.2e}")
    assert torch.isfinite(desc).all() and err <= 2e-6


def test_mutations_of_the_stage_outputs_are_caught(dev):
    """The comparisons above, applied to views corrupted the way a subtly wrong kernel would leave them (the exact difference
    each mistake makes, added to what the GPU produced): every oracle mutation fails the bit comparison of the family that
    judges its layer, and every one fails the Gaussian comparison.  The faint ones move no descriptor entry by 5e-7."""
    C, B = 128, 3
    layer = lambda mu: mu[1][0] if mu[0] == "drop_segment" else mu[1] if mu[0] == "act_order" else 2 if mu[0] in ("hidden_bf16", "drop_b2_s") else 0
    for family, skip in (("E1", 2), ("E2", 1)):
        tokens, w, o = o32.exact_case(family, C, B)
        judged = o32.FAMILIES[family][1]
        good = _run_exact(dev, family, C, B, "split")
        for mutation in o32.MUTATIONS:
            if layer(mutation) == skip:
                continue
            mo = o32.f32_stage_outputs(tokens, w, mutation)
            bad = {k: (good[k].double() + (mo[k].double() - o[k].double())).float() for k in KEYS}
            with pytest.raises(AssertionError, match="differ from the plane model"):
                _assert_bits(bad, o, judged)
    tokens, w, true, cpu32, bound = _gaussian(C, B, 0.02)
    td, wd = tokens.to(dev), _to_dev(w, dev, 0.7)
    _aggregate(td, wd, "hub")
    good = _views(dev, B, 256, wd)
    _assert_gaussian(good, true, cpu32, bound, "unmutated")
    model = o32.f32_stage_outputs(tokens, w)
    for mutation in o32.MUTATIONS:
        mo = o32.f32_stage_outputs(tokens, w, mutation)
        bad = {k: good[k].double() + (mo[k].double() - model[k].double()) for k in KEYS}
        with pytest.raises(AssertionError, match="rms ratio|element bound"):
            _assert_gaussian(bad, true, cpu32, bound, str(mutation))
