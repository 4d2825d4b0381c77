"""GPU: stage A of the SALAD aggregation — Sinkhorn, V = F^T P^T on the hi/lo planes, the three normalisations — judged per
element on all three kernels through their public stage entry points: ops.salad_sinkhorn_aggregate (salad.hip, n = 256, K in
registers), _n (salad_anyres.hip, K in LDS, columns tid + 256 q) and _hires (salad_hires.hip, K recomputed, P in 512-column
blocks; called directly, so it also runs at small n).  The descriptor averages the transport plan over the tokens: the lo plane of P
lost on the last of 1369 tokens moves no descriptor entry by more than 3.4e-6, the size of the max-abs gates of the other SALAD
tests (2e-6 … 5e-6), and a per-cluster factor moves nothing.  Here:
  * probes (oracle/salad_stage_a.py): one-hot features turn descriptor entries into single entries of P, every token of
    every image judged against f64 by a bound derived from a rounding model and by rms <= G x plain torch f32 on the CPU, at
    every token count where a kernel changes path, in two block alignments so that no token stands alone in its block;
  * Gaussian features, iterations 1 / 3 / 7, dustbin 0.7: the same two criteria over the whole descriptor;
  * powers of two on feats / tokfeat leave the f32 and bf16 bits; the eps rule of F.normalize on zero blocks;
  * every oracle mutation, added to what the GPU produced, fails a comparison.
tests/test_salad_stage_a_cpu.py asserts on the oracle alone what these comparisons accept and reject."""
import pytest
import torch

from oracle import salad_stage_a as sa

pytestmark = pytest.mark.gpu
ENTRY = {"fixed": "salad_sinkhorn_aggregate", "anyres": "salad_sinkhorn_aggregate_n", "hires": "salad_sinkhorn_aggregate_hires"}
KERNEL_N = [(k, n) for k in ("fixed", "anyres", "hires") for n in sa.PROBE_N[k]]


def _run(dev, kernel, scores, feats, tok, dustbin, iters, want_bf16=False):
    from vpr_amd import ops
    out, out16 = getattr(ops, ENTRY[kernel])(scores.to(dev), feats.to(dev), tok.to(dev), dustbin, iters, want_bf16=want_bf16)
    assert out.dtype == torch.float32 and out.shape == (scores.shape[0], sa.D_OUT)
    return (out.cpu(), out16.cpu()) if want_bf16 else out.cpu()


def _run_case(dev, kernel, case):
    return _run(dev, kernel, case["scores"], case["feats"], case["tok"], case["dustbin"], case["iters"])


@pytest.mark.parametrize("kernel,n", KERNEL_N)
def test_probes_every_plan_entry_is_inside_the_bound_and_has_the_error_of_plain_f32(dev, kernel, n):
    """Image r holds x_j at [j][l], 128 r + l = j + shift: descriptor entry 256 + 64 l + m of image r is x_j P[m][j] /
    ||x . P[m, block r]|| / sqrt(65).  Every entry of every image — the token block and the exact zeros of the columns without a
    token included — is within descriptor_bound of f64, and the rms of the judged entries' relative error is at most G = 4 x
    that of stage_a_f32_cpu.  Measured on an MI355X: worst |err| / bound 0.039 (fixed), 0.055 (anyres, n = 129),
    0.041 (hires, n = 65); rms ratio 0.98 … 1.01 on all three; worst relative error of one entry 3.1e-5."""
    for shift in sa.SHIFTS:
        case = sa.probe_case(n, shift)
        got = _run_case(dev, kernel, case)
        worst, ratio, rel, at = sa.compare_probes(got, case)
        print(f"\n[{kernel} n={n} shift={shift}] worst |err| / bound {worst:.4f}, rms ratio {ratio:.3f}, relative error max {rel:.2e} at (token, cluster) {at}")
        sa.assert_within(worst, ratio, f"{kernel} n={n} shift={shift}")


@pytest.mark.parametrize("iters", sa.GAUSS_ITERS)
@pytest.mark.parametrize("kernel,n", [(k, n) for k in ("fixed", "anyres", "hires") for n in sa.GAUSS_N[k]])
def test_gaussian_features_whole_descriptor_inside_the_bound_with_the_error_of_plain_f32(dev, kernel, n, iters):
    """The _stage_inputs of the existing stage tests (B = 2, seed n), dustbin 0.7.  Measured on an MI355X: worst
    |err| / bound 0.066 (fixed), 0.106 (anyres and hires, n = 65, one iteration); rms ratio 0.995 … 1.01."""
    case = sa.gaussian_case(n, sa.GAUSS_DUSTBIN, iters)
    got = _run_case(dev, kernel, case)
    worst, ratio = sa.compare_descriptor(got, case)
    print(f"\n[{kernel} n={n} iters={iters}] worst |err| / bound {worst:.4f}, rms ratio {ratio:.3f}, max |err| {(got.double() - case['true']['desc']).abs().max().item():.2e}")
    sa.assert_within(worst, ratio, f"{kernel} n={n} iters={iters}")


@pytest.mark.parametrize("kernel,n", [("fixed", 256), ("anyres", 65), ("anyres", 529), ("hires", 577), ("hires", 1369)])
def test_powers_of_two_on_feats_or_tokfeat_leave_the_bits(dev, kernel, n):
    """2^10 and 2^-10 commute with the split, the products, the sums, the square roots and the divisions: the f32 and the bf16
    output are bit-identical, with no oracle in between."""
    case = sa.gaussian_case(n, sa.GAUSS_DUSTBIN, 3)
    scores, feats, tok = case["scores"], case["feats"], case["tok"]
    base, base16 = _run(dev, kernel, scores, feats, tok, sa.GAUSS_DUSTBIN, 3, want_bf16=True)
    assert torch.equal(base16, base.to(torch.bfloat16)) and sa.compare_descriptor(base, case)[0] <= 1
    for k in (10, -10):
        for f_scale, t_scale in ((2.0 ** k, 1.0), (1.0, 2.0 ** k)):
            out, out16 = _run(dev, kernel, scores, feats * f_scale, tok * t_scale, sa.GAUSS_DUSTBIN, 3, want_bf16=True)
            assert torch.equal(out.view(torch.int32), base.view(torch.int32)), (k, f_scale, t_scale, (out != base).sum().item())
            assert torch.equal(out16.view(torch.int16), base16.view(torch.int16)), (k, f_scale, t_scale)


@pytest.mark.parametrize("kernel,n", [("fixed", 256), ("anyres", 80), ("anyres", 529), ("hires", 80), ("hires", 577)])
def test_eps_rule_of_normalize_on_zero_blocks(dev, kernel, n):
    """Image 1 has all-zero features, image 2 an all-zero token vector, image 3 both; image 0 is an ordinary neighbour in the
    same batch.  max(||v||, 1e-12) keeps every output finite, the zero blocks are exactly 0 (the oracle's bound there is 0), the
    rest equals f64 within the bound, and the neighbour's bits are those of a batch without any zero image."""
    scores, feats, tok = sa.gaussian_inputs(4, n, seed=7 * n)
    plain = _run(dev, kernel, scores, feats, tok, sa.GAUSS_DUSTBIN, 3)
    feats, tok = feats.clone(), tok.clone()
    feats[1], tok[2], feats[3], tok[3] = 0, 0, 0, 0
    case = sa.general_case(scores, feats, tok, sa.GAUSS_DUSTBIN, 3)
    assert (case["bound"][1, 256:] == 0).all() and (case["bound"][2, :256] == 0).all() and (case["bound"][3] == 0).all()
    got = _run(dev, kernel, scores, feats, tok, sa.GAUSS_DUSTBIN, 3)
    assert torch.isfinite(got).all()
    assert (got[1, 256:] == 0).all() and (got[2, :256] == 0).all() and (got[3] == 0).all()
    worst, ratio = sa.compare_descriptor(got, case)
    print(f"\n[{kernel} n={n}] zero blocks: worst |err| / bound {worst:.4f}, rms ratio {ratio:.3f}")
    sa.assert_within(worst, ratio, f"{kernel} n={n}")
    assert abs(got[1, :256].double().norm().item() - 1) < 1e-6 and abs(got[2, 256:].double().norm().item() - 1) < 1e-6
    assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))


def test_mutations_are_caught(dev):
    """The comparisons above, applied to outputs corrupted the way a subtly wrong kernel would leave them: the exact
    difference each mistake makes in the f32 restatement, added to what the GPU produced.  Every mutation of the oracle is
    rejected on at least one case — by the element bound or by the rms criterion — and a lost plane, cross term or token on
    every probe case.  Measured on an MI355X: the mildest is the lo plane of P lost on token 1024, 3.2 x the gate."""
    best = {mu: 0.0 for mu in sa.MUTATIONS}
    for kernel, spec in sa.MUTATION_RUNS:
        case = sa.case_of(spec)
        got = _run_case(dev, kernel, case)
        sa.assert_within(*sa.compare(got, case), f"unmutated {kernel} {spec}")
        for mu, margin in sa.mutation_margins(got, case).items():
            best[mu] = max(best[mu], margin)
            if spec[0] == "probe" and mu[0] in ("p_lo_token", "p_lo_all", "f_lo_all", "no_cross_term", "token_not_aggregated"):
                assert margin > 1, (kernel, spec, mu, margin)
    mildest = min(best, key=best.get)
    print(f"\nmildest mutation: {mildest} at {best[mildest]:.2f} x the gate; all: " + ", ".join(f"{m[0]}:{m[1]} {v:.1f}" for m, v in best.items()))
    assert best[mildest] > 1, best
