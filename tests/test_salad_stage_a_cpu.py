"""CPU: everything tests/test_salad_stage_a_gpu.py relies on, asserted on oracle/salad_stage_a.py alone — the plain-f32
restatement of stage A stays inside the derived bounds of f64 on every probe and Gaussian case of the GPU file, the probes read
single entries of the transport plan (probe_expected == a brute-force evaluation from P, every judged product >= 2^-60), and
every mutation, put in the place of a kernel's mistake, fails at least one of the GPU file's comparisons on the GPU file's own
inputs.  The mildest margin is printed: it pins the bounds from above."""
import math

import pytest
import torch

from oracle import salad_stage_a as sa

ALL_PROBE_N = sorted({n for ns in sa.PROBE_N.values() for n in ns})
ALL_GAUSS_N = sorted({n for ns in sa.GAUSS_N.values() for n in ns})


@pytest.mark.parametrize("shift", sa.SHIFTS)
@pytest.mark.parametrize("n", ALL_PROBE_N)
def test_probes_read_single_plan_entries_and_the_restatement_is_inside_the_bound(n, shift):
    c = sa.probe_case(n, shift)
    B, x, P = (n + shift + 127) // 128, c["x"].double(), c["true"]["P"]
    assert c["scores"].shape == (B, n, 64) and c["feats"].shape == (B, n, 128) and c["tok"].shape == (B, 256) and B <= 12
    assert all(torch.equal(c["scores"][0], c["scores"][r]) for r in range(B))
    assert (c["feats"] != 0).sum().item() == n and (x.abs() >= 0.5).all() and (x.abs() < 2).all() and (x < 0).any() and (x > 0).any()
    assert (c["x"].to(torch.bfloat16).float() != c["x"]).float().mean() > 0.9        # the F split has a lo plane to lose
    assert torch.equal(c["x"], sa.probe_case(n, 0)["x"]) and torch.equal(c["scores"][0], sa.probe_case(n, 0)["scores"][0])
    # the judged products are normal numbers in every plane
    prod = x.abs().unsqueeze(0) * P[0]
    assert prod.min().item() >= 2.0 ** -60, prod.min().item()
    # brute force from P: entry 256 + 64 l + m of image r is x_j P[m][j] / ||x . P[m, block r]|| / sqrt(65), 128 r + l = j + shift
    desc = c["true"]["desc"]
    worst = 0.0
    for r in range(B):
        lo, hi = max(128 * r - shift, 0), min(128 * r - shift + 128, n)                # the tokens of image r
        w = x[lo:hi].unsqueeze(0) * P[0][:, lo:hi]                                    # [64, tokens of the block]
        want = (w / w.pow(2).sum(1, keepdim=True).sqrt() / math.sqrt(65.0)).T         # [tokens, 64]
        l0 = lo + shift - 128 * r
        got = desc[r, 256:].reshape(128, 64)
        assert (got[:l0] == 0).all() and (got[l0 + hi - lo:] == 0).all()
        assert torch.equal(c["expected"][lo:hi], got[l0:l0 + hi - lo])
        worst = max(worst, ((got[l0:l0 + hi - lo] - want) / want).abs().max().item())
    assert worst <= 1e-13, worst
    assert c["expected"].shape == (n, 64) and (c["expected"] != 0).all()
    # the restatement against f64
    worst, ratio, rel, at = sa.compare_probes(c["cpu"]["desc"], c)
    relb = sa.probe_entries(c["bound"], n, shift) / c["expected"].abs()
    print(f"\n[probes n={n} shift={shift}] plain f32: worst |err| / bound {worst:.4f}, relative error max {rel:.2e} at (token, cluster) {at}, "
          f"rms {c['cpu_rms']:.2e}; relative bound {relb.min().item():.2e} .. {relb.max().item():.2e}")
    assert ratio == 1.0
    sa.assert_within(worst, ratio, f"probes n={n} shift={shift}")


@pytest.mark.parametrize("n", ALL_PROBE_N)
def test_every_token_has_block_mates_in_one_of_the_two_probe_families(n):
    """A token alone in its block is normalised to +-1 / sqrt(65) whatever its plan entries are — at shift 0 that is the last
    token of n = 129, 257, 513, 769, 1025, 1281.  Over both shifts every token shares a block with at least 63 others."""
    j = torch.arange(n)
    mates = torch.stack([torch.bincount((j + s) // 128)[(j + s) // 128] for s in sa.SHIFTS]).max(0).values
    assert mates.min().item() >= 64 or n < 128 and mates.min().item() == n
    if n % 128 == 1 and n > 128:
        c = sa.probe_case(n, 0)
        assert (c["expected"][n - 1].abs() - 1 / math.sqrt(65.0)).abs().max().item() < 1e-15


@pytest.mark.parametrize("iters", sa.GAUSS_ITERS)
@pytest.mark.parametrize("n", ALL_GAUSS_N)
def test_restatement_is_inside_the_descriptor_bound_on_gaussian_features(n, iters):
    c = sa.gaussian_case(n, sa.GAUSS_DUSTBIN, iters)
    worst, ratio = sa.compare_descriptor(c["cpu"]["desc"], c)
    err = (c["cpu"]["desc"].double() - c["true"]["desc"]).abs().max().item()
    print(f"\n[gaussian n={n} iters={iters}] plain f32: worst |err| / bound {worst:.4f}, max |err| {err:.2e}, rms {c['cpu_rms']:.2e}")
    sa.assert_within(worst, ratio, f"gaussian n={n} iters={iters}")
    for k in ("P", "V", "cnorm", "gnorm"):                     # the intermediates of the two statements are the same quantities
        rel = ((c["cpu"][k].double() - c["true"][k]).abs().max() / c["true"][k].abs().max()).item()
        assert rel < 1e-3, (k, rel)


@pytest.mark.parametrize("n,iters", [(65, 1), (257, 3), (576, 7), (1369, 3)])
def test_plan_of_the_restatement_is_inside_the_plan_model(n, iters):
    """The Sinkhorn half of the rounding model on its own: every entry of the f32 plan is within eP + ea of f64 (ea: the last
    alpha, the factor of a whole cluster that the descriptor cannot see), and within eP once each row's factor is taken out."""
    c = sa.gaussian_case(n, sa.GAUSS_DUSTBIN, iters)
    P, eP, ea = sa.plan_error(c["scores"], sa.GAUSS_DUSTBIN, iters)
    rel = c["cpu"]["P"].double() / P - 1
    worst = (rel.abs() / (eP + ea.unsqueeze(2))).max().item()
    centred = rel - (rel.max(2, keepdim=True).values + rel.min(2, keepdim=True).values) / 2      # any one factor per row
    worst_c = (centred.abs() / eP).max().item()
    print(f"\n[n={n} iters={iters}] plan: worst |rel err| / (eP + ea) {worst:.3f}, with the row factor taken out / eP {worst_c:.3f}; "
          f"eP {eP.min().item():.1e} .. {eP.max().item():.1e}, observed {rel.abs().max().item():.1e}")
    assert worst <= 1 and worst_c <= 1


def test_true_stage_a_is_the_oracle_of_the_existing_tests():
    from oracle import salad
    scores, feats, tok = sa.gaussian_inputs(2, 97, seed=5)
    t = sa.true_stage_a(scores, feats, tok, 0.7, 3)
    assert (t["desc"] - salad.sinkhorn_aggregate(scores, feats, tok, 0.7, 3)).abs().max().item() < 1e-15   # f64 rounding of another order
    assert t["P"].shape == (2, 64, 97) and t["V"].shape == (2, 128, 64) and t["cnorm"].shape == (2, 64) and t["gnorm"].shape == (2,)
    assert torch.allclose(t["gnorm"], torch.full((2,), math.sqrt(65.0), dtype=torch.float64), rtol=1e-14)


def test_every_mutation_fails_a_comparison_of_the_gpu_file():
    """The restatement in the kernel's place on the cases of test_mutations_are_caught: every mutation is rejected on at least
    one of them, and a lost plane, cross term or token on EVERY probe case (their blocks are chosen so that no token is alone)."""
    best = {mu: 0.0 for mu in sa.MUTATIONS}
    for spec in dict.fromkeys(spec for _, spec in sa.MUTATION_RUNS):
        case = sa.case_of(spec)
        assert sa.compare(case["cpu"]["desc"], case)[0] <= 1
        for mu, margin in sa.mutation_margins(case["cpu"]["desc"], case).items():
            print(f"  {spec} {mu}: {margin:.2f}")
            best[mu] = max(best[mu], margin)
            if spec[0] == "probe" and mu[0] in ("p_lo_token", "p_lo_all", "f_lo_all", "no_cross_term", "token_not_aggregated"):
                assert margin > 1, (spec, mu, margin)
    mildest = min(best, key=best.get)
    print(f"  mildest mutation: {mildest} at {best[mildest]:.2f} x the gate (the element bound, or G = {sa.G} x the rms of plain f32)")
    assert best[mildest] > 1, best


def test_split_is_hi_plus_lo_to_2_pow_minus_17_of_the_binade():
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.randn(200000, generator=g) * torch.exp2(torch.randint(-60, 20, (200000,), generator=g).float()),
                   torch.tensor([1 + 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -23, 1 + 2.0 ** -9 + 2.0 ** -17, 2 - 2.0 ** -23])])
    hi, lo = sa._split(v)
    binade = torch.exp2(torch.floor(torch.log2(v.double().abs())))
    err = (v.double() - hi.double() - lo.double()).abs() / binade
    assert err.max().item() <= 2.0 ** -17 and err.max().item() > 2.0 ** -17.5        # the figure is attained, not merely safe
    assert ((lo.double() * hi.double()).abs() <= 2.0 ** -8 * 1.01 * v.double().pow(2)).all()


def test_a_per_cluster_factor_on_the_plan_is_invisible():
    """Why no mutation scales a cluster: V[:, m] times 2^k leaves the f32 descriptor's bits, any other factor its value to
    rounding — the last alpha, `scale` and a uniform b_col cannot be judged through the descriptor, and are not."""
    c = sa.gaussian_case(65, sa.GAUSS_DUSTBIN, 3)
    V, tok = c["cpu"]["V"], c["tok"]
    base = sa._norms(V, tok)[2]
    pow2 = torch.exp2(torch.randint(-8, 9, (1, 1, 64), generator=torch.Generator().manual_seed(1)).float())
    assert torch.equal(sa._norms(V * pow2, tok)[2], base)
    other = 1 + torch.rand(1, 1, 64, generator=torch.Generator().manual_seed(2))
    assert (sa._norms(V * other, tok)[2] - base).abs().max().item() < 1e-8
