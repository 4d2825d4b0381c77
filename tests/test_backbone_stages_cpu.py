"""CPU: the backbone stage checker (oracle/backbone.py check_trace) can fail.  The real recorder needs the device, so the
launch chain is restated in plain torch (oracle.backbone.restate: f32 accumulation, one bf16 rounding where the kernels
round, the deferred biases as an f32 running sum) and emits the same stage records.  The faithful restatement passes in
every mode; each single fault of oracle.backbone.MUTATIONS is rejected, at the stage that carries it.  vit_small cut to
3 blocks, 168 px (n = 144, T = 145), B = 2, the model of tests/backbone_trace.py make_model."""
import pytest
import torch

import backbone_trace as bt
from oracle import backbone as ob

IMG, B, L = 168, 2, 3


@pytest.fixture(scope="module")
def case():
    m = bt.make_model("vit_small", IMG, L)
    return ob.Params(m), bt.make_image(B, IMG)


@pytest.mark.parametrize("gelu", ["tanh", "erf"])
@pytest.mark.parametrize("mode", ob.MODES)
def test_faithful_restatement_passes(case, mode, gelu):
    p, img = case
    worst = ob.check_trace(ob.restate(p, img, mode, gelu), p, mode, gelu)
    print(f"{mode} {gelu}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert worst and max(worst.values()) <= 1.0
    assert {"qkv", "attention"} <= set(worst) and any(k.startswith("fc1") for k in worst) and any(k.startswith("ln_next") for k in worst)


# mutation -> (the mode it is planted in, gelu, the stages that may report it)
PLANTED = {
    "c_att_for_c_mlp": ("split_after", "tanh", {"ln_next"}),
    "c_mlp_for_c_att": ("split_side", "tanh", {"ln2"}),
    "cls_proj_bias_missing": ("split_side", "tanh", {"ln2"}),
    "swap_norms": ("cf_resid", "tanh", {"ln2"}),
    "fc1_wrong_block": ("split_before", "tanh", {"fc1"}),
    "cum_bf16": ("split_after", "tanh", {"consts", "ln2", "ln_next"}),
    "two_roundings": ("split_after", "tanh", {"proj_add", "fc2_add"}),
    "gelu_form": ("split_side", "tanh", {"fc1"}),
    "cls_pos_on_patch0": ("split_after", "tanh", {"embed_add_ln"}),
    "ln_before_add": ("split_after", "tanh", {"ln2"}),
    "patch_writes_cls": ("split_after", "tanh", {"proj_add"}),
    "consts_wrong_bias": ("fused", "tanh", {"consts"}),
}


def test_every_mutation_is_planted():
    assert set(PLANTED) == set(ob.MUTATIONS)


@pytest.mark.parametrize("mutation", ob.MUTATIONS)
def test_mutation_is_rejected_at_its_stage(case, mutation):
    p, img = case
    mode, gelu, stages = PLANTED[mutation]
    with pytest.raises(ob.StageFailure) as e:
        ob.check_trace(ob.restate(p, img, mode, gelu, mutate=mutation), p, mode, gelu)
    print(f"{mutation}: {e.value}")
    assert e.value.stage in stages, str(e.value)


@pytest.mark.parametrize("mutation,mode,gelu,stages", [
    ("gelu_form", "cf_resid", "erf", {"fc1"}),              # tanh where erf is configured
    ("cum_bf16", "cf_resid", "tanh", {"consts", "ln2", "ln_next"}),
    ("two_roundings", "cf_resid", "tanh", {"proj_add", "fc2_add"}),
    ("c_att_for_c_mlp", "fused", "tanh", {"fc2_add", "ln_next"}),   # the skinny launch's statistics take the same bias row
])
def test_mutation_is_rejected_in_other_modes(case, mutation, mode, gelu, stages):
    p, img = case
    with pytest.raises(ob.StageFailure) as e:
        ob.check_trace(ob.restate(p, img, mode, gelu, mutate=mutation), p, mode, gelu)
    assert e.value.stage in stages, str(e.value)


def test_cumulative_bias_in_bf16_fails_the_layernorm_bound_too(case):
    """Without the constant check in front of it: the LayerNorm stages alone reject a bf16 cumulative bias."""
    p, img = case
    tr = ob.restate(p, img, "split_after", "tanh", mutate="cum_bf16")
    tr.cum = None
    with pytest.raises(ob.StageFailure) as e:
        ob.check_trace(tr, p, "split_after", "tanh")
    assert e.value.stage in ("ln2", "ln_next"), str(e.value)


def test_inputs_tell_the_gelu_forms_apart(case):
    """On the reference alone: at least 0.5 % of the fc1 outputs have |GELU_tanh - GELU_erf| above the stage bound."""
    p, img = case
    tr = ob.restate(p, img, "split_after", "tanh")
    over = {i: [] for i in range(L)}
    zs = {i: [] for i in range(L)}
    for s in tr.stages:
        if s.stage == "fc1":
            ref, bound, z = ob.fc1_ref_bound(s.inp["h"], *p.blocks[s.block]["fc1"], "tanh")
            over[s.block].append(((ob.gelu_f64(z, "erf") - ref).abs() / bound).reshape(-1))
            zs[s.block].append(z.reshape(-1))
    for i in range(L):                      # per block, its patch and cls rows together (B = 2 cls rows are no sample)
        o, z = torch.cat(over[i]), torch.cat(zs[i])
        share = float((o > 1).double().mean())
        print(f"block {i}: {100 * share:.2f} % of {o.numel()} fc1 outputs tell the forms apart, worst {float(o.max()):.2f} x the bound, "
              f"pre-activation std {float(z.std()):.2f}")
        assert share >= 0.005 and float(z.std()) >= 1.0


def test_inputs_tell_bias_rows_and_norms_apart(case):
    """On the reference alone: at every LayerNorm stage, the reference computed with ANY other deferred-bias row, or with
    any other norm, is more than 100 bounds away from the right one at some element — a wrong operand cannot hide.
    (Read per element: the folded biases are 0.5 N x 0.3 N, so two bias rows differ by ~0.6 at most, while the largest
    bound of a stage, 2^-8 of its largest output, is ~0.02; the bound at the element that moves is what a fault meets.)"""
    p, img = case
    tr = ob.restate(p, img, "split_after", "tanh")
    rows = [c for pair in zip(p.c_att, p.c_mlp) for c in pair]
    norms = [b[k] for b in p.blocks for k in ("norm1", "norm2")] + [p.norm]
    lows = []
    for s in tr.stages:
        if s.stage not in ("ln2", "ln_next"):
            continue
        norm = p.blocks[s.block]["norm2"] if s.stage == "ln2" else p.norm_after[s.block]
        c = (p.c_att if s.stage == "ln2" else p.c_mlp)[s.block]
        ref, bound = ob.ln_stage(s.inp["x"], c, norm, p.eps, p.e_c)
        for other in rows:
            if other is not c:
                lows.append(float(((ob.ln_stage(s.inp["x"], other, norm, p.eps)[0] - ref).abs() / bound).max()))
        for other in norms:
            if other is not norm:
                lows.append(float(((ob.ln_stage(s.inp["x"], c, other, p.eps)[0] - ref).abs() / bound).max()))
    print(f"{len(lows)} wrong operands, the least visible is {min(lows):.0f} bounds away")
    assert len(lows) == 2 * L * (2 * L - 1 + 2 * L) and min(lows) > 100


def test_schedules_of_the_helper_match_the_stage_set_of_the_restatement(case):
    """The annotated schedules (what the recorder's calls are checked against on the GPU) and the restatement name the
    same launches: same (block, stage, part, label) sets in every mode and GELU form."""
    p, img = case
    rename = {"attention_qkv_split_bf16": "attention", "attention_qkv_bf16": "attention"}
    for mode in ob.MODES:
        for gelu in ("tanh", "erf"):
            want = {(b, s, pt, rename.get(lab, lab)) for lab, _, _, b, s, pt in bt.schedule(mode, B, p.n, L, gelu) if s is not None}
            got = {s.key() for s in ob.restate(p, img, mode, gelu).stages}
            assert got == want, (mode, gelu, sorted(got ^ want, key=str))
