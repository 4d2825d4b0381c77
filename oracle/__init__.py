"""CPU oracle of the VPR + geopose hot path — TEST INFRASTRUCTURE, NOT PRODUCT.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package;
the product package (vpr_amd) never does and has no CPU fallback.

Pinning status:
  * heads.py / postproc.py  — pinned against the reference's own classes/functions imported in
    the build container (tests/golden/make_golden.py -> tests/golden/*.npz, *.json) and against
    the reference's committed CSVs.
  * salad.py                — PARITY UNPINNED by the reference: the aggregator is fetched by
    torch.hub from the third-party repo serizba/salad (unpinned default branch;
    dinov2salad/dinov2salad_validation.py:65), absent offline.  Restates the published algorithm
    (arXiv:2311.15937, optimal-transport aggregation); pinned by closed-form known answers, and — round 2 — its
    log-domain Sinkhorn solver against an independent importable implementation of the same iteration, Hugging Face's
    SuperGlue port (transformers ...superglue.modeling_superglue.log_sinkhorn_iterations, the routine SALAD's solver
    descends from): tests/test_oracle_selfchecks.py.  The SALAD-specific wiring (marginals, dustbin row, MLP layout,
    normalisation order) remains unpinned.
  * salad_stages.py         — the same MLPs stage by stage (hidden activations, partial-sum slabs, token features), inputs
    on which f32 arithmetic is exact in any order, and the per-element error bound of an f32-accumulating kernel; every
    property the GPU tests rely on is asserted on the oracle alone in tests/test_oracle_selfchecks.py.
  * salad_f32_stages.py     — the f32-accurate path's stages: the three bf16 planes of an operand, the six-product plane
    GEMM of both layers, its true-f64 statement, the outputs a wrong kernel would leave, and three input families on which
    f32 accumulation is exact in any order; asserted on the oracle alone in tests/test_oracle_selfchecks.py as well.
  * salad_stage_a.py        — stage A (Sinkhorn, V = F^T P^T on hi/lo planes, three normalisations) per element: the f64
    statement with its intermediates, the kernels' arithmetic in plain torch f32, one-hot feature probes that read single
    entries of the transport plan, a per-element bound derived from a stated rounding model, and the outputs a wrong kernel
    would leave; asserted on the oracle alone in tests/test_salad_stage_a_cpu.py.
  * knn.py                  — PARITY UNPINNED by the reference: it has no retrieval code at all
    (SURVEY.md fact 3).  Brute-force definition of the stage's contract.
"""
