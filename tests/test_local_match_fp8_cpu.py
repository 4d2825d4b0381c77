"""CPU: the e4m3 form of local-feature re-ranking (include/vpr_amd_patch_fp8.h) — header, binding table and exported symbols
agree and the older tables are what they were; every refusal comes back with its status in the stated order before a device
is touched and leaves the outputs alone; the workspace query is monotone; the bit-level restatement of the quantiser
(tests/local_match_fp8_ref.py) equals torch's float8_e4m3fn cast of the clamped value on every bf16 pattern and on f32 edge
values; the LDS swizzle of the match kernel is conflict-free for every width of both element types; the torch ops have fake
implementations and export; the wrappers, the gallery format and the sharded searches take the e4m3 store; the recipe the
GPU tests use keeps its answers after the quantisation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import local_match_fp8_ref as ref8
import local_match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def test_header_table_and_symbols_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_patch_fp8.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    assert "vpr_local" not in header and "include/vpr_amd_local.h" in header      # the bf16 contract by file, never by symbol
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.PATCH_FP8_PROTOTYPES) == {"vpr_patch_quantize_fp8", "vpr_patch_workspace_bytes_fp8",
                                                          "vpr_patch_rerank_fp8"}
    for name, (restype, argtypes) in _lib.PATCH_FP8_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    assert len(_lib.PATCH_FP8_PROTOTYPES["vpr_patch_rerank_fp8"][1]) == 22
    assert _lib.PATCH_FP8_PROTOTYPES["vpr_patch_rerank_fp8"][1] == _lib.LOCAL_PROTOTYPES["vpr_local_rerank"][1]
    const = lambda n: int(re.search(rf"#define {n} (\d+)", code).group(1))
    assert const("VPR_PATCH_FP8_SHIFT") == _lib.PATCH_FP8_SHIFT == ref8.SHIFT == 8
    assert const("VPR_PATCH_FP8_MIN_L") == _lib.PATCH_FP8_MIN_L == 64 and const("VPR_PATCH_FP8_MAX_L") == _lib.PATCH_FP8_MAX_L == 256
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.LOCAL_PROTOTYPES) == {"vpr_local_workspace_bytes", "vpr_local_rerank"} and len(_lib.PROTOTYPES) == 61
    assert set(_lib.RERANK_PROTOTYPES) == {"vpr_rerank_workspace_bytes", "vpr_rerank_rows"}
    assert set(_lib.SALAD_F32_STAGES_PROTOTYPES) == {"vpr_salad_f32_stage_outputs"}
    new = set(_lib.PATCH_FP8_PROTOTYPES)
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES, _lib.RERANK_PROTOTYPES,
                  _lib.SALAD_STAGES_PROTOTYPES, _lib.SALAD_ANYRES_PROTOTYPES, _lib.SALAD_HIRES_PROTOTYPES, _lib.LOCAL_PROTOTYPES,
                  _lib.SALAD_F32_STAGES_PROTOTYPES):
        assert not new & set(older)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "vpr_amd_patch_fp8.h":
            assert not re.search(r"vpr_patch_|_fp8\.h", open(os.path.join(ROOT, "include", other)).read()), other


def test_refusals_come_back_without_a_device_and_write_nothing(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 8192)()
    ctypes.memset(buf, 0xA5, 8192)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 8)                       # 8-byte aligned only
    odd2 = ctypes.c_void_p(p.value + 2)                      # not even 4-byte aligned
    odd1 = ctypes.c_void_p(p.value + 1)
    big = 1 << 40
    nan = float("nan")

    def call(q=p, n_q=16, idx=p, B=1, kc=10, g=p, n_g=16, l=64, n_local=5, base=0, min_sim=0.0, k=3, vals=p, out=p, mt=p,
             ps=null, pm=null, rn=null, cn=null, ws=p, ws_bytes=big):
        st = lib.vpr_patch_rerank_fp8(q, n_q, idx, B, kc, g, n_g, l, n_local, base, min_sim, k, vals, out, mt, ps, pm, rn, cn, ws,
                                      ws_bytes, null)
        assert bytes(buf) == b"\xa5" * 8192, "a refused call (and B == 0) writes nothing"
        return st

    for kw in (dict(q=null), dict(idx=null), dict(g=null), dict(vals=null), dict(out=null), dict(ws=null), dict(B=-1), dict(n_q=-1),
               dict(n_g=-5), dict(l=-64), dict(kc=-1, k=1), dict(n_local=-1), dict(base=-1), dict(k=0), dict(k=11), dict(k=-2),
               dict(kc=0, k=0), dict(min_sim=nan), dict(B=0, q=null),
               # double faults: the invalid argument is reported ahead of what is merely unsupported
               dict(kc=200, k=201), dict(q=null, l=96), dict(k=0, n_q=300), dict(min_sim=nan, ws_bytes=0), dict(base=-1, q=odd),
               dict(n_local=-1, kc=129, k=1)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(kc=129, k=1), dict(kc=129, k=129), dict(n_q=0), dict(n_g=0), dict(n_q=257), dict(n_g=257), dict(n_g=1 << 20),
               dict(l=0), dict(l=16), dict(l=32), dict(l=48), dict(l=96), dict(l=160), dict(l=224), dict(l=320), dict(l=1 << 20),
               dict(q=odd), dict(g=odd), dict(ws=odd),
               dict(idx=odd2), dict(vals=odd2), dict(out=odd2), dict(mt=odd2), dict(ps=odd2), dict(pm=odd2), dict(rn=odd2), dict(cn=odd2),
               dict(ws_bytes=0),
               # double faults: a shape or alignment fault together with a short workspace is still UNSUPPORTED
               dict(l=96, ws_bytes=0), dict(q=odd, ws_bytes=0), dict(n_q=257, l=32)):
        assert call(**kw) == UNSUPPORTED, kw
    for B, kc in ((1, 1), (1, 10), (64, 64), (37, 128), (100000, 128)):                # workspace: one byte short is refused
        need = lib.vpr_patch_workspace_bytes_fp8(B, kc)
        assert need >= 8 * B * kc and call(B=B, kc=kc, k=1, ws_bytes=need - 1) == UNSUPPORTED
    # what the rules leave alone: B = 0 launches nothing; the largest legal sizes; element-aligned lists; no matches_out
    assert call(B=0) == 0 and call(B=0, n_q=256, n_g=256, l=256, kc=128, k=128) == 0 and call(B=0, n_q=1, n_g=1, l=64, kc=1, k=1) == 0
    assert call(B=0, idx=odd, vals=odd, out=odd, mt=null) == 0 and call(B=0, n_local=0, base=2 ** 31 - 1) == 0
    assert call(B=0, ps=p, pm=p, rn=p, cn=p, min_sim=float("inf")) == 0 and call(B=0, min_sim=-float("inf")) == 0
    assert call(B=0, ws_bytes=lib.vpr_patch_workspace_bytes_fp8(0, 10)) == 0
    for l in (64, 128, 192, 256):
        assert call(B=0, l=l) == 0

    # the quantiser: NULL and a negative count are invalid, a misaligned x unsupported, count 0 fine; nothing is written
    def quant(x=p, bf16=0, count=5, out=p):
        st = lib.vpr_patch_quantize_fp8(x, bf16, count, out, null)
        assert bytes(buf) == b"\xa5" * 8192
        return st

    for kw in (dict(x=null), dict(out=null), dict(count=-1), dict(count=-(1 << 40)), dict(x=null, count=0), dict(x=odd1, count=-1),
               dict(x=null, out=null, bf16=1)):
        assert quant(**kw) == INVALID, kw
    for kw in (dict(x=odd2), dict(x=odd1), dict(x=odd1, bf16=1), dict(x=odd2, count=0), dict(x=odd1, bf16=1, count=0)):
        assert quant(**kw) == UNSUPPORTED, kw
    assert quant(count=0) == 0 and quant(count=0, bf16=1, x=odd2, out=odd1) == 0 and quant(count=0, x=odd, out=odd1) == 0


def test_workspace_query_is_monotone(lib):
    w = lib.vpr_patch_workspace_bytes_fp8
    for kc in (1, 2, 63, 64, 65, 128):
        sizes = [w(B, kc) for B in list(range(0, 300)) + [4096, 65536, 1 << 20]]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), kc
    for B in (0, 1, 3, 37, 64, 5000):
        sizes = [w(B, kc) for kc in range(1, 129)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), B
        assert sizes == [lib.vpr_local_workspace_bytes(B, kc) for kc in range(1, 129)]      # the rule of the bf16 form
    for B, kc in ((-1, 10), (1, 0), (1, -3), (1, 129), (64, 1000), (-5, 200)):
        assert w(B, kc) == 0, (B, kc)


# --------------------------------------------------------------------------------------------------- the quantiser
def torch_cast(x32):
    """torch's float8_e4m3fn cast of the clamped scaled value; the non-finite inputs are the contract's own rule."""
    t = torch.from_numpy(x32)
    b = (t * 256).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    b[~np.isfinite(x32)] = 0x7F
    return b


def test_quantiser_restatement_is_the_e4m3_cast_of_the_clamped_value():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.uint16).view(torch.bfloat16)      # every bf16 pattern
    got = ref8.quantize(bits)
    assert np.array_equal(got, torch_cast(bits.float().numpy()))
    edges = ref8.f32_edges()
    got = ref8.quantize(edges)
    want = torch_cast(edges)
    assert np.array_equal(got, want), [(float(e), hex(g), hex(w)) for e, g, w in zip(edges, got, want) if g != w][:8]
    # the named cases, by hand
    q = lambda *v: ref8.quantize(np.array(v, dtype=np.float32)).tolist()
    assert q(0.0, -0.0, 1.0, -1.0) == [0x00, 0x80, 0x78, 0xF8]                      # 256 = 2^8: exponent field 15, mantissa 0
    assert q(1.75, 1.76, 2.0, 1e30, -1.76, -3e38) == [0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0xFE]   # 448 and everything beyond
    assert q(np.nan, np.inf, -np.inf) == [0x7F, 0x7F, 0x7F]
    assert q(2.0 ** -17, 2.0 ** -18, -(2.0 ** -18), 1.5 * 2.0 ** -17, 2.5 * 2.0 ** -17) == [0x01, 0x00, 0x80, 0x02, 0x02]   # ties to even
    assert q(7.5 * 2.0 ** -17, 2.0 ** -14) == [0x08, 0x08]                          # the last subnormal tie goes up to the first normal
    # the decode table inverts it on every finite byte, and only 0x7F / 0xFF are NaN
    finite = np.isfinite(ref8.BYTE_VALUE)
    assert finite.sum() == 254 and not finite[0x7F] and not finite[0xFF]
    b = np.arange(256, dtype=np.uint8)[finite]
    assert np.array_equal(ref8.quantize(ref8.DECODE[b].astype(np.float32)), b)
    assert ref8.BYTE_VALUE[0x7E] == 448 and ref8.BYTE_VALUE[0x01] == 2.0 ** -9 and ref8.DECODE[0x78] == 1.0
    # a stop at bf16 before the cast rounds twice: it changes bytes, so the quantiser must start from f32
    x = ref.unit(np.random.default_rng(1).standard_normal((64, 128))).astype(np.float32)
    twice = ref8.quantize(torch.from_numpy(x).to(torch.bfloat16))
    changed = (twice != ref8.quantize(x)).mean()
    print("bytes changed by a bf16 stop:", changed)
    assert 0.01 < changed < 0.06
    assert np.array_equal(ref8.encode_ints([-2, -1, 0, 1, 2]), [0xC0, 0xB8, 0x00, 0x38, 0x40])


# ---------------------------------------------------------------------------------------------------- the LDS swizzle
def lm_off(row, chunk, cpr):
    """csrc/local_match.hip::lm_off: chunk c of row r sits at chunk c ^ ((r >> SH) & MASK) of its row of cpr 16-byte chunks."""
    sh, mask = (0, 15) if cpr % 16 == 0 else (1, 7) if cpr % 8 == 0 else (2, 3)
    return (row * cpr + (chunk ^ ((row >> sh) & mask))) << 4


def test_lds_swizzle_is_conflict_free():
    """Every ds_read_b128 lane group (16 lanes served together; tests/test_library_cpu.py has the groups) of the B-operand reads
    must hit 16 distinct 16-byte slots of the 256-byte bank row: e4m3 rows of l bytes, the two reads of a lane's 32 K-bytes
    (chunks 4 ks + 2 h and 4 ks + 2 h + 1, h = lane >> 5); bf16 rows of 2 l bytes, one read (chunk 2 ks + h).  Every column
    tile, every k-step, every supported width; and the XOR is a bijection inside the row that keeps an e4m3 pair together."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[x + 32 for x in g] for g in groups]
    for l in (64, 128, 192, 256):
        cpr = l // 16
        assert cpr in (4, 8, 12, 16)
        for jt in range(8):
            for ks in range(l // 64):
                for which in (0, 1):
                    for g in groups:
                        slots = {(lm_off(jt * 32 + (ln & 31), 4 * ks + 2 * (ln >> 5) + which, cpr) // 16) % 16 for ln in g}
                        assert len(slots) == 16, (l, jt, ks, which)
    for l in range(32, 257, 32):
        cpr = l // 8
        for jt in range(8):
            for ks in range(l // 16):
                for g in groups:
                    slots = {(lm_off(jt * 32 + (ln & 31), 2 * ks + (ln >> 5), cpr) // 16) % 16 for ln in g}
                    assert len(slots) == 16, (l, jt, ks)
    for cpr in (4, 8, 12, 16, 20, 24, 28, 32):
        for row in range(256):
            phys = [lm_off(row, c, cpr) // 16 - row * cpr for c in range(cpr)]
            assert sorted(phys) == list(range(cpr))                                  # inside the row, onto the row
            assert all(phys[c] >> 1 == phys[c + 1] >> 1 for c in range(0, cpr, 2))   # chunks 2 m, 2 m + 1: one 32-byte pair


# ------------------------------------------------------------------------------------------------------- the ops
def test_fake_ops_give_shapes_and_dtypes_and_export():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert {"patch_quantize_fp8", "local_rerank_fp8"} <= set(torch_ops.OPS)
    schema = str(torch.ops.vpr.local_rerank_fp8.default._schema)
    assert schema.startswith("vpr::local_rerank_fp8(") and "int index_base=0" in schema.replace("Int", "int")
    assert "k=None" in schema and "float min_sim=0" in schema.replace("Float", "float")
    assert str(torch.ops.vpr.patch_quantize_fp8.default._schema).startswith("vpr::patch_quantize_fp8(Tensor x) -> Tensor")
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        idx = mk(37, 64, dtype=torch.int32)
        for dt in (torch.float32, torch.bfloat16):
            b = torch.ops.vpr.patch_quantize_fp8(mk(37, 256, 128, dtype=dt))
            assert b.shape == (37, 256, 128) and b.dtype == torch.uint8 and b.device.type == "cuda"
        assert torch.ops.vpr.patch_quantize_fp8(mk(5, dtype=torch.float32)).shape == (5,)
        q, g = mk(37, 256, 128, dtype=torch.uint8), mk(500, 196, 128, dtype=torch.uint8)
        for args, k in (((q, idx, g), 64), ((q, idx, g, 1000), 64), ((q, idx, g, 0, 10), 10), ((q, idx, g, 7, 1, 0.5), 1)):
            v, i, m = torch.ops.vpr.local_rerank_fp8(*args)
            assert v.shape == i.shape == m.shape == (37, k) and v.device.type == "cuda"
            assert v.dtype == torch.float32 and i.dtype == torch.int32 and m.dtype == torch.int32

    class Rerank(torch.nn.Module):
        def forward(self, q, idx, g):
            v, i, m = torch.ops.vpr.local_rerank_fp8(torch.ops.vpr.patch_quantize_fp8(q), idx, g, 3, 5, 0.25)
            return v * 2, i, m

    ep = torch.export.export(Rerank(), (torch.zeros(4, 64, 64, dtype=torch.bfloat16), torch.zeros(4, 8, dtype=torch.int32),
                                        torch.zeros(9, 50, 64, dtype=torch.uint8)))
    assert "vpr.local_rerank_fp8" in str(ep.graph) and "vpr.patch_quantize_fp8" in str(ep.graph)
    assert [tuple(n.meta["val"].shape) for n in ep.graph.nodes if n.op == "output" for n in n.args[0]] == [(4, 5)] * 3


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    B, n, l, kc, N = 2, 16, 64, 4, 5
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    q, i, g = u8(B, n, l), torch.zeros(B, kc, dtype=torch.int32), u8(N, n, l)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.local_rerank_fp8(q, i, g)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.local_rerank_fp8(q, i, g)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.quantize_patch_fp8(torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.patch_quantize_fp8(torch.zeros(3, 4, dtype=torch.bfloat16))
    # the remaining checks, with the device test answered "yes": nothing below reaches the library
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    for bad, match in (((q.float(), i, g), "q_local: expected dtype"), ((q, i, g.float()), "g_local: expected dtype"),
                       ((bf(B, n, l), i, g), "q_local: expected dtype"), ((q, i, bf(N, n, l)), "g_local: expected dtype"),
                       ((q.view(torch.int8), i, g), "q_local: expected dtype"), ((q, i.long(), g), "idx: expected dtype"),
                       ((q[0], i, g), "q_local: expected 3 dims"), ((q, i[0], g), "idx: expected 2 dims"), ((q, i, g[0]), "g_local: expected 3 dims"),
                       ((q, i[:, :2], g), "contiguous"), ((q[:, :, :16], i, g), "contiguous"),
                       ((q[:1], i, g), "disagree on B"), ((q, i, u8(N, n, 128)), "disagree on l"),
                       ((u8(B, n, 32), i, u8(N, n, 32)), "multiple of 64"), ((u8(B, n, 96), i, u8(N, n, 96)), "multiple of 64"),
                       ((u8(B, n, 320), i, u8(N, n, 320)), "multiple of 64"),
                       ((u8(B, 257, l), i, g), "q_local must hold 1..256 patches"), ((q, i, u8(N, 257, l)), "g_local must hold 1..256 patches"),
                       ((u8(B, 0, l), i, g), "q_local must hold 1..256 patches"),
                       ((q, torch.zeros(B, 129, dtype=torch.int32), g), "1..128 candidates"),
                       ((q, torch.zeros(B, 0, dtype=torch.int32), g), "1..128 candidates")):
        with pytest.raises(RuntimeError, match=match):
            ops.local_rerank_fp8(*bad)
    for kw, match in ((dict(k=0), "k must be"), (dict(k=kc + 1), "k must be"), (dict(k=-1), "k must be"),
                      (dict(min_sim=float("nan")), "min_sim must be")):
        with pytest.raises(RuntimeError, match="local_rerank_fp8: " + match):
            ops.local_rerank_fp8(q, i, g, **kw)
    for bad, match in ((torch.zeros(4, dtype=torch.float64), "expected dtype"), (torch.zeros(4, dtype=torch.uint8), "expected dtype"),
                       (torch.zeros(4, 8)[:, :3], "contiguous")):
        with pytest.raises(RuntimeError, match=match):
            ops.quantize_patch_fp8(bad)


# ------------------------------------------------------------------------------------------------- gallery format
def test_gallery_round_trips_keep_one_local_file(tmp_path):
    from vpr_amd import gallery as G
    rng = np.random.default_rng(5)
    N, D, n, l = 23, 128, 9, 64
    rows = torch.from_numpy(rng.standard_normal((N, D))).to(torch.bfloat16)
    local = torch.from_numpy(ref.unit(rng.standard_normal((N, n, l)))).to(torch.bfloat16)
    local8 = ref8.quantize_t(local)
    labels = rng.standard_normal((N, 4))
    assert G.LOCAL_FP8_FILE == "local_features_fp8.npy" and G.LOCAL_FP8_FILE in G.__doc__ and "local_features.npy" in G.__doc__
    d = str(tmp_path / "g")
    has = lambda: (os.path.exists(os.path.join(d, G.LOCAL_FILE)), os.path.exists(os.path.join(d, G.LOCAL_FP8_FILE)))
    cpu = torch.device("cpu")
    G.save_gallery(d, rows, labels, local=local8)                                   # the e4m3 file only
    assert has() == (False, True)
    stored = np.load(os.path.join(d, G.LOCAL_FP8_FILE))
    assert stored.dtype == np.uint8 and stored.shape == (N, n, l) and np.array_equal(stored, local8.numpy())
    assert stored.nbytes * 2 == local.numel() * 2                                   # half the bf16 store
    assert G.load_gallery_shard(d, cpu).local is None                               # load_local defaults to False
    for rank, world in ((0, 1), (0, 3), (1, 3), (2, 3)):
        s = G.load_gallery_shard(d, cpu, rank, world, load_local=True)
        lo, hi = N * rank // world, N * (rank + 1) // world
        assert s.index_base == lo and s.local.dtype == torch.uint8 and torch.equal(s.local, local8[lo:hi])
        sg = G.sharded_gallery_from(s, rank, world)
        assert sg.local_feats is s.local
    G.save_gallery(d, rows, labels, local=local)                                    # written over with bf16: the e4m3 file goes
    assert has() == (True, False)
    s = G.load_gallery_shard(d, cpu, load_local=True)
    assert s.local.dtype == torch.bfloat16 and torch.equal(s.local, local)
    G.save_gallery(d, rows, labels, local=local8)                                   # and back: the bf16 file goes
    assert has() == (False, True) and G.load_gallery_shard(d, cpu, load_local=True).local.dtype == torch.uint8
    G.save_gallery(d, rows, labels)                                                 # without: neither stays
    assert has() == (False, False)
    with pytest.raises(ValueError, match="no local_features.npy"):
        G.load_gallery_shard(d, cpu, load_local=True)
    for bad in (local8[:20], local8.float(), local8.to(torch.int8), local8.to(torch.int32), local8[0], local8[:, 0]):
        with pytest.raises(ValueError, match="local must be"):
            G.save_gallery(str(tmp_path / "bad"), rows, labels, local=bad)


# ------------------------------------------------------------------------ search_local_reranked, CPU engine
class CpuEngine:
    """oracle/knn.py searches and merge; the local re-ranks and the quantiser are the restatements."""

    def __init__(self):
        self.quantised = []

    def local_topk(self, q, gallery, k, index_base, scales=None):
        from oracle import knn as oknn
        return oknn.knn_topk(q, gallery, k, index_base)

    def merge(self, vals, idxs):
        from oracle import knn as oknn
        return oknn.topk_merge(vals, idxs)

    def local_rerank(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0):
        assert q_local_feats.dtype == local_feats.dtype == torch.bfloat16
        out = ref.local_rerank(q_local_feats, idx, local_feats, index_base, k, min_sim)
        return torch.from_numpy(out["vals"]), torch.from_numpy(out["idx"]), torch.from_numpy(out["matches"])

    def local_rerank_fp8(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0):
        assert q_local_feats.dtype == local_feats.dtype == torch.uint8 and q_local_feats.is_contiguous()
        out = ref8.local_rerank_fp8(q_local_feats, idx, local_feats, index_base, k, min_sim)
        return torch.from_numpy(out["vals"]), torch.from_numpy(out["idx"]), torch.from_numpy(out["matches"])

    def quantize_patch_fp8(self, feats):
        self.quantised.append(tuple(feats.shape))
        return ref8.quantize_t(feats)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_search_local_reranked_on_an_e4m3_gallery_is_the_restatement_on_the_coarse_union(monkeypatch, R):
    """Shards of N = 83 rows at the uneven cuts of shard_bounds; the collective is replaced by a stack of every rank's list.
    bf16 query features are quantised once at entry; uint8 ones are taken as they are; the two give identical results."""
    from vpr_amd import retrieval
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    N, D, B, n, l, kc, k = 83, 64, 5, 12, 64, 8, 5
    rows, local, q, ql, true = ref.places(11 + R, N, D, B, n, l)
    local8, ql8 = ref8.quantize_t(local), ref8.quantize_t(ql)
    eng = CpuEngine()
    shards = []
    for r in range(R):
        lo, hi = shard_bounds(N, r, R)
        shards.append(ShardedGallery(rows[lo:hi], N, r, R, engine=eng, local_feats=local8[lo:hi], force_collectives=R == 1))
    union = torch.cat([eng.local_topk(q, sg.rows, kc, sg.index_base)[1] for sg in shards], 1)
    want = ref8.local_rerank_fp8(ql8, union, local8, 0, k, 0.3)
    for feats in (ql, ql8):
        sent = {}

        def record(v, i, world, group=None):                     # first pass: what each rank would send
            sent[rank] = (v.clone(), i.clone())
            return torch.stack([v] * world), torch.stack([i] * world)

        def stacked(v, i, world, group=None):                    # second pass: every rank receives all of them, in rank order
            assert torch.equal(v, sent[rank][0]) and torch.equal(i, sent[rank][1])
            return torch.stack([sent[r][0] for r in range(world)]), torch.stack([sent[r][1] for r in range(world)])

        for fn in (record, stacked):
            monkeypatch.setattr(retrieval, "all_gather_topk", fn)
            results = []
            eng.quantised.clear()
            for rank, sg in enumerate(shards):
                results.append(sg.search_local_reranked(q, k, kc, feats, 0.3))
            assert eng.quantised == ([(B, n, l)] * R if feats is ql else [])         # once per call, never for bytes
        for v, i in results:                                     # the same on every rank, for either kind of query features
            assert np.array_equal(i.numpy(), want["idx"]) and np.array_equal(v.numpy().view(np.int32), want["vals"].view(np.int32))
    assert np.array_equal(want["idx"][:, 0], true) and (want["matches"][:, 0] == n).all()
    # the data-parallel form quantises BEFORE the query gather: bytes are what travels
    sg = shards[0]
    seen = []
    monkeypatch.setattr(sg, "gather_queries", lambda t: (seen.append((t.dtype, tuple(t.shape))), t)[1])
    if R == 1:
        monkeypatch.setattr(retrieval, "all_gather_topk", lambda v, i, world, group=None: (v[None], i[None]))
        for feats in (ql, ql8):
            seen.clear()
            v, i = sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=feats, min_sim=0.3)
            assert (torch.uint8, (B, n, l)) in seen and (torch.bfloat16, (B, n, l)) not in seen
            assert np.array_equal(i.numpy(), want["idx"]) and np.array_equal(v.numpy(), want["vals"])


def test_sharded_wrappers_refuse_what_they_cannot_take():
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    N, D, B, n, l = 6, 64, 2, 5, 64
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    rows, local, q, ql = bf(N, D), u8(N, n, l), bf(B, D), u8(B, n, l)
    with pytest.raises(ValueError, match="local_feats must be"):
        ShardedGallery(rows, N, local_feats=local[:4])
    with pytest.raises(ValueError, match="^local_feats: bf16"):
        ShardedGallery(rows, N, local_feats=local.float())
    with pytest.raises(ValueError, match="^local_feats: bf16"):
        ShardedGallery(rows, N, local_feats=local.to(torch.int8))
    sg = ShardedGallery(rows, N, engine=CpuEngine(), local_feats=local, fine_rows=rows)
    for args, match in (((q, 3, 65, ql), "at most 64"), ((q, 5, 4, ql), "1..kc"), ((q, 2, 4, u8(B, n, 128)), "wide"),
                        ((q, 2, 4, u8(B + 1, n, l)), "disagree on B"), ((q, 2, 4, ql.float()), "must be bf16 or uint8"),
                        ((q, 2, 4, ql[0]), "must be bf16 or uint8"), ((q, 2, 4, None), "must be bf16 or uint8"),
                        ((q, 2, 4, u8(B, 257, l)), "at most 256 patches")):
        with pytest.raises(ValueError, match=match):
            sg.search_local_reranked(*args)
    # a bf16 gallery still takes bf16 query features only
    sgb = ShardedGallery(rows, N, engine=CpuEngine(), local_feats=bf(N, n, l))
    with pytest.raises(ValueError, match="must be bf16 \\["):
        sgb.search_local_reranked(q, 2, 4, ql)
    for call in (lambda: sg.search_gathered(q, 2, rerank=4, local_rerank=4, q_local_feats=ql),
                 lambda: sg.search_local_queries(q, 2, None, 4, local_rerank=4, q_local_feats=ql)):
        with pytest.raises(ValueError, match="local_rerank and rerank"):
            call()
    with pytest.raises(ValueError, match="does not combine with expand"):
        sg.search_gathered(q, 2, (2, 3.0), local_rerank=4, q_local_feats=ql)
    with pytest.raises(ValueError, match="needs q_local_feats"):
        sg.search_local_queries(q, 2, local_rerank=4)
    with pytest.raises(ValueError, match="neither with rerank nor with expand"):
        GraphedRetrieval(sg, B, 2, rerank=4, local_rerank=4)
    from vpr_amd.modules import DinoV2Salad, SaladAggregator
    agg = SaladAggregator(64, hidden=64)
    with pytest.raises(ValueError, match="at most 256"):
        agg.local_features(torch.zeros(1, 257, 64), fp8=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):       # the quantiser is a device kernel: no CPU stand-in
        agg.local_features(torch.randn(1, 16, 64), fp8=True)
    with pytest.raises(ValueError, match="want_local must be"):
        DinoV2Salad("vit_small").features(torch.zeros(1, 3, 224, 224), want_local="bf8")
    from vpr_amd import evaluate
    with pytest.raises(ValueError, match="keep_local must be"):
        evaluate.build_gallery_from_images(None, "x.csv", ".", ".", keep_local="e4m3")


# ------------------------------------------------------------------------------------------------ the recipe
@pytest.mark.parametrize("n,l", [(64, 64), (256, 128)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recipe_separates_the_true_image_after_quantisation(seed, n, l):
    """The recipe of tests/local_match_ref.py cast to the e4m3 store: the true image still comes back first with all n patches
    matched, and with min_sim = 0.6 every distractor scores 0 at l = 128.  (e4m3 keeps 4 significant bits: a relative error of
    at most 2^-4 per entry, independent between entries, costs the cosine of a matching pair well under 1 %.)"""
    q, gal = ref.recipe(seed, n, l)
    q8, gal8 = ref8.quantize_t(q), ref8.quantize_t(gal)
    idx = torch.arange(gal.shape[0], dtype=torch.int32)[None]
    out = ref8.local_rerank_fp8(q8, idx, gal8, 0, None, 0.0)
    base = ref.local_rerank(q, idx, gal, 0, None, 0.0)
    true = gal.shape[0] - 1
    print("true", out["pair_matches"][0, true], out["pair_score"][0, true], "bf16", base["pair_score"][0, true], "distractors",
          out["pair_matches"][0, :true].max(), out["pair_score"][0, :true].max(), "row neighbours kept",
          (out["row_nn"][0] == base["row_nn"][0]).mean())
    assert out["idx"][0, 0] == true and out["matches"][0, 0] == n
    assert 0.99 * n <= out["vals"][0, 0] <= 1.004 * n
    most = n / 2 + 3 * np.sqrt(n)                                # the bf16 test's bounds on a distractor
    assert out["pair_matches"][0, :true].max() <= most
    assert out["pair_score"][0, :true].max() <= most * np.sqrt(2 * np.log(20 * n * n) / l) < 0.99 * n
    if l == 128:
        hard = ref8.local_rerank_fp8(q8, idx, gal8, 0, None, 0.6)
        assert (hard["pair_score"][0, :true] == 0).all() and (hard["pair_matches"][0, :true] == 0).all()
        assert hard["idx"][0, 0] == true and hard["matches"][0, 0] == n
