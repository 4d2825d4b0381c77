"""What v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 operands, unit block scales) keeps of a sum inside one 64-deep step and between
steps, probed with exact powers of two through ops.local_rerank_fp8 on an MI355X (needs a GPU).
Usage: python scripts/mfma_e4m3_probe.py [--out FILE]

A probe is one (query row, candidate row) pair with n_q = n_g = 1: its only similarity S is matched (min_sim far below) and the
score is S itself (the score's sum adds zeros), so pair_score * 2^16 is the accumulator the MFMA left, in units of byte-value
products.  Every probe holds one BIG product 2^16 (bytes 2^8 * 2^8) and small products 2^R; the exact sum is representable in
f32 for every line printed with exact_f32 = yes, so a single correctly rounded sum would return it.

  window   big at k = 0 and m copies of +-2^R at k = 1 ..: which R still arrive, in full or in part
  mant     big at k = 0 and ONE product 1.875 * 1.875 * 2^R = 3.515625 * 2^R (eight significant bits): what is left of it,
           (result - 2^16) / 2^R, shows where the low end of the window sits and whether it truncates or rounds
  acc      l = 128: the big product in step 0, so it reaches step 1 as the accumulator C; the m small products in step 1
  acc_rev  l = 128: the m small products in step 0 (their sum is C), the big product in step 1
  map      big at k = 5 (or 37) and ONE product 2^0 at k: got - big is 1 where k lies outside the big product's narrow window"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BIG_E = 8                       # the big product is 2^8 * 2^8


def pow2_byte(e, neg=False):
    """The e4m3fn byte of +-2^e, -9 <= e <= 8."""
    assert -9 <= e <= 8
    b = (e + 7) << 3 if e >= -6 else 1 << (e + 9)
    return b | (0x80 if neg else 0)


def split(R):
    """2^R = 2^x * 2^y with both factors e4m3 powers of two."""
    x = max(-9, min(8, R // 2))
    y = R - x
    assert -9 <= y <= 8, R
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mfma_e4m3_probe: needs a GPU")
    from vpr_amd import ops
    dev = torch.device("cuda:0")
    probes = []                 # (kind, R, m, sign, q row [128], g row [128], exact value as a Python float (f64: exact here))

    def add(kind, R, m, sign, l_used, big_k, small_k0, mant=False):
        q, g = np.zeros(128, np.uint8), np.zeros(128, np.uint8)
        q[big_k], g[big_k] = pow2_byte(BIG_E), pow2_byte(BIG_E)
        if mant:                # 1.875 * 2^x: mantissa bits 111
            x, y = split(R)
            assert x >= -6 and y >= -6
            enc = lambda e, neg: ((e + 7) << 3) | 7 | (0x80 if neg else 0)
            q[small_k0], g[small_k0] = enc(x, sign < 0), enc(y, False)
            small = sign * 3.515625 * 2.0 ** R
        else:
            x, y = split(R)
            for t in range(m):
                q[small_k0 + t], g[small_k0 + t] = pow2_byte(x, sign < 0), pow2_byte(y)
            small = sign * m * 2.0 ** R
        probes.append((kind, R, m, sign, l_used, q, g, 2.0 ** (2 * BIG_E) + small))

    for sign in (1, -1):
        for R in range(15, -19, -1):
            add("window m=1", R, 1, sign, 64, 0, 1)
            add("window m=31 same half", R, 31, sign, 64, 0, 1)          # k = 1 .. 31: the big product's lane half
            add("window m=32 other half", R, 32, sign, 64, 0, 32)        # k = 32 .. 63: the other lane half
            add("acc m=32", R, 32, sign, 128, 0, 64)
            add("acc_rev m=32", R, 32, sign, 128, 64, 0)
        for R in range(12, -13, -1):
            add("mant", R, 1, sign, 64, 0, 1, mant=True)
            add("mant other half", R, 1, sign, 64, 0, 40, mant=True)
            add("mant acc", R, 1, sign, 128, 0, 64, mant=True)
    for big_k in (5, 37):
        for k in range(64):
            if k != big_k:
                add("map big@%d small@%d" % (big_k, k), 0, 1, 1, 64, big_k, k)
    lines = ["# mfma_e4m3_probe: pair_score * 2^16 of one-similarity pairs; big = 2^16; got - big and exact - big in units of 2^R",
             "%-24s %4s %3s %4s %12s %14s %14s %6s" % ("kind", "R", "m", "sign", "exact_f32", "exact-big/2^R", "got-big/2^R", "same")]
    for l_used in (64, 128):
        sel = [p for p in probes if p[4] == l_used]
        q = torch.from_numpy(np.stack([p[5][:l_used] for p in sel]))[:, None, :].contiguous()
        g = torch.from_numpy(np.stack([p[6][:l_used] for p in sel]))[:, None, :].contiguous()
        got = []
        for lo in range(0, len(sel), 64):                          # B = 64 probes per call, candidate b of query b
            n = min(64, len(sel) - lo)
            idx = torch.arange(lo, lo + n, dtype=torch.int32)[:, None]
            out = ops.local_rerank_fp8(q[lo:lo + n].to(dev), idx.to(dev), g.to(dev), 0, None, -3.0e38, debug=True)
            got.append(out[3].pair_score[:, 0].double().cpu().numpy() * 2.0 ** 16)
        got = np.concatenate(got)
        for (kind, R, m, sign, _, _, _, exact), v in zip(sel, got):
            big = 2.0 ** (2 * BIG_E)
            in_f32 = float(np.float32(exact)) == exact
            lines.append("%-24s %4d %3d %4d %12s %14.6f %14.6f %6s" % (kind, R, m, sign, "yes" if in_f32 else "no", (exact - big) / 2.0 ** R,
                                                                      (v - big) / 2.0 ** R, "yes" if v == exact else "NO"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
