#!/usr/bin/env python3
"""Generates tests/golden/exact_vectors_edges.json from the exact big-integer model (exact_model.py) at the structured and extreme
operands of tests/edge_operands.py -- no oracle, no product code.

exact_vectors.json pins the oracle (and the HIP path) on uniformly random operands; this fixture pins them where the lazy arithmetic
of both is argued from worst cases: every residue q - 1, digits that are all q_j - 1, key-switch keys that are all q_t - 1 or the
identity on one digit, and coefficients planted on the edges of every floor.  Per case (ring, chain) a few (operand families, key kind)
pairs; per pair: multiply, relinearize of a size-3 ciphertext of the family, its rescale, multiply -> relinearize -> rescale, the
rescale of the size-3 ciphertext, one rotation and the NAF rotation by 3 (CKKS); relinearize, the BEHZ multiply, its relinearization
and the two rotations (BFV).  Expected outputs are stored as in exact_vectors.json: SHA-256 of the little-endian u64 array plus the
first coefficients of every residue polynomial.

The inputs are built by `build_inputs` below from a context-like object -- here the exact model's own ring (its NTT by recursive
splitting), in tests/test_edge_operands_cpu.py the oracle, in tests/test_gpu_edge_operands.py the oracle again -- so all sides work on
identical data; the uniform parts come from the splitmix64 stream of exact_inputs.py, not from a library generator.
Usage: python tests/golden/make_exact_vectors_edges.py   (a few minutes)."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import edge_operands as eo  # noqa: E402
import exact_inputs as xi  # noqa: E402

# name, scheme, N, key-level bit sizes, seed, pairs of (family of a, family of b and of the size-3 ciphertext, key kind, j0)
CASES = [
    # fold chain {60, 40, 60}: the u64 engine's fold build around one fp64-engine prime
    dict(name="ckks_n1024_60_40_60", scheme="ckks", N=1024, bits=[60, 40, 60], seed=0xED01,
         pairs=[("qm1", "qm1_coeff", "qm1", 0), ("planted", "planted", "identity", 0)]),
    # fold chain {60, 45, 45, 60} at N1 = 2: a column pass in front of the row pass
    dict(name="ckks_n2048_60_45_45_60", scheme="ckks", N=2048, bits=[60, 45, 45, 60], seed=0xED02,
         pairs=[("qm1_coeff", "alt", "uniform", 0), ("half", "half1", "identity", 2)]),
    # primes of 50 .. 59 bits: the Shoup build of the u64 engine (kAccRun = 6)
    dict(name="ckks_n1024_55_52_50_58", scheme="ckks", N=1024, bits=[55, 52, 50, 58], seed=0xED03,
         pairs=[("qm1", "qm1_coeff", "qm1", 0), ("alt_half", "impulseN1_coeff", "identity", 2)]),
    # 46- and 47-bit primes: fp64-engine primes whose digit lifts re-centre; the special prime (46 bits) is below q_2 (60 bits), so
    # identity(2) drives the mod-down through every residue edge at quotients up to 2^14
    dict(name="ckks_n2048_46_47_60_46", scheme="ckks", N=2048, bits=[46, 47, 60, 46], seed=0xED04,
         pairs=[("qm1_coeff", "qm1", "qm1", 0), ("planted", "planted", "identity", 2)]),
    dict(name="bfv_n1024_60_40_60", scheme="bfv", N=1024, bits=[60, 40, 60], seed=0xED05,
         pairs=[("qm1", "qm1", "qm1", 0), ("planted", "alt", "identity", 1)]),
]


class SeededRng:
    """the one call of numpy's Generator that edge_operands makes -- integers(0, q, size, dtype) -- served from exact_inputs' stream"""

    def __init__(self, seed, tag):
        self.seed, self.tag = seed, tag

    def integers(self, lo, hi, size, dtype=np.uint64):
        assert lo == 0
        shape = (size,) if isinstance(size, int) else tuple(size)
        self.tag += 1
        return xi.uniform_poly_np(self.seed, self.tag, int(hi), int(np.prod(shape))).reshape(shape)


def pair_label(p):
    fa, fb, kind, j0 = p
    return f"{fa}.{fb}.{kind}{j0 if kind == 'identity' else ''}"


def galois_elt(step, N):
    m = 2 * N
    return pow(3, step, m) if step > 0 else pow(3, N // 2 - (-step), m)


def build_inputs(case, ctx, pair):
    """the operands of one pair as numpy arrays: a, b [2, L, N], c3 [3, L, N], rk and the Galois keys of 1, -1, 4 ([Ltop][2][K][N])"""
    fa, fb, kind, j0 = pair
    L, N = ctx.L, ctx.N
    cf = case["scheme"] == "bfv"
    rng = SeededRng(case["seed"], 1000 * case["pairs"].index(pair))
    d = dict(a=eo.family(ctx, fa, L, 2, rng, coeff_form=cf), b=eo.family(ctx, fb, L, 2, rng, coeff_form=cf),
             c3=eo.family(ctx, fb, L, 3, rng, coeff_form=cf), rk=eo.key(ctx, kind, rng, j0))
    if kind == "identity":  # the digit the identity key selects, planted on every edge of the mod-down's floor
        d["c3"][2] = eo.planted_digit(ctx, L, j0, rng, coeff_form=cf)
        d["a"][1] = eo.planted_digit(ctx, L, j0, rng, coeff_form=cf)
    d["gk"] = {galois_elt(s, N): eo.key(ctx, kind, rng, j0) for s in (1, -1, 4)}
    return d


def run_ops(case, d, ops):
    """ops: the evaluator calls (the exact model here, the oracle and the HIP path in the tests); yields (name, result)"""
    N = case["N"]
    a, b, c3, rk, gk = d["a"], d["b"], d["c3"], d["rk"], d["gk"]
    g1, gm1, g4 = galois_elt(1, N), galois_elt(-1, N), galois_elt(4, N)
    rl = ops.relinearize(c3, rk)
    yield "relinearize", rl
    if case["scheme"] == "ckks":
        m3 = ops.multiply(a, b)
        yield "multiply", m3
        yield "relinearize_rescale", ops.rescale(rl)
        yield "multiply_relin_rescale", ops.rescale(ops.relinearize(m3, rk))
        yield "rescale_size3", ops.rescale(c3)
    else:
        m3 = ops.multiply(a, b)  # BEHZ
        yield "bfv_multiply", m3
        yield "bfv_multiply_relin", ops.relinearize(m3, rk)
    yield "rotate_1", ops.apply_galois(a, g1, gk[g1])
    yield "rotate_3_naf", ops.apply_galois(ops.apply_galois(a, gm1, gk[gm1]), g4, gk[g4])


def main():
    from exact_model import Model
    from make_exact_vectors import digest, head
    from make_primes import coeff_modulus_create, get_primes

    class ModelCtx:  # what edge_operands needs of a context, from the exact model's ring
        def __init__(self, M, primes):
            self.M, self.N, self.moduli, self.L = M, M.N, primes, len(primes) - 1

        def ntt(self, i, v):
            return np.array(self.M.R.ntt(i, [int(x) for x in v]), dtype=np.uint64)

        def intt(self, i, v):
            return np.array(self.M.R.intt(i, [int(x) for x in v]), dtype=np.uint64)

    class ModelOps:
        def __init__(self, M, t):
            self.M, self.t = M, t

        def multiply(self, a, b):
            return self.M.multiply_ckks(a, b) if self.M.ntt_form else self.M.bfv_multiply(a, b, self.t)

        def relinearize(self, c3, rk): return self.M.relinearize(c3, rk)
        def rescale(self, ct): return self.M.rescale(ct)
        def apply_galois(self, ct, g, key): return self.M.apply_galois(ct, g, key)

    doc = {}
    for case in CASES:
        t0 = time.time()
        N, bits = case["N"], case["bits"]
        primes = coeff_modulus_create(N, bits)
        ckks = case["scheme"] == "ckks"
        M = Model(N, primes, ntt_form=ckks)
        ctx = ModelCtx(M, primes)
        t = 0 if ckks else get_primes(2 * N, 20, 1)[0]
        out = {"N": N, "bits": bits, "scheme": case["scheme"], "seed": case["seed"], "primes": [hex(p) for p in primes],
               "pairs": [pair_label(p) for p in case["pairs"]], "expected": {}}
        if not ckks:
            out["plain_modulus"] = t
        for pair in case["pairs"]:
            d = build_inputs(case, ctx, pair)
            lists = {k: (v.tolist() if isinstance(v, np.ndarray) else {g: x.tolist() for g, x in v.items()}) for k, v in d.items()}
            for name, ct in run_ops(case, lists, ModelOps(M, t)):
                out["expected"][pair_label(pair) + ":" + name] = {"sha256": digest(ct), "shape": [len(ct), len(ct[0]), N], "head": head(ct)}
        doc[case["name"]] = out
        print(case["name"], "%.1f s" % (time.time() - t0), file=sys.stderr)
    with open(os.path.join(HERE, "exact_vectors_edges.json"), "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
