#!/usr/bin/env python3
"""RGSW selectors expanded on the device from ONE packed query ciphertext, for N = 8192 {60,40,60} (L_top = 2) and N = 32768 {60,40,40,60}
(L_top = 3), everything at L = L_top.
(a) he355_bfv_rgsw_from_bfv against its defining composition, made of calls that exist without it: per selector (its E slot ciphertexts follow
    one another) he355_bfv_transform_to_ntt into the k = 0 rows, he355_bfv_external_product(L, key_bits, E, 1, .., key, 0, 1, ..) into the k = 1
    rows and he355_bfv_transform_to_ntt of those in place.  digit_bits = 20, key_bits in {20, 10}, (n, n_sel) in {(1, 1), (1, 32), (16, 32)}.
    The two are compared bit for bit before anything is timed, then alternate inside one process (a, b, a, b, ...), every region HIP-event
    timed on the context's stream after a warm-up; min / median / max over the regions.  Acceptance: (a)'s median is not above (b)'s by more
    than the spread (max - min) of (b)'s own regions; a shape that misses is reported as open.
(c) the two-dimensional retrieval of tools/bfv_external_probe.py, section (c) (1024 entries as 32 x 32, 1 and 16 queries), with the packed
    query: ONE ciphertext per query (he355_encrypt of the first dimension plus he355_bfv_selector_encrypt of the 32 column selectors at
    first_slot = 32), expand(32 + 32 E), scan(32), rgsw_from_bfv (key_bits = 20, the key from he355_bfv_rgsw_encrypt_secret), external product
    (v = 20, inner 32), mod_switch to L = 1, one decrypt.  Time per answer set, query bytes per query against the 84148224 (N = 8192) and
    337117184 (N = 32768) bytes of the RGSW-upload route, the noise budget after every stage, and the answers against the database.
Usage: python tools/bfv_selector_probe.py [regions] [scale of the calls per region] [rings: a comma list of N]"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle as ho  # keys only: nothing timed goes through it
from tools.probe_common import At, alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1
only = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else None
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
UPLOAD_ROUTE = {8192: 84148224, 32768: 337117184}  # profiles/bfv_external_product.txt (c) and the issue's N = 32768 figure


def verdict(ta, tb):
    spread = tb[2] - tb[0]
    return spread, "accepted" if ta[1] <= tb[1] + spread else "OPEN: slower than the composition"


def from_bfv_against_composition(g, N, n, n_sel, v, kv):
    L = g.L
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    per = 2 * L * N
    S = n * n_sel  # selectors
    ct, key = g.alloc(S * E * per), g.alloc(rows * per)
    out, ref = g.alloc(S * 2 * E * per), g.alloc(S * 2 * E * per)
    g.fill_uniform(ct, S * E * 2 * L, list(range(L)), 17)
    g.fill_uniform(key, rows * 2 * L, list(range(L)), 18)

    def fused():
        g.bfv_rgsw_from_bfv(L, v, kv, n, n_sel, ct, n_sel * E, 1, key, out)

    def composed():
        for s in range(S):
            src, k0, k1 = At(ct, s * E * per), At(ref, s * 2 * E * per), At(ref, (s * 2 * E + E) * per)
            g.bfv_transform_to_ntt(L, 2, E, src, k0)
            g.bfv_external_product(L, kv, E, 1, src, 1, 1, key, 0, 1, k1)
            g.bfv_transform_to_ntt(L, 2, E, k1, k1)

    fused()
    composed()
    w = 2 * E * per
    for lo, k in ((0, S),) if S <= 32 else ((0, 8), (S - 8, 8)):
        if not np.array_equal(out.download_range(lo * w, (k * w,)), ref.download_range(lo * w, (k * w,))):
            raise SystemExit(f"N {N} n {n} n_sel {n_sel} v {v} key_bits {kv}: he355_bfv_rgsw_from_bfv and the composition differ")
    calls = scale * (10 if S <= 32 else 1)
    ta, tb = alternated(g, [fused, composed], [calls, calls], repeats)
    spread, word = verdict(ta, tb)
    print(f"N = {N} L = {L} v = {v} (E = {E}) key_bits = {kv} (2 E_key = {rows})  n {n:3d} n_sel {n_sel:3d} ({S * E:5d} slot ciphertexts)   "
          f"(a) fused {fmt(ta)}   (b) composition {fmt(tb)}   (b) / (a) {tb[1] / ta[1]:6.3f}   spread of (b) {spread:9.1f} us ({spread / tb[1] * 100:4.1f} %)   {word}",
          flush=True)
    for b in (ct, key, out, ref):
        b.free()
    g.pool_trim()


def retrieval(g, N, n, db, dbn, key, kv):
    """1024 entries as 32 x 32, the second dimension by the external product, the query ONE ciphertext"""
    L, t, n1, n2, v = g.L, g.t, 32, 32, 20
    per = 2 * L * N
    E = g.bfv_gadget_count(L, v)[0]
    count = n1 + n2 * E
    d = (count - 1).bit_length()
    rng = np.random.default_rng(5 + n)
    idx = [(int(rng.integers(n1)), int(rng.integers(n2))) for _ in range(n)]
    want = np.stack([db[i * n2 + j] for i, j in idx])
    qp = np.zeros((n, N), dtype=np.uint64)
    sel = np.zeros((n, n2), dtype=np.uint64)
    for r, (i, j) in enumerate(idx):
        qp[r, i] = pow(1 << d, -1, t)
        sel[r, j] = 1
    first_dim, packed, query = g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
    g.encrypt(n, g.to_device(qp), 12, 0, first_dim)                                      # the client's: not timed
    g.bfv_selector_encrypt(L, v, n, n2, n1, count, g.to_device(sel), 14, 0, packed)
    g.add(L, 2, n, first_dim, packed, be.Context.pairwise(), query)
    kids, res1 = g.alloc(count * n * per), g.alloc(n * n2 * per)
    rg, one, low = g.alloc(n * n2 * 2 * E * per), g.alloc(n * per), g.alloc(n * 2 * N)
    bud = {"fresh (first dimension)": g.bfv_noise_budget(L, 2, n, first_dim)}

    def answer(budgets=None):
        g.bfv_expand(L, n, query, count, kids)
        if budgets is not None:
            budgets["children 0..31"] = g.bfv_noise_budget(L, 2, n1 * n, kids)
        g.bfv_transform_to_ntt(L, 2, n1 * n, kids, kids)
        g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids, 1, n, dbn, n2, 1, res1)
        g.bfv_transform_from_ntt(L, 2, n * n2, res1, res1)
        g.bfv_rgsw_from_bfv(L, v, kv, n, n2, At(kids, n1 * n * per), 1, n, key, rg)
        g.bfv_external_product(L, v, n, n2, res1, n2, 1, rg, n2, 1, one)
        g.bfv_mod_switch(L, 1, 2, n, one, low)
        if budgets is not None:
            budgets["scan"] = g.bfv_noise_budget(L, 2, n * n2, res1)
            budgets["external product"] = g.bfv_noise_budget(L, 2, n, one)
            budgets["reply (L = 1)"] = g.bfv_noise_budget(1, 2, n, low)

    answer(bud)
    final = g.alloc(n * N)
    g.decrypt(1, 2, n, low, final)
    ok = np.array_equal(final.download((n, N)), want)
    (ta,) = alternated(g, [answer], [scale], repeats)
    rows = 2 * g.bfv_gadget_count(L, kv)[0]
    print(f"N = {N} L = {L}  1024 entries as 32 x 32, {n} quer{'y' if n == 1 else 'ies'}   us per answer set, min / median / max of {repeats} regions")
    print(f"  packed query: expand({count}) (d = {d}), scan(32), rgsw_from_bfv (v = {v}, E = {E}, key_bits = {kv}), external product at L = {L} (inner 32), "
          f"mod_switch to L = 1  {fmt(ta)}")
    print(f"     query per query: 1 ciphertext = {per * 8} bytes, against {UPLOAD_ROUTE[N]} bytes with uploaded RGSW selectors ({UPLOAD_ROUTE[N] / (per * 8):.0f} x); "
          f"once per client: RGSW(s) = {rows * per * 8} bytes;   reply per query: 1 ciphertext at L = 1, {2 * N * 8} bytes, one decrypt")
    print("  noise budgets (bits): " + ", ".join(f"{k} {b.min()}..{b.max()}" for k, b in bud.items()))
    print(f"  answers equal the database entries: {ok}", flush=True)
    for b in (first_dim, packed, query, kids, res1, rg, one, low, final):
        b.free()
    g.pool_trim()


for N, bits in RINGS:
    if only and N not in only:
        continue
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    E = g.bfv_gadget_count(g.L, 20)[0]
    for j, e in enumerate(g.bfv_expand_galois_elts(32 + 32 * E)):
        g.keygen_galois(e, 20 + j)
    print(f"== N = {N} {bits}  L_top = {g.L}  t = {g.t}  gadget digits at L_top: v = 10 {g.bfv_gadget_count(g.L, 10)}, v = 20 {g.bfv_gadget_count(g.L, 20)}", flush=True)
    print("-- (a) he355_bfv_rgsw_from_bfv against its composition: us per call, min / median / max", flush=True)
    for kv in (20, 10):
        for n, n_sel in ((1, 1), (1, 32), (16, 32)):
            from_bfv_against_composition(g, N, n, n_sel, 20, kv)
    print("-- (c) two-dimensional retrieval, the query ONE ciphertext", flush=True)
    db = np.random.default_rng(3).integers(0, g.t, (1024, N), dtype=np.uint64)  # full-range plaintexts
    dbn = g.alloc(1024 * g.L * N)
    g.bfv_plain_to_ntt(g.L, 1024, g.to_device(db), dbn)
    kv = 20
    key = g.alloc(2 * g.bfv_gadget_count(g.L, kv)[0] * 2 * g.L * N)
    g.bfv_rgsw_encrypt_secret(g.L, kv, 15, 0, key)
    for n in (1, 16):
        retrieval(g, N, n, db, dbn, key, kv)
    g.close()
