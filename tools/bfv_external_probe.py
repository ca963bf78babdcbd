#!/usr/bin/env python3
"""The BFV external product RGSW x ciphertext on the device, for N = 8192 {60,40,60} (L_top = 2) and N = 32768 {60,40,40,60} (L_top = 3).
(a) fused against its defining composition at L = L_top: n in {1, 64, 1024} results, inner in {1, 8}, digit width v in {10, 20}, one
    selector row for all results (rg_stride_r = 0; n = 64 also with a row per result).  (a) he355_bfv_external_product; (b) per result
    he355_bfv_gadget_decompose_ntt of its inner ciphertexts + he355_bfv_multiply_plain_accumulate(L, 2, 1, 1, inner 2E) with the RGSW rows as
    the ciphertext operand, then ONE he355_bfv_transform_from_ntt of all results.  The two alternate inside one process (a, b, a, b, ...),
    every region is HIP-event timed on the context's stream, every shape is warmed up first, the figures are min / median / max over the
    regions.  (a) and (b) are compared bit for bit before anything is timed (every result up to n = 64, the first and the last 32 of 1024).
    Acceptance: (a)'s median is not above (b)'s by more than the spread (max - min) of (b)'s own regions.
(b) he355_bfv_gadget_decompose_ntt against a composition the device can run: for 2^v <= (t + 1) / 2 and 2^v below every prime the centred
    lift of a digit is the digit, so he355_bfv_gadget_decompose + he355_bfv_plain_to_ntt is bit-identical to it: v in {10, 18}, n in
    {1, 64, 1024} size-2 ciphertexts at L = L_top.  (For wider digits the composition needs a reduction the library has no call for.)
(c) a two-dimensional retrieval over 1024 = 32 x 32 entries, 1 and 16 queries: second dimension by the external product (expand(32),
    scan(32), mod_switch to L = 2, external product with inner = 32 and one RGSW(delta) per column and query at v = 20, mod_switch to L = 1:
    ONE reply ciphertext per query, one decrypt) against the decompose recursion of tools/bfv_recursion_probe.py (expand(64), scan(32),
    mod_switch to L = 1, decompose_ntt, scan(32): F reply ciphertexts per query, decrypt, compose, decrypt).  Time per answer set, reply
    ciphertexts and bytes, query bytes (the RGSW selectors are the client's to send), noise budgets, and both answers against the database.
Usage: python tools/bfv_external_probe.py [regions] [scale of the calls per region]"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle as ho  # keys only: nothing timed goes through it
from tools.probe_common import At, alternated, fmt, verdict

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))


def external_against_composition(g, N, n, inner, v, shared):
    L = g.L
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    n_rg = inner if shared else n * inner
    gr = 0 if shared else inner
    ct, rg = g.alloc(n * inner * per), g.alloc(n_rg * rows * per)
    out, ref, dig = g.alloc(n * per), g.alloc(n * per), g.alloc(inner * rows * L * N)
    g.fill_uniform(ct, n * inner * 2 * L, list(range(L)), 7)
    g.fill_uniform(rg, n_rg * rows * 2 * L, list(range(L)), 8)

    def fused():
        g.bfv_external_product(L, v, n, inner, ct, inner, 1, rg, gr, 1, out)

    def composed():
        for r in range(n):
            g.bfv_gadget_decompose_ntt(L, v, 2, inner, At(ct, r * inner * per), dig)
            g.bfv_multiply_plain_accumulate(L, 2, 1, 1, inner * rows, At(rg, r * gr * rows * per), 1, 1, dig, 1, 1, At(ref, r * per))
        g.bfv_transform_from_ntt(L, 2, n, ref, ref)

    fused()
    composed()
    for lo, k in ((0, n),) if n <= 64 else ((0, 32), (n - 32, 32)):
        if not np.array_equal(out.download_range(lo * per, (k * per,)), ref.download_range(lo * per, (k * per,))):
            raise SystemExit(f"N {N} n {n} inner {inner} v {v}: he355_bfv_external_product and the composition differ")
    calls = scale * (10 if n * inner <= 64 else 1)
    ta, tb = alternated(g, [fused, composed], [calls, calls], repeats)
    spread, word = verdict(ta, tb)
    print(f"N = {N} L = {L} v = {v} (2E = {rows})  n {n:5d} inner {inner}  {'one selector row' if shared else 'a row per result '}   "
          f"(a) fused {fmt(ta)}   (b) composition {fmt(tb)}   (b) / (a) {tb[1] / ta[1]:6.3f}   spread of (b) {spread:9.1f} us ({spread / tb[1] * 100:4.1f} %)   {word}",
          flush=True)
    for b in (ct, rg, out, ref, dig):
        b.free()
    g.pool_trim()


def cut_against_composition(g, N, n, v):
    L, size = g.L, 2
    assert 2 ** v <= (g.t + 1) // 2 and all(2 ** v < q for q in g.moduli[:L])  # the centred lift of a digit is the digit
    F = size * g.bfv_gadget_count(L, v)[0]
    ct, plain = g.alloc(n * size * L * N), g.alloc(n * F * N)
    out, ref = g.alloc(n * F * L * N), g.alloc(n * F * L * N)
    g.fill_uniform(ct, n * size * L, list(range(L)), 9)

    def fused():
        g.bfv_gadget_decompose_ntt(L, v, size, n, ct, out)

    def composed():
        g.bfv_gadget_decompose(L, v, size, n, ct, plain)
        g.bfv_plain_to_ntt(L, n * F, plain, ref)

    fused()
    composed()
    for lo, k in ((0, n),) if n <= 64 else ((0, 16), (n - 16, 16)):
        w = F * L * N
        if not np.array_equal(out.download_range(lo * w, (k * w,)), ref.download_range(lo * w, (k * w,))):
            raise SystemExit(f"N {N} n {n} v {v}: he355_bfv_gadget_decompose_ntt and the composition differ")
    calls = scale * (20 if n <= 64 else 2)
    ta, tb = alternated(g, [fused, composed], [calls, calls], repeats)
    spread, word = verdict(ta, tb)
    moved = (n * size * L * N + n * F * L * N) * 8  # the fused call's compulsory bytes: every ciphertext word read, every digit word written
    print(f"N = {N} L = {L} v = {v} (F = {F})  n {n:5d}   (a) he355_bfv_gadget_decompose_ntt {fmt(ta)} ({moved / ta[1] / 1e6:5.2f} TB/s of compulsory bytes)   "
          f"(b) gadget_decompose + plain_to_ntt {fmt(tb)}   (b) / (a) {tb[1] / ta[1]:6.3f}   spread of (b) {spread:9.1f} us   {word}", flush=True)
    for b in (ct, plain, out, ref):
        b.free()
    g.pool_trim()


def retrieval(g, N, n, db, dbn):
    """1024 entries as 32 x 32: the second dimension by the external product against the decompose recursion"""
    L, t, n1, n2, v, Le = g.L, g.t, 32, 32, 20, 2
    per = 2 * L * N
    rng = np.random.default_rng(5 + n)
    idx = [(int(rng.integers(n1)), int(rng.integers(n2))) for _ in range(n)]
    want = np.stack([db[i * n2 + j] for i, j in idx])
    # ---- the external product
    qp = np.zeros((n, N), dtype=np.uint64)
    sel = np.zeros((n, n2, N), dtype=np.uint64)
    for r, (i, j) in enumerate(idx):
        qp[r, i] = pow(n1, -1, t)
        sel[r, j, 0] = 1
    rows = 2 * g.bfv_gadget_count(Le, v)[0]
    query, kids = g.alloc(n * per), g.alloc(n1 * n * per)
    res1, mid = g.alloc(n * n2 * per), g.alloc(n * n2 * 2 * Le * N)
    rg, one, low = g.alloc(n * n2 * rows * 2 * Le * N), g.alloc(n * 2 * Le * N), g.alloc(n * 2 * N)
    g.encrypt(n, g.to_device(qp), 12, 0, query)
    g.bfv_rgsw_encrypt(Le, v, n * n2, g.to_device(sel.reshape(n * n2, N)), 14, 0, rg)  # the client's: not timed
    bud = {}

    def by_external_product(budgets=None):
        g.bfv_expand(L, n, query, n1, kids)
        if budgets is not None:
            budgets["children"] = g.bfv_noise_budget(L, 2, n1 * n, kids)
        g.bfv_transform_to_ntt(L, 2, n1 * n, kids, kids)
        g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids, 1, n, dbn, n2, 1, res1)
        g.bfv_transform_from_ntt(L, 2, n * n2, res1, res1)
        g.bfv_mod_switch(L, Le, 2, n * n2, res1, mid)
        g.bfv_external_product(Le, v, n, n2, mid, n2, 1, rg, n2, 1, one)
        g.bfv_mod_switch(Le, 1, 2, n, one, low)
        if budgets is not None:
            budgets["scan 1"] = g.bfv_noise_budget(L, 2, n * n2, res1)
            budgets[f"mod switch (L = {Le})"] = g.bfv_noise_budget(Le, 2, n * n2, mid)
            budgets["external product"] = g.bfv_noise_budget(Le, 2, n, one)
            budgets["reply (L = 1)"] = g.bfv_noise_budget(1, 2, n, low)

    by_external_product(bud)
    final = g.alloc(n * N)
    g.decrypt(1, 2, n, low, final)
    ok_e = np.array_equal(final.download((n, N)), want)
    # ---- the decompose recursion (tools/bfv_recursion_probe.py)
    Ld = 1
    F = 2 * g.bfv_digit_count(Ld)[0]
    q2 = np.zeros((n, N), dtype=np.uint64)
    for r, (i, j) in enumerate(idx):
        q2[r, i] = q2[r, n1 + j] = pow(64, -1, t)
    query2, kids2 = g.alloc(n * per), g.alloc(64 * n * per)
    res1b, lowb = g.alloc(n * n2 * per), g.alloc(n * n2 * 2 * Ld * N)
    cut, res2 = g.alloc(n * n2 * F * L * N), g.alloc(n * F * per)
    g.encrypt(n, g.to_device(q2), 13, 0, query2)

    def by_recursion():
        g.bfv_expand(L, n, query2, 64, kids2)
        g.bfv_transform_to_ntt(L, 2, 64 * n, kids2, kids2)
        g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids2, 1, n, dbn, n2, 1, res1b)
        g.bfv_transform_from_ntt(L, 2, n * n2, res1b, res1b)
        g.bfv_mod_switch(L, Ld, 2, n * n2, res1b, lowb)
        g.bfv_decompose_ntt(Ld, 2, n * n2, lowb, L, cut)
        for r in range(n):
            g.bfv_multiply_plain_accumulate(L, 2, 1, F, n2, At(kids2, (n1 * n + r) * per), 1, n, At(cut, r * n2 * F * L * N), F, 1, At(res2, r * F * per))
        g.bfv_transform_from_ntt(L, 2, n * F, res2, res2)

    by_recursion()
    bud2 = g.bfv_noise_budget(L, 2, n * F, res2)
    pieces, glued, final2 = g.alloc(n * F * N), g.alloc(n * 2 * Ld * N), g.alloc(n * N)
    g.decrypt(L, 2, n * F, res2, pieces)
    g.bfv_compose(Ld, 2, n, pieces, glued)
    g.decrypt(Ld, 2, n, glued, final2)
    ok_r = np.array_equal(final2.download((n, N)), want)
    te, tr = alternated(g, [by_external_product, by_recursion], [scale, scale], repeats)
    ct_bytes = lambda lv: 2 * lv * N * 8
    print(f"N = {N} L = {L}  1024 entries as 32 x 32, {n} quer{'y' if n == 1 else 'ies'}   us per answer set, min / median / max of {repeats} regions")
    print(f"  external product: expand(32), scan(32), mod_switch to L = {Le}, external product (v = {v}, 2E = {rows}, inner 32), mod_switch to L = 1  {fmt(te)}")
    print(f"     reply per query: 1 ciphertext at L = 1, {ct_bytes(1)} bytes, one decrypt;   query per query: 1 ciphertext + 32 RGSW at L = {Le} = "
          f"{ct_bytes(L) + n2 * rows * ct_bytes(Le)} bytes")
    print(f"  decompose recursion: expand(64), scan(32), mod_switch to L = 1, decompose_ntt (F = {F}), scan(32)  {fmt(tr)}   recursion / external {tr[1] / te[1]:6.3f}")
    print(f"     reply per query: {F} ciphertexts at L = {L}, {F * ct_bytes(L)} bytes, {F} + 1 decrypts and a compose;   query per query: 1 ciphertext = {ct_bytes(L)} bytes")
    print("  noise budgets (bits), external product: " + ", ".join(f"{k} {b.min()}..{b.max()}" for k, b in bud.items())
          + f"; recursion: scan 2 {bud2.min()}..{bud2.max()}")
    print(f"  answers equal the database entries: external product (one decrypt) {ok_e}, recursion (decrypt, compose, decrypt) {ok_r}", flush=True)
    for b in (query, kids, res1, mid, rg, one, low, final, query2, kids2, res1b, lowb, cut, res2, pieces, glued, final2):
        b.free()
    g.pool_trim()


for N, bits in RINGS:
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    for j, e in enumerate(g.bfv_expand_galois_elts(64)):
        g.keygen_galois(e, 20 + j)
    print(f"== N = {N} {bits}  L_top = {g.L}  t = {g.t}  gadget digits at L_top: v = 10 {g.bfv_gadget_count(g.L, 10)}, v = 20 {g.bfv_gadget_count(g.L, 20)}", flush=True)
    print("-- (a) he355_bfv_external_product against its composition: us per call, min / median / max", flush=True)
    for v in (10, 20):
        for inner in (1, 8):
            for n in (1, 64, 1024):
                external_against_composition(g, N, n, inner, v, True)
            external_against_composition(g, N, 64, inner, v, False)
    print("-- (b) he355_bfv_gadget_decompose_ntt against gadget_decompose + plain_to_ntt: us per call, min / median / max", flush=True)
    for v in (10, 18):
        for n in (1, 64, 1024):
            cut_against_composition(g, N, n, v)
    print("-- (c) two-dimensional retrieval", flush=True)
    db = np.random.default_rng(3).integers(0, g.t, (1024, N), dtype=np.uint64)  # full-range plaintexts
    dbn = g.alloc(1024 * g.L * N)
    g.bfv_plain_to_ntt(g.L, 1024, g.to_device(db), dbn)
    for n in (1, 16):
        retrieval(g, N, n, db, dbn)
    g.close()
