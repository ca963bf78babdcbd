#!/usr/bin/env python3
"""The ciphertext decomposition of a recursive (two-dimensional) PIR on the device, for N = 8192 {60,40,60} (L_top = 2) and
N = 32768 {60,40,40,60} (L_top = 3).
* fused against the composition: n in {1, 32, 1024} size-2 ciphertexts at L = 1 cut into NTT-form plaintexts at L_out = L_top,
  (a) he355_bfv_decompose_ntt (the digits are cut and lifted inside the forward column pass), (b) he355_bfv_decompose +
  he355_bfv_plain_to_ntt, the definition and the yardstick.  The two alternate inside one process (a, b, a, b, ...), every region is
  HIP-event timed on the context's stream (he355_timer_begin / _end), every shape is warmed up first, and the figures are min / median / max
  over the regions.  (a) and (b) are compared bit for bit (the whole slab) before anything is timed.  Acceptance: (a)'s median is not above
  (b)'s by more than the spread (max - min) of (b)'s own regions.
* streaming rate: he355_bfv_decompose and he355_bfv_compose over 1024 ciphertexts in compulsory bytes (every word read once, written once)
  per second, beside he355_add (k_addsub) in the same run.
* two dimensions against one, 1024 entries, 1 and 16 queries: expand(64) + scan(32) + mod_switch + decompose_ntt + scan(32) against
  expand(1024) + scan(1024); real queries and a database of full-range plaintexts, so the noise budgets are read off the same run and the
  two-dimensional answer is decrypted, composed, decrypted again and compared with the database entry.  The two paths compute different
  ciphertexts by construction: this is a time, not a parity.
Usage: python tools/bfv_recursion_probe.py [regions] [scale of the calls per region]"""
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
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))


def fused_against_composition(g, N, n):
    L, L_out, size = 1, g.L, 2
    F = size * g.bfv_digit_count(L)[0]
    ct, plain = g.alloc(n * size * L * N), g.alloc(n * F * N)
    out, ref = g.alloc(n * F * L_out * N), g.alloc(n * F * L_out * N)
    g.fill_uniform(ct, n * size * L, list(range(L)), 7)

    def fused(dst=out):
        g.bfv_decompose_ntt(L, size, n, ct, L_out, dst)

    def composed(dst=ref):
        g.bfv_decompose(L, size, n, ct, plain)
        g.bfv_plain_to_ntt(L_out, n * F, plain, dst)

    fused()
    composed()
    step = 64 * F * L_out * N  # compared in pieces: the whole slab, without a host copy of all of it at once
    for off in range(0, n * F * L_out * N, step):
        k = min(step, n * F * L_out * N - off)
        if not np.array_equal(out.download_range(off, (k,)), ref.download_range(off, (k,))):
            raise SystemExit(f"N {N} n {n}: he355_bfv_decompose_ntt and the composition differ")
    calls = scale * (20 if n <= 32 else 2)
    ta, tb = alternated(g, [fused, composed], [calls, calls], repeats)
    spread = tb[2] - tb[0]
    verdict = "accepted" if ta[1] <= tb[1] + spread else "NOT accepted: slower than the composition"
    print(f"N = {N} L = {L} -> L_out = {L_out}  n {n} (F = {F}, {n * F} plaintexts)   us per call, min / median / max of {repeats} regions")
    print(f"  (a) he355_bfv_decompose_ntt                    {fmt(ta)}")
    print(f"  (b) he355_bfv_decompose + he355_bfv_plain_to_ntt {fmt(tb)}   (b) / (a) {tb[1] / ta[1]:6.3f}   spread of (b) {spread:9.1f} us"
          f" ({spread / tb[1] * 100:4.1f} %)   {verdict}", flush=True)
    for b in (ct, plain, out, ref):
        b.free()
    g.pool_trim()


def streaming_rate(g, N):
    L, size, n = 1, 2, 1024
    F = size * g.bfv_digit_count(L)[0]
    per = size * L * N
    ct, back, plain = g.alloc(n * per), g.alloc(n * per), g.alloc(n * F * N)
    g.fill_uniform(ct, n * size * L, list(range(L)), 8)
    g.bfv_decompose(L, size, n, ct, plain)
    g.bfv_compose(L, size, n, plain, back)
    if not np.array_equal(ct.download_head((4 * per,)), back.download_head((4 * per,))):
        raise SystemExit(f"N {N}: compose(decompose(x)) != x")
    a, b, o = (g.alloc(n * F * N // 2) for _ in range(3))  # he355_add over slabs of comparable size: [n F / 4][2][1][N]
    m = n * F // 4
    g.fill_uniform(a, m * 2 * L, list(range(L)), 9)
    g.fill_uniform(b, m * 2 * L, list(range(L)), 10)
    fs = [lambda: g.bfv_decompose(L, size, n, ct, plain), lambda: g.bfv_compose(L, size, n, plain, back),
          lambda: g.add(L, 2, m, a, b, be.Context.pairwise(), o)]
    ts = alternated(g, fs, [10 * scale] * 3, repeats)
    moved = (n * per + n * F * N) * 8
    for name, t, nbytes in (("he355_bfv_decompose", ts[0], moved), ("he355_bfv_compose  ", ts[1], moved), ("he355_add          ", ts[2], 3 * m * 2 * L * N * 8)):
        print(f"N = {N} L = {L}  {name} over {n if 'add' not in name else m} ciphertexts ({nbytes} compulsory bytes): {fmt(t)} us -> {nbytes / t[1] / 1e6:6.3f} TB/s at the median",
              flush=True)
    for x in (ct, back, plain, a, b, o):
        x.free()
    g.pool_trim()


def two_against_one(g, N, n, db, dbn):
    """1024 entries: 32 x 32 through the recursion against one dimension of 1024"""
    L, t, n1, n2, Ld = g.L, g.t, 32, 32, 1
    per = 2 * L * N
    rng = np.random.default_rng(5 + n)
    idx = [(int(rng.integers(n1)), int(rng.integers(n2))) for _ in range(n)]
    F = 2 * g.bfv_digit_count(Ld)[0]
    # ---- two dimensions
    qp = np.zeros((n, N), dtype=np.uint64)
    for r, (i, j) in enumerate(idx):
        qp[r, i] = qp[r, n1 + j] = pow(64, -1, t)
    query, kids = g.alloc(n * per), g.alloc(64 * n * per)
    res1, low = g.alloc(n * n2 * per), g.alloc(n * n2 * 2 * Ld * N)
    cut, res2 = g.alloc(n * n2 * F * L * N), g.alloc(n * F * per)
    g.encrypt(n, g.to_device(qp), 12, 0, query)
    bud = {}

    def first_half():
        g.bfv_expand(L, n, query, 64, kids)

    def rest(budgets=None):
        if budgets is not None:
            budgets["children"] = g.bfv_noise_budget(L, 2, 64 * n, kids)
        g.bfv_transform_to_ntt(L, 2, 64 * n, kids, kids)
        g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids, 1, n, dbn, n2, 1, res1)
        g.bfv_transform_from_ntt(L, 2, n * n2, res1, res1)
        g.bfv_mod_switch(L, Ld, 2, n * n2, res1, low)
        g.bfv_decompose_ntt(Ld, 2, n * n2, low, L, cut)
        for r in range(n):
            g.bfv_multiply_plain_accumulate(L, 2, 1, F, n2, At(kids, (n1 * n + r) * per), 1, n, At(cut, r * n2 * F * L * N), F, 1, At(res2, r * F * per))
        g.bfv_transform_from_ntt(L, 2, n * F, res2, res2)
        if budgets is not None:
            budgets["scan 1"] = g.bfv_noise_budget(L, 2, n * n2, res1)
            budgets["mod switch"] = g.bfv_noise_budget(Ld, 2, n * n2, low)
            budgets["scan 2"] = g.bfv_noise_budget(L, 2, n * F, res2)

    def two_d():
        first_half()
        rest()

    first_half()
    rest(bud)
    pieces, glued, final = g.alloc(n * F * N), g.alloc(n * 2 * Ld * N), g.alloc(n * N)
    g.decrypt(L, 2, n * F, res2, pieces)
    g.bfv_compose(Ld, 2, n, pieces, glued)
    g.decrypt(Ld, 2, n, glued, final)
    ok2 = np.array_equal(final.download((n, N)), np.stack([db[i * n2 + j] for i, j in idx]))
    # ---- one dimension
    q1 = np.zeros((n, N), dtype=np.uint64)
    for r, (i, j) in enumerate(idx):
        q1[r, i * n2 + j] = pow(1024, -1, t)
    query1, kids1, res = g.alloc(n * per), g.alloc(1024 * n * per), g.alloc(n * per)
    g.encrypt(n, g.to_device(q1), 13, 0, query1)

    def one_d():
        g.bfv_expand(L, n, query1, 1024, kids1)
        g.bfv_transform_to_ntt(L, 2, 1024 * n, kids1, kids1)
        g.bfv_multiply_plain_accumulate(L, 2, n, 1, 1024, kids1, 1, n, dbn, 1, 0, res)
        g.bfv_transform_from_ntt(L, 2, n, res, res)

    one_d()
    bud1 = g.bfv_noise_budget(L, 2, n, res)
    dec1 = g.alloc(n * N)
    g.decrypt(L, 2, n, res, dec1)
    ok1 = np.array_equal(dec1.download((n, N)), np.stack([db[i * n2 + j] for i, j in idx]))
    t2, t1 = alternated(g, [two_d, one_d], [scale, scale], repeats)
    print(f"N = {N} L = {L}  1024 entries, {n} quer{'y' if n == 1 else 'ies'}   us per answer set, min / median / max of {repeats} regions")
    print(f"  two dimensions: expand(64), scan(32), mod_switch to L = 1, decompose_ntt (F = {F}), scan(32)  {fmt(t2)}")
    print(f"  one dimension : expand(1024), scan(1024)                                                   {fmt(t1)}   one / two {t1[1] / t2[1]:6.3f}")
    print("  noise budgets (bits), two dimensions: " + ", ".join(f"{k} {v.min()}..{v.max()}" for k, v in bud.items())
          + f"; one dimension: result {bud1.min()}..{bud1.max()}")
    print(f"  answers equal the database entries: two dimensions (decrypt, compose, decrypt) {ok2}, one dimension {ok1}", flush=True)
    for b in (query, kids, res1, low, cut, res2, pieces, glued, final, query1, kids1, res, dec1):
        b.free()
    g.pool_trim()


for N, bits in RINGS:
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    for j, e in enumerate(g.bfv_expand_galois_elts(1024)):
        g.keygen_galois(e, 20 + j)
    print(f"== N = {N} {bits}  L_top = {g.L}  t = {g.t}  digits of level 1: {g.bfv_digit_count(1)}", flush=True)
    for n in (1, 32, 1024):
        fused_against_composition(g, N, n)
    streaming_rate(g, N)
    db = np.random.default_rng(3).integers(0, g.t, (1024, N), dtype=np.uint64)  # full-range plaintexts
    dbn = g.alloc(1024 * g.L * N)
    g.bfv_plain_to_ntt(g.L, 1024, g.to_device(db), dbn)
    for n in (1, 16):
        two_against_one(g, N, n, db, dbn)
    g.close()
