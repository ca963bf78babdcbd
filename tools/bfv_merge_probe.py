#!/usr/bin/env python3
"""The BFV ciphertext merge on the device, for N = 8192 {60,40,60} (L = 2) and N = 32768 {60,40,40,60} (L = 3), count in {64, 1024} inputs per
result, n in {1, 16} results.  Two ways to the same results:
(a) he355_bfv_merge: per level one k_bfv_merge launch (S = even + X^s odd, D = even - X^s odd) and one batched key switch of D with S as its
    addend;
(b) the same tree from the public calls, the yardstick: per level he355_bfv_multiply_monomial, he355_add, he355_sub, he355_apply_galois,
    he355_add -- five launches-plus-key-switch and three intermediate slabs.
The two alternate inside one process (a, b, a, b, ...), every region is HIP-event timed on the context's stream (he355_timer_begin / _end),
every shape is warmed up first, and the figures are min / median / max over the regions.  (a) and (b) are compared bit for bit (all results)
before anything is timed.  The inputs are fresh encryptions of full-range plaintexts (keys: the oracle's secret and public key, Galois keys by
he355_keygen_galois), so the noise budget before and after the merge is read off the same run, and result 0 is decrypted and held to the
closed form (coefficient k + 2^d m is 2^d mu_(k, 2^d m)).
`kernel`: he355_bfv_merge at count 2 (one k_bfv_merge<ODD> launch over 1024 pairs, s = 1) and count 4 (k_bfv_merge<even> over 1024 pairs,
s = 2), and he355_add over slabs of the same size, a few calls each and nothing else: the run to put under a kernel trace, whose per-kernel
times give the streaming rate of k_bfv_merge (four slabs: two read, two written) beside k_addsub's (three).
Usage: python tools/bfv_merge_probe.py [regions] [scale of the calls per region] [all | kernel]"""
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
mode = sys.argv[3] if len(sys.argv) > 3 else "all"
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
SHAPES = ((64, 1), (64, 16), (1024, 1), (1024, 16))  # (count, n)
BATCH = 256  # plaintexts of one he355_encrypt call; input i encrypts plaintext i % BATCH


def fresh_inputs(g, N, L, total, plain, dplain):
    """`total` fresh encryptions, input i of plaintext i % BATCH"""
    per = 2 * L * N
    buf = g.alloc(total * per)
    for b in range(0, total, BATCH):
        g.encrypt(min(BATCH, total - b), dplain, 12, b, At(buf, b * per))
    return buf


def merge_run(g, N, L, count, n, plain, dplain):
    d = (count - 1).bit_length()
    assert count == 1 << d
    t, per = g.t, 2 * L * N
    elts = g.bfv_expand_galois_elts(count)
    din = fresh_inputs(g, N, L, count * n, plain, dplain)  # child-major: input k of result r at k n + r
    fresh = g.bfv_noise_budget(L, 2, min(count * n, 1024), din)
    out, ref = g.alloc(n * per), g.alloc(n * per)
    half = (count // 2) * n
    mono, S, D = g.alloc(half * per), g.alloc(half * per), g.alloc(half * per)
    ping = [g.alloc(half * per), g.alloc(max(half // 2, 1) * per)]
    pw = be.Context.pairwise()

    def new(dst=out):
        g.bfv_merge(L, n, count, din, n, 1, dst)

    def composed(dst=ref):
        cur = din
        for i, j in enumerate(range(d - 1, -1, -1)):
            s = 1 << j
            m = s * n
            to = dst if j == 0 else ping[i % 2]
            g.bfv_multiply_monomial(L, 2, m, At(cur, m * per), s, mono)
            g.add(L, 2, m, cur, mono, pw, S)
            g.add(L, 2, m, cur, mono, pw, D, sub=True)
            g.apply_galois(L, m, D, elts[j], mono)  # the monomial product is consumed: its slab takes the Galois image
            g.add(L, 2, m, S, mono, pw, to)
            cur = to

    new()
    composed()
    if not np.array_equal(out.download((n * per,)), ref.download((n * per,))):
        raise SystemExit(f"N {N} count {count} n {n}: he355_bfv_merge and the composition differ")
    budget = g.bfv_noise_budget(L, 2, n, out)
    dec = g.alloc(N)
    g.decrypt(L, 2, 1, out, dec)
    want = np.zeros(N, dtype=np.uint64)
    for k in range(count):  # result 0: input k is encryption k n of plaintext (k n) % BATCH
        want[k::count] = (plain[(k * n) % BATCH, ::count].astype(object) * count % t).astype(np.uint64)
    ok = np.array_equal(dec.download((N,)), want)
    dec.free()
    calls = scale * (4 if count * n <= 1024 else 1)
    ta, tb = alternated(g, [new, composed], [calls, calls], repeats)
    ks = ((1 << d) - 1) * n
    print(f"N = {N} L = {L}  count {count} (d = {d})  n {n}: {ks} key switches   us per call, min / median / max of {repeats} regions")
    print(f"  (a) he355_bfv_merge                             {fmt(ta)}   per key switch {ta[1] / ks:8.2f}")
    print(f"  (b) multiply_monomial, add, sub, apply_galois, add {fmt(tb)}   per key switch {tb[1] / ks:8.2f}   (b) / (a) {tb[1] / ta[1]:6.3f}"
          f"   spread of (b) {(tb[2] - tb[0]) / tb[1] * 100:4.1f} %   (b) - (a) {(tb[1] - ta[1]) / tb[1] * 100:4.1f} % of (b)")
    print(f"  noise budget: fresh inputs {fresh.min()}..{fresh.max()} bits, merged {budget.min()}..{budget.max()} bits; result 0 decrypts to the closed form: {ok}")
    print(f"  bytes back to the client: {n * per * 8} instead of {count * n * per * 8}", flush=True)
    for b in [din, out, ref, mono, S, D] + ping:
        b.free()
    g.pool_trim()  # the next shape's slabs are of other sizes


def kernel_run(g, N, L, plain, dplain):
    pairs, per = 1024, 2 * L * N
    din = fresh_inputs(g, N, L, 2 * pairs, plain, dplain)
    out, a = g.alloc(pairs * per), g.alloc(pairs * per)
    for _ in range(6):
        g.bfv_merge(L, pairs, 2, din, pairs, 1, out)      # s = 1 over 1024 pairs
        g.bfv_merge(L, pairs // 2, 4, din, pairs // 2, 1, out)  # s = 2 over 1024 pairs, then s = 1 over 512
        g.add(L, 2, pairs, din, At(din, pairs * per), be.Context.pairwise(), a)
    g.sync()
    print(f"N = {N} L = {L}: k_bfv_merge over {pairs} pairs moves {4 * pairs * per * 8} bytes, he355_add over {pairs} ciphertexts {3 * pairs * per * 8}", flush=True)
    for b in (din, out, a):
        b.free()


for N, bits in RINGS:
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    L = g.L
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    for j, e in enumerate(g.bfv_expand_galois_elts(1024)):
        g.keygen_galois(e, 20 + j)
    plain = np.random.default_rng(5).integers(0, g.t, (BATCH, N), dtype=np.uint64)
    dplain = g.to_device(plain)
    print(f"== N = {N} {bits}  L = {L}  t = {g.t}", flush=True)
    if mode == "kernel":
        kernel_run(g, N, L, plain, dplain)
    else:
        for count, n in SHAPES:
            merge_run(g, N, L, count, n, plain, dplain)
    g.close()
