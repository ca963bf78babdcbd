#!/usr/bin/env python3
"""The oblivious query expansion and the monomial multiply on the device, for N = 8192 {60,40,60} (L = 2) and N = 32768 {60,40,40,60}
(L = 3), count in {64, 1024} children, n in {1, 16} queries.  Two ways to the same children:
(a) he355_bfv_expand: per level one batched key switch with the node as its addend (the even children) and one k_bfv_shift launch (the odd);
(b) the same tree from the calls the library had before, the yardstick: per level he355_apply_galois, he355_add (even), he355_sub and
    he355_bfv_multiply_plain by the monomial plaintext (t - 1) X^(N - s) (odd: a forward and an inverse transform per polynomial).
The two alternate inside one process (a, b, a, b, ...), every region is HIP-event timed on the context's stream (he355_timer_begin / _end),
every shape is warmed up first, and the figures are min / median / max over the regions.  (a) and (b) are compared bit for bit (first and
last children) before anything is timed.  The queries are real encryptions of 2^-d X^idx (keys: the oracle's secret and public key, Galois
keys by he355_keygen_galois), so the noise budget of the children is read off the same run.  Beside them:
* the scan the children feed: he355_bfv_transform_to_ntt + he355_bfv_multiply_plain_accumulate (one column) + he355_bfv_transform_from_ntt,
  and what uploading `count` ciphertexts per query would take at the host-to-device rate he355_upload reaches in this run (arithmetic);
* he355_bfv_multiply_monomial over 1024 size-2 ciphertexts at e = 1 (odd shift: two aligned 16-byte reads per lane and a select), e = 2 and
  e = 1024 (a whole row), in compulsory bytes (every word read once, written once) per second, and he355_add (k_addsub) over slabs of the
  same size.
`monomial`: the monomial multiply alone (the A/B of two builds of the library, HE355_LIB_PATH: one process each, alternated by the caller).
Usage: python tools/bfv_expand_probe.py [regions] [scale of the calls per region] [all | monomial]"""
import importlib
import os
import statistics
import sys
import time

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


def expand_run(g, N, L, count, n, h2d):
    d = (count - 1).bit_length()
    t, per = g.t, 2 * L * N
    elts = g.bfv_expand_galois_elts(count)
    qp = np.zeros((n, N), dtype=np.uint64)
    for r in range(n):
        qp[r, (7 * r + 3) % count] = pow(1 << d, -1, t)
    query, out = g.alloc(n * per), g.alloc(count * n * per)
    g.encrypt(n, g.to_device(qp), 11, 0, query)
    fresh = g.bfv_noise_budget(L, 2, n, query)
    half = (count // 2) * n
    ping, gal, dif = g.alloc(half * per), g.alloc(half * per), g.alloc(half * per)
    mono = np.zeros((d, N), dtype=np.uint64)  # X^(-s) = -X^(N - s)
    for j in range(d):
        mono[j, N - (1 << j)] = t - 1
    dmono = g.to_device(mono)
    pw = be.Context.pairwise()

    def new(dst=out):
        g.bfv_expand(L, n, query, count, dst)

    def composed(dst=out):
        cur = query
        for j in range(d):
            s = 1 << j
            m = s * n
            to = dst if (d - 1 - j) % 2 == 0 else ping
            g.apply_galois(L, m, cur, elts[j], gal)
            g.add(L, 2, m, cur, gal, pw, to)
            g.add(L, 2, m, cur, gal, pw, dif, sub=True)
            g.bfv_multiply_plain(L, 2, min(s, count - s) * n, dif, dmono, be.Context.outer(0, 1, j, 1), At(to, m * per))  # the odd children's place
            cur = to

    # the same children, bit for bit: the first and the last of them
    ref = g.alloc(count * n * per)
    new()
    composed(ref)
    k = min(count * n, 4)
    if not (np.array_equal(out.download_head((k * per,)), ref.download_head((k * per,)))
            and np.array_equal(out.download_range((count * n - k) * per, (k * per,)), ref.download_range((count * n - k) * per, (k * per,)))):
        raise SystemExit(f"N {N} count {count} n {n}: he355_bfv_expand and the composition differ")
    ref.free()
    budget = g.bfv_noise_budget(L, 2, count * n, out)
    kc = min(count, 128)  # the first children of every query, decrypted: the indicator of the query's index
    dec = g.alloc(kc * n * N)
    g.decrypt(L, 2, kc * n, out, dec)
    got = dec.download((kc, n, N))
    ok = all(got[k, r, 0] == (1 if k == (7 * r + 3) % count else 0) and not got[k, r, 1:].any() for k in range(kc) for r in range(n))
    dec.free()
    calls = scale * (4 if count * n <= 1024 else 1)
    ta, tb = alternated(g, [new, composed], [calls, calls], repeats)
    ks = ((1 << d) - 1) * n
    print(f"N = {N} L = {L}  count {count} (d = {d})  n {n}: {ks} key switches   us per call, min / median / max of {repeats} regions")
    print(f"  (a) he355_bfv_expand                {fmt(ta)}   per key switch {ta[1] / ks:8.2f}")
    print(f"  (b) apply_galois, add, sub, multiply_plain {fmt(tb)}   per key switch {tb[1] / ks:8.2f}   (b) / (a) {tb[1] / ta[1]:6.3f}"
          f"   spread of (b) {(tb[2] - tb[0]) / tb[1] * 100:4.1f} %")
    print(f"  noise budget: fresh {fresh.min()}..{fresh.max()} bits, children {budget.min()}..{budget.max()} bits; the first {kc} children of every query decrypt to the indicator: {ok}")
    # the scan the children feed, one database column (timing only: every region transforms the slab again where it lies)
    ptn, res = g.alloc(count * L * N), g.alloc(n * per)
    g.fill_uniform(ptn, count * L, list(range(L)), 4)

    def scan():
        g.bfv_transform_to_ntt(L, 2, count * n, out, out)
        g.bfv_multiply_plain_accumulate(L, 2, n, 1, count, out, 1, n, ptn, 1, 0, res)
        g.bfv_transform_from_ntt(L, 2, n, res, res)

    (ts,) = alternated(g, [scan], [calls], repeats)
    up = count * n * per * 8 / h2d * 1e6
    print(f"  scan (to_ntt of the children, multiply_plain_accumulate over {count}, from_ntt) {fmt(ts)}")
    print(f"  expand + scan {ta[1] + ts[1]:11.1f} us   against {up:11.1f} us to upload {count * n} ciphertexts ({count * n * per * 8} bytes) at {h2d / 1e9:5.2f} GB/s:"
          f" upload / (expand + scan) {up / (ta[1] + ts[1]):6.2f}", flush=True)
    for b in (query, out, ping, gal, dif, dmono, ptn, res):
        b.free()
    g.pool_trim()  # the next shape's slabs are of other sizes


def monomial_rate(g, N, L):
    n, per = 1024, 2 * L * N
    a, b, o = (g.alloc(n * per) for _ in range(3))
    g.fill_uniform(a, n * 2 * L, list(range(L)), 5)
    # what is timed is what he355_bfv_multiply_plain computes for the monomial plaintext: the first and the last ciphertexts at an odd wrap
    pl = np.zeros((1, N), dtype=np.uint64)
    pl[0, N - 1] = g.t - 1  # X^(2N - 1) = -X^(N - 1)
    g.bfv_multiply_monomial(L, 2, n, a, 2 * N - 1, o)
    g.bfv_multiply_plain(L, 2, n, a, g.to_device(pl), be.Context.outer(0, n, 0, 1), b)
    if not (np.array_equal(o.download_head((2 * per,)), b.download_head((2 * per,)))
            and np.array_equal(o.download_range((n - 2) * per, (2 * per,)), b.download_range((n - 2) * per, (2 * per,)))):
        raise SystemExit(f"N {N}: he355_bfv_multiply_monomial and he355_bfv_multiply_plain by the monomial differ")
    g.fill_uniform(b, n * 2 * L, list(range(L)), 6)
    fs = [lambda e=e: g.bfv_multiply_monomial(L, 2, n, a, e, o) for e in (1, 2, 1024)] + [lambda: g.add(L, 2, n, a, b, be.Context.pairwise(), o)]
    ts = alternated(g, fs, [10 * scale] * 4, repeats)
    for name, t, slabs in (("monomial e = 1   ", ts[0], 2), ("monomial e = 2   ", ts[1], 2), ("monomial e = 1024", ts[2], 2), ("he355_add        ", ts[3], 3)):
        print(f"N = {N} L = {L}  {name} over {n} ciphertexts ({slabs * n * per * 8} bytes): {fmt(t)} us -> {slabs * n * per * 8 / t[1] / 1e6:6.3f} TB/s at the median")
    print(f"  odd shift against even: e = 1 takes {ts[0][1] / ts[1][1]:5.3f} of e = 2's time", flush=True)
    for x in (a, b, o):
        x.free()


def upload_rate(g):
    """host-to-device bytes per second of he355_upload from a pageable numpy array of 256 MiB (the call returns when the copy is done)"""
    h = np.ones(1 << 25, dtype=np.uint64)
    dbuf = g.alloc(h.size)
    dbuf.upload(h)
    best = []
    for _ in range(5):
        t0 = time.perf_counter()
        dbuf.upload(h)
        best.append(h.nbytes / (time.perf_counter() - t0))
    dbuf.free()
    return statistics.median(best)


for N, bits in RINGS:
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    L = g.L
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    for j, e in enumerate(g.bfv_expand_galois_elts(1024)):
        g.keygen_galois(e, 20 + j)
    h2d = upload_rate(g)
    print(f"== N = {N} {bits}  L = {L}  t = {g.t}  he355_upload {h2d / 1e9:6.2f} GB/s (pageable host memory, 256 MiB)", flush=True)
    for count, n in SHAPES if mode == "all" else ():
        expand_run(g, N, L, count, n, h2d)
    monomial_rate(g, N, L)
    g.close()
