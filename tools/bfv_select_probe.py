#!/usr/bin/env python3
"""The BFV selection tree on the device.
`call`: he355_bfv_select against its defining composition, for N = 8192 {60,40,60} (L = 2) and N = 32768 {60,40,40,60} (L = 3), L = L_top,
v = 20, count in {32, 256} leaves per result, n in {1, 16} results, one set of bits for all results (rg_stride_r = 0):
(a) he355_bfv_select over row-major leaves;
(b) the same tree from the public calls, the yardstick: per level he355_sub, he355_bfv_external_product with inner 1, he355_add.  The public
    calls cannot address "node 2p of result r", so (b) gets its leaves in the one layout that needs no gather: position-major, leaf k of result r
    at (bit reversal of k) n + r, where every level's even nodes are the first half of the slab and its odd nodes the second.  (A caller whose
    leaves lie as a scan leaves them pays a gather per level on top of (b); it is not timed.)
The two alternate inside one process (a, b, a, b, ...), every region is HIP-event timed on the context's stream (he355_timer_begin / _end),
every shape is warmed up first, and the figures are min / median / max over the regions.  (a) and (b) are compared bit for bit before anything
is timed.  The "RGSW" slabs are uniform (the comparison is arithmetic).
`retrieval`: a 32 x 32 retrieval at N = 8192, real keys, nq queries per answer set: the second dimension folded (1) by he355_bfv_select with 5
bit selectors and (2) by he355_bfv_external_product with 32 one-hot selectors, each with the RGSW selectors uploaded by the client
(he355_bfv_rgsw_encrypt) and with the selectors packed into the query ciphertext (he355_bfv_selector_encrypt; the server expands and converts
with he355_bfv_rgsw_from_bfv).  Reports the server's time per answer set (median of the alternated regions), the children expanded and
converted, the query slots, and the noise budget after every stage; every reply is decrypted and held to db[i][j].
`n1024`: `call` on N = 1024 {50,40,50}, the ring without a column pass, whose tail is routed to launch_ntt_inverse and a streaming add.
Usage: python tools/bfv_select_probe.py [regions] [call | retrieval | all | n1024]"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle as ho  # keys only: nothing timed goes through it
from tools.probe_common import At, alternated

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mode = sys.argv[2] if len(sys.argv) > 2 else "all"
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
SMALL = ((1024, [50, 40, 50]),)  # no column pass: the streaming cut and the routed tail (launch_ntt_inverse + k_bfv_select_add)
SHAPES = ((32, 1), (32, 16), (256, 1), (256, 16))  # (count, n)
V = 20


def fmt(t):
    return " / ".join(f"{v:10.1f}" for v in t)


def bitrev(k, m):
    return int(format(k, f"0{m}b")[::-1], 2) if m else 0


def call_run(g, N, L, count, n):
    m = (count - 1).bit_length()
    assert count == 1 << m
    per = 2 * L * N
    rows = 2 * g.bfv_gadget_count(L, V)[0]
    leaves = g.alloc(count * n * per)  # row-major: leaf k of result r at r count + k
    g.fill_uniform(leaves, count * n * 2 * L, list(range(L)), 7)
    rev = g.alloc(count * n * per)  # position-major: leaf k of result r at bitrev(k) n + r
    for r in range(n):
        for k in range(count):
            assert be.lib().he355_copy(g.h, At(rev, (bitrev(k, m) * n + r) * per).ptr, At(leaves, (r * count + k) * per).ptr, per * 8) == 0
    rg = g.alloc(m * rows * per)
    g.fill_uniform(rg, m * rows * 2 * L, list(range(L)), 8)
    out, ref = g.alloc(n * per), g.alloc(n * per)
    half = (count // 2) * n
    diff, pick = g.alloc(half * per), g.alloc(half * per)
    ping = [g.alloc(half * per), g.alloc(max(half // 2, 1) * per)]
    pw = be.Context.pairwise()

    def fused():
        g.bfv_select(L, V, n, count, leaves, count, 1, rg, 0, 1, out)

    def composed():
        cur = rev
        for j in range(m):
            h = (count >> (j + 1)) * n  # pairs: even nodes cur[0 .. h), odd nodes cur[h .. 2h)
            to = ref if j == m - 1 else ping[j % 2]
            g.add(L, 2, h, At(cur, h * per), cur, pw, diff, sub=True)
            g.bfv_external_product(L, V, h, 1, diff, 1, 1, At(rg, j * rows * per), 0, 1, pick)
            g.add(L, 2, h, cur, pick, pw, to)
            cur = to

    fused()
    composed()
    if not np.array_equal(out.download((n * per,)), ref.download((n * per,))):
        raise SystemExit(f"N {N} count {count} n {n}: he355_bfv_select and the composition differ")
    g.bfv_route_stats(reset=True)
    fused()
    routes = {k: c for k, c in g.bfv_route_stats(reset=True).items() if c}
    calls = 4 if count * n <= 512 else 1
    ta, tb = alternated(g, [fused, composed], [calls, calls], repeats)
    pairs = (count - 1) * n
    print(f"N = {N} L = {L}  count {count} (m = {m})  n {n}: {pairs} CMUXes   us per call, min / median / max of {repeats} regions")
    print(f"  (a) he355_bfv_select                        {fmt(ta)}   per CMUX {ta[1] / pairs:8.2f}   routes {routes}")
    print(f"  (b) sub, external_product(inner 1), add     {fmt(tb)}   per CMUX {tb[1] / pairs:8.2f}   (b) / (a) {tb[1] / ta[1]:6.3f}"
          f"   spread of (b) {(tb[2] - tb[0]) / tb[1] * 100:4.1f} %   (b) - (a) {(tb[1] - ta[1]) / tb[1] * 100:5.1f} % of (b)", flush=True)
    for b in [leaves, rev, rg, out, ref, diff, pick] + ping:
        b.free()
    g.pool_trim()  # the next shape's slabs are of other sizes


def retrieval_run(N, bits, nq=4):
    n1 = n2 = 32
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    L, t = g.L, g.t
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    E = g.bfv_gadget_count(L, V)[0]
    rows, per = 2 * E, 2 * L * N
    for j, e in enumerate(g.bfv_expand_galois_elts(n1 + n2 * E)):
        g.keygen_galois(e, 20 + j)
    rng = np.random.default_rng(6)
    db = rng.integers(0, t, (n1, n2, N), dtype=np.uint64)
    dbn = g.alloc(n1 * n2 * L * N)
    g.bfv_plain_to_ntt(L, n1 * n2, g.to_device(db.reshape(n1 * n2, N)), dbn)
    idx = [(int(rng.integers(n1)), int(rng.integers(n2))) for _ in range(nq)]
    idx[0] = (n1 - 1, n2 - 1)
    want = np.stack([db[i, j] for i, j in idx])
    key = g.alloc(rows * per)
    g.bfv_rgsw_encrypt_secret(L, V, 96, 0, key)
    pw = be.Context.pairwise()
    print(f"== 32 x 32 retrieval, N = {N} {bits}  L = {L}  v = {V}  E = {E}, {nq} queries per answer set", flush=True)

    def route(bits_route, packed):
        n_sel = 5 if bits_route else n2
        sel = np.zeros((nq, n_sel), dtype=np.uint64)
        for r, (_, j) in enumerate(idx):
            if bits_route:
                sel[r] = [(j >> b) & 1 for b in range(5)]
            else:
                sel[r, j] = 1
        count = n1 + (n_sel * E if packed else 0)
        d = (count - 1).bit_length()
        qp = np.zeros((nq, N), dtype=np.uint64)
        for r, (i, _) in enumerate(idx):
            qp[r, i] = pow(1 << d, -1, t)
        # the client
        query = g.alloc(nq * per)
        g.encrypt(nq, g.to_device(qp), 94, 0, query)
        rg = g.alloc(nq * n_sel * rows * per)
        if packed:
            pk_ct = g.alloc(nq * per)
            g.bfv_selector_encrypt(L, V, nq, n_sel, n1, count, g.to_device(sel), 95, 0, pk_ct)
            g.add(L, 2, nq, query, pk_ct, pw, query)
            g.sync()
            pk_ct.free()
        else:
            msg = np.zeros((nq * n_sel, N), dtype=np.uint64)
            msg[:, 0] = sel.reshape(-1)
            g.bfv_rgsw_encrypt(L, V, nq * n_sel, g.to_device(msg), 95, 0, rg)
        kids, res1, one, low = g.alloc(count * nq * per), g.alloc(nq * n2 * per), g.alloc(nq * per), g.alloc(nq * 2 * N)
        budgets = {}

        def server(measure=False):
            g.bfv_expand(L, nq, query, count, kids)
            if measure:
                budgets["expand"] = g.bfv_noise_budget(L, 2, n1 * nq, kids)
            if packed:
                g.bfv_rgsw_from_bfv(L, V, V, nq, n_sel, At(kids, n1 * nq * per), 1, nq, key, rg)
            g.bfv_transform_to_ntt(L, 2, n1 * nq, kids, kids)
            g.bfv_multiply_plain_accumulate(L, 2, nq, n2, n1, kids, 1, nq, dbn, n2, 1, res1)
            g.bfv_transform_from_ntt(L, 2, nq * n2, res1, res1)
            if measure:
                budgets["scan"] = g.bfv_noise_budget(L, 2, nq * n2, res1)
            if bits_route:
                g.bfv_select(L, V, nq, n2, res1, n2, 1, rg, n_sel, 1, one)
            else:
                g.bfv_external_product(L, V, nq, n2, res1, n2, 1, rg, n_sel, 1, one)
            if measure:
                budgets["second dimension"] = g.bfv_noise_budget(L, 2, nq, one)
            g.bfv_mod_switch(L, 1, 2, nq, one, low)
            if measure:
                budgets["reply (L = 1)"] = g.bfv_noise_budget(1, 2, nq, low)

        server(measure=True)
        dec = g.alloc(nq * N)
        g.decrypt(1, 2, nq, low, dec)
        ok = np.array_equal(dec.download((nq, N)), want)
        name = f"{'5 bit selectors, he355_bfv_select' if bits_route else '32 one-hot selectors, he355_bfv_external_product'}, {'packed query' if packed else 'uploaded RGSW'}"
        info = (f"children expanded {count} (d = {d}), converted {n_sel * E if packed else 0}, query slots {n_sel * E}, "
                f"query bytes {per * 8 if packed else per * 8 + n_sel * rows * per * 8}; budgets (bits) "
                + ", ".join(f"{k} {b.min()}..{b.max()}" for k, b in budgets.items()) + f"; replies decrypt to db[i][j]: {ok}")
        return name, server, info, [query, rg, kids, res1, one, low, dec]

    for packed in (False, True):
        a, b = route(True, packed), route(False, packed)
        ta, tb = alternated(g, [a[1], b[1]], [2, 2], repeats)
        for (name, _, info, _), tt in ((a, ta), (b, tb)):
            print(f"  {name}: us per answer set, min / median / max of {repeats} regions {fmt(tt)}\n      {info}")
        print(f"      one-hot / bits {tb[1] / ta[1]:6.3f}   spread of one-hot {(tb[2] - tb[0]) / tb[1] * 100:4.1f} %", flush=True)
        for x in a[3] + b[3]:
            x.free()
        g.pool_trim()
    g.close()


if mode in ("call", "all", "n1024"):
    for N, bits in (SMALL if mode == "n1024" else RINGS):
        g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
        print(f"== N = {N} {bits}  L = {g.L}  v = {V}  E = {g.bfv_gadget_count(g.L, V)[0]}", flush=True)
        for count, n in SHAPES:
            call_run(g, N, g.L, count, n)
        g.close()
if mode in ("retrieval", "all"):
    retrieval_run(*RINGS[0])
