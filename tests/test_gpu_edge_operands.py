"""The evaluator kernels held to the oracle at structured and extreme operands (run with -m gpu on an MI355X).

Every other GPU test draws its ciphertexts and keys uniformly, and the kernels here are fast because they are lazy: their worst-case
magnitude arguments (the u64 engine's accumulation runs of kAccRun products, the fp64 engine's 48-bit digit rows and |sum| < 2^52
accumulators, the floors' branches on the dropped residue) are reached by uniform data with probability close to zero.  This module
feeds the composed pipelines the families of tests/edge_operands.py -- every residue q - 1, digits that are all q_j - 1, alternating
and impulse patterns in both forms, coefficients planted on every edge of every floor -- under key-switch keys that are uniform, all
q_t - 1, or the identity on the first or the last data prime's digit (the key switch then has a closed form in Python integers, held
here next to the oracle).  Each batch mixes the extremes (positions 0, 2, 4 of n = 5) with uniform neighbours and is cut into ragged
chunks of 2, so an offset or a leak between batch rows shows.  Everything is bit-exact (np.array_equal); every input is a valid residue.

Chains: {60,45,45,60} N = 4096 (mixed engines, fold build), {60,60,60,60} N = 2048 (fold only), {55,52,50,58} (Shoup build, runs of six),
{60,45,45,60} with every prime forced onto the u64 engine, {47,46,45,44,47} N = 32768 and {46,47,60,46} N = 4096 (the re-centring and
general-path digit lifts; the latter's special prime is far below q_2, so identity(2) drives the mod-down through every residue edge at
large quotients), {60,45,45,58} (special prime below q_0), {60 x 7} and nine primes of 50 - 59 bits (full accumulation runs of both builds), {60,50,40,60} at N = 16384 (the Shoup build at LOGN1 = 4: tests/shoup_rings.py), the headline chain {60, 45 x 15, 60} at N = 32768, and BFV {60,40,40,60}.
For N <= 8192 the key-switching ops run under the ring-in-LDS, latency and throughput shapes, he355_path_stats proving which ran.
tests/test_edge_operands_cpu.py holds the oracle to the exact model and to the closed form at the same operands, without a GPU."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import edge_operands as eo  # noqa: E402
import make_exact_vectors_edges as mk  # noqa: E402
import shoup_rings as sr  # noqa: E402

CHAINS = {
    # name: (N, key-level bit sizes, force_u64)
    "n4096_60_45_45_60_mixed_engines_fold": (4096, [60, 45, 45, 60], False),
    "n2048_60_60_60_60_fold_only": (2048, [60, 60, 60, 60], False),
    "n4096_55_52_50_58_shoup_runs_of_6": (4096, [55, 52, 50, 58], False),
    "n4096_60_45_45_60_force_u64": (4096, [60, 45, 45, 60], True),
    "n32768_47_46_45_44_47_recentring_lifts": (32768, [47, 46, 45, 44, 47], False),
    "n4096_46_47_60_46_general_path_lifts": (4096, [46, 47, 60, 46], False),
    "n4096_60_45_45_58_special_below_q0": (4096, [60, 45, 45, 58], False),
    # chains long enough for FULL lazy accumulation runs in the key product (a run is cut short by the end of the digits: three data
    # primes never reach kAccRun products): six 60-bit digits on the fold build (a run of 5, then 1), eight Shoup-form digits (6, then 2)
    "n4096_60x7_fold_full_runs": (4096, [60] * 7, False),
    "n4096_50_to_59_x9_shoup_full_runs": (4096, [55, 52, 50, 58, 53, 51, 54, 56, 57], False),
    # the Shoup build at LOGN1 = 4 (tests/shoup_rings.py): a 60- and a 50-bit prime on its u64 engine, an fp64 prime between them
    "n16384_60_50_40_60_shoup": (16384, sr.bits("n16384_60_50_40_60_shoup"), False),
}
KEYS = ["uniform", "qm1", "identity_first", "identity_last"]
# the families that take turns at positions 2 and 4 of a batch (position 0: qm1_coeff, or planted under an identity key)
OTHERS = [f for f in eo.CT_FAMILIES if f not in ("qm1_coeff", "planted")]
SHAPES = ["lds", "latency", "throughput"]


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    return mod


def make_pair(be, oracle, N, bits, force, scheme="ckks", primes=None, t=0):
    """primes (and t for BFV): the moduli themselves instead of bit sizes (tests/explicit_moduli.py)"""
    bfv = scheme == "bfv"
    if primes is not None:
        assert not force
        sid = (be.SCHEME_BFV, oracle.SCHEME_BFV) if bfv else (be.SCHEME_CKKS, oracle.SCHEME_CKKS)
        g = be.Context(sid[0], N, primes=list(primes), plain_modulus=t, device=0)
        o = oracle.Context(sid[1], N, primes=list(primes), plain_modulus=t)
        assert g.moduli == o.moduli == list(primes) and g.t == o.t == t
        return g, o
    if force:
        os.environ["HE355_FORCE_U64"] = "1"
    try:
        g = be.Context(be.SCHEME_BFV if bfv else be.SCHEME_CKKS, N, bit_sizes=bits, plain_bits=20 if bfv else 0, sec128=False, device=0)
    finally:
        os.environ.pop("HE355_FORCE_U64", None)
    o = oracle.Context(oracle.SCHEME_BFV if bfv else oracle.SCHEME_CKKS, N, bit_sizes=bits, plain_bits=20 if bfv else 0, sec128=False)
    assert g.moduli == o.moduli
    if force:
        assert not any(g.fp64)
    return g, o


@pytest.fixture(scope="module", params=list(CHAINS))
def pair(request, be, oracle):
    N, bits, force = CHAINS[request.param]
    g, o = make_pair(be, oracle, N, bits, force)
    if request.param in sr.RINGS:
        sr.check_device(request.param, g)
    yield g, o, request.param
    g.close()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first at [poly, prime, coefficient] = {bad[0].tolist()}: "
                             f"{int(got[tuple(bad[0])])} != {int(want[tuple(bad[0])])}")


# ---------------------------------------------------------------------------------------------------------------------------------
# ops without a key switch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_add_sub_multiply_plain_ops_rescale_and_sums(pair, be):
    g, o, chain = pair
    L, N, n = g.L, g.N, 5
    rng = np.random.default_rng(len(chain))
    pw = be.Context.pairwise()
    g.set_chunk(2)
    try:
        # add / sub: qm1 + qm1, zero - qm1, half + half1 (each pair both added and subtracted), uniform neighbours between them
        a = eo.batch(o, ["qm1", None, "zero", None, "half"], L, 2, rng)
        b = eo.batch(o, ["qm1", None, "qm1", None, "half1"], L, 2, rng)
        da, db = g.to_device(a), g.to_device(b)
        out = g.alloc(n * 2 * L * N)
        g.add(L, 2, n, da, db, pw, out)
        got = out.download((n, 2, L, N))
        for r in range(n):
            same(got[r], o.add(a[r], b[r]), (chain, "add", r))
        g.add(L, 2, n, da, db, pw, out, sub=True)
        got = out.download((n, 2, L, N))
        for r in range(n):
            same(got[r], o.sub(a[r], b[r]), (chain, "sub", r))
        assert not got[0].any() and np.array_equal(got[2], eo.family(o, "one", L))  # (q-1) - (q-1) = 0, 0 - (q-1) = 1
        # multiply: 2 x 2 and 3 x 2 outer products, every dyadic product at its top ((q-1)^2) in the qm1 rows
        ma = eo.batch(o, ["qm1", None, "qm1_coeff"], L, 2, rng)
        mb = eo.batch(o, ["qm1", "half1"], L, 2, rng)
        dma, dmb = g.to_device(ma), g.to_device(mb)
        for b0 in (2, 3):
            o3 = g.alloc(b0 * 2 * 3 * L * N)
            g.multiply(L, b0 * 2, dma, dmb, be.Context.outer(0, b0, 0, 2), o3)
            got = o3.download((b0 * 2, 3, L, N))
            for i in range(b0):
                for x in range(2):
                    same(got[i * 2 + x], o.multiply_ntt(ma[i], mb[x]), (chain, "multiply", b0, i, x))
        # multiply_plain / add_plain, per-op plaintexts
        cts = eo.batch(o, ["qm1", None, "half", None, "alt"], L, 2, rng)
        pts = eo.batch(o, ["qm1", None, "half1", None, "alt_half"], L, 1, rng)[:, 0]
        dc, dp = g.to_device(cts), g.to_device(pts)
        g.multiply_plain(L, 2, n, dc, dp, pw, out)
        got = out.download((n, 2, L, N))
        for r in range(n):
            same(got[r], o.multiply_plain(cts[r], pts[r]), (chain, "multiply_plain", r))
        g.add_plain(L, 2, n, dc, dp, pw, out)
        got = out.download((n, 2, L, N))
        for r in range(n):
            same(got[r], o.add_plain(cts[r], pts[r]), (chain, "add_plain", r))
        # rescale, sizes 2 and 3: `planted` puts the last data prime's residue on every edge of the floor
        for size in (2, 3):
            src = eo.batch(o, ["planted", None, "qm1", None, "half1_coeff"], L, size, rng)
            back = o.intt(L - 1, src[0, 0, L - 1])
            assert set(eo.edge_values(int(o.moduli[L - 1]))) <= {int(x) for x in back[:400]}
            o2 = g.alloc(n * size * (L - 1) * N)
            g.rescale(L, size, n, g.to_device(src), o2)
            got = o2.download((n, size, L - 1, N))
            for r in range(n):
                same(got[r], o.rescale(src[r]), (chain, "rescale", size, r))
        # sum and multiply_accumulate over 33 terms that are all q - 1 (row 0; row 1 of the matrix product: uniform neighbours)
        inner = 33
        allq = eo.batch(o, ["qm1"] * inner, L, 2, rng)
        ds = g.alloc(2 * L * N)
        g.sum(L, 2, inner, g.to_device(allq), ds)
        want = allq[0]
        for r in range(1, inner):
            want = o.add(want, allq[r])
        same(ds.download((2, L, N)), want, (chain, "sum"))
        assert int(want[0, 0, 0]) == int(o.moduli[0]) - inner
        rows = 2
        ma = np.concatenate([allq, eo.batch(o, [None] * inner, L, 2, rng)])  # a(i, k) at i * inner + k
        d3 = g.alloc(rows * 3 * L * N)
        g.multiply_accumulate(L, rows, 1, inner, g.to_device(ma), inner, 1, g.to_device(allq), 1, 1, d3)
        got = d3.download((rows, 3, L, N))
        for i in range(rows):
            acc = o.multiply_ntt(ma[i * inner], allq[0])
            for k in range(1, inner):
                acc = o.add(acc, o.multiply_ntt(ma[i * inner + k], allq[k]))
            same(got[i], acc, (chain, "multiply_accumulate", i))
    finally:
        g.set_chunk(1024)


# ---------------------------------------------------------------------------------------------------------------------------------
# key-switching ops
# ---------------------------------------------------------------------------------------------------------------------------------
def _naf_terms(step, N):
    """SEAL's NAF terms of a rotation step, least significant first (Evaluator::rotate_internal); a term of N/2 is no rotation."""
    neg, x, i, out = step < 0, abs(step), 0, []
    while x:
        z = 2 - (x & 3) if x & 1 else 0
        x = (x - z) >> 1
        if z and (1 << i) != N // 2:
            out.append((-z if neg else z) * (1 << i))
        i += 1
    return out


KEY_STEPS = [1, 2, 4, -1]
SUM_STEPS = [1, 3, 5]  # 3 = -1 + 4, 5 = 1 + 4: NAF chains that share nothing with a key of their own


def key_set(o, kind, rng, L, steps=KEY_STEPS, conj=True):
    """(relinearization key, {Galois element: key}, j0 or None) of one kind for a level-L test: identity_first / identity_last select the
    digit of the first / the last data prime of the level"""
    ident = kind.startswith("identity")
    j0 = (0 if kind == "identity_first" else L - 1) if ident else None
    base = "identity" if ident else kind
    rk = eo.key(o, base, rng, j0 or 0)
    elts = [o.galois_elt(s) for s in steps] + ([2 * o.N - 1] if conj else [])
    gk = {e: (rk if base != "uniform" else eo.key(o, base, rng)) for e in elts}  # (only uniform keys differ from one another)
    return rk, gk, j0


def install(g, rk, gk):
    g.set_relin_key(rk)
    for e, k in gk.items():
        g.set_galois_key(e, k)


def operands(o, kind, rng, L, n, slot, coeff_form=False):
    """a, b [n, 2, L, N] and c3 [n, 3, L, N]: extremes at the even positions, uniform neighbours at the odd ones.  Position 0: qm1_coeff
    (every coefficient of every digit q_j - 1), or under an identity key `planted` with the selected digit on every edge of the
    mod-down.  Position 2: qm1 -- in NTT form the constant -1, whose digits are the constant q_j - 1 at EVERY point of every target
    prime's transform, so that with an all-(q_t - 1) key every term of every accumulator is the same near-top product -- or, under an
    identity key, qm1_coeff.  Position 4: the other families take turns (OTHERS[slot])."""
    ident = kind.startswith("identity")
    j0 = (0 if kind == "identity_first" else L - 1) if ident else None
    fixed = ["planted", "qm1_coeff"] if ident else ["qm1_coeff", "qm1"]
    names = [(fixed[r // 2] if r < 4 else OTHERS[slot % len(OTHERS)]) if r % 2 == 0 else None for r in range(n)]
    a = eo.batch(o, names, L, 2, rng, coeff_form=coeff_form)
    b = eo.batch(o, [nm if nm is None else ("qm1" if k == 0 else nm) for k, nm in enumerate(names)], L, 2, rng, coeff_form=coeff_form)
    c3 = eo.batch(o, names, L, 3, rng, coeff_form=coeff_form)
    if ident:
        c3[0, 2] = eo.planted_digit(o, L, j0, rng, coeff_form=coeff_form)
        a[0, 1] = eo.planted_digit(o, L, j0, rng, coeff_form=coeff_form)
    return names, a, b, c3


def rotate_chain(ks, o, ct, step, gk):
    terms = [step] if o.galois_elt(step) in gk else _naf_terms(step, o.N)
    for t in terms:
        ct = ks.apply_galois(ct, o.galois_elt(t), gk[o.galois_elt(t)])
    return ct


def expected_ckks(o, ks, L, a, b, c3, rk, gk):
    """{op: [result of row r]} with the two key-switching primitives taken from ks: the oracle itself, or eo.IdentityOps (closed form)"""
    n, N = a.shape[0], o.N
    e1, conj = o.galois_elt(1), 2 * N - 1
    w = {}
    w["relinearize"] = [ks.relinearize(c3[r], rk) for r in range(n)]
    w["multiply_relin"] = [ks.relinearize(o.multiply_ntt(a[r], b[r]), rk) for r in range(n)]
    if L >= 2:
        w["relinearize_rescale"] = [o.rescale(x) for x in w["relinearize"]]
        w["multiply_relin_rescale"] = [o.rescale(x) for x in w["multiply_relin"]]
    w["apply_galois_1"] = [ks.apply_galois(a[r], e1, gk[e1]) for r in range(n)]
    w["apply_galois_conj"] = [ks.apply_galois(a[r], conj, gk[conj]) for r in range(n)]
    w["rotate_3_naf"] = [rotate_chain(ks, o, a[r], 3, gk) for r in range(n)]
    w["rotate_add_1"] = [o.add(b[r], w["apply_galois_1"][r]) for r in range(n)]
    w["rotate_add_3_naf"] = [o.add(b[r], w["rotate_3_naf"][r]) for r in range(n)]
    acc = []
    for r in range(n):  # accumulateCKKS(count = 5): rotations by 1, 2, 4, each added to the running sum
        t = a[r]
        for i in range(3):
            e = o.galois_elt(1 << i)
            t = o.add(t, ks.apply_galois(t, e, gk[e]))
        acc.append(t)
    w["accumulate_5"] = acc
    rs = []
    for r in range(n):
        t = a[r].copy()
        for s in SUM_STEPS:
            t = o.add(t, rotate_chain(ks, o, a[r], s, gk))
        rs.append(t)
    w["rotate_sum"] = rs
    return w


def run_ckks(g, be, L, a, b, c3):
    """the same ops on the device, {op: [n, 2, L', N]}"""
    n, N = a.shape[0], g.N
    pw = be.Context.pairwise()
    da, db, d3 = g.to_device(a), g.to_device(b), g.to_device(c3)
    got = {}

    def run(name, f, Lo=L):
        out = g.alloc(n * 2 * Lo * N)
        f(out)
        got[name] = out.download((n, 2, Lo, N))

    run("relinearize", lambda out: g.relinearize(L, n, d3, out))
    run("multiply_relin", lambda out: g.multiply_relin(L, n, da, db, pw, out))
    if L >= 2:
        run("relinearize_rescale", lambda out: g.relinearize_rescale(L, n, d3, out), L - 1)
        run("multiply_relin_rescale", lambda out: g.multiply_relin(L, n, da, db, pw, out, rescale=True), L - 1)
    run("apply_galois_1", lambda out: g.apply_galois(L, n, da, g.galois_elt(1), out))
    run("apply_galois_conj", lambda out: g.apply_galois(L, n, da, 2 * N - 1, out))
    run("rotate_3_naf", lambda out: g.rotate(L, n, da, 3, out))
    run("rotate_add_1", lambda out: g.rotate_add(L, n, da, 1, db, out))
    run("rotate_add_3_naf", lambda out: g.rotate_add(L, n, da, 3, db, out))
    inplace = g.to_device(b)
    g.rotate_add(L, n, da, 1, inplace, inplace)  # the addend is the output
    got["rotate_add_1_in_place"] = inplace.download((n, 2, L, N))
    acc, tmp = g.to_device(a), g.alloc(n * 2 * L * N)
    g.accumulate(L, n, acc, 5, tmp)
    got["accumulate_5"] = acc.download((n, 2, L, N))
    return got


def select_shape(g, shape):
    """ring-in-LDS, latency or throughput for every chunk that follows (he355_set_lds_max / he355_set_latency_max); None: the library's rule"""
    if shape == "lds":
        g.set_lds_max(64)
    elif shape == "latency":
        g.set_lds_max(0)
        g.set_latency_max(64)
    elif shape == "throughput":
        g.set_lds_max(0)
        g.set_latency_max(0)
    else:
        g.set_lds_max(None)
        g.set_latency_max(None)


def assert_shape_ran(st, shape, what):
    if shape == "lds":
        assert st["ks_lds"] > 0 and st["ks_fused"] == st["ks_unfused"] == st["ks_latency"] == 0, (what, st)
    elif shape == "latency":
        assert st["ks_latency"] > 0 and st["ks_lds"] == st["ks_fused"] == st["ks_unfused"] == 0, (what, st)
    elif shape == "throughput":
        assert st["ks_fused"] + st["ks_unfused"] > 0 and st["ks_lds"] == st["ks_latency"] == 0, (what, st)


def check_all(got, want, what, alias=None):
    alias = alias or {}
    for name, res in got.items():
        w = want[alias.get(name, name)]
        for r in range(len(w)):
            same(res[r], w[r], what + (name, r))


ALIAS = {"rotate_add_1_in_place": "rotate_add_1"}


@pytest.mark.parametrize("kind", KEYS)
def test_key_switching_ops(pair, be, kind):
    """relinearize, multiply_relin (with and without rescale), relinearize_rescale, apply_galois (a rotation and the conjugation), a
    rotation through NAF steps, rotate_add out of place, through NAF steps and in place, accumulate and rotate_sum -- under one kind of
    key, in every key-switch shape the ring admits.  Under an identity key the expectations are also built from the closed form."""
    g, o, chain = pair
    L, N, n = g.L, g.N, 5
    slot = list(CHAINS).index(chain) * len(KEYS) + KEYS.index(kind)
    rng = np.random.default_rng(1000 + slot)
    rk, gk, j0 = key_set(o, kind, rng, L)
    install(g, rk, gk)
    names, a, b, c3 = operands(o, kind, rng, L, n, slot)
    want = expected_ckks(o, o, L, a, b, c3, rk, gk)
    what = (chain, kind, tuple(names))
    if j0 is not None:  # the oracle against the closed form in Python integers, then the device against both
        closed = expected_ckks(o, eo.IdentityOps(o, j0), L, a, b, c3, rk, gk)
        for name in want:
            for r in range(n):
                same(want[name][r], closed[name][r], what + ("oracle against the closed form", name, r))
    # (the ring-in-LDS shape holds up to six data primes: ks_lds_supported)
    shapes = [sh for sh in SHAPES if sh != "lds" or L <= 6] if N <= 8192 else [None]
    try:
        g.set_chunk(2)  # ragged: 2 + 2 + 1
        for shape in shapes:
            select_shape(g, shape)
            g.path_stats(reset=True)
            got = run_ckks(g, be, L, a, b, c3)
            assert_shape_ran(g.path_stats(), shape, what)
            check_all(got, want, what + (shape,), ALIAS)
            if j0 is not None:
                check_all(got, closed, what + (shape, "closed form"), ALIAS)
            out = g.alloc(n * 2 * L * N)
            g.rotate_sum(L, n, g.to_device(a), SUM_STEPS, out)  # (grouped key switches choose between the fused and unfused shapes only)
            check_all({"rotate_sum": out.download((n, 2, L, N))}, want, what + (shape,))
        if N > 8192:
            # a batch large enough for the fused key product (k_k3 with the floor in its epilogue; small rings would need hundreds of
            # ciphertexts): the same five rows repeated to the first batch with 128 special-prime blocks (fuse_pays, ks_shape.h:
            # N / 1024 blocks per op-group of eight -- 32 ciphertexts at N = 32768, 64 at N = 16384), one chunk
            big = 8 * -(-128 // (N // 1024))
            idx = np.arange(big) % n
            g.set_chunk(1024)
            g.path_stats(reset=True)
            d3, da, db = g.to_device(c3[idx]), g.to_device(a[idx]), g.to_device(b[idx])
            out = g.alloc(big * 2 * L * N)
            g.relinearize(L, big, d3, out)
            got = {"relinearize": out.download((big, 2, L, N))}
            g.rotate(L, big, da, 3, out)
            got["rotate_3_naf"] = out.download((big, 2, L, N))
            out2 = g.alloc(big * 2 * (L - 1) * N)
            g.multiply_relin(L, big, da, db, be.Context.pairwise(), out2, rescale=True)
            got["multiply_relin_rescale"] = out2.download((big, 2, L - 1, N))
            st = g.path_stats()
            assert st["ks_fused"] >= 4 and st["ks_lds"] == st["ks_latency"] == st["ks_unfused"] == 0, (what, st)
            for name, res in got.items():
                for r in range(big):
                    same(res[r], want[name][r % n], what + ("fused", name, r))
    finally:
        select_shape(g, None)
        g.set_chunk(1024)


@pytest.mark.parametrize("kind", KEYS)
def test_key_switching_ops_one_level_down(pair, be, kind):
    """The same at level L - 1 (the key's first L - 1 digits, the special prime still last) for the ops a lower level changes most:
    relinearize, multiply_relin with rescale, a rotation -- in the shape the library's own rule picks."""
    g, o, chain = pair
    L, N, n = g.L - 1, g.N, 5
    slot = list(CHAINS).index(chain) * len(KEYS) + KEYS.index(kind) + 9
    rng = np.random.default_rng(2000 + slot)
    rk, gk, j0 = key_set(o, kind, rng, L)
    install(g, rk, gk)
    names, a, b, c3 = operands(o, kind, rng, L, n, slot)
    pw = be.Context.pairwise()
    ops = [o] + ([eo.IdentityOps(o, j0)] if j0 is not None else [])
    e1 = o.galois_elt(1)
    g.set_chunk(2)
    try:
        out = g.alloc(n * 2 * L * N)
        g.relinearize(L, n, g.to_device(c3), out)
        got = out.download((n, 2, L, N))
        for ks in ops:
            for r in range(n):
                same(got[r], ks.relinearize(c3[r], rk), (chain, kind, names[r], "relinearize", r))
        g.apply_galois(L, n, g.to_device(a), e1, out)
        got = out.download((n, 2, L, N))
        for ks in ops:
            for r in range(n):
                same(got[r], ks.apply_galois(a[r], e1, gk[e1]), (chain, kind, names[r], "apply_galois", r))
        if L >= 2:
            out2 = g.alloc(n * 2 * (L - 1) * N)
            g.multiply_relin(L, n, g.to_device(a), g.to_device(b), pw, out2, rescale=True)
            got = out2.download((n, 2, L - 1, N))
            for ks in ops:
                for r in range(n):
                    same(got[r], o.rescale(ks.relinearize(o.multiply_ntt(a[r], b[r]), rk)), (chain, kind, names[r], "multiply_relin_rescale", r))
    finally:
        g.set_chunk(1024)


@pytest.mark.parametrize("kind", KEYS)
def test_headline_chain(be, oracle, kind):
    """N = 32768, {60, 45 x 15, 60}: the most digits per key product (16 terms per accumulator: three lazy runs on the u64 engine's two
    primes, 16 centred products on the fp64 engine's accumulators) and five column stages.  n = 3: extremes at 0 and 2."""
    N, bits = 32768, [60] + [45] * 15 + [60]
    g, o = make_pair(be, oracle, N, bits, False)
    try:
        L, n = g.L, 3
        rng = np.random.default_rng(3000 + KEYS.index(kind))
        rk, gk, j0 = key_set(o, kind, rng, L, steps=[1], conj=False)
        e1 = o.galois_elt(1)
        g.set_relin_key(rk)
        g.set_galois_key(e1, gk[e1])
        names, a, b, c3 = operands(o, kind, rng, L, n, KEYS.index(kind))
        ops = [o] + ([eo.IdentityOps(o, j0)] if j0 is not None else [])
        pw = be.Context.pairwise()
        g.set_chunk(2)
        out = g.alloc(n * 2 * L * N)
        g.relinearize(L, n, g.to_device(c3), out)
        got = out.download((n, 2, L, N))
        for ks in ops:
            for r in range(n):
                same(got[r], ks.relinearize(c3[r], rk), (kind, names[r], "relinearize", r))
        g.rotate(L, n, g.to_device(a), 1, out)
        got = out.download((n, 2, L, N))
        for ks in ops:
            for r in range(n):
                same(got[r], ks.apply_galois(a[r], e1, gk[e1]), (kind, names[r], "rotate", r))
        out2 = g.alloc(n * 2 * (L - 1) * N)
        g.multiply_relin(L, n, g.to_device(a), g.to_device(b), pw, out2, rescale=True)
        got = out2.download((n, 2, L - 1, N))
        for ks in ops:
            for r in range(n):
                same(got[r], o.rescale(ks.relinearize(o.multiply_ntt(a[r], b[r]), rk)), (kind, names[r], "multiply_relin_rescale", r))
    finally:
        g.close()


@pytest.mark.parametrize("kind", KEYS)
def test_bfv_key_switching_ops(be, oracle, kind):
    """A BFV context ({60,40,40,60}, N = 4096; coefficient-form ciphertexts, so a family and its `_coeff` twin are the same operand):
    relinearize, apply_galois (rotate_rows and rotate_columns) and the matrix product bfv_multiply_relin_accumulate over an inner index
    of 3 whose operands are the extremes.  A BFV context's key switches always take the coefficient-form pipeline (KsShape::BfvCoeff:
    the ring-in-LDS and latency shapes are for the NTT-domain pipeline, and he355_path_stats has no counter for this one), so there is
    no shape to select or to assert here; he355_set_latency_max only moves the walk of the rotation chains."""
    N, bits = 4096, [60, 40, 40, 60]
    g, o = make_pair(be, oracle, N, bits, False, scheme="bfv")
    try:
        L, n = g.L, 5
        slot = 4 * KEYS.index(kind) + 2
        rng = np.random.default_rng(4000 + slot)
        rk, gk, j0 = key_set(o, kind, rng, L)
        install(g, rk, gk)
        names, a, b, c3 = operands(o, kind, rng, L, n, slot, coeff_form=True)
        ops = [o] + ([eo.IdentityOps(o, j0, coeff_form=True)] if j0 is not None else [])
        g.set_chunk(2)
        for lat in (None, 0):
            g.set_latency_max(lat)
            out = g.alloc(n * 2 * L * N)
            g.relinearize(L, n, g.to_device(c3), out)
            got = out.download((n, 2, L, N))
            for ks in ops:
                for r in range(n):
                    same(got[r], ks.relinearize(c3[r], rk), (kind, names[r], "bfv relinearize", r))
            da = g.to_device(a)
            for elt in (o.galois_elt(1), 2 * N - 1):
                g.apply_galois(L, n, da, elt, out)
                got = out.download((n, 2, L, N))
                for ks in ops:
                    for r in range(n):
                        same(got[r], ks.apply_galois(a[r], elt, gk[elt]), (kind, names[r], "bfv apply_galois", elt, r))
            # out(i, 0) = sum_k relin(a(i, k) * b(k, 0)), a(i, k) at i * inner + k: row 0 = the extremes at 0, 2, 4, row 1 = rows 1, 3 and 0
            inner = 3
            am = np.stack([a[0], a[2], a[4], a[1], a[3], a[0]])
            bm = np.stack([b[0], b[2], b[4]])
            acc = g.alloc(2 * 2 * L * N)
            g.bfv_multiply_relin_accumulate(L, 2, 1, inner, g.to_device(am), inner, 1, g.to_device(bm), 1, 1, acc)
            got = acc.download((2, 2, L, N))
            for ks in ops:
                for i in range(2):
                    t = ks.relinearize(o.bfv_multiply(am[i * inner], bm[0]), rk)
                    for k in range(1, inner):
                        t = o.add(t, ks.relinearize(o.bfv_multiply(am[i * inner + k], bm[k]), rk))
                    same(got[i], t, (kind, "bfv_multiply_relin_accumulate", i))
    finally:
        g.set_latency_max(None)
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# a searched worst column of the fp64 engine's digit lift
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,bits", [(32768, [60] + [45] * 15 + [60]), (4096, [60, 45, 45, 60])])
def test_searched_worst_column_digit(be, oracle, N, bits):
    """The digit of prime 1 is the column found by eo.worst_column for target prime 2 (a larger lazy magnitude after the forward column
    pass than any of 10^5 uniform columns: tests/test_edge_operands_cpu.py measures both), replicated across the columns of the digit
    lift: relinearize under uniform and all-(q - 1) keys equals the oracle."""
    w = eo.worst_column(N, bits, 1, 2)
    assert w["magnitude"] > w["uniform_max"]
    g, o = make_pair(be, oracle, N, bits, False)
    try:
        L, n = g.L, 3
        rng = np.random.default_rng(N)
        digit = eo.column_digit(o, L, 1, w["column"])
        assert np.array_equal(o.intt(1, digit[1])[::N // len(w["column"])], w["column"])
        c3 = eo.batch(o, ["qm1", None, "qm1_coeff"], L, 3, rng)
        c3[0, 2] = digit
        c3[2, 2] = digit
        d3 = g.to_device(c3)
        for kind in ("uniform", "qm1"):
            rk = eo.key(o, kind, rng)
            g.set_relin_key(rk)
            want = [o.relinearize(c3[r], rk) for r in range(n)]
            for shape in (SHAPES if N <= 8192 else [None]):
                select_shape(g, shape)
                g.path_stats(reset=True)
                out = g.alloc(n * 2 * L * N)
                g.relinearize(L, n, d3, out)
                got = out.download((n, 2, L, N))
                assert_shape_ran(g.path_stats(), shape, (N, kind))
                for r in range(n):
                    same(got[r], want[r], (N, kind, shape, "relinearize of the searched column", r))
    finally:
        select_shape(g, None)
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the small rings of tests/golden/exact_vectors_edges.json: the HIP path against the exact big-integer model, no oracle arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
FIX = json.load(open(os.path.join(HERE, "golden", "exact_vectors_edges.json")))


@pytest.mark.parametrize("name", list(FIX))
def test_exact_model_edge_fixture_gpu(be, oracle, name):
    from test_exact_model import check
    f = FIX[name]
    case = next(c for c in mk.CASES if c["name"] == name)
    ckks = f["scheme"] == "ckks"
    N = f["N"]
    pw = be.Context.pairwise()
    seen = set()
    for pair_ in case["pairs"]:
        g, o = make_pair(be, oracle, N, f["bits"], False, scheme=f["scheme"])
        try:
            assert [int(q) for q in g.moduli] == [int(p, 16) for p in f["primes"]]
            d = mk.build_inputs(case, o, pair_)  # (the oracle's transforms only, as the CPU test that pins them)
            install(g, d["rk"], d["gk"])

            class HipOps:
                def multiply(self, a, b):
                    out = g.alloc(3 * a.shape[1] * N)
                    (g.multiply if ckks else g.bfv_multiply)(a.shape[1], 1, g.to_device(a[None]), g.to_device(b[None]), pw, out)
                    return out.download((3, a.shape[1], N))

                def relinearize(self, c3, rk):
                    out = g.alloc(2 * c3.shape[1] * N)
                    g.relinearize(c3.shape[1], 1, g.to_device(np.ascontiguousarray(c3)[None]), out)
                    return out.download((2, c3.shape[1], N))

                def rescale(self, ct):
                    out = g.alloc(ct.shape[0] * (ct.shape[1] - 1) * N)
                    g.rescale(ct.shape[1], ct.shape[0], 1, g.to_device(np.ascontiguousarray(ct)[None]), out)
                    return out.download((ct.shape[0], ct.shape[1] - 1, N))

                def apply_galois(self, ct, elt, key):
                    out = g.alloc(ct.size)
                    g.apply_galois(ct.shape[1], 1, g.to_device(np.ascontiguousarray(ct)[None]), elt, out)
                    return out.download(ct.shape)

            label = mk.pair_label(pair_)
            for opname, got in mk.run_ops(case, d, HipOps()):
                check(f, label + ":" + opname, got)
                seen.add(label + ":" + opname)
            L = g.L
            if ckks:  # the fused sequences land on the same ciphertexts
                da, db = g.to_device(d["a"][None]), g.to_device(d["b"][None])
                out2 = g.alloc(2 * (L - 1) * N)
                g.multiply_relin(L, 1, da, db, pw, out2, rescale=True)
                check(f, label + ":multiply_relin_rescale", out2.download((2, L - 1, N)))
                g.relinearize_rescale(L, 1, g.to_device(d["c3"][None]), out2)
                check(f, label + ":relinearize_rescale", out2.download((2, L - 1, N)))
            out = g.alloc(2 * L * N)
            g.rotate(L, 1, g.to_device(d["a"][None]), 3, out)  # no key for 3: the NAF terms -1, +4
            check(f, label + ":rotate_3_naf", out.download((2, L, N)))
        finally:
            g.close()
    assert seen == set(f["expected"])
