"""The fused BFV PIR calls at the ring sizes they were built and measured for, N = 8192, 16384 and 32768, bit-exact (np.array_equal, no
tolerance) against references that use no device (bfv_ring_ref.py: numpy cuts, the oracle's transforms and products; held to Python integers
in test_bfv_ring_ref_cpu.py).  The column-pass kernels are templated on LOGN1 = log2(N / 1024) and compiled once per form of the u64 engine;
the other PIR modules stop at N = 4096 (LOGN1 <= 2).  Chains, each with a 40-bit prime so that both engines run wherever L >= 2:

    n8192_fold   (8192, {60, 40, 60})       LOGN1 3, fold form       n8192_shoup  (8192, {50, 40, 50})       LOGN1 3, Shoup form
    n16384_fold  (16384, {60, 40, 40, 60})  LOGN1 4, fold form       n32768_shoup (32768, {50, 40, 40, 50})  LOGN1 5, Shoup form
    n32768_fold  (32768, {60, 40, 40, 60})  LOGN1 5, fold form       n16384_shoup (16384, {60, 50, 40, 60})  LOGN1 4, Shoup form, two u64 data primes

Operands are uniform rows mixed with all-0, all-(q - 1) and alternating 0 / (q - 1) rows; every output lies between a ring's worth of
sentinel words before and after it; every operand is read back.  The routes of a call are bit-identical by definition, so every case resets
he355_bfv_route_stats first and asserts afterwards which route ran (printed: `routes <chain> <case>`).  Lt = the chain's data level, 2E = 14
rows at Lt = 3 and 10 at Lt = 2 for v = 20.  The shapes are the smallest that reach each route:

* he355_bfv_decompose_ntt: sizes 2 and 3, n = 3, (L, L_out) in {(Lt, Lt), (1, Lt), (Lt, 1)}: k_bfv_digits_cols_fwd, digits_fused = 1 per call;
* he355_bfv_unpack_bytes_ntt: n = 3 plaintexts of bytes_per_plain bytes from byte 5 of the slab, stride B + 3, the first all 0 and the last
  all 0xFF, L_out in {Lt, 1}: k_bfv_bytes_cols_fwd, bytes_fused = 1; he355_bfv_unpack_bytes then he355_bfv_pack_bytes gives the bytes back;
* he355_bfv_gadget_decompose_ntt, v in {20, 45}, every word: the column pass (n size L = 66 at Lt = 3, 64 at Lt = 2), exactly at its threshold
  (L = 1, size 2, n = 32: 64) and one short of it (63: the streaming cut);
* he355_bfv_external_product, v = 20, L = Lt, every result: (a) n = 4 with n inner L >= 32 and one selector row per result, column pass +
  k_bfv_gadget_mac; (b) the same child-major with one selector row for all; (c) 3 x 3, streaming cut + k_bfv_gadget_mac; (d) ONE result over
  inner L >= 32 contiguous rows: column pass + k_bfv_plain_mac; (e) one result, inner = 3: streaming cut + k_bfv_plain_mac; (f) N = 8192 only,
  L = 1, v = 4, inner = 9, n = 16: on the fold chain 270 terms (above the 256-term run of the 60-bit prime) in two passes through the pool
  block, the last one ragged (its one result takes the streaming cut); on the Shoup chain 2E = 26, so inner = 9 is one pass and inner = 10
  is run as well for the two; results 0, 7 and 15 against the oracle, all 16 against the composition on the device.  (Two passes at
  N = 32768 would take a 3.2 GB pool block: not run);
* he355_bfv_rgsw_from_bfv, L = Lt, (v, key_bits) = (20, 20), a uniform key, every row: slots L >= 32 for k_bfv_gadget_cols_fwd<LOGN1, true>
  (unit strides, and child-major behind two leading children), n = n_sel = 1 for k_bfv_gadget_spread<true>; (63, 4) once on n8192_fold;
* he355_bfv_multiply_monomial: n = 3, sizes 2 and 3, e in {1, 1023, 1024, 1025, N - 1, N, N + 1, 2N - 1} against the numpy shift;
* he355_bfv_expand: count = 8, n = 3 (one real encryption, two random_poly queries), L = Lt, keys from oracle.keygen_galois, every child against
  the oracle's tree; he355_path_stats printed (which key-switch shapes carried it), not asserted.

Not run: the pass split at N = 32768."""

import numpy as np
import pytest

import bfv_ring_ref as ring
import bfv_selector_ref as sel
import shoup_rings as shoup
from bfv_expand_ref import children, expand_levels, np_shift
from bfv_gpu_helpers import SENT, At, be, edged, ep_composition, expand_keys, inner_of, pair, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

CHAINS = {
    "n8192_fold": "n8192_default",
    "n16384_fold": (16384, [60, 40, 40, 60], 20),
    "n32768_fold": "n32768_d3",
    "n8192_shoup": (8192, [50, 40, 50], 20),
    "n32768_shoup": (32768, [50, 40, 40, 50], 20),
    "n16384_shoup": shoup.spec("n16384_60_50_40_60_shoup"),  # LOGN1 = 4 in the Shoup form: a 60- and a 50-bit prime on its u64 engine
}
SHOUP_RINGS = {"n16384_shoup": "n16384_60_50_40_60_shoup"}  # chain: its entry of shoup_rings.RINGS
IDS = list(CHAINS)
V = 20


_PAIRS = {}


def chain_pair(be, oracle, cid):
    """(g, o, N, sk, pk) of one chain, made once for the module; the keys matter to the expansion only"""
    if cid not in _PAIRS:
        g, o, N, sk, pk = pair(be, oracle, CHAINS[cid], keys=True)
        assert N >= 8192 and g.L in (2, 3)
        data = o.moduli[:g.L]  # a prime for each engine under the default assignment (below 2^47: fp64), whatever HE355_FORCE_U64 says
        assert any(q < 2 ** 47 for q in data) and any(q >= 2 ** 47 for q in data), "both engines"
        if cid in SHOUP_RINGS:
            shoup.check_device(SHOUP_RINGS[cid], g)
            shoup.check(SHOUP_RINGS[cid], o.moduli, g.t)
        _PAIRS[cid] = (g, o, N, sk, pk)
    return _PAIRS[cid]


def begin(g):
    g.bfv_route_stats(reset=True)


def routed(g, cid, case, want):
    """the counters since begin(), printed, and nothing but `want` counted"""
    got = {k: c for k, c in g.bfv_route_stats().items() if c}
    print(f"routes {cid} {case}: " + ", ".join(f"{k} = {c}" for k, c in got.items()))
    assert got == want, (cid, case, got)


# ---- he355_bfv_decompose_ntt ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_decompose_ntt(be, oracle, cid):
    g, o, N, *_ = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(301)
    Lt, n = g.L, 3
    for L, L_out in ((Lt, Lt), (1, Lt), (Lt, 1)):
        total = g.bfv_digit_count(L)[0]
        for size in (2, 3):
            what = (L, L_out, size)
            F = size * total
            x = edged(o, rng, n, L, size)
            dx = g.to_device(x)
            buf = sentinelled(g, n * F * L_out * N, N)
            begin(g)
            g.bfv_decompose_ntt(L, size, n, dx, L_out, At(buf, N))
            got = inner_of(buf, N, what).reshape(n, F, L_out, N)
            routed(g, cid, f"decompose_ntt L = {L}, L_out = {L_out}, size = {size}", {"digits_fused": 1})
            assert np.array_equal(got, ring.decompose_ntt_ref(o, x, L_out)), what
            assert np.array_equal(dx.download(x.shape), x), (what, "input")
            dx.free()
            buf.free()


# ---- he355_bfv_unpack_bytes_ntt ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_unpack_bytes_ntt(be, oracle, cid):
    g, o, N, *_ = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(302)
    n, base = 3, 5
    B, w = g.bfv_bytes_per_plain()
    assert w == o.t.bit_length() - 1 and B == N * w // 8
    stride = B + 3
    data = rng.integers(0, 256, (n, B), dtype=np.uint8)
    data[0], data[n - 1] = 0, 0xFF
    img = np.full((base + (n - 1) * stride + B + 16 + 7) // 8 * 8, 0xA5, dtype=np.uint8)  # the filler before, between and after
    for j in range(n):
        img[base + j * stride: base + j * stride + B] = data[j]
    src = g.to_device(img.view(np.uint64))
    for L_out in (g.L, 1):
        buf = sentinelled(g, n * L_out * N, N)
        begin(g)
        g.bfv_unpack_bytes_ntt(L_out, n, src, base, stride, B, At(buf, N))
        got = inner_of(buf, N, L_out).reshape(n, L_out, N)
        routed(g, cid, f"unpack_bytes_ntt L_out = {L_out}", {"bytes_fused": 1})
        assert np.array_equal(got, ring.unpack_bytes_ntt_ref(o, data, L_out)), L_out
        buf.free()
    # the streaming codec at the same ring: unpack, then pack gives the bytes back
    W8 = (B + 7) // 8 * 8
    plain, back = sentinelled(g, n * N, N), g.to_device(np.full(n * W8 // 8 + 2, SENT, dtype=np.uint64))
    begin(g)
    g.bfv_unpack_bytes(n, src, base, stride, B, At(plain, N))
    g.bfv_pack_bytes(n, At(plain, N), B, W8, back, 8)
    routed(g, cid, "unpack_bytes + pack_bytes", {})
    assert np.array_equal(inner_of(plain, N, "fields").reshape(n, N), ring.np_fields(data, w, N))
    exp = np.full(back.n, SENT, dtype=np.uint64).view(np.uint8)
    for j in range(n):
        exp[8 + j * W8: 8 + (j + 1) * W8] = 0
        exp[8 + j * W8: 8 + j * W8 + B] = data[j]
    assert np.array_equal(back.download().view(np.uint8), exp)
    assert np.array_equal(src.download().view(np.uint8), img), "input"
    for b in (src, plain, back):
        b.free()


# ---- he355_bfv_gadget_decompose_ntt -----------------------------------------------------------------------------------------------------
def gadget_shapes(Lt):
    """(L, size, n, counter): the column pass, exactly at its threshold of 256 blocks = n size L of 64, one short of it"""
    if Lt == 3:
        return [(3, 2, 11, "cut_cols"), (1, 2, 32, "cut_cols"), (3, 3, 7, "cut_stream")]
    return [(2, 2, 16, "cut_cols"), (1, 2, 32, "cut_cols"), (1, 3, 21, "cut_stream")]


@pytest.mark.parametrize("v", [20, 45])
@pytest.mark.parametrize("cid", IDS)
def test_gadget_decompose_ntt(be, oracle, cid, v):
    g, o, N, *_ = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(303 + v)
    for L, size, n, counter in gadget_shapes(g.L):
        assert (n * size * L >= 64) == (counter == "cut_cols") and 63 <= n * size * L <= 66
        what = (L, size, n, v)
        F = size * g.bfv_gadget_count(L, v)[0]
        x = edged(o, rng, n, L, size)
        dx = g.to_device(x)
        buf = sentinelled(g, n * F * L * N, N)
        begin(g)
        g.bfv_gadget_decompose_ntt(L, v, size, n, dx, At(buf, N))
        got = inner_of(buf, N, what).reshape(n, F, L, N)
        routed(g, cid, f"gadget_decompose_ntt v = {v}, L = {L}, size = {size}, n = {n}", {counter: 1})
        assert np.array_equal(got, ring.gadget_ntt_ref(o, x, v)), what
        assert np.array_equal(dx.download(x.shape), x), (what, "input")
        dx.free()
        buf.free()


# ---- he355_bfv_external_product ---------------------------------------------------------------------------------------------------------
def ep_case(g, o, rng, cid, L, v, n, inner, shared, child_major, N, case, want, check=None):
    """one call against external_product_ref: every result, or the results `check` against the oracle and all of them against the composition"""
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    n_rg = inner if shared else n * inner
    rg = g.alloc(n_rg * rows * per)
    g.fill_uniform(rg, n_rg * rows * 2 * L, list(range(L)), 3000 + n * 10 + inner)
    rg_h = rg.download((n_rg, rows, 2, L, N))
    x = edged(o, rng, n * inner, L)
    dx = g.to_device(x)
    sr, sk = (1, n) if child_major else (inner, 1)
    gr = 0 if shared else inner
    buf = sentinelled(g, n * per, N)
    begin(g)
    g.bfv_external_product(L, v, n, inner, dx, sr, sk, rg, gr, 1, At(buf, N))
    got = inner_of(buf, N, case).reshape(n, 2, L, N)
    routed(g, cid, f"external_product {case}", want)
    digits = ring.gadget_ntt_ref(o, x, v) if check is None else None  # the digits of every ciphertext once
    for r in range(n) if check is None else check:
        at = [r * sr + k * sk for k in range(inner)]
        rows_r = rg_h[:inner] if shared else rg_h[r * inner:(r + 1) * inner]
        ref = ring.external_product_ref(o, x[at], rows_r, v, None if digits is None else digits[at])
        assert np.array_equal(got[r], ref), (case, "result", r)
    if check is not None:
        assert np.array_equal(got, ep_composition(g, L, v, n, inner, x, lambda r, k: r * sr + k * sk, rg, gr, rows, N)), (case, "composition")
    assert np.array_equal(dx.download(x.shape), x), (case, "ciphertexts")
    assert np.array_equal(rg.download(rg_h.shape), rg_h), (case, "RGSW")
    for b in (rg, dx, buf):
        b.free()


@pytest.mark.parametrize("cid", IDS)
def test_external_product_many_results(be, oracle, cid):
    g, o, N, *_ = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(304)
    L = g.L
    inner = {3: 3, 2: 4}[L]
    assert 4 * inner * L >= 32 > 3 * 3 * L  # 4 x inner x 2 x L x 4 blocks reach the column pass, 3 x 3 does not
    cols, stream = {"cut_cols": 1, "mac_gadget": 1, "passes": 1}, {"cut_stream": 1, "mac_gadget": 1, "passes": 1}
    ep_case(g, o, rng, cid, L, V, 4, inner, False, False, N, f"(a) n = 4, inner = {inner}, a selector row per result", cols)
    ep_case(g, o, rng, cid, L, V, 4, inner, True, True, N, f"(b) n = 4, inner = {inner}, child-major, one selector row", cols)
    ep_case(g, o, rng, cid, L, V, 3, 3, False, False, N, "(c) n = 3, inner = 3", stream)


@pytest.mark.parametrize("cid", IDS)
def test_external_product_one_result(be, oracle, cid):
    """n = 1 over contiguous rows is k_bfv_plain_mac's; with inner L >= 32 the cut before it is the column pass"""
    g, o, N, *_ = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(305)
    L = g.L
    inner = {3: 11, 2: 16}[L]
    assert inner * L >= 32 > (inner - 1) * L and 3 * L < 32
    ep_case(g, o, rng, cid, L, V, 1, inner, False, False, N, f"(d) n = 1, inner = {inner}", {"cut_cols": 1, "mac_plain": 1, "passes": 1})
    ep_case(g, o, rng, cid, L, V, 1, 3, False, False, N, "(e) n = 1, inner = 3", {"cut_stream": 1, "mac_plain": 1, "passes": 1})


@pytest.mark.parametrize("cid,inner,passes", [("n8192_fold", 9, 2), ("n8192_shoup", 9, 1), ("n8192_shoup", 10, 2)])
def test_external_product_passes_through_the_pool_block(be, oracle, cid, inner, passes):
    """L = 1, v = 4, n = 16.  The 60-bit prime has 2E = 30 rows: inner = 9 is 270 terms, above its 256-term run (a fold inside every result),
    and 15 results fill the pool block of 4096 digit polynomials, so the call takes two passes, the last one ragged.  The 50-bit prime has
    2E = 26 rows: inner = 9 is 234 terms and one pass of 17 would hold all 16 results (run as it is, one pass); inner = 10 is 260 terms and
    takes the two passes there"""
    g, o, N, *_ = chain_pair(be, oracle, cid)
    L, v, n = 1, 4, 16
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    terms = inner * rows
    assert rows == 2 * -(-o.moduli[0].bit_length() // v)
    if cid == "n8192_fold":
        assert terms == 270 > (2 ** 128 - 1) // (o.moduli[0] - 1) ** 2 == 256
    per_pass = min(n, 4096 // terms)
    assert -(-n // per_pass) == passes and (passes == 1 or n - per_pass == 1)
    if passes == 2:  # the last pass cuts the inner ciphertexts of ONE result: 9 or 10 x 2 x 4 blocks, below the column pass
        want = {"cut_cols": 1, "cut_stream": 1, "mac_gadget": 2, "passes": 2}
    else:
        want = {"cut_cols": 1, "mac_gadget": 1, "passes": 1}
    ep_case(g, o, np.random.default_rng(306), cid, L, v, n, inner, True, False, N, f"(f) L = 1, v = 4, n = 16, inner = {inner}", want, check=(0, 7, 15))


# ---- he355_bfv_rgsw_from_bfv ------------------------------------------------------------------------------------------------------------
def from_bfv_call(g, cid, L, v, kv, n, n_sel, dx, x, lead, child_major, key, refs, N, case, want):
    """one call on the slab x (already on the device); refs(c) = (row k = 0, row k = 1) of slab entry c by the oracle, made once"""
    E = g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    S = n_sel * E
    if child_major:  # the strides of an expansion: d_ct points behind `lead` leading children
        sr, sk, order = 1, n, [(lead + s) * n + r for r in range(n) for s in range(S)]
    else:
        sr, sk, order, lead = S, 1, list(range(n * S)), 0
    buf = sentinelled(g, n * n_sel * 2 * E * per, N)
    begin(g)
    g.bfv_rgsw_from_bfv(L, v, kv, n, n_sel, At(dx, lead * n * per), sr, sk, key, At(buf, N))
    got = inner_of(buf, N, case).reshape(n * n_sel, 2 * E, 2, L, N)
    routed(g, cid, f"rgsw_from_bfv {case}", want)
    k0, k1 = zip(*(refs(c) for c in order))
    assert np.array_equal(got, sel.np_rows(np.stack(k0), np.stack(k1), E)), case
    assert np.array_equal(dx.download(x.shape), x), (case, "ciphertexts")
    buf.free()


def from_bfv_setup(g, o, rng, L, kv, entries, N, seed):
    rows = 2 * g.bfv_gadget_count(L, kv)[0]
    key = g.alloc(rows * 2 * L * N)
    g.fill_uniform(key, rows * 2 * L, list(range(L)), seed)
    key_h = key.download((rows, 2, L, N))
    x = edged(o, rng, entries, L)
    memo = {}

    def refs(c):
        if c not in memo:
            memo[c] = ring.rgsw_from_bfv_rows(o, x[c], key_h, kv)
        return memo[c]

    return key, key_h, x, g.to_device(x), refs


@pytest.mark.parametrize("cid", IDS)
def test_rgsw_from_bfv(be, oracle, cid):
    g, o, N, *_ = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(307)
    L, kv, lead = g.L, V, 2
    E = g.bfv_gadget_count(L, V)[0]
    n, n_sel = {3: (2, 1), 2: (2, 2)}[L]
    S = n_sel * E
    assert n * S * L >= 32 > E * L  # slots x 2 L x 4 blocks: the column pass from 256 on
    key, key_h, x, dx, refs = from_bfv_setup(g, o, rng, L, kv, (lead + S) * n, N, 4000)
    cols = {"own_cols": 1, "passes": 1}
    from_bfv_call(g, cid, L, V, kv, n, n_sel, dx, x, lead, False, key, refs, N, f"n = {n}, n_sel = {n_sel}", cols)
    from_bfv_call(g, cid, L, V, kv, n, n_sel, dx, x, lead, True, key, refs, N, f"n = {n}, n_sel = {n_sel}, child-major behind {lead} children", cols)
    from_bfv_call(g, cid, L, V, kv, 1, 1, dx, x, lead, False, key, refs, N, "n = 1, n_sel = 1", {"own_stream": 1, "passes": 1})
    assert np.array_equal(key.download(key_h.shape), key_h), "key"
    key.free()
    dx.free()


def test_rgsw_from_bfv_one_digit_per_prime_and_a_narrow_key(be, oracle):
    cid = "n8192_fold"
    g, o, N, *_ = chain_pair(be, oracle, cid)
    L, v, kv = g.L, 63, 4
    assert g.bfv_gadget_count(L, v)[0] == L and g.bfv_gadget_count(L, kv)[0] == 15 + 10
    key, key_h, x, dx, refs = from_bfv_setup(g, o, np.random.default_rng(308), L, kv, L, N, 4001)
    from_bfv_call(g, cid, L, v, kv, 1, 1, dx, x, 0, False, key, refs, N, "(v, key_bits) = (63, 4)", {"own_stream": 1, "passes": 1})
    assert np.array_equal(key.download(key_h.shape), key_h), "key"
    key.free()
    dx.free()


# ---- he355_bfv_multiply_monomial, he355_bfv_expand --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_multiply_monomial(be, oracle, cid):
    g, o, N, *_ = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(309)
    L, n = g.L, 3
    for size in (2, 3):
        per = size * L * N
        x = edged(o, rng, n, L, size)
        dx = g.to_device(x)
        for e in (1, 1023, 1024, 1025, N - 1, N, N + 1, 2 * N - 1):
            buf = sentinelled(g, n * per, N)
            g.bfv_multiply_monomial(L, size, n, dx, e, At(buf, N))
            assert np.array_equal(inner_of(buf, N, (size, e)).reshape(n, size, L, N), np_shift(x, e, o.moduli)), (size, e)
            buf.free()
        assert np.array_equal(dx.download(x.shape), x), (size, "input")
        dx.free()


@pytest.mark.parametrize("cid", IDS)
def test_expand(be, oracle, cid):
    g, o, N, sk, pk = chain_pair(be, oracle, cid)
    rng = np.random.default_rng(310)
    L, n, count = g.L, 3, 8
    gks = expand_keys(g, o, sk, count, 190)
    assert list(gks) == [N // (1 << j) + 1 for j in range(len(gks))]
    q = np.stack([o.encrypt(pk, rng.integers(0, o.t, N, dtype=np.uint64), 191)] + [o.random_poly(rng, L, 2) for _ in range(n - 1)])
    assert q.shape == (n, 2, L, N)
    dq = g.to_device(q)
    buf = sentinelled(g, count * n * 2 * L * N, N)
    g.path_stats(reset=True)
    g.bfv_expand(L, n, dq, count, At(buf, N))
    got = inner_of(buf, N, "expand").reshape(count, n, 2, L, N)  # child k of query r at k n + r
    print(f"paths {cid} expand count = {count}, n = {n}: " + ", ".join(f"{k} = {c}" for k, c in g.path_stats().items() if c))
    for r in range(n):
        kids = children(expand_levels(o, q[r], 3, gks, L), count)
        for k in range(count):
            assert np.array_equal(got[k, r], kids[k]), ("child", k, "query", r)
    assert np.array_equal(dq.download(q.shape), q), "queries"
    dq.free()
    buf.free()
