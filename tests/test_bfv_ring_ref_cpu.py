"""The device-free references of bfv_ring_ref.py, held to Python integers before test_gpu_bfv_large_rings.py and test_gpu_bfv_chain_layouts.py
trust them (no GPU).  The first four run at N = 1024 on {50, 40, 50} and on the N = 1024 versions of the chain layouts: {45, 55, 50},
{60, 60, 60}, {42, 38, 44} and {40, 60, 50, 60} (the counts pinned on the first chain stay pinned there):

* external_product_ref and rgsw_from_bfv_ref (its k = 1 rows after oracle.intt) against the schoolbook negacyclic sum, at 8
  output coefficients (0, 1, 511, 512, 1022, 1023 and two random ones), both polynomials, every prime: N products per coefficient and term;
  the k = 0 rows are oracle.ntt of the slot ciphertext, and every row lies where bfv_selector_ref.row says;
* decompose_ntt_ref, unpack_bytes_ntt_ref and gadget_ntt_ref against oracle.ntt of digits cut and lifted in Python integers (bfv_gadget_ref.digit /
  lift, int.from_bytes), whole polynomials of the source words those coefficients belong to; np_lift against bfv_gadget_ref.lift at its edges;
* the six chains of test_gpu_bfv_large_rings.py build in the oracle, and their engines are what that module means: a 40-bit prime (fp64 engine)
  beside 60-bit primes of the form 2^60 - c ... (fold form) or 50-bit primes (Shoup form; n16384_shoup: a 60-bit beside a 50-bit one); the
  plain moduli are the ones its shapes assume;
* the six prime-size layouts of test_gpu_bfv_chain_layouts.py build in the oracle: bit lengths, t, the engine of every prime, the form by the rule of
  he_params.cpp, the two data primes of {60, 60, 60}, the gadget totals at v = 20 and v = 4, and the reply widths each first prime accepts."""
import numpy as np
import pytest

import bfv_gadget_ref as gad
import bfv_ring_ref as ring
import bfv_selector_ref as sel

N, BITS, PB = 1024, [50, 40, 50], 20
# the chain every count below was first pinned on, then the N = 1024 versions of the layouts of test_gpu_bfv_chain_layouts.py: an fp64 prime 0
# beside a u64 one, no fp64 prime, no u64 prime, and 60-bit primes in the Shoup form around a 40-bit one
CTX_CHAINS = {"n1024": BITS, "f64_first": [45, 55, 50], "u64_only": [60, 60, 60], "f64_only": [42, 38, 44], "shoup_60": [40, 60, 50, 60]}
LARGE = {
    "n8192_fold": (8192, [60, 40, 60], 20),
    "n16384_fold": (16384, [60, 40, 40, 60], 20),
    "n32768_fold": (32768, [60, 40, 40, 60], 20),
    "n8192_shoup": (8192, [50, 40, 50], 20),
    "n32768_shoup": (32768, [50, 40, 40, 50], 20),
    "n16384_shoup": (16384, [60, 50, 40, 60], 20),  # tests/shoup_rings.py: 60-bit primes in the Shoup form, two data primes on the u64 engine
}


@pytest.fixture(scope="module", params=list(CTX_CHAINS))
def ctx(oracle, request):
    bits = CTX_CHAINS[request.param]
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=PB, sec128=False)
    assert [q.bit_length() for q in o.moduli] == bits and o.L == len(bits) - 1
    return o


def pinned(o):
    """the original chain, whose counts stay as they were asserted before the other chains came"""
    return [q.bit_length() for q in o.moduli] == BITS


def coefficients(rng):
    return [0, 1, 511, 512, 1022, 1023] + [int(c) for c in rng.choice(np.arange(2, 1022), 2, replace=False)]


def edged(o, rng, n, L, size=2):
    c = np.stack([o.random_poly(rng, L, size) for _ in range(n)])
    c[0, 0, 0, :] = 0
    for i, q in enumerate(o.moduli[:L]):
        c[n - 1, size - 1, i, :] = q - 1
        c[1 % n, 0, i, 1::2] = 0
        c[1 % n, 0, i, 0::2] = q - 1
    return c


def uniform_rows(o, rng, T, L):
    """[T][2][L][N] uniform residues: "RGSW rows" in NTT form (the identity is arithmetic)"""
    return np.stack([o.random_poly(rng, L, 2) for _ in range(T)])


def schoolbook(a, b, j, q):
    """coefficient j of a b mod (X^N + 1, q): a, b lists of Python integers"""
    n = len(a)
    return (sum(a[i] * b[j - i] for i in range(j + 1)) - sum(a[i] * b[n + j - i] for i in range(j + 1, n))) % q


def schoolbook_sum(o, rows_ntt, cts, v, coeffs):
    """{(k, i, j): sum over terms of (row polynomial k under prime i, coefficient form by oracle.intt) times (digit polynomial: Python integers)}"""
    T = rows_ntt.shape[0]
    L = cts.shape[2]
    E, off = gad.table(o.moduli[:L], v)
    digits = []  # term order: ciphertext kappa, polynomial k', prime i', digit g
    for ct in cts:
        for kp in range(2):
            for ip in range(L):
                for g in range(E[ip]):
                    digits.append([gad.digit(int(c), g, v) for c in ct[kp, ip]])
    assert len(digits) == T
    out = {}
    for k in range(2):
        for i, q in enumerate(o.moduli[:L]):
            rows = [[int(c) for c in o.intt(i, rows_ntt[f, k, i])] for f in range(T)]
            for j in coeffs:
                out[(k, i, j)] = sum(schoolbook(rows[f], [d % q for d in digits[f]], j, q) for f in range(T)) % q
    return out


def test_external_product_ref_is_the_schoolbook_sum(ctx):
    o, rng = ctx, np.random.default_rng(201)
    L, v, inner = o.L, 20, 2
    rows = 2 * gad.table(o.moduli[:L], v)[1][-1]
    assert rows == 2 * sum(-(-q.bit_length() // v) for q in o.moduli[:L]) and rows >= 2 * L
    if pinned(o):
        assert (L, rows) == (2, 10)
    cts = edged(o, rng, inner, L)
    rg = uniform_rows(o, rng, inner * rows, L)
    got = ring.external_product_ref(o, cts, rg.reshape(inner, rows, 2, L, N), v)
    want = schoolbook_sum(o, rg, cts, v, coefficients(rng))
    assert len(want) == 2 * L * 8
    for (k, i, j), w in want.items():
        assert int(got[k, i, j]) == w, (k, i, j)


def test_rgsw_from_bfv_ref_is_the_schoolbook_sum_and_the_row_rule(ctx):
    o, rng = ctx, np.random.default_rng(202)
    L, v, kv, n_rg = o.L, 45, 20, 2
    E = gad.table(o.moduli[:L], v)[1][-1]
    rows = 2 * gad.table(o.moduli[:L], kv)[1][-1]
    assert E == sum(-(-q.bit_length() // v) for q in o.moduli[:L]) and rows == 2 * sum(-(-q.bit_length() // kv) for q in o.moduli[:L])
    if pinned(o):
        assert (E, rows) == (3, 10)
    slots = edged(o, rng, n_rg * E, L)
    key = uniform_rows(o, rng, rows, L)
    got = ring.rgsw_from_bfv_ref(o, slots, key, v, kv)
    assert got.shape == (n_rg, 2 * E, 2, L, N)
    flat = got.reshape(n_rg * 2 * E, 2, L, N)
    coeffs = coefficients(rng)
    for c in (0, E - 1, E, n_rg * E - 1):  # the first and last slot of each RGSW ciphertext
        own, prod = flat[sel.row(c, E, 0)], flat[sel.row(c, E, 1)]
        for k in range(2):
            for i in range(L):
                assert np.array_equal(own[k, i], o.ntt(i, slots[c, k, i])), (c, k, i)
        want = schoolbook_sum(o, key, slots[c][None], kv, coeffs)
        back = ring.intt_all(o, prod)
        for (k, i, j), w in want.items():
            assert int(back[k, i, j]) == w, (c, k, i, j)


def test_np_lift_is_the_centred_lift(ctx):
    t = ctx.t
    m = np.array([0, 1, (t + 1) // 2 - 1, (t + 1) // 2, t - 1], dtype=np.uint64)
    for q in ctx.moduli:
        assert [int(x) for x in ring.np_lift(m, t, q)] == [gad.lift(int(x), t) % q for x in m]


def test_the_cuts_are_ntt_of_python_integer_digits(ctx):
    o, rng = ctx, np.random.default_rng(203)
    L, t = o.L, o.t
    w = t.bit_length() - 1
    x = edged(o, rng, 3, L, 3)
    # decompose_ntt_ref: digits of width w, lifted
    E, off = gad.table(o.moduli[:L], w)
    for L_out in (L, 1):
        got = ring.decompose_ntt_ref(o, x, L_out)
        assert got.shape == (3, 3 * off[-1], L_out, N)
        for r, k, i in ((0, 0, 0), (1, 0, 1), (2, 2, L - 1), (2, 1, 0)):
            for g in range(E[i]):
                d = [gad.digit(int(c), g, w) for c in x[r, k, i]]
                for ip in range(L_out):
                    q = o.moduli[ip]
                    want = o.ntt(ip, np.array([gad.lift(c, t) % q for c in d], dtype=np.uint64))
                    assert np.array_equal(got[r, k * off[-1] + off[i] + g, ip], want), (L_out, r, k, i, g, ip)
    # gadget_ntt_ref: plain digits of width v under every prime, reduced where they are not below it (v = 45 against the 40-bit prime)
    for v in (20, 45):
        E, off = gad.table(o.moduli[:L], v)
        got = ring.gadget_ntt_ref(o, x, v)
        assert got.shape == (3, 3 * off[-1], L, N)
        for r, k, i in ((0, 0, 0), (1, 0, 1), (2, 2, L - 1)):
            for g in range(E[i]):
                d = [gad.digit(int(c), g, v) for c in x[r, k, i]]
                for ip, q in enumerate(o.moduli[:L]):
                    want = o.ntt(ip, np.array([c % q for c in d], dtype=np.uint64))
                    assert np.array_equal(got[r, k * off[-1] + off[i] + g, ip], want), (v, r, k, i, g, ip)
    # unpack_bytes_ntt_ref: fields of width w of the little-endian integer of the bytes
    B = N * w // 8
    data = rng.integers(0, 256, (3, B), dtype=np.uint8)
    data[0], data[2] = 0, 0xFF
    for L_out in (L, 1):
        got = ring.unpack_bytes_ntt_ref(o, data, L_out)
        for r in range(3):
            big = int.from_bytes(data[r].tobytes(), "little")
            f = [(big >> (e * w)) & ((1 << w) - 1) for e in range(N)]
            for ip in range(L_out):
                q = o.moduli[ip]
                assert np.array_equal(got[r, ip], o.ntt(ip, np.array([gad.lift(c, t) % q for c in f], dtype=np.uint64))), (L_out, r, ip)


@pytest.mark.parametrize("name", list(LARGE))
def test_the_large_chains_build_and_their_engines_are_what_is_meant(oracle, name):
    n, bits, pb = LARGE[name]
    o = oracle.Context(oracle.SCHEME_BFV, n, bit_sizes=bits, plain_bits=pb, sec128=False)
    assert o.N == n and o.L == len(bits) - 1 and [q.bit_length() for q in o.moduli] == bits
    assert o.t == {8192: 1032193, 16384: 786433, 32768: 786433}[n] and o.t.bit_length() == 20
    data = o.moduli[:o.L]
    assert any(q < 2 ** 47 for q in data), "a prime of the fp64 engine"
    assert any(q >= 2 ** 47 for q in data), "a prime of the u64 engine"
    wide = [q for q in o.moduli if q >= 2 ** 47]  # the form is the context's: the key prime counts
    if name.endswith("fold"):  # the fold form takes primes 2^60 - c with c < 2^26 only (he_params.h, u64_fold)
        assert all(0 < 2 ** 60 - q < 2 ** 26 for q in wide)
    elif name == "n16384_shoup":  # 60-bit primes of the fold's own shape, in the Shoup form because of the 50-bit prime
        import shoup_rings as shoup
        shoup.check("n16384_60_50_40_60_shoup", o.moduli, o.t)
        assert [q.bit_length() for q in wide] == [60, 50, 60] and all(0 < 2 ** 60 - q < 2 ** 26 for q in wide if q.bit_length() == 60)
    else:
        assert all(q.bit_length() == 50 for q in wide)
    # the counts the large-ring shapes are sized by (a 50-bit prime beside the 60-bit one: three digits of 20 bits more)
    assert gad.table(data, 20)[1][-1] == (8 if name == "n16384_shoup" else {2: 5, 3: 7}[o.L])


# the layouts of test_gpu_bfv_chain_layouts.py: (N, bit sizes), t, the u64 form by the rule of he_params.cpp (None: no u64 prime), the gadget
# totals E(L) at v = 20 and v = 4 its shapes are sized by, the largest accepted reply width, whether the safe reply widths are accepted
LAYOUTS = {
    "f64_first": ((2048, [40, 60, 60]), 1032193, "fold", 5, 25, 28, False),
    "u64_only": ((2048, [60, 60, 60]), 1032193, "fold", 6, 30, 48, True),
    "f64_only": ((2048, [42, 38, 45, 44]), 1032193, None, 8, 33, 30, False),
    "shoup_60": ((2048, [60, 50, 40, 60]), 1032193, "shoup", 8, 38, 48, True),
    "f64_first_1024": ((1024, [45, 55, 50]), 1038337, "shoup", 6, 26, 34, True),
    "n16384_shoup": ((16384, [60, 50, 40, 60]), 786433, "shoup", 8, 38, 45, True),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_chain_layouts_build_and_their_engines_are_what_is_meant(oracle, name):
    import bfv_reply_ref as rep
    (n, bits), t, form, e20, e4, top, safe = LAYOUTS[name]
    o = oracle.Context(oracle.SCHEME_BFV, n, bit_sizes=bits, plain_bits=20, sec128=False)
    assert o.N == n and o.L == len(bits) - 1 and [q.bit_length() for q in o.moduli] == bits
    assert o.t == t and t.bit_length() == 20
    assert len(set(o.moduli)) == len(bits) and all(q % (2 * n) == 1 for q in o.moduli)
    wide = [q for q in o.moduli if q >= 2 ** 47]  # the u64 engine's primes; the form is the context's, so the key prime counts
    assert [q >= 2 ** 47 for q in o.moduli] == [b >= 47 for b in bits]
    if form is None:
        assert not wide
    else:  # the fold form takes primes 2^60 - c with c < 2^26 only; one prime that is not selects the Shoup form for all
        assert (form == "fold") == all(0 < 2 ** 60 - q < 2 ** 26 for q in wide)
    if name == "u64_only":
        assert o.moduli[:2] == [2 ** 60 - 0x27fff, 2 ** 60 - 0x17fff]
    if name in ("shoup_60", "n16384_shoup"):  # 60-bit primes of the fold's own shape, in the Shoup form because of the 50-bit prime
        assert 0 < 2 ** 60 - o.moduli[0] < 2 ** 26 and o.moduli[1].bit_length() == 50
    data = o.moduli[:o.L]
    assert gad.table(data, 20)[1][-1] == e20 and gad.table(data, 4)[1][-1] == e4
    assert gad.table(data, 63)[0] == [1] * o.L  # v = 63: the digit is the residue
    q0 = o.moduli[0]
    assert rep.max_width(n, q0) == top and rep.accepted(n, q0, *rep.safe_bits(n, t)) == safe
    assert rep.safe_bits(n, t) == (22, 22 + n.bit_length() - 1)
