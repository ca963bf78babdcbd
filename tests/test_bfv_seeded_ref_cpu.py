"""The definition of seeded BFV queries and Galois keys (tests/bfv_seeded_ref.py) held to the library's own sampler and to the oracle, on the CPU:

* the restated sampler equals csrc/client/sampler.h (tests/csim/sim_bfv_seeded.cpp calls sample_uniform_at, sample_cbd_at, sample_word and the
  stream functions as they stand): a 60-bit 2^60 - c prime, a 50-, 40- and 35-bit one and a generic 60-bit one, at the first N coefficients and
  at every coefficient of a search of 2^20 whose first draw was rejected (the generic prime rejects 3 % of all draws; the 2^k - c primes
  reject one in 2^25 .. 2^46, so for them a seed is BUILT with the inverse of splitmix64); under a modulus just above 2^63, which rejects
  every second draw, coefficients of 1 .. 8 draws exist and an eighth draw above the limit is kept and reduced;
* a restored seeded ciphertext's phase c0 + c1 s is Delta_L(m) - e EXACTLY, e the error of the ciphertext's own stream, at L = L_top and
  L = 1; restore(1) is the forward transform of restore(0); the oracle's decrypt_phase / bfv_decode_phase gives back m;
* the selector c0 restored carries the plants of he355_bfv_selector_encrypt: minus the seeded zero it is np_pack's polynomial 0 of a zero slab;
* a reference key (b, a) fed to oracle.apply_galois decrypts to the permuted plaintext, and its b half is what the definition says;
* the stream ranges of seeded ciphertexts are disjoint from enc_stream (indices below 2^40) and keygen_stream (every key id, digit and chain
  length the library admits) over a grid of r up to 2^40 - 1.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import bfv_seeded_ref as ref
import bfv_selector_ref as selr
import csim_lib

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
U = C.c_uint64
PRIMES = {"60_fold": 0xfffffffffff2801, "50": 0x3ffffffffa801, "40": 0xffffff7801, "35": 0x7ffffc801, "60_generic": 0x9e3779b97f4a7cd}
N, BITS, PB = 1024, [50, 40, 50], 20
A_SEED, E_SEED = 0x5EEDED0A, 0x5EC4E7


def declare(L):
    for name, res, args in (("sim_seeded_sampler_uniform", None, [U, U, u64p, U, U, u64p]), ("sim_seeded_sampler_cbd", None, [U, U, u64p, U, i32p]),
                            ("sim_seeded_word", U, [U, U, U]), ("sim_seeded_a_stream", U, [U, U]), ("sim_seeded_e_stream", U, [U]),
                            ("sim_seeded_enc_stream", U, [U, C.c_int]), ("sim_seeded_keygen_stream", U, [U, U, U, U]), ("sim_seeded_max_index", U, [])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


@pytest.fixture(scope="module")
def sim():
    return declare(csim_lib.load())


@pytest.fixture(scope="module")
def ctx(oracle):
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=PB, sec128=False)
    return o, o.keygen_secret(21)


def lib_uniform(sim, seed, stream, ns, q):
    ns = np.ascontiguousarray(ns, dtype=np.uint64)
    out = np.empty(len(ns), dtype=np.uint64)
    sim.sim_seeded_sampler_uniform(seed, stream, ns.ctypes.data_as(u64p), len(ns), q, out.ctypes.data_as(u64p))
    return out


@pytest.mark.parametrize("name", sorted(PRIMES))
def test_restated_sampler_equals_sampler_h(sim, name):
    q = PRIMES[name]
    seed, stream = 0xA5EED + q % 97, ref.a_stream(12345, 1)
    ns = np.arange(2048, dtype=np.uint64)
    assert np.array_equal(ref.uniform(seed, stream, 2048, q), lib_uniform(sim, seed, stream, ns, q))
    for n in (0, 1, 2047):
        assert int(ref.words(seed, stream, [n])[0]) == sim.sim_seeded_word(seed, stream, n)
    got = np.empty(2048, dtype=np.int32)
    sim.sim_seeded_sampler_cbd(seed, stream, ns.ctypes.data_as(u64p), 2048, got.ctypes.data_as(i32p))
    want = ref.cbd(seed, stream, 2048)
    assert np.array_equal(got, want) and int(np.abs(want).max()) <= 21 and want.min() < 0 < want.max()
    built = ref.seed_with_second_draw(stream, 777, q, salt=q % 5)
    assert 777 in ref.second_draws(built, stream, 1024, q)
    assert np.array_equal(ref.uniform(built, stream, 1024, q), lib_uniform(sim, built, stream, ns[:1024], q))
    if name == "60_generic":  # rejection has probability (2^64 mod q) / 2^64 >= 2^-14 here: a search of 2^20 coefficients finds second draws
        assert (ref.M64 - ref.limit(q)) * 2 ** 14 >= 2 ** 64
        far = np.arange(1 << 20, dtype=np.uint64)
        v, draws = ref.uniform_draws(seed, stream, far, q)
        again = far[draws > 1]
        assert len(again) > 0
        assert np.array_equal(v[draws > 1] % np.uint64(q), lib_uniform(sim, seed, stream, again, q))


def test_rejection_loop_reaches_and_keeps_the_eighth_draw(sim):
    """a modulus just above 2^63 rejects about half of all draws: coefficients with 2, 3, .. 8 draws and with all eight rejected exist among 2^14"""
    q = (1 << 63) + 29
    seed, stream = 77, ref.a_stream(5, 0)
    ns = np.arange(1 << 14, dtype=np.uint64)
    v, draws = ref.uniform_draws(seed, stream, ns, q)
    assert set(draws.tolist()) == set(range(1, 9))
    assert (v[draws == 8] > np.uint64(ref.limit(q))).any(), "the fallback: an eighth draw above the limit is kept and reduced"
    assert np.array_equal(v % np.uint64(q), lib_uniform(sim, seed, stream, ns, q))


def phase(o, sk, ct):
    """c0 + c1 s per prime, coefficient form, Python integers through the oracle's transforms"""
    out = []
    for i in range(ct.shape[1]):
        q = o.moduli[i]
        c1s = o.intt(i, ((o.ntt(i, ct[1, i]).astype(object) * sk[i].astype(object)) % q).astype(np.uint64))
        out.append(((ct[0, i].astype(object) + c1s.astype(object)) % q).astype(np.uint64))
    return np.stack(out)


@pytest.mark.parametrize("L", [2, 1])
def test_phase_is_delta_minus_e_exactly(ctx, L):
    o, sk = ctx
    rng = np.random.default_rng(40 + L)
    m = rng.integers(0, o.t, (3, N), dtype=np.uint64)
    m[1] = 0
    first = (1 << 40) - 3  # the last three indices
    c0 = ref.encrypt(o, sk, L, m, A_SEED, E_SEED, first)
    cts = ref.restore(o, L, 0, c0, A_SEED, first)
    ntt = ref.restore(o, L, 1, c0, A_SEED, first)
    for r in range(3):
        e = ref.error(o, E_SEED, first + r).astype(object)
        d = ref.delta(o, L, m[r])
        ph = phase(o, sk, cts[r])
        for i in range(L):
            assert np.array_equal(ph[i], ((d[i].astype(object) - e) % o.moduli[i]).astype(np.uint64)), (r, i)
            assert np.array_equal(ntt[r, 0, i], o.ntt(i, cts[r, 0, i])) and np.array_equal(ntt[r, 1, i], o.ntt(i, cts[r, 1, i]))
        assert np.array_equal(o.bfv_decode_phase(o.decrypt_phase(cts[r], sk)), m[r]), r
    z0, z1 = ref.seeded_zero(o, sk, L, A_SEED, E_SEED, first + 1)
    assert np.array_equal(z0, c0[1]) and np.array_equal(z1, cts[1, 1]), "Delta(0) = 0: the zero plaintext's c0 is the seeded zero"


def test_selector_c0_carries_the_plants(ctx):
    o, sk = ctx
    L, v, count, first_slot = 2, 16, 64, 3
    E = len(selr.slots(o.moduli[:L], v, 1, 0))
    sel = np.array([[1, 0, o.t - 1], [0, 5, 1]], dtype=np.uint64)
    assert first_slot + 3 * E <= count
    c0 = ref.selector_c0(o, sk, L, v, sel, first_slot, count, A_SEED, E_SEED, 9)
    zeros = np.stack([np.stack(ref.seeded_zero(o, sk, L, A_SEED, E_SEED, 9 + r)) for r in range(2)])
    want = selr.np_pack(zeros, sel, o.moduli, o.t, v, first_slot, count)
    assert np.array_equal(c0, want[:, 0])
    assert np.array_equal(ref.restore(o, L, 0, c0, A_SEED, 9), want), "and polynomial 1 is the seeded half"


def test_reference_key_switches_under_the_oracle(ctx):
    o, sk = ctx
    elt = N // 2 + 1  # an expansion's element
    b, a = ref.galois_key(o, sk, elt, A_SEED, E_SEED)
    K, Lt = o.K, o.L
    assert b.shape == a.shape == (Lt, K, N)
    rng = np.random.default_rng(7)
    m = rng.integers(0, o.t, (1, N), dtype=np.uint64)
    ct = ref.restore(o, Lt, 0, ref.encrypt(o, sk, Lt, m, A_SEED, E_SEED, 0), A_SEED, 0)[0]
    got = o.apply_galois(ct, elt, ref.full_key(b, a))
    want = o.bfv_decode_phase(o.decrypt_phase(np.stack([np.stack([o.apply_galois_poly(i, elt, False, ct[k, i]) for i in range(Lt)]) for k in range(2)]),
                                               np.stack([o.apply_galois_poly(i, elt, True, sk[i]) for i in range(K)])))
    assert np.array_equal(o.bfv_decode_phase(o.decrypt_phase(got, sk)), want)
    # m(X^elt): coefficient e of m lands at e elt mod 2N, negated past N
    perm = np.zeros(N, dtype=np.uint64)
    for e in range(N):
        at = e * elt % (2 * N)
        perm[at % N] = m[0, e] if at < N else (o.t - int(m[0, e])) % o.t
    assert np.array_equal(want, perm)
    # digit j's b + a s under prime i is -NTT(e) + [i == j] (P mod q_j) s(X^elt)
    P = o.moduli[K - 1]
    for j in range(Lt):
        e = ref.cbd(E_SEED, ref.keygen_stream(2 + elt, j, K, K), N).astype(object)
        for i in range(K):
            q = o.moduli[i]
            lhs = (b[j, i].astype(object) + a[j, i].astype(object) * sk[i].astype(object)) % q
            rhs = -o.ntt(i, (e % q).astype(np.uint64)).astype(object)
            if i == j:
                rhs = rhs + (P % q) * o.apply_galois_poly(i, elt, True, sk[i]).astype(object)
            assert np.array_equal(lhs.astype(np.uint64), (rhs % q).astype(np.uint64)), (j, i)


def test_streams_are_disjoint(sim):
    top = sim.sim_seeded_max_index()
    assert top == ref.MAX_INDEX == 1 << 40
    grid = sorted({0, 1, 2, 62, 63, 64, 1000, (1 << 20) - 1, 1 << 20, (1 << 32) + 5, top // 3, top // 3 + 1, top - 2, top - 1})
    lo, hi = None, None
    for r in grid:
        ss = [sim.sim_seeded_a_stream(r, i) for i in range(63)] + [sim.sim_seeded_e_stream(r)]
        assert ss == [ref.a_stream(r, i) for i in range(63)] + [ref.e_stream(r)]
        assert ss == list(range(ss[0], ss[0] + 64)), "the 64 streams of one index are consecutive"
        lo, hi = min(ss[0], lo or ss[0]), max(ss[-1], hi or 0)
        for w in range(3):
            assert sim.sim_seeded_enc_stream(r, w) == ref.enc_stream(r, w) == 3 * r + w
    # consecutive indices do not share a stream, and the whole range lies in [2^48, 2^48 + 2^46)
    assert sim.sim_seeded_a_stream(1, 0) == sim.sim_seeded_e_stream(0) + 1
    assert lo == 1 << 48 and hi == (1 << 48) + (1 << 46) - 1
    # enc_stream of every index below 2^40 ends below 3 * 2^40
    assert sim.sim_seeded_enc_stream(top - 1, 2) == 3 * top - 1 < lo
    # keygen_stream: key ids up to 2 + (2 N - 1) at N = 32768, 64 digits, chains of up to 63 primes
    worst = sim.sim_seeded_keygen_stream(2 + 2 * 32768 - 1, 63, 63, 63)
    assert worst == ref.keygen_stream(2 + 2 * 32768 - 1, 63, 63, 63) < 1 << 41 < lo
    assert sim.sim_seeded_keygen_stream(0, 0, 2, 0) == 1 << 40
