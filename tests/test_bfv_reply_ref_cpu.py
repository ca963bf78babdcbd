"""The reference of BFV reply compression (tests/bfv_reply_ref.py: the definition of include/he355.h in Python integers) held to itself, at
N = 1024 under a 60-bit fold prime, a 50-bit prime and the 45-bit first prime of {45, 55, 50}, with a ternary key of full weight:

* an L = 1 ciphertext is built whose invariant noise t phase mod q (centred) lies ON the largest norm that leaves exactly 2 bits of noise
  budget, 2^(bitlen(q) - 3) - 1, with both signs (coefficients 0 and 1; the message there is what the congruence forces), and within t of
  it for random messages everywhere else; compressed with the safe widths and decrypted, every coefficient is the message;
* the budget and noise_bits the reference reports equal the ones computed here from the residue of the unreduced integer
  z = y0 2^(k1 - k0) + y1^ s by exact fractions, and that residue stays below the 3/8 the safe widths promise;
* layout: the reply is N (k0 + k1) / 8 bytes, c1 starts on a word boundary, pack and unpack are inverse, all-ones fields survive;
* the switch: q - 1 and everything that rounds to 2^k wraps to 0, q is odd so no numerator is a tie;
* widths: the limits the issue states (46 at N = 8192, 44 at N = 32768 for a 60-bit prime, none for the safe pair under a 35-bit prime),
  58 368 and 241 664 bytes for the safe widths, and k1 one above the accepted limit is refused by compress and decrypt;
* the numpy helpers the GPU tests use equal the integer functions.
No GPU, no library code."""
from fractions import Fraction

import numpy as np
import pytest

import bfv_reply_ref as ref

N = 1024
T = 1038337
PRIMES = {"fold60": 0xfffffffffff2801, "shoup50": 0x3ffffffffa801, "f64_45": 0x1fffffff9001}  # the last: prime 0 of (1024, {45, 55, 50}), fp64 engine
Q35 = 0x7ffffc801


def planted(q, t, rng):
    """(c0, c1, s, m): phase = c0 + c1 s has t phase = M q + x with |x| on (coefficients 0, 1) or within t of (the rest) the 2-bit bound"""
    bound = 2 ** (q.bit_length() - 3) - 1
    s = [int(v) for v in rng.choice([-1, 1], N)]  # full weight
    qinv = pow(q, -1, t)
    phase, m = [], []
    for e in range(N):
        sign = 1 if e % 2 == 0 else -1
        if e < 2:
            x = sign * bound
            M = (-x * qinv) % t
        else:
            M = int(rng.integers(0, t))
            x = sign * bound
            x -= sign * ((sign * (x + M * q)) % t)  # towards zero, by less than t, until t divides M q + x
        assert (M * q + x) % t == 0 and bound - t < abs(x) <= bound
        phase.append((M * q + x) // t % q)
        m.append(M)
    c1 = [int(v) for v in rng.integers(0, q, N, dtype=np.uint64)]
    prod = ref.negacyclic(c1, s)
    c0 = [(p - v) % q for p, v in zip(phase, prod)]
    # the invariant noise budget of what was built: exactly 2 bits
    norm = max(abs(ref.centred_mod(t * ((a + b) % q), q)) for a, b in zip(c0, prod))
    assert q.bit_length() - norm.bit_length() - 1 == 2
    return c0, c1, s, m


@pytest.mark.parametrize("name", sorted(PRIMES))
def test_safe_widths_decrypt_noise_on_the_bound(name):
    q, t = PRIMES[name], T
    rng = np.random.default_rng(len(name))
    c0, c1, s, m = planted(q, t, rng)
    k0, k1 = ref.safe_bits(N, t)
    assert (k0, k1) == (22, 32) and ref.accepted(N, q, k0, k1)
    data = ref.compress(c0, c1, q, k0, k1)
    assert len(data) == ref.reply_bytes(N, k0, k1) == N * 54 // 8
    plain, budget, noise_bits = ref.decrypt(data, N, k0, k1, q, t, s)
    assert plain == m
    # the residue once more, from the unreduced integer z and exact fractions
    y0, y1 = ref.unpack(data, N, k0, k1)
    prod = ref.negacyclic([ref.centre(y, k1) for y in y1], s)
    assert max(abs(p) for p in prod) < q // 2  # the integer product is its own centred representative
    worst = Fraction(0)
    for a, p in zip(y0, prod):
        v = Fraction(t * (a * 2 ** (k1 - k0) + p), 2 ** k1)
        worst = max(worst, abs(v - round(v)))
    assert worst < Fraction(3, 8)
    r = worst * 2 ** k1
    assert r.denominator == 1
    nb = int(r).bit_length()
    assert (budget, noise_bits) == (max(0, k1 - nb - 1), nb)
    print(f"{name}: residue {float(worst):.4f} of a unit, noise_bits {noise_bits}, budget {budget}")


def test_layout():
    rng = np.random.default_rng(5)
    for n_, k0, k1 in ((64, 2, 2), (64, 22, 28), (64, 31, 33), (128, 3, 46)):
        y0 = [int(v) for v in rng.integers(0, 2 ** k0, n_)]
        y1 = [int(v) for v in rng.integers(0, 2 ** k1, n_)]
        y0[-1], y1[0], y1[-1] = 2 ** k0 - 1, 2 ** k1 - 1, 2 ** k1 - 1
        data = ref.pack(y0, y1, k0, k1)
        assert len(data) == n_ * (k0 + k1) // 8 and len(data) % 8 == 0 and (n_ * k0) % 64 == 0
        assert ref.unpack(data, n_, k0, k1) == (y0, y1)
        v = int.from_bytes(data, "little")
        assert (v >> (n_ * k0)) & (2 ** k1 - 1) == y1[0] and v >> (n_ * (k0 + k1) - k1) == y1[-1]
        ones = ref.pack([2 ** k0 - 1] * n_, [2 ** k1 - 1] * n_, k0, k1)
        assert ones == b"\xff" * len(ones)


def test_switch_edges():
    for q in list(PRIMES.values()) + [Q35]:
        for k in (2, 22, 24):
            assert ref.cut(0, k, q) == 0 and ref.cut(q - 1, k, q) == 0  # q - 1 rounds to 2^k
            wrap = -(-(2 ** (k + 1) - 1) * q // 2 ** (k + 1))  # the smallest x that rounds to 2^k
            assert ref.cut(wrap, k, q) == 0 and ref.cut(wrap - 1, k, q) == 2 ** k - 1
            assert ref.cut(q // 2, k, q) == 2 ** (k - 1) == ref.cut(q // 2 + 1, k, q)  # 2^(k-1) -+ 2^(k-1) / q, and 2^k is far below q
            assert ref.cut(1, k, q) == 0
            for x in (1, 12345, q // 3, q // 2, q - 2):
                assert (2 * x * 2 ** k + q) % (2 * q) != 0  # no tie: q is odd
                assert abs(Fraction(x * 2 ** k, q) - ((x * 2 ** k + q // 2) // q)) < Fraction(1, 2)


def test_widths():
    q60 = PRIMES["fold60"]
    assert ref.max_width(8192, q60) == 46 and ref.max_width(32768, q60) == 44 and ref.max_width(1024, q60) == 49
    assert ref.max_width(N, PRIMES["f64_45"]) == 34 and ref.accepted(N, PRIMES["f64_45"], *ref.safe_bits(N, T))
    assert ref.safe_bits(8192, T) == (22, 35) and ref.reply_bytes(8192, 22, 35) == 58368
    assert ref.safe_bits(32768, T) == (22, 37) and ref.reply_bytes(32768, 22, 37) == 241664
    assert not ref.accepted(1024, Q35, *ref.safe_bits(1024, T))  # a 35-bit first prime cannot hold the safe pair
    assert not ref.accepted(N, q60, 1, 22) and not ref.accepted(N, q60, 23, 22) and ref.accepted(N, q60, 2, 2)
    for q in PRIMES.values():
        top = ref.max_width(N, q)
        assert N * 2 ** (top - 1) <= (q - 1) // 2 < N * 2 ** top
        zeros = [0] * N
        good = ref.compress(zeros, zeros, q, 2, top)
        assert ref.decrypt(good, N, 2, top, q, T, [1] + [0] * (N - 1))[0] == zeros
        with pytest.raises(ValueError):
            ref.compress(zeros, zeros, q, 2, top + 1)
        with pytest.raises(ValueError):
            ref.decrypt(bytes(ref.reply_bytes(N, 2, top + 1)), N, 2, top + 1, q, T, [1] * N)


def test_numpy_helpers_equal_the_integer_functions():
    rng = np.random.default_rng(6)
    n_, q, t = 64, PRIMES["shoup50"], T
    for k0, k1 in ((2, 2), (22, 28), (31, 33), (40, 40)):
        assert ref.accepted(n_, q, k0, k1)
        ct = rng.integers(0, q, (3, 2, 1, n_), dtype=np.uint64)
        ct[0, 0, 0, :4] = (0, 1, q // 2, q - 1)
        data = ref.np_compress(ct, q, k0, k1)
        for j in range(3):
            assert data[j].tobytes() == ref.compress(ct[j, 0, 0], ct[j, 1, 0], q, k0, k1)
        y0, y1 = ref.np_unpack(data, n_, k0, k1)
        s = [int(v) for v in rng.choice([-1, 0, 1], n_)]
        for j in range(3):
            a, b = ref.unpack(data[j].tobytes(), n_, k0, k1)
            assert [int(v) for v in y0[j]] == a and [int(v) for v in y1[j]] == b
            assert [int(v) for v in ref.np_lift(y1, k1, q)[j]] == [ref.centre(v, k1) % q for v in b]
        w = np.array([[v % q for v in ref.negacyclic([ref.centre(int(y), k1) for y in y1[j]], s)] for j in range(3)], dtype=np.uint64)
        plain, budget, bits = ref.np_finish(y0, w, k0, k1, q, t)
        for j in range(3):
            p, bu, nb = ref.decrypt(data[j].tobytes(), n_, k0, k1, q, t, s)
            assert [int(v) for v in plain[j]] == p and (int(budget[j]), int(bits[j])) == (bu, nb)
