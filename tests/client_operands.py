"""Structured and extreme operands for the client-side tests (a plain helper module in the style of tests/edge_operands.py:
tests/test_client_edges_cpu.py, tests/test_gpu_client_edges.py and tests/golden/make_client_edge_vectors.py import it).

Every other operand the encoders, the encryptor and the decryptor see in the suite is uniformly random and small: CKKS coefficients
below 2^31, BFV phases nowhere near a rounding tie, dropped residues of the special prime nowhere near floor(P/2).  The lists below put
those values there on purpose and give each operation a closed form in Python integers, so the expectation shares no code with the
product.  Every value handed to a kernel is a valid residue (< q_i, asserted).

The operands the committed fixture (tests/golden/client_edge_vectors.json) was computed for draw from random.Random(seed).getrandbits
only (the Mersenne Twister's raw words), so the tests rebuild them everywhere; each fixture case carries a digest of its operand, and the
tests compare it before they trust the recorded values.  Operands whose expectation is computed on the spot (ciphertext tails, uniform
rows) take a numpy generator from the caller."""
from __future__ import annotations

import hashlib
import json
import os
import random

import numpy as np

from edge_operands import edge_values

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "client_edge_vectors.json")

# the chains of the fixture and of the tests: name -> (N, bit sizes with the special prime last)
CKKS_ENCODE_CHAIN = [60, 45, 45, 60]
CKKS_ENCODE_N = (1024, 4096)
CKKS_SCALES = (2.0 ** 30, 2.0 ** 40, 2.0 ** 45)
DECODE_CHAINS = {"c45x15": (1024, [60] + [45] * 15 + [60], list(range(1, 17))), "c60x4": (2048, [60] * 5, [4])}
BFV_DECRYPT_CHAINS = {  # name -> (N, bits, plain bits)
    "b60_40_40": (1024, [60, 40, 40, 60], 20), "b45x15": (1024, [60] + [45] * 15 + [60], 20),
    "b50_40_t16": (1024, [50, 40, 50], 16), "b60x4_t31": (2048, [60] * 5, 31)}
ENCRYPT_CHAINS = {  # name -> (scheme, N, bits, plain bits)
    "bfv_60_40_40_60": ("bfv", 1024, [60, 40, 40, 60], 20), "bfv_60_40_40_46": ("bfv", 1024, [60, 40, 40, 46], 20),
    "ckks_60_45_45_60": ("ckks", 1024, [60, 45, 45, 60], 0),
    # the Shoup build of the u64 engine at LOGN1 = 4 (tests/shoup_rings.py, "n16384_60_50_40_60_shoup")
    "bfv_n16384_shoup": ("bfv", 16384, [60, 50, 40, 60], 20)}


def prod(xs) -> int:
    out = 1
    for x in xs:
        out *= int(x)
    return out


def _uniform_below(rng: random.Random, bound: int) -> int:
    """uniform in [0, bound) from raw generator words (rejection)"""
    bits = bound.bit_length()
    while True:
        v = rng.getrandbits(bits)
        if v < bound:
            return v


def _uniform_centred(rng: random.Random, lo: int, hi: int) -> int:
    """uniform in [lo, hi]"""
    return lo + _uniform_below(rng, hi - lo + 1)


def digest(values) -> str:
    """a short digest of a list of integers or of a float64 array (its exact bits)"""
    if isinstance(values, np.ndarray):
        data = np.ascontiguousarray(values, dtype=np.float64).tobytes()
    else:
        data = ",".join(str(int(v)) for v in values).encode()
    return hashlib.sha256(data).hexdigest()[:16]


def to_residues(values, moduli) -> np.ndarray:
    """[len(moduli)][len(values)] residues of (signed) Python integers, asserted valid"""
    out = np.empty((len(moduli), len(values)), dtype=np.uint64)
    for i, q in enumerate(moduli):
        q = int(q)
        r = [int(v) % q for v in values]
        assert all(0 <= x < q for x in r)
        out[i] = np.array(r, dtype=np.uint64)
    return out


# ---- coefficient families for decode and decrypt -----------------------------------------------------------------------------------
def centred_edges(Q: int) -> list[int]:
    """the centred integers at which the multiword decoder changes word, sign or branch, all inside (-Q/2, Q/2]"""
    h = Q // 2  # Q is odd: the centred range is [-h, h]
    vals = [0, 1, -1, h, h - 1, -h, 2 ** 64, -(2 ** 64), 2 ** 64 - 1, -(2 ** 64 - 1), 2 ** 128, -(2 ** 128)]
    k = 1
    while 64 * k < Q.bit_length():  # every word boundary below log2 Q
        vals += [2 ** (64 * k) - 1, -(2 ** (64 * k) - 1), 2 ** (64 * k), -(2 ** (64 * k))]
        k += 1
    out = []
    for v in vals:
        if -h <= v <= h and v not in out:
            out.append(v)
    return out


DECODE_FAMILIES = ["edges", "u90", "uQ", "halfQ"]
# the scale each family is decoded at in the fixture ("Q": float(Q)); every scale of the list is used, the edge list at two
DECODE_SCALES = {"edges": ["2^30", "Q"], "u90": ["2^90"], "uQ": ["Q"], "halfQ": ["Q"]}


def decode_scale(name: str, Q: int) -> float:
    return {"2^30": 2.0 ** 30, "2^90": 2.0 ** 90, "Q": float(Q)}[name]


def decode_coefficients(family: str, Q: int, N: int, seed: int = 20261017) -> list[int]:
    """N centred integer coefficients in [-(Q//2), Q//2] of one family.  edges: the list of centred_edges once in order, then seeded draws
    from it to fill N; u90: uniform in (-2^90, 2^90), cut to the centred range where Q is smaller; uQ: uniform over the whole centred range;
    halfQ: every coefficient Q//2.
    (Why the edge list is not simply tiled: a tiled list is a periodic signal, its transform has a peak of N / period times the coefficient
    size, and the error any double-precision transform leaves at the butterfly partner of that peak is set by the peak's last bit, not by
    the slot's own size.  What numpy happens to leave there is then no yardstick for another butterfly order: tiled, at L = 1 and scale Q,
    the peak is 141, the radix-2 codec leaves 4.4e-14 = 1.6 ulp(141) on its partner slot and numpy 1.8e-15, 4.75 times numpy's largest error
    anywhere -- profiles/client_edges.txt.)"""
    h = Q // 2
    rng = random.Random(f"{family}/{Q}/{N}/{seed}")
    if family == "edges":
        e = centred_edges(Q)
        out = [e[n] if n < len(e) else e[rng.getrandbits(16) % len(e)] for n in range(N)]
    elif family == "u90":
        b = min(2 ** 90 - 1, h)
        out = [_uniform_centred(rng, -b, b) for _ in range(N)]
    elif family == "uQ":
        out = [_uniform_centred(rng, -h, h) for _ in range(N)]  # (Q odd: (-Q/2, Q/2] and [-h, h] hold the same integers)
    elif family == "halfQ":
        out = [h] * N
    else:
        raise KeyError(family)
    assert all(-h <= v <= h for v in out)
    return out


# ---- planted BFV phases ------------------------------------------------------------------------------------------------------------
def bfv_round_closed_form(x: int, Q: int, t: int) -> int:
    """round(t x / Q) mod t for x in [0, Q)"""
    return ((t * x + Q // 2) // Q) % t


def planted_phases(Q: int, t: int, N: int, seed: int = 7) -> list[int]:
    """N phases in [0, Q): around every tie point b = ceil((2k+1) Q / 2t) of the rounding for the k at the ends and the middle of [0, t) and
    40 seeded k, plus the ends and the middle of [0, Q), plus the one x with t x + floor(Q/2) an exact multiple of Q (where the quotient's
    correction loop compares equal) and its neighbours; repeated to fill N"""
    rng = random.Random(f"phases/{Q}/{t}/{seed}")
    ks = [0, 1, 2, t // 2 - 1, t // 2, t - 2, t - 1] + [_uniform_below(rng, t) for _ in range(40)]
    vals = []
    for k in ks:
        b = -((-(2 * k + 1) * Q) // (2 * t))
        vals += [b - 2, b - 1, b, b + 1]
    vals += [0, 1, Q - 1, Q - 2, Q // 2, Q // 2 - 1, Q // 2 + 1]
    on = (-(Q // 2) * pow(t, -1, Q)) % Q
    assert (t * on + Q // 2) % Q == 0
    vals += [on - 1, on, on + 1]
    vals = [v % Q for v in vals]
    return [vals[n % len(vals)] for n in range(N)]


def uniform_phases(Q: int, N: int, seed: int) -> list[int]:
    rng = random.Random(f"uphase/{Q}/{seed}")
    return [_uniform_below(rng, Q) for _ in range(N)]


def phase_batch(Q: int, t: int, N: int, n: int, seed: int = 7) -> list[list[int]]:
    """n phase vectors: planted at the even rows, uniform at the odd ones"""
    return [planted_phases(Q, t, N, seed + r) if r % 2 == 0 else uniform_phases(Q, N, seed + r) for r in range(n)]


def const_secret_key(moduli, N: int, kind: str) -> np.ndarray:
    """the NTT form of the constant polynomial 1 ("one") or -1 ("minus_one") under every key prime"""
    sk = np.empty((len(moduli), N), dtype=np.uint64)
    for i, q in enumerate(moduli):
        sk[i] = 1 if kind == "one" else int(q) - 1
    return sk


def bfv_ct_with_phase(phases, moduli_L, size: int, kind: str, rng, phase_of_tail=None) -> np.ndarray:
    """[size][L][N] coefficient-form BFV ciphertext whose phase is `phases` (integers in [0, Q)); rng: a numpy generator for c1, c2.
    kind "zero": (c0, 0[, 0]) -- phase c0 under any key; "one" / "minus_one": c1 (and c2) uniform, phase c0 + c1 + c2 / c0 - c1 + c2 under
    const_secret_key; "tail": c1 (and c2) uniform and c0 = phase - phase_of_tail(ct with c0 = 0), the caller's map to the [L][N] phase of
    the rest under its key."""
    L, N = len(moduli_L), len(phases)
    ct = np.zeros((size, L, N), dtype=np.uint64)
    want = to_residues(phases, moduli_L)
    if kind == "zero":
        ct[0] = want
        return ct
    for i, q in enumerate(moduli_L):
        ct[1:, i] = rng.integers(0, int(q), (size - 1, N), dtype=np.uint64)
    rest = phase_of_tail(ct) if kind == "tail" else None
    for i, q in enumerate(moduli_L):
        q = int(q)
        w = want[i].astype(object)
        if kind == "tail":
            c0 = (w - rest[i].astype(object)) % q
        else:
            c1 = ct[1, i].astype(object)
            c2 = ct[2, i].astype(object) if size == 3 else 0
            c0 = (w - c1 - c2) % q if kind == "one" else (w + c1 - c2) % q
        ct[0, i] = np.array([int(v) for v in c0], dtype=np.uint64)
        assert int(ct[:, i].max()) < q
    return ct


# ---- a constant public key and the closed form of encryption under it -------------------------------------------------------------
def const_public_key(moduli, N: int, seed: int = 3):
    """pk_k = the constant polynomial C_k (residue C_k mod q_i at every NTT point), C_0 = floor(P/2), C_1 = floor(P/2) + 1 modulo the special
    prime P with random multiples of P on top: u = +-1 with e = 0 then leaves the dropped residue on floor(P/2) or floor(P/2) + 1, u = 0 on
    0, P - 1 and their neighbours.  Returns (pk [2][K][N], (C_0, C_1))."""
    P, QP = int(moduli[-1]), prod(moduli)
    rng = random.Random(f"pk/{QP}/{seed}")
    Cs = []
    for k in range(2):
        C = P // 2 + k + P * _uniform_below(rng, QP // P - 1)
        assert 0 <= C < QP and C % P == P // 2 + k
        Cs.append(C)
    pk = np.empty((2, len(moduli), N), dtype=np.uint64)
    for k in range(2):
        for i, q in enumerate(moduli):
            pk[k, i] = Cs[k] % int(q)
    return pk, tuple(Cs)


def bfv_edge_plain(t: int, N: int, shift: int = 0) -> np.ndarray:
    vals = [0, 1, t - 1, t // 2, t // 2 + 1]
    return np.array([vals[(n + shift) % len(vals)] for n in range(N)], dtype=np.uint64)


def encrypt_closed_form(o, Cs, plain, u, e0, e1):
    """The ciphertext [2][L][N] of `plain` under const_public_key's (C_0, C_1) with the sampled small polynomials u, e_0, e_1 (int arrays):
    z_k = (C_k u + e_k) mod QP, v_k = (z_k + P // 2) // P; BFV (plain [N] mod t): floor((Q m + floor((t + 1) / 2)) / t) is added to v_0;
    CKKS (plain [L][N], NTT form, or None): v_k is transformed and the plaintext added to v_0.  o: an oracle context (moduli, transforms).
    Also returns how many of the 2N coefficients have the dropped residue z_k mod P on an edge of P."""
    mods = [int(q) for q in o.moduli]
    P, QP, L, N = mods[-1], prod(mods), o.L, o.N
    Q = QP // P
    ckks = plain is None or np.ndim(plain) == 2
    edges = set(edge_values(P))
    out = np.empty((2, L, N), dtype=np.uint64)
    on_edge = 0
    for k, e in enumerate((e0, e1)):
        z = [(Cs[k] * int(u[n]) + int(e[n])) % QP for n in range(N)]
        on_edge += sum(1 for x in z if x % P in edges)
        v = [(x + P // 2) // P for x in z]
        if k == 0 and not ckks:
            t = int(o.t)
            v = [x + (Q * int(m) + (t + 1) // 2) // t for x, m in zip(v, plain)]
        res = to_residues(v, mods[:L])
        for i in range(L):
            r = o.ntt(i, res[i]) if ckks else res[i]
            if ckks and k == 0 and plain is not None:
                r = ((r.astype(object) + plain[i].astype(object)) % mods[i]).astype(np.uint64)
            out[k, i] = r
    return out, on_edge


# ---- encoder inputs ----------------------------------------------------------------------------------------------------------------
def _unit_uniform(N2: int, tag: str) -> np.ndarray:
    """N2 doubles k / 2^52 - 1, k < 2^53: uniform in [-1, 1), exact"""
    rng = random.Random(f"enc/{tag}/{N2}")
    return np.array([rng.getrandbits(53) / 2.0 ** 52 - 1.0 for _ in range(N2)], dtype=np.float64)


CKKS_INPUTS = ["uniform", "uniform_c1", "uniform_c5", "ones", "uniform_x4096", "single_8192"]


def ckks_input(name: str, N: int) -> np.ndarray:
    """the `count` slot values (count = len) of one encoder input at ring size N"""
    half = N // 2
    if name == "uniform":
        return _unit_uniform(half, name)
    if name == "uniform_c1":
        return _unit_uniform(half, name)[:1].copy()
    if name == "uniform_c5":
        return _unit_uniform(half, name)[:5].copy()
    if name == "ones":
        return np.ones(half)
    if name == "uniform_x4096":
        return _unit_uniform(half, name) * 4096.0  # exact: a power of two
    if name == "single_8192":
        v = np.zeros(half)
        v[half // 3] = 8192.0
        return v
    raise KeyError(name)


def ckks_refused_inputs(N: int, scale: float):
    """(name, values): each must be refused -- a coefficient that reaches 2^63 (all slots equal: the constant coefficient is value * scale),
    +inf and NaN"""
    half = N // 2
    big = np.full(half, 2.0 ** 63 / scale)
    inf = _unit_uniform(half, "refuse")
    inf[3] = np.inf
    nan = _unit_uniform(half, "refuse")
    nan[half - 1] = np.nan
    return [("coeff_2^63", big), ("inf", inf), ("nan", nan)]


def negative_prime_multiples(o):
    """(rows [n][N/2], [(i, k)]): row r is the constant -k q_i in every slot, for the 45-bit data primes of the encode chain (k q_i < 2^53: an
    exact double).  At scale 1 the encoder's transform of a constant is exact, so coefficient 0 is -k q_i and every other one is 0."""
    picks = [(i, k) for i in range(1, o.L) for k in (1, 3)]
    assert picks and all(k * int(o.moduli[i]) < 2 ** 53 for i, k in picks)
    return np.stack([np.full(o.N // 2, -float(k * int(o.moduli[i]))) for i, k in picks]), picks


def check_negative_prime_multiple(o, plain_ntt, i: int, k: int):
    for j in range(o.L):
        c = o.intt(j, plain_ntt[j])
        assert int(c[0]) == (-k * int(o.moduli[i])) % int(o.moduli[j]) and not c[1:].any(), (i, k, j)
    assert int(o.intt(i, plain_ntt[i])[0]) == 0


def bfv_extreme_values(t: int) -> list[int]:
    vals = [0, 1, -1, t - 1, t, -t, t // 2, -(t // 2), t // 2 + 1, 2 ** 63 - 1, -(2 ** 63), -(2 ** 63) + 1, 5 * t, -5 * t, -5 * t - 1]
    assert all(-(2 ** 63) <= v < 2 ** 63 for v in vals)
    return vals


def bfv_encoder_input(t: int, count: int, shift: int = 0) -> np.ndarray:
    vals = bfv_extreme_values(t)
    return np.array([vals[(n + shift) % len(vals)] for n in range(count)], dtype=np.int64)


def centre_mod_t(values, t: int) -> np.ndarray:
    """what BatchEncoder::decode returns for these encoder inputs: the representative of v mod t in (-t/2, t/2], in Python integers"""
    out = []
    for v in values:
        r = int(v) % t
        out.append(r - t if r > t // 2 else r)
    return np.array(out, dtype=np.int64)


# ---- the high-precision fixture and the bounds against it -------------------------------------------------------------------------
ENCODE_FACTOR = 2.0  # codec error <= 2 E_np: the two double-precision transforms differ in butterfly order (radix 2 / mixed radix)
DECODE_FACTOR = 4.0  # codec error <= 4 E_np (profiles/client_edges.txt: measured ratios; a wrong word or sign is off by orders of magnitude)
TIE_WINDOW = 2.0 ** -10  # at scale 2^30 a coefficient whose exact fractional part is this close to 1/2 may round either way
TIE_SHARE_CAP = 0.01


def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def coeffs_from_plain(o, plain_ntt: np.ndarray) -> list[int]:
    """the centred integer coefficients of an encoder output, from its prime-0 residues (|c| < q_0 / 2 for every encoder input here)"""
    q0 = int(o.moduli[0])
    c = o.intt(0, plain_ntt[0])
    return [int(v) - q0 if int(v) > q0 // 2 else int(v) for v in c]


def check_encode_case(case: dict, coeffs: list[int], who: str) -> dict:
    """`coeffs`: the integer coefficients some encoder produced for the case's input.  Asserts the two bounds against the exact
    values the fixture records at its sampled positions; returns the measured figures."""
    pos, exact16 = case["positions"], [int(x) for x in case["exact_x65536"]]
    err = max(abs(coeffs[p] * 65536 - x) for p, x in zip(pos, exact16)) / 65536.0
    bound = ENCODE_FACTOR * float.fromhex(case["E_np"])
    assert err <= bound, (who, case["id"], err, bound)
    skipped = 0
    if case["tie_rule"]:  # scale 2^30 and every |coefficient| < 2^31: the correctly rounded integer, except next to a tie
        for p, x in zip(pos, exact16):
            frac = x % 65536  # exact fractional part, in units of 2^-16 (floor convention, so it is in [0, 1))
            if abs(frac - 32768) <= TIE_WINDOW * 65536:
                skipped += 1
                continue
            assert coeffs[p] == (x + 32768) // 65536, (who, case["id"], p, coeffs[p], x / 65536.0)
        assert skipped <= TIE_SHARE_CAP * len(pos), (who, case["id"], skipped)
        # and the whole vector: every coefficient outside the recorded near-tie positions is the correctly rounded integer
        near = set(case["near_ties"])
        assert len(near) <= TIE_SHARE_CAP * len(coeffs), (who, case["id"])
        assert digest([c for n, c in enumerate(coeffs) if n not in near]) == case["rounded_digest"], (who, case["id"])
    return {"err": err, "bound": bound, "skipped": skipped}


def check_decode_case(case: dict, slots: np.ndarray, who: str) -> dict:
    pos = case["positions"]
    exact = np.array([float.fromhex(x) for x in case["exact"]])
    got = np.asarray(slots, dtype=np.float64)[pos]
    assert np.all(np.isfinite(got)), (who, case["id"])
    err = float(np.max(np.abs(got - exact)))
    bound = DECODE_FACTOR * float.fromhex(case["E_np"])
    assert err <= bound, (who, case["id"], err, bound, float.fromhex(case["magnitude"]))
    return {"err": err, "bound": bound}


# ---- the product's host client (tests/csim) -----------------------------------------------------------------------------------------
def host_sim():
    """tests/csim's library with the client entry points typed"""
    import ctypes as C
    import csim_lib
    S = csim_lib.load()
    vp, u64p, dp, ip = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    S.sim_params_create.restype = vp
    S.sim_params_create.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.c_int, C.c_int]
    S.sim_params_destroy.argtypes = [vp]
    S.simc_create.restype = vp
    S.simc_create.argtypes = [vp, C.c_uint64]
    for name, args in {"simc_destroy": [vp], "simc_secret_key": [vp, u64p], "simc_ckks_encode": [vp, dp, C.c_size_t, C.c_double, u64p],
                       "simc_ckks_decode": [vp, u64p, C.c_size_t, C.c_double, dp], "simc_bfv_encode": [vp, ip, C.c_size_t, u64p],
                       "simc_bfv_decode": [vp, u64p, ip], "simc_decrypt": [vp, u64p, C.c_size_t, C.c_size_t, u64p],
                       "simc_decrypt_with_key": [vp, u64p, u64p, C.c_size_t, C.c_size_t, u64p]}.items():
        getattr(S, name).argtypes = args
        getattr(S, name).restype = None
    return S


class HostClient:
    """the product's host client of one parameter set, numpy in and out"""

    def __init__(self, S, scheme: str, N: int, bits, plain_bits: int = 0):
        import ctypes as C
        self.S, self.N, self.ckks = S, N, scheme == "ckks"
        self.p = S.sim_params_create(2 if self.ckks else 1, N, (C.c_int * len(bits))(*bits), len(bits), plain_bits, 0)
        assert self.p
        self.c = S.simc_create(self.p, 42)
        self.K, self.Ltop = len(bits), max(1, len(bits) - 1)

    def close(self):
        self.S.simc_destroy(self.c)
        self.S.sim_params_destroy(self.p)

    @staticmethod
    def _u(a):
        import ctypes as C
        assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(C.POINTER(C.c_uint64))

    def secret_key(self):
        sk = np.empty((self.K, self.N), dtype=np.uint64)
        self.S.simc_secret_key(self.c, self._u(sk))
        return sk

    def ckks_encode(self, values, scale):
        import ctypes as C
        v = np.ascontiguousarray(values, dtype=np.float64)
        out = np.empty((self.Ltop, self.N), dtype=np.uint64)
        self.S.simc_ckks_encode(self.c, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), scale, self._u(out))
        return out

    def ckks_decode(self, plain_ntt, scale):
        import ctypes as C
        out = np.empty(self.N // 2)
        self.S.simc_ckks_decode(self.c, self._u(np.ascontiguousarray(plain_ntt)), plain_ntt.shape[0], scale, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def bfv_encode(self, values):
        import ctypes as C
        v = np.ascontiguousarray(values, dtype=np.int64)
        out = np.empty(self.N, dtype=np.uint64)
        self.S.simc_bfv_encode(self.c, v.ctypes.data_as(C.POINTER(C.c_int64)), len(v), self._u(out))
        return out

    def bfv_decode(self, plain):
        import ctypes as C
        out = np.empty(self.N, dtype=np.int64)
        self.S.simc_bfv_decode(self.c, self._u(np.ascontiguousarray(plain)), out.ctypes.data_as(C.POINTER(C.c_int64)))
        return out

    def decrypt(self, ct, sk=None):
        """[size][L][N] -> the CKKS phase [L][N] or the BFV plaintext [N]; sk: a key [K][N] in place of the client's own"""
        size, L, _ = ct.shape
        out = np.empty((L, self.N) if self.ckks else self.N, dtype=np.uint64)
        ct = np.ascontiguousarray(ct)
        if sk is None:
            self.S.simc_decrypt(self.c, self._u(ct), size, L, self._u(out))
        else:
            self.S.simc_decrypt_with_key(self.c, self._u(np.ascontiguousarray(sk)), self._u(ct), size, L, self._u(out))
        return out


def decode_operands(o, chain: str, fixture: dict):
    """yields (L, family, plaintext [L][N] in NTT form, the fixture's cases of it with `positions` filled in) for every level and family
    of one decode chain; o: an oracle context of the chain (moduli and transforms).  The operand's digest is checked against the cases'."""
    N, _, levels = DECODE_CHAINS[chain]
    by_id = {c["id"]: c for c in fixture["decode"]}
    for L in levels:
        mods = [int(q) for q in o.moduli[:L]]
        Q = prod(mods)
        for fam in DECODE_FAMILIES:
            coeffs = decode_coefficients(fam, Q, N)
            res = to_residues(coeffs, mods)
            plain = np.stack([o.ntt(i, res[i]) for i in range(L)])
            cases = []
            for s in DECODE_SCALES[fam]:
                c = by_id[f"{chain}/L{L}/{fam}/{s}"]
                assert c["digest"] == digest(coeffs), c["id"]
                assert float.fromhex(c["scale"]) == decode_scale(s, Q), c["id"]
                cases.append(dict(c, positions=fixture["slot_positions"][str(N)]))
            yield L, fam, plain, cases
