"""Structured and extreme operands for the evaluator tests (a plain helper module: tests/test_edge_operands_cpu.py,
tests/test_gpu_edge_operands.py, tests/code_path_core.py and tools/fuzz_parity.py import it).

Every other operand of the suite is uniformly random, and uniform data reaches the worst cases the lazy kernels are argued from with
probability close to zero: a key-product run whose every term is at its top, a lifted digit whose every coefficient is q_j - 1, a
floor whose dropped residue is exactly 0, P - 1 or floor(P/2) +- 1.  The families below put those values there on purpose.  Every
value returned is a valid residue (< q_i, asserted): nothing here can take a kernel outside its documented input range.

A context is anything with `N`, `moduli` (the key-level chain, special prime last) and `L` (data primes): the oracle's or the
device's.  The `*_coeff` families and `planted` pass coefficient-form values through `ntt(i, poly)`, which the oracle context has; give
`transform=` (an oracle context of the same chain) when the first argument is a device context."""
from __future__ import annotations

import numpy as np

PLAIN = ["zero", "one", "qm1", "half", "half1", "alt", "alt_half", "impulse0", "impulseN1"]
CT_FAMILIES = PLAIN + [f + "_coeff" for f in PLAIN] + ["planted"]
KEY_KINDS = ["uniform", "zero", "qm1", "identity"]


def edge_values(q: int) -> list[int]:
    """the list of tests/test_bfv_level_core_cpu.py: the values around which a floor by q (or a sum with floor(q/2)) changes branch"""
    return [0, 1, q - 1, q - 2, q // 2, q // 2 - 1, q // 2 + 1, q - q // 2, q - q // 2 - 1, q - q // 2 + 1]


def droppable(ctx, L: int) -> list[int]:
    """the primes a floor can divide by at level L: the special prime (mod-down of a key switch) and the data primes 1 .. L-1 (rescale)"""
    return [int(ctx.moduli[-1])] + [int(q) for q in ctx.moduli[1:L]]


def _pattern(name: str, q: int, N: int) -> np.ndarray:
    v = np.zeros(N, dtype=np.uint64)
    if name == "zero":
        pass
    elif name == "one":
        v[:] = 1
    elif name == "qm1":
        v[:] = q - 1
    elif name == "half":
        v[:] = q // 2
    elif name == "half1":
        v[:] = q // 2 + 1
    elif name == "alt":
        v[1::2] = q - 1
    elif name == "alt_half":
        v[0::2] = q // 2
        v[1::2] = q - q // 2
    elif name == "impulse0":
        v[0] = q - 1
    elif name == "impulseN1":
        v[N - 1] = q - 1
    else:
        raise KeyError(name)
    return v


def planted_values(ctx, L: int, i: int) -> list[int]:
    """what `planted` puts into the first slots of residue i: the edges of every droppable prime p, taken modulo q_i, and (p < q_i) the
    same edges on top of the largest multiple of p that keeps them below q_i -- so a floor by p sees residue edges at a large quotient too"""
    q = int(ctx.moduli[i])
    out = []
    for p in droppable(ctx, L) + [q]:
        for e in edge_values(p):
            out.append(e % q)
            if p < q:
                top = ((q - 1 - e) // p) * p + e
                out.append(top)
    return out


def family(ctx, name: str, L: int, size: int = 2, rng=None, transform=None, coeff_form: bool = False) -> np.ndarray:
    """[size, L, N] residues of one family under the primes q_0 .. q_{L-1}.  `planted` needs rng (uniform elsewhere).
    coeff_form: the context's data are coefficients (BFV), so `planted` and `*_coeff` are not transformed -- for such a context
    `x_coeff` is the same operand as `x`."""
    N = ctx.N
    tr = transform if transform is not None else ctx
    out = np.empty((size, L, N), dtype=np.uint64)
    for i in range(L):
        q = int(ctx.moduli[i])
        if name == "planted":
            assert rng is not None, "planted: uniform outside the planted slots, needs rng"
            vals = planted_values(ctx, L, i)
            assert len(vals) <= N
            for k in range(size):
                v = rng.integers(0, q, N, dtype=np.uint64)
                v[:len(vals)] = np.array(vals, dtype=np.uint64)
                out[k, i] = v if coeff_form else tr.ntt(i, v)
        else:
            base = name[:-6] if name.endswith("_coeff") else name
            v = _pattern(base, q, N)
            if name.endswith("_coeff") and not coeff_form:
                v = tr.ntt(i, v)
            out[:, i] = v
        assert int(out[:, i].max()) < q, (name, i)
    return out


def batch(ctx, names, L: int, size: int = 2, rng=None, transform=None, coeff_form: bool = False) -> np.ndarray:
    """[len(names), size, L, N]: one ciphertext per entry of names; None (or "uniform") is a uniform neighbour"""
    cts = []
    for nm in names:
        if nm is None or nm == "uniform":
            c = np.empty((size, L, ctx.N), dtype=np.uint64)
            for i in range(L):
                c[:, i] = rng.integers(0, int(ctx.moduli[i]), (size, ctx.N), dtype=np.uint64)
            cts.append(c)
        else:
            cts.append(family(ctx, nm, L, size, rng, transform, coeff_form))
    return np.stack(cts)


def mixed(n: int, names) -> list:
    """the batch layout of the device tests: extremes at the even positions, uniform neighbours between them"""
    names = list(names)
    return [names[(r // 2) % len(names)] if r % 2 == 0 else None for r in range(n)]


def key(ctx, kind: str, rng=None, j0: int = 0) -> np.ndarray:
    """a key-switch key [Ltop][2][K][N] (NTT form).  identity: the constant polynomial 1 (all ones in NTT form) on digit j0, both halves,
    zero on every other digit: the key switch then returns floor((d + floor(P/2)) / P) of the integers d = iNTT_{j0}(target[j0])."""
    Ltop, K, N = ctx.L, len(ctx.moduli), ctx.N
    out = np.zeros((Ltop, 2, K, N), dtype=np.uint64)
    if kind == "uniform":
        for t in range(K):
            out[:, :, t] = rng.integers(0, int(ctx.moduli[t]), (Ltop, 2, N), dtype=np.uint64)
    elif kind == "qm1":
        for t in range(K):
            out[:, :, t] = int(ctx.moduli[t]) - 1
    elif kind == "identity":
        assert 0 <= j0 < Ltop
        out[j0] = 1
    elif kind != "zero":
        raise KeyError(kind)
    for t in range(K):
        assert int(out[:, :, t].max()) < int(ctx.moduli[t])
    return out


def identity_key_switch(o, L: int, j0: int, target: np.ndarray, coeff_form: bool = False) -> np.ndarray:
    """Closed form of a key switch under key(ctx, "identity", j0), in Python integers: both output polynomials are
    (d + P // 2) // P mod q_i with d = iNTT_{j0}(target[j0]) in [0, q_{j0}).  target [L][N] in the context's data form; returns [L][N]
    in that form (o: an oracle context, for the transforms only)."""
    assert j0 < L
    P = int(o.moduli[-1])
    d = target[j0] if coeff_form else o.intt(j0, target[j0])
    v = [(int(x) + P // 2) // P for x in d]
    out = np.empty((L, o.N), dtype=np.uint64)
    for i in range(L):
        q = int(o.moduli[i])
        r = np.array([x % q for x in v], dtype=np.uint64)
        out[i] = r if coeff_form else o.ntt(i, r)
    return out


def planted_digit(o, L: int, j0: int, rng, coeff_form: bool = False) -> np.ndarray:
    """one polynomial [L][N] whose digit j0 -- iNTT_{j0} of residue j0 -- starts with every edge of the special prime P, alone (when it is
    below q_{j0}) and on top of the largest multiple of P below q_{j0}: under identity(j0) the mod-down's residue d mod P is each edge"""
    P, q = int(o.moduli[-1]), int(o.moduli[j0])
    vals = []
    for e in edge_values(P):
        if e < q:
            vals.append(e)
        if P < q:
            vals.append(((q - 1 - e) // P) * P + e)
    assert vals
    out = np.empty((L, o.N), dtype=np.uint64)
    for i in range(L):
        qi = int(o.moduli[i])
        v = rng.integers(0, qi, o.N, dtype=np.uint64)
        if i == j0:
            v[:len(vals)] = np.array(vals, dtype=np.uint64)
        out[i] = v if coeff_form else o.ntt(i, v)
        assert int(out[i].max()) < qi
    return out


class IdentityOps:
    """The two key-switching primitives of the oracle restated for an identity(j0) key through identity_key_switch -- relinearize and
    apply_galois; everything without a key switch (sums, the Galois permutation) is the oracle's.  Composite expectations (NAF rotations,
    accumulate, rotate_sum) are built from these two, so a test can run one expectation function against both."""

    def __init__(self, o, j0: int, coeff_form: bool = False):
        self.o, self.j0, self.cf = o, j0, coeff_form

    def relinearize(self, ct3, key=None):
        L = ct3.shape[1]
        ks = identity_key_switch(self.o, L, self.j0, ct3[2], self.cf)
        return self.o.add(np.ascontiguousarray(ct3[:2]), np.stack([ks, ks]))

    def apply_galois(self, ct, elt, key=None):
        L = ct.shape[1]
        r = np.stack([np.stack([self.o.apply_galois_poly(i, elt, not self.cf, ct[k, i]) for i in range(L)]) for k in range(2)])
        ks = identity_key_switch(self.o, L, self.j0, r[1], self.cf)
        return np.stack([self.o.add(r[0][None], ks[None])[0], ks])


# ---- a searched worst column for the fp64 engine's digit lift --------------------------------------------------------------------
def _csim():
    import ctypes as C
    import csim_lib
    S = csim_lib.load(fold=False)  # (the fp64 engine's code is the same in both builds)
    S.sim_params_create.restype = C.c_void_p
    S.sim_params_create.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.c_int, C.c_int]
    S.sim_params_create_primes.restype = C.c_void_p
    S.sim_params_create_primes.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint64]
    S.sim_params_destroy.argtypes = [C.c_void_p]
    S.sim_modulus.restype = C.c_uint64
    S.sim_modulus.argtypes = [C.c_void_p, C.c_size_t]
    S.sim_is_f64.argtypes = [C.c_void_p, C.c_size_t]
    S.sim_logn1.argtypes = [C.c_void_p]
    S.sim_col_fwd_maxmag.restype = C.c_double
    S.sim_col_fwd_maxmag.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    S.sim_col_fwd_maxmag_uniform.restype = C.c_double
    S.sim_col_fwd_maxmag_uniform.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_size_t, C.c_uint64]
    return S


def fits_48_bound(m0: float, q: float, logn1: int) -> float:
    """the worst-case magnitude after the forward column pass from inputs |x| < m0, as the host's lift classes
    (k2_lift_class, csrc/device_tables.h) compute it: per stage m -> m + q (1/2 + m 2^-51); the 48-bit rows need it below 2^47"""
    m = m0
    for _ in range(logn1):
        m += q * (0.5 + m * 2.0 ** -51)
    return m


def worst_column(N: int, bits, j: int, t: int, seed: int = 20261017, uniform_columns: int = 100000, primes=None, restarts: int = 30) -> dict:
    """Hill-climb over the N1 coefficients (< q_j) of one column of digit j for the largest |x| the direct-path forward column pass of
    fp64-engine target prime t leaves (tests/csim: sim_col_fwd_maxmag, the product's col_fwd_w on the CPU).  Returns the column, its
    magnitude, the largest magnitude over `uniform_columns` uniform columns and fits_48's bound for this (q_j, q_t, N1).  With exactly centred
    products (|t| <= q_t / 2 per stage) no column could pass q_j + LOGN1 q_t / 2; fits_48's bound lies above that by the slack it
    allows the quotient estimate of every stage, and the search ends close to the former, not to the bound.  primes: the chain's moduli
    themselves in place of `bits` (tests/explicit_moduli.py); restarts: of the hill climb."""
    import ctypes as C
    S = _csim()
    if primes is not None:
        h = S.sim_params_create_primes(2, N, (C.c_uint64 * len(primes))(*primes), len(primes), 0)
    else:
        h = S.sim_params_create(2, N, (C.c_int * len(bits))(*bits), len(bits), 0, 0)
    assert h
    try:
        assert S.sim_is_f64(h, t) and S.sim_is_f64(h, j)
        qj, qt, logn1 = int(S.sim_modulus(h, j)), int(S.sim_modulus(h, t)), int(S.sim_logn1(h))
        assert qj <= 2 * qt, "the direct path: the digit enters the column pass as it is"
        n1 = 1 << logn1
        u64p = C.POINTER(C.c_uint64)

        def mag(col):
            return S.sim_col_fwd_maxmag(h, t, col.ctypes.data_as(u64p))

        rng = np.random.default_rng(seed)
        best = np.full(n1, qj - 1, dtype=np.uint64)
        best_m = mag(best)
        for _ in range(restarts):  # each: coordinate ascent in random order until a whole sweep raises nothing
            c = rng.integers(0, qj, n1, dtype=np.uint64)
            m = mag(c)
            for _ in range(20):
                improved = False
                for a in rng.permutation(n1):
                    for v in [0, qj - 1] + [int(x) for x in rng.integers(0, qj, 60, dtype=np.uint64)]:
                        d = c.copy()
                        d[a] = v
                        md = mag(d)
                        if md > m:
                            c, m, improved = d, md, True
                if not improved:
                    break
            if m > best_m:
                best, best_m = c, m
        uni = S.sim_col_fwd_maxmag_uniform(h, t, qj, uniform_columns, seed)
        assert int(best.max()) < qj
        return dict(column=best, magnitude=best_m, uniform_max=uni, bound=fits_48_bound(float(qj), float(qt), logn1), qj=qj, qt=qt, logn1=logn1)
    finally:
        S.sim_params_destroy(h)


def column_digit(o, L: int, j: int, column: np.ndarray, coeff_form: bool = False) -> np.ndarray:
    """a polynomial [L][N] whose digit j -- iNTT_j of residue j -- is `column` replicated across the columns of the N1 x (N / N1) layout of
    the digit lift (coefficient a * (N / N1) + b = column[a]); the other residues are the same integers reduced"""
    n1 = len(column)
    d = np.repeat(np.asarray(column, dtype=np.uint64), o.N // n1)
    out = np.empty((L, o.N), dtype=np.uint64)
    for i in range(L):
        r = d % np.uint64(int(o.moduli[i]))
        out[i] = r if coeff_form else o.ntt(i, r)
    return out
