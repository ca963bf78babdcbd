"""The floor steps that take k_k3's accumulator (csrc/modarith.h: floor_fin_acc, floor_fin2_acc, floor_fin_s_acc, floor_fin2_s_acc) against
Python integers and against the composition they replace (floor_fin*(acc_canon(acc), ...)), bit for bit, at the edges of the ranges the
forms state; the raw tail's acc_to_inv / acc_park; and the host-side rule that decides which launches may take the direct forms.

tests/floor_forms_host.cpp includes the header and is compiled here with the host compiler, once per form of the u64 engine
(HE355_U64_FOLD = 0 / 1), and loaded through ctypes.  Constants are floor_const's (csrc/device_tables.h), the ones DeviceContext uploads."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reference-seal-backend_amd", "csrc")
FORMS = ["floor_fin", "floor_fin2", "floor_fin_s", "floor_fin2_s"]
OLD, ACC_DIRECT, ACC_PREP = 0, 1, 2  # floor_forms_host.cpp: run()'s modes
N_UNIFORM = 100000
B_ACC = B_X = 1 << 49  # the bounds the direct forms state (modarith.h: kFloorAccMax, kFloorXMax)

with open(os.path.join(HERE, "golden", "primes.json")) as _f:
    _G = json.load(_f)


def _chain(N, bits):
    for c in _G["chains"]:
        if c["N"] == N and c["bit_sizes"] == bits:
            return [int(p, 16) for p in c["primes"]]
    raise KeyError((N, bits))


HEADLINE = _chain(32768, [60] + [45] * 15 + [60])
CHAIN_60_40 = _chain(8192, [60, 40, 40, 60])
ALL_F64 = sorted({int(p, 16) for e in _G["get_primes"] + _G["chains"] for p in e["primes"] if int(p, 16) < 1 << 47})
# (q, s1 = the special prime of its chain, s2 = the prime a rescale divides by)
F64_CASES = []
for _q in [ALL_F64[0], ALL_F64[-1]]:
    F64_CASES.append((_q, HEADLINE[-1], [p for p in ALL_F64 if p != _q][-1]))
for _q in HEADLINE[1:-1]:
    F64_CASES.append((_q, HEADLINE[-1], HEADLINE[-2] if _q != HEADLINE[-2] else HEADLINE[-3]))
for _q in CHAIN_60_40[1:-1]:
    F64_CASES.append((_q, CHAIN_60_40[-1], CHAIN_60_40[2] if _q != CHAIN_60_40[2] else CHAIN_60_40[1]))
U64_CASES = [(HEADLINE[0], HEADLINE[-1], HEADLINE[-2]), (HEADLINE[-1], HEADLINE[0], HEADLINE[1]), (CHAIN_60_40[0], CHAIN_60_40[-1], CHAIN_60_40[2])]

u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)


@pytest.fixture(scope="module", params=[0, 1], ids=["shoup_build", "fold_build"])
def lib(request, tmp_path_factory):
    fold = request.param
    so = str(tmp_path_factory.mktemp("floor_forms") / f"libfloor_forms_{fold}.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-DHE355_U64_FOLD={fold}", "-I", CSRC,
                    os.path.join(HERE, "floor_forms_host.cpp"), os.path.join(CSRC, "he_params.cpp"), "-o", so], check=True)
    S = C.CDLL(so)
    assert S.ff_fold_build() == fold
    for fn, t in ((S.ff_f64, f64p), (S.ff_u64, u64p)):
        fn.restype = None
        fn.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_size_t, t, t, u64p, u64p, u64p]
    S.ff_f64_to_inv.restype = None
    S.ff_f64_to_inv.argtypes = [C.c_uint64, C.c_size_t, f64p, u64p, u64p, C.POINTER(C.c_ubyte)]
    S.ff_direct_terms.restype = C.c_uint32
    S.ff_direct_terms.argtypes = [C.c_uint64]
    for fn in (S.ff_term_bound, S.ff_x_bound):
        fn.restype = C.c_double
        fn.argtypes = [C.c_uint64]
    S.ff_direct.argtypes = [C.c_uint32, C.c_uint32]
    S.ff_acc_max.restype = S.ff_x_max.restype = C.c_double
    return S


def acc_values(q, B, rng):
    """+-B, +-(B - 1), k q and k q +- 1 for the k that reach B (and small k), 0; then N_UNIFORM uniform values in [-B, B]"""
    kmax = B // q
    edge = {0, B, -B, B - 1, -(B - 1)}
    for k in {1, 2, kmax // 2, kmax - 1, kmax}:
        for s in (1, -1):
            for d in (0, 1, -1):
                v = s * k * q + d
                if abs(v) <= B:
                    edge.add(v)
    return sorted(edge), rng.integers(-B, B, N_UNIFORM, dtype=np.int64, endpoint=True)


def x_values(q, B):
    h = q // 2
    out = {0, 1, -1, B, -B}
    for d in (0, 1, -1):
        out |= {h + d, -(h + d)}
    return sorted(out)


def want_ints(form, q, inv1, inv2, acc, x, addend):
    if form == 0:
        return [((a - b) * inv1 + c) % q for a, b, c in zip(acc, x, addend)]
    if form == 1:
        return [((a * inv1 + c - b) * inv2) % q for a, b, c in zip(acc, x, addend)]
    if form == 2:
        return [(a - b * inv1) % q for a, b in zip(acc, x)]
    return [((a - b) * inv2) % q for a, b in zip(acc, x)]


def operands(q, rng):
    """every edge acc x every edge x x every addend, then the uniform acc values with x cycling through its edges and uniform values"""
    acc_e, acc_u = acc_values(q, B_ACC, rng)
    xs = x_values(q, B_X)
    adds = [0, 1, q - 1]
    grid = list(itertools.product(acc_e, xs, adds))
    acc = [g[0] for g in grid] + [int(v) for v in acc_u]
    x_u = rng.integers(-B_X, B_X, N_UNIFORM, dtype=np.int64, endpoint=True)
    x_u[::3] = np.array(xs, dtype=np.int64)[np.arange(len(x_u[::3])) % len(xs)]
    x = [g[1] for g in grid] + [int(v) for v in x_u]
    addend = [g[2] for g in grid] + [adds[i % 3] if i % 2 else int(v) for i, v in enumerate(rng.integers(0, q, N_UNIFORM, dtype=np.uint64))]
    return acc, x, addend


_WANT = {}  # (q, form) -> the operands and the integers' results, computed once and shared by both builds


def case_data(q, s1, s2, form):
    key = (q, form)
    if key not in _WANT:
        rng = np.random.default_rng(q % (1 << 32))
        acc, x, addend = operands(q, rng)
        inv1, inv2 = pow(s1 % q, -1, q), pow(s2 % q, -1, q)
        _WANT[key] = (np.array(acc, dtype=np.float64), np.array(x, dtype=np.float64), np.array(addend, dtype=np.uint64),
                      np.array(want_ints(form, q, inv1, inv2, acc, x, addend), dtype=np.uint64), inv1, inv2, len(acc) - N_UNIFORM)
    return _WANT[key]


def call(fn, q, s1, s2, form, mode, acc, x, addend, ptr):
    out = np.empty(len(acc), dtype=np.uint64)
    inv = np.zeros(2, dtype=np.uint64)
    fn(q, s1, s2, form, mode, len(acc), acc.ctypes.data_as(ptr), x.ctypes.data_as(ptr), addend.ctypes.data_as(u64p), out.ctypes.data_as(u64p),
       inv.ctypes.data_as(u64p))
    return out, [int(v) for v in inv]


@pytest.mark.parametrize("form", range(4), ids=FORMS)
@pytest.mark.parametrize("case", F64_CASES, ids=[hex(c[0]) for c in F64_CASES])
def test_f64_forms_at_their_bounds(lib, case, form):
    q, s1, s2 = case
    acc, x, addend, want, inv1, inv2, n_edge = case_data(q, s1, s2, form)
    assert n_edge > 300 and float(np.abs(acc).max()) == float(B_ACC) and float(np.abs(x).max()) == float(B_X)
    assert (acc.astype(np.int64) == acc).all() and (x.astype(np.int64) == x).all()  # exact integers in the doubles
    results = {}
    for mode in (OLD, ACC_DIRECT, ACC_PREP):
        got, inv = call(lib.ff_f64, q, s1, s2, form, mode, acc, x, addend, f64p)
        assert inv == [inv1, inv2]
        assert int(got.max()) < q
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (FORMS[form], hex(q), ["old", "direct", "floor_prep + direct"][mode], len(bad), int(bad[0]), float(acc[bad[0]]), float(x[bad[0]]),
                               int(addend[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
        results[mode] = got
    assert np.array_equal(results[OLD], results[ACC_DIRECT]) and np.array_equal(results[OLD], results[ACC_PREP])


@pytest.mark.parametrize("form", range(4), ids=FORMS)
@pytest.mark.parametrize("case", F64_CASES, ids=[hex(c[0]) for c in F64_CASES])
def test_f64_fallback_beyond_the_bounds(lib, case, form):
    """what a launch beyond the host-side bound runs -- floor_prep, then the same forms -- on sums and rows up to 2^51 (acc_canon's own
    range is 2^52), against the integers and the old composition"""
    q, s1, s2 = case
    B = 1 << 51
    rng = np.random.default_rng(q % (1 << 32) + 7 + form)
    acc_e, acc_u = acc_values(q, B, rng)
    xs = x_values(q, B)
    adds = [0, 1, q - 1]
    grid = list(itertools.product(acc_e, xs, adds))
    m = 20000
    acc = [g[0] for g in grid] + [int(v) for v in acc_u[:m]]
    x = [g[1] for g in grid] + [int(v) for v in rng.integers(-B, B, m, dtype=np.int64, endpoint=True)]
    addend = [g[2] for g in grid] + [int(v) for v in rng.integers(0, q, m, dtype=np.uint64)]
    inv1, inv2 = pow(s1 % q, -1, q), pow(s2 % q, -1, q)
    want = np.array(want_ints(form, q, inv1, inv2, acc, x, addend), dtype=np.uint64)
    a, b, c = np.array(acc, dtype=np.float64), np.array(x, dtype=np.float64), np.array(addend, dtype=np.uint64)
    got = call(lib.ff_f64, q, s1, s2, form, ACC_PREP, a, b, c, f64p)[0]
    assert np.array_equal(got, want)
    if form != 1:  # (floor_fin2's old form puts addend - x beside a centred product: its own range ends below 2^51)
        assert np.array_equal(call(lib.ff_f64, q, s1, s2, form, OLD, a, b, c, f64p)[0], want)


@pytest.mark.parametrize("case", F64_CASES, ids=[hex(c[0]) for c in F64_CASES])
def test_f64_raw_tail_forms(lib, case):
    """acc_to_inv and acc_park / acc_unpark: the sum's residue, |value| <= q/2 + 1, the parked word gives the same double back"""
    q = case[0]
    rng = np.random.default_rng(q % (1 << 32) + 1)
    B = 1 << 51  # any |acc| < 2^52
    acc_e, acc_u = acc_values(q, B, rng)
    acc = np.array(acc_e + [int(v) for v in acc_u], dtype=np.float64)
    n = len(acc)
    d, p, ok = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint8)
    lib.ff_f64_to_inv(q, n, acc.ctypes.data_as(f64p), d.ctypes.data_as(u64p), p.ctypes.data_as(u64p), ok.ctypes.data_as(C.POINTER(C.c_ubyte)))
    want = np.array([int(a) % q for a in acc], dtype=np.uint64)
    assert np.array_equal(d, want) and np.array_equal(p, want) and ok.all()


@pytest.mark.parametrize("form", range(4), ids=FORMS)
@pytest.mark.parametrize("case", U64_CASES, ids=[hex(c[0]) for c in U64_CASES])
def test_u64_forms_are_the_old_composition(lib, case, form):
    """the u64 engine implements the same signatures through acc_canon: sums below 4q (any 64-bit value in the fold build), x lazy below 4q"""
    q, s1, s2 = case
    fold = lib.ff_fold_build()
    if fold and ((1 << 60) - q >= 1 << 26 or q >> 59 != 1):
        pytest.fail("the chains' 60-bit primes are all 2^60 - c")
    rng = np.random.default_rng(q % (1 << 32) + form)
    top = (1 << 64) if fold else 4 * q
    edge = [0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1, 4 * q - 1] + ([top - 1, 1 << 63, (1 << 61) - 1, 1 << 61] if fold else [])
    xs = [0, 1, q - 1, q, q // 2, q // 2 + 1, 2 * q, 4 * q - 1]
    adds = [0, 1, q - 1]
    grid = list(itertools.product(edge, xs, adds))
    m = 20000
    acc = [g[0] for g in grid] + [int(v) for v in rng.integers(0, top - 1, m, dtype=np.uint64, endpoint=True)]
    x = [g[1] for g in grid] + [int(v) for v in rng.integers(0, 4 * q, m, dtype=np.uint64)]
    addend = [g[2] for g in grid] + [int(v) for v in rng.integers(0, q, m, dtype=np.uint64)]
    inv1, inv2 = pow(s1 % q, -1, q), pow(s2 % q, -1, q)
    want = np.array(want_ints(form, q, inv1, inv2, acc, x, addend), dtype=np.uint64)
    a, b, c = (np.array(v, dtype=np.uint64) for v in (acc, x, addend))
    res = [call(lib.ff_u64, q, s1, s2, form, mode, a, b, c, u64p)[0] for mode in (OLD, ACC_DIRECT, ACC_PREP)]
    for got in res:
        assert np.array_equal(got, want)


def test_host_rule_routes_beyond_the_bound_to_the_fallback(lib):
    """PrimeDev::acc_terms = floor_direct_terms(q): the largest number of terms whose bound stays inside the forms' range; one more
    term, or a prime whose correction rows alone can pass the x bound, takes floor_prep first"""
    assert lib.ff_acc_max() == float(B_ACC) and lib.ff_x_max() == float(B_X)
    for q in ALL_F64 + [(1 << 46) - 1, (1 << 46) + 1, (1 << 47) - 1, (1 << 45) + 1, (1 << 44) + 1]:
        T, per, xb = lib.ff_direct_terms(q), lib.ff_term_bound(q), lib.ff_x_bound(q)
        # the bounds themselves, restated: a butterfly stage takes m to m + q (1/2 + m 2^-51)
        m = float(1 << 47)
        for _ in range(10):
            m += q * (0.5 + m * 2.0 ** -51)
        assert per == pytest.approx(q * (0.5 + m * 2.0 ** -51), rel=1e-12) and per >= q / 2
        m = 4.0 * q
        for _ in range(15):
            m += q * (0.5 + m * 2.0 ** -51)
        assert xb == pytest.approx(m, rel=1e-12)
        if xb > B_X:
            assert T == 0, hex(q)
        else:
            assert T >= 1 and T * per <= B_ACC < (T + 1) * per, hex(q)
        assert lib.ff_direct(T, T) == 1 and lib.ff_direct(T, T + 1) == 0
        if T:
            assert lib.ff_direct(T, 1) == 1
    for q in (1 << 47, (1 << 47) + 1, HEADLINE[0], (1 << 61) - 1):
        assert lib.ff_direct_terms(q) == 0  # not an fp64-engine prime
    # the headline chain (L = 16: 16 digits and the two operand products) and {60,40,40,60} take the direct forms
    for q in HEADLINE[1:-1]:
        assert lib.ff_direct(lib.ff_direct_terms(q), 16 + 2) == 1, hex(q)
    for q in CHAIN_60_40[1:-1]:
        assert lib.ff_direct(lib.ff_direct_terms(q), 3 + 2) == 1 and lib.ff_direct(lib.ff_direct_terms(q), 64 + 2) == 1, hex(q)
    # 46- and 47-bit primes never do; a 45-bit prime stops at L = 22
    assert lib.ff_direct_terms((1 << 47) - 1) == 0 and lib.ff_direct_terms((1 << 46) - 1) == 0
    t45 = lib.ff_direct_terms(HEADLINE[1])
    assert lib.ff_direct(t45, 22 + 2) == 1 and lib.ff_direct(t45, 64 + 2) == 0
