"""The refusals of he355_combine_scalars, he355_ckks_scalar_residues and he355_ckks_eval_poly that need no device (csrc/poly_args.h), through the
C ABI on contexts without one: every bad argument is HE355_E_INVALID_ARGS with a message that names the call, decided on the host before a
device is asked for -- valid arguments then fail with HE355_E_DEVICE (no CPU fallback) -- and no buffer is touched, nothing is allocated
(he355_alloc_stats of the process is unchanged):

* he355_combine_scalars: L of 0 and L_top + 1; a term level below L and above L_top; sizes 1 and 4; null term list, null scalars, a null
  term, null d_out; more than 2^20 terms; a scalar and a constant of q_i; n past 2^60 words, a slab that wraps; d_out overlapping a term
  (one word inside the ignored rows of a higher term; right behind is accepted); a constant alone; n == 0 and no term without a constant
  succeed without a device;
* he355_ckks_scalar_residues: host only -- int(round(v)) % q_i; non-finite v and |v| >= 2^126 refused;
* he355_ckks_eval_poly: a BFV context; L of 0 and L_top + 1; a constant polynomial, no and 1025 coefficients; log_baby 0 and 7; nan and
  infinite coefficients; scales of 0, -1, inf, nan; depth == L; a scalar past 2^126; d_out overlapping d_in; null pointers; n == 0
  succeeds; he355_ckks_eval_poly_plan needs no device and restates tests/ckks_eval_poly_ref.py's counters;
* all five symbols are exported, declared in include/he355.h and bound; he355_poly_plan_t is 256 bytes, he355_poly_stats_t 64.
And the checks themselves under the sanitizers: tests/ckks_eval_poly_args_main.cpp, a stand-alone program compiled with
g++ -fsanitize=address,undefined and run as a child process: exit status 0.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import sanitized_program

N, BITS = 4096, [60, 40, 40, 40, 40, 60]
FILL = 0xABCD
NAMES = ("he355_combine_scalars", "he355_ckks_scalar_residues", "he355_ckks_eval_poly_plan", "he355_ckks_eval_poly", "he355_poly_stats")
SIGMOID = [0.5, 0.15012, 0.0, -0.0015930078125]


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def alloc_totals(be):
    st = be.AllocStats()
    assert be.lib().he355_alloc_stats(None, C.byref(st)) == be.OK
    return [int(getattr(st, k)) for k, _ in be.AllocStats._fields_]


def test_the_c_abi_has_the_calls(be):
    lib = be.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "he355.h")).read()
    for name in NAMES:
        assert name in be.C_ABI_SYMBOLS and getattr(lib, name), name
        assert name + "(" in header, name
    for m in ("combine_scalars", "ckks_scalar_residues", "ckks_eval_poly_plan", "ckks_eval_poly", "poly_stats"):
        assert hasattr(be.Context, m), m
    assert C.sizeof(be.PolyPlan) == 256 and C.sizeof(be.PolyStats) == 64 and C.sizeof(be.Term) == 16


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    before = alloc_totals(be)
    bfv = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    ckks = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    Lt = ckks.L
    q = [int(lib.he355_modulus(ckks.h, i)) for i in range(Lt)]
    per = 2 * Lt * N
    src = np.full(4 * per, FILL, dtype=np.uint64)
    dst = np.full(4 * per, FILL, dtype=np.uint64)
    at = lambda arr, words=0: arr.ctypes.data + 8 * int(words)
    u64s = lambda v: (C.c_uint64 * max(1, len(v)))(*v)
    L = 3

    def comb(h=ckks.h, L=L, size=2, n=2, terms=((at(src), 3), (at(src), 5)), s=None, c=None, o=at(dst), nt=None, null_s=False):
        tt = (be.Term * max(1, len(terms)))(*[be.Term(p, lv, 0) for p, lv in terms]) if terms is not None else None
        count = (len(terms) if terms is not None else 0) if nt is None else nt
        sc = None if null_s else u64s(s if s is not None else [1] * (max(1, count if count < 100 else 1) * max(L, 1)))
        return lib.he355_combine_scalars(h, L, size, n, tt, count, sc, u64s(c) if c is not None else None, C.c_void_p(o) if o else None)

    w3, w5 = 2 * 2 * 3 * N, 2 * 2 * 5 * N
    bad = {
        "L 0": lambda: comb(L=0), "L past the top": lambda: comb(L=Lt + 1), "size 1": lambda: comb(size=1), "size 4": lambda: comb(size=4),
        "a term below L": lambda: comb(terms=((at(src), 3), (at(src), 2))), "a term above the top": lambda: comb(terms=((at(src), Lt + 1),)),
        "null terms": lambda: comb(terms=None, nt=2), "null scalars": lambda: comb(null_s=True), "a null term": lambda: comb(terms=((at(src), 3), (None, 3))),
        "null d_out": lambda: comb(o=None), "too many terms": lambda: comb(nt=(1 << 20) + 1),
        "a scalar of q": lambda: comb(s=[1, 1, 1, 1, q[1], 1]), "a constant of q": lambda: comb(c=[0, 0, q[2]]),
        "span": lambda: comb(n=1 << 60), "wraps": lambda: comb(terms=((2 ** 64 - 4096, 3),), o=0x1000),
        "out at a term": lambda: comb(o=at(src)), "out one word inside a term": lambda: comb(terms=((at(src), 3),), o=at(src, w3 - 1)),
        "out inside the ignored rows of a higher term": lambda: comb(terms=((at(src), 5),), o=at(src, w5 - 1)),
        "a constant alone": lambda: comb(terms=(), c=[1, 1, 1]), "n == 0, L 0": lambda: comb(L=0, n=0),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        assert msg.startswith(b"he355_combine_scalars: ") and len(msg) > 23, (name, msg)
    good = {
        "combine": lambda: comb(), "with a constant of q - 1": lambda: comb(c=[v - 1 for v in q[:3]]), "scalars of q - 1": lambda: comb(s=[v - 1 for v in q[:3]] * 2),
        "size 3": lambda: comb(size=3, n=1), "on NTT-form BFV": lambda: comb(h=bfv.h, L=2, terms=((at(src), 3),)),
        "out right behind a term": lambda: comb(terms=((at(src), 3),), o=at(src, w3)), "out right behind a higher term": lambda: comb(terms=((at(src), 5),), o=at(src, w5)),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    assert comb(n=0, terms=None, nt=0, o=None) == be.OK
    assert comb(terms=(), o=None) == be.OK

    # he355_ckks_scalar_residues: host only
    for v in (0.5, -0.5, 1.5, 2.5, -2.5, 2.0 ** 52 + 1, 2.0 ** 53 + 2, -(2.0 ** 90), 2.0 ** 125, float(q[0]), -3.0 * q[1], 123456789.5):
        assert ckks.ckks_scalar_residues(Lt, v) == [int(round(v)) % m for m in q], v
    out = (C.c_uint64 * Lt)()
    for v, lv in ((float("inf"), Lt), (float("nan"), Lt), (2.0 ** 126, Lt), (-(2.0 ** 126), Lt), (1.0, 0), (1.0, Lt + 1)):
        assert lib.he355_ckks_scalar_residues(ckks.h, lv, v, out) == be.E_INVALID_ARGS, (v, lv)
        assert lib.he355_last_error().startswith(b"he355_ckks_scalar_residues: ")
    assert lib.he355_ckks_scalar_residues(ckks.h, Lt, 1.0, None) == be.E_INVALID_ARGS

    # he355_ckks_eval_poly
    s40 = 2.0 ** 40
    f64s = lambda v: (C.c_double * max(1, len(v)))(*v)

    def ev(h=ckks.h, L=Lt, n=4, i=at(src), c=SIGMOID, lb=1, si=s40, so=s40, o=at(dst), nc=None, null_c=False):
        return lib.he355_ckks_eval_poly(h, L, n, C.c_void_p(i) if i else None, None if null_c else f64s(c), len(c) if nc is None else nc, lb, si, so, C.c_void_p(o) if o else None)

    bad = {
        "BFV": lambda: ev(h=bfv.h, L=3), "L 0": lambda: ev(L=0), "L past the top": lambda: ev(L=Lt + 1), "a constant polynomial": lambda: ev(c=[1.0, 0.0]),
        "no coefficients": lambda: ev(c=[]), "1025 coefficients": lambda: ev(c=[0.0, 1.0] + [0.0] * 1023), "null coefficients": lambda: ev(null_c=True),
        "log_baby 0": lambda: ev(lb=0), "log_baby 7": lambda: ev(lb=7), "nan coefficient": lambda: ev(c=[0.5, float("nan"), 1.0]), "inf coefficient": lambda: ev(c=[0.5, float("inf"), 1.0]),
        "in_scale 0": lambda: ev(si=0.0), "in_scale -1": lambda: ev(si=-1.0), "out_scale inf": lambda: ev(so=float("inf")), "out_scale nan": lambda: ev(so=float("nan")),
        "depth == L": lambda: ev(L=2), "a scalar past 2^126": lambda: ev(c=[0.5, 2.0 ** 100, 0.0, 1.0]),
        "out at in": lambda: ev(o=at(src)), "out one word inside in": lambda: ev(o=at(src, 4 * per - 1)), "null d_in": lambda: ev(i=None), "null d_out": lambda: ev(o=None),
        "span": lambda: ev(n=1 << 60), "n == 0, L 0": lambda: ev(L=0, n=0),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        assert msg.startswith(b"he355_ckks_eval_poly: ") and len(msg) > 22, (name, msg)
    for name, f in {"sigmoid": lambda: ev(), "depth == L - 1": lambda: ev(L=3), "four babies": lambda: ev(lb=2), "out right behind in": lambda: ev(o=at(src, 4 * per))}.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    assert ev(n=0, i=None, o=None) == be.OK
    # the plan needs no device
    pl = ckks.ckks_eval_poly_plan(Lt, SIGMOID, 1, s40, s40, n=4)
    assert (pl["depth"], pl["L_out"], pl["degree"], pl["products"], pl["combinations"], pl["rescales"], pl["adds"], pl["drops"], pl["powers"]) == (2, Lt - 2, 3, 2, 2, 2, 1, 0, 1)
    assert pl["powers_computed"] == [2] and pl["chunks"] == 1 and pl["out_scale"] == s40 and pl["min_scalar_bits"] >= 20
    assert pl["pool_bytes"] >= 4 * 2 * (Lt - 1) * N * 8
    assert ckks.ckks_eval_poly_plan(Lt, SIGMOID, 1, s40, s40, n=0)["pool_bytes"] == 0
    assert ckks.ckks_eval_poly_plan(Lt, SIGMOID, 1, s40, s40, n=3000)["chunks"] == 3
    assert lib.he355_ckks_eval_poly_plan(ckks.h, Lt, f64s(SIGMOID), 4, 1, s40, s40, 4, None) == be.E_INVALID_ARGS
    st = be.PolyStats()
    assert lib.he355_poly_stats(ckks.h, C.byref(st), 0) == be.E_DEVICE  # (counters live with the device)
    for c in (bfv, ckks):
        c.close()
    assert (src == FILL).all() and (dst == FILL).all()
    assert alloc_totals(be) == before


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "ckks_eval_poly_args_main.cpp", "ckks_eval_poly_args ok")
