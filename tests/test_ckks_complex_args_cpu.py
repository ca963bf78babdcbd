"""The refusals of the five complex-slot call families that need no device (csrc/cplx_args.h, csrc/poly_args.h), through the C ABI on
contexts without one: every bad argument is HE355_E_INVALID_ARGS with a message that names the call, decided on the host before a device is
asked for -- valid arguments then fail with HE355_E_DEVICE (no CPU fallback) -- and no buffer is touched, nothing is allocated:

* he355_ckks_encode_complex / he355_ckks_decode_complex / _slots: a BFV context, count past N / 2, levels 0 and L_top + 1, scales of 0 and
  nan, a range outside the slots, null pointers; n == 0 succeeds without a device;
* he355_ckks_complex_unit, he355_ckks_complex_scalar_residues: host only (their values: tests/test_ckks_complex_ref_cpu.py);
* he355_combine_scalars_complex: he355_combine_scalars' list, with a scalar and a constant of q_i in the SECOND half;
* he355_ckks_eval_poly_complex: he355_ckks_eval_poly's list, a null and a nan imaginary list; the plan needs no device;
* all eight symbols are exported, declared in include/he355.h and bound; he355_poly_stats_t is still 64 bytes.
And the checks themselves under the sanitizers: tests/ckks_complex_args_main.cpp, a stand-alone program compiled with
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
NAMES = ("he355_ckks_encode_complex", "he355_ckks_decode_complex", "he355_ckks_decode_complex_slots", "he355_ckks_complex_unit",
         "he355_ckks_complex_scalar_residues", "he355_combine_scalars_complex", "he355_ckks_eval_poly_complex_plan", "he355_ckks_eval_poly_complex")
CUBIC = [0.5 + 0.1j, 0.15012 - 0.25j, 0.0, -0.0015930078125 + 0.05j]


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
        assert hasattr(be.Context, name[len("he355_"):]), name
    assert C.sizeof(be.PolyStats) == 64 and "complex_combinations" in dict(be.PolyStats._fields_)


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
    f64s = lambda v: (C.c_double * max(1, len(v)))(*v)
    vp = lambda a: C.c_void_p(a) if a else None
    s40 = 2.0 ** 40

    def named(call, cases, good):
        for name, f in cases.items():
            assert f() == be.E_INVALID_ARGS, (call, name)
            msg = lib.he355_last_error()
            assert msg.startswith(call.encode() + b": ") and len(msg) > len(call) + 2, (call, name, msg)
        for name, f in good.items():
            assert f() == be.E_DEVICE, (call, name, lib.he355_last_error())
            assert b"no CPU fallback" in lib.he355_last_error(), (call, name)

    # the codec
    enc = lambda h=ckks.h, n=2, v=at(src), count=8, s=s40, o=at(dst): lib.he355_ckks_encode_complex(h, n, vp(v), count, s, vp(o))
    named("he355_ckks_encode_complex", {
        "BFV": lambda: enc(h=bfv.h), "count": lambda: enc(count=N // 2 + 1), "scale 0": lambda: enc(s=0.0), "scale nan": lambda: enc(s=float("nan")),
        "null values": lambda: enc(v=None), "null plain": lambda: enc(o=None), "span": lambda: enc(n=1 << 60), "wraps": lambda: enc(o=2 ** 64 - 4096),
    }, {"encode": enc, "every slot": lambda: enc(count=N // 2), "no slot": lambda: enc(v=None, count=0)})
    assert enc(n=0, v=None, o=None) == be.OK
    dec = lambda h=ckks.h, L=Lt, n=2, p=at(src), s=s40, o=at(dst): lib.he355_ckks_decode_complex(h, L, n, vp(p), s, vp(o))
    named("he355_ckks_decode_complex", {
        "BFV": lambda: dec(h=bfv.h, L=2), "L 0": lambda: dec(L=0), "L past the top": lambda: dec(L=Lt + 1), "scale -1": lambda: dec(s=-1.0),
        "null plain": lambda: dec(p=None), "null out": lambda: dec(o=None), "span": lambda: dec(n=1 << 60),
    }, {"decode": dec, "level 1": lambda: dec(L=1)})
    assert dec(n=0, p=None, o=None) == be.OK
    decs = lambda r=(0, 3, N // 2 - 2, 2), nr=None, rn=False, o=at(dst), L=Lt: lib.he355_ckks_decode_complex_slots(
        ckks.h, L, 2, vp(at(src)), s40, None if rn else u64s(r), len(r) // 2 if nr is None else nr, vp(o))
    named("he355_ckks_decode_complex_slots", {
        "a range past the slots": lambda: decs(r=(N // 2 - 1, 2)), "five ranges": lambda: decs(r=(0, 1) * 5), "no range": lambda: decs(nr=0), "null ranges": lambda: decs(rn=True),
        "null out": lambda: decs(o=None), "L 0": lambda: decs(L=0),
    }, {"two ranges": decs})
    assert decs(r=(5, 0), o=None) == be.OK  # nothing to write

    # units and residues: host only
    out = (C.c_uint64 * (2 * Lt))()
    u = ckks.ckks_complex_unit(Lt)
    assert all((x * x + 2) % m == 0 for x, m in zip(u, q))
    assert ckks.ckks_complex_scalar_residues(Lt, 3.0, 2.0 ** 0.5) == [[(3 + x) % m for x, m in zip(u, q)], [(3 - x) % m for x, m in zip(u, q)]]
    for lv, o in ((0, out), (Lt + 1, out), (Lt, None)):
        assert lib.he355_ckks_complex_unit(ckks.h, lv, o) == be.E_INVALID_ARGS
        assert lib.he355_last_error().startswith(b"he355_ckks_complex_unit: ")
    for re, im, lv, o in ((float("inf"), 0.0, Lt, out), (0.0, float("nan"), Lt, out), (2.0 ** 126, 0.0, Lt, out), (0.0, 2.0 ** 127, Lt, out), (1.0, 1.0, 0, out), (1.0, 1.0, Lt, None)):
        assert lib.he355_ckks_complex_scalar_residues(ckks.h, lv, re, im, o) == be.E_INVALID_ARGS, (re, im, lv)
        assert lib.he355_last_error().startswith(b"he355_ckks_complex_scalar_residues: ")

    # he355_combine_scalars_complex
    L = 3

    def comb(h=ckks.h, L=L, size=2, n=2, terms=((at(src), 3), (at(src), 5)), s=None, c=None, o=at(dst), nt=None, null_s=False):
        tt = (be.Term * max(1, len(terms)))(*[be.Term(p, lv, 0) for p, lv in terms]) if terms is not None else None
        count = (len(terms) if terms is not None else 0) if nt is None else nt
        sc = None if null_s else u64s(s if s is not None else [1] * (max(1, count if count < 100 else 1) * 2 * max(L, 1)))
        return lib.he355_combine_scalars_complex(h, L, size, n, tt, count, sc, u64s(c) if c is not None else None, vp(o))

    w3, w5 = 2 * 2 * 3 * N, 2 * 2 * 5 * N
    named("he355_combine_scalars_complex", {
        "L 0": lambda: comb(L=0), "L past the top": lambda: comb(L=Lt + 1), "size 1": lambda: comb(size=1), "size 4": lambda: comb(size=4),
        "a term below L": lambda: comb(terms=((at(src), 3), (at(src), 2))), "a term above the top": lambda: comb(terms=((at(src), Lt + 1),)),
        "null terms": lambda: comb(terms=None, nt=2), "null scalars": lambda: comb(null_s=True), "a null term": lambda: comb(terms=((at(src), 3), (None, 3))),
        "null d_out": lambda: comb(o=None), "too many terms": lambda: comb(nt=(1 << 20) + 1),
        "a scalar of q in the first half": lambda: comb(s=[1, q[1], 1] + [1] * 9), "a scalar of q in the second half": lambda: comb(s=[1] * 9 + [1, 1, q[2]]),
        "a constant of q in the second half": lambda: comb(c=[0, 0, 0, 0, q[1], 0]),
        "span": lambda: comb(n=1 << 60), "wraps": lambda: comb(terms=((2 ** 64 - 4096, 3),), o=0x1000),
        "out at a term": lambda: comb(o=at(src)), "out one word inside a term": lambda: comb(terms=((at(src), 3),), o=at(src, w3 - 1)),
        "out inside the ignored rows of a higher term": lambda: comb(terms=((at(src), 5),), o=at(src, w5 - 1)),
        "a constant alone": lambda: comb(terms=(), c=[1] * 6), "n == 0, L 0": lambda: comb(L=0, n=0),
    }, {
        "combine": comb, "with a constant of q - 1": lambda: comb(c=[v - 1 for v in q[:3]] * 2), "scalars of q - 1": lambda: comb(s=[v - 1 for v in q[:3]] * 4),
        "size 3": lambda: comb(size=3, n=1), "on NTT-form BFV": lambda: comb(h=bfv.h, L=2, terms=((at(src), 3),)),
        "out right behind a higher term": lambda: comb(terms=((at(src), 5),), o=at(src, w5)),
    })
    assert comb(n=0, terms=None, nt=0, o=None) == be.OK
    assert comb(terms=(), o=None) == be.OK

    # he355_ckks_eval_poly_complex
    def ev(h=ckks.h, L=Lt, n=4, i=at(src), c=CUBIC, lb=1, si=s40, so=s40, o=at(dst), nc=None, null_re=False, null_im=False, im=None):
        re_, im_ = f64s([complex(x).real for x in c]), f64s(im if im is not None else [complex(x).imag for x in c])
        return lib.he355_ckks_eval_poly_complex(h, L, n, vp(i), None if null_re else re_, None if null_im else im_, len(c) if nc is None else nc, lb, si, so, vp(o))

    named("he355_ckks_eval_poly_complex", {
        "BFV": lambda: ev(h=bfv.h, L=3), "L 0": lambda: ev(L=0), "L past the top": lambda: ev(L=Lt + 1), "a constant polynomial": lambda: ev(c=[1.0 + 1j, 0.0]),
        "no coefficients": lambda: ev(c=[]), "1025 coefficients": lambda: ev(c=[0.0, 1j] + [0.0] * 1023), "null real parts": lambda: ev(null_re=True),
        "null imaginary parts": lambda: ev(null_im=True), "log_baby 0": lambda: ev(lb=0), "log_baby 7": lambda: ev(lb=7),
        "nan imaginary part": lambda: ev(im=[0.0, float("nan"), 0.0, 1.0]), "inf imaginary part": lambda: ev(im=[0.0, float("inf"), 0.0, 1.0]),
        "in_scale 0": lambda: ev(si=0.0), "out_scale nan": lambda: ev(so=float("nan")), "depth == L": lambda: ev(L=2),
        "an imaginary scalar past 2^126": lambda: ev(im=[0.0, 2.0 ** 100, 0.0, 1.0]),
        "out at in": lambda: ev(o=at(src)), "out one word inside in": lambda: ev(o=at(src, 4 * per - 1)), "null d_in": lambda: ev(i=None), "null d_out": lambda: ev(o=None),
        "span": lambda: ev(n=1 << 60), "n == 0, L 0": lambda: ev(L=0, n=0),
    }, {"cubic": ev, "depth == L - 1": lambda: ev(L=3), "four babies": lambda: ev(lb=2), "a purely imaginary line": lambda: ev(c=[0.0, 1j]),
        "out right behind in": lambda: ev(o=at(src, 4 * per))})
    assert ev(n=0, i=None, o=None) == be.OK
    # the plan needs no device and is the real call's tree
    pl = ckks.ckks_eval_poly_complex_plan(Lt, CUBIC, 1, s40, s40, n=4)
    rl = ckks.ckks_eval_poly_plan(Lt, [1.0, 1.0, 0.0, 1.0], 1, s40, s40, n=4)
    for k in ("depth", "L_out", "degree", "products", "combinations", "rescales", "adds", "drops", "powers", "powers_computed", "chunks", "pool_bytes"):
        assert pl[k] == rl[k], k
    assert pl["out_scale"] == s40 and pl["min_scalar_bits"] >= 20
    assert lib.he355_ckks_eval_poly_complex_plan(ckks.h, Lt, f64s([0.0, 1.0]), f64s([0.0, 1.0]), 2, 1, s40, s40, 4, None) == be.E_INVALID_ARGS
    for c in (bfv, ckks):
        c.close()
    assert (src == FILL).all() and (dst == FILL).all()
    assert alloc_totals(be) == before


def test_refusal_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "ckks_complex_args_main.cpp", "ckks_complex_args ok")
