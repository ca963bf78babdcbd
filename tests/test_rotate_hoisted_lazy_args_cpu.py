"""The refusals of he355_rotate_hoisted_plain_sum_lazy and he355_plain_extend_special that need no device (csrc/hoist_args.h), through the C
ABI on contexts without one: every bad argument is HE355_E_INVALID_ARGS with a message that names the call, decided on the host before a
device is asked for -- valid arguments then fail with HE355_E_DEVICE (no CPU fallback) -- and neither touches a buffer:

* L of 0 and L_top + 1; a chain without a special prime (K < 2); a step of +-N / 2; null steps and null plaintexts;
* n 2 L N past 2^60 words, a slab that wraps the address space;
* d_out overlapping d_in and d_plain_qp -- one word inside the special-prime row of the last plaintext, which the eager call's [L][N] span
  would not reach; right behind is accepted;
* he355_plain_extend_special: the levels, K < 2, null pointers with n > 0, spans past 2^60 words, d_plain_qp overlapping d_plain_ntt from
  either side; right behind is accepted;
* n == 0 and n_steps == 0 return success without a device and touch nothing; a bad level is refused all the same.
And the checks themselves under the sanitizers: tests/rotate_hoisted_lazy_args_main.cpp, a stand-alone program compiled with
g++ -fsanitize=address,undefined and run as a child process: exit status 0.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import sanitized_program

N, BITS = 4096, [60, 40, 40, 60]
FILL = 0xABCD


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def test_the_c_abi_has_the_lazy_calls(be):
    lib = be.lib()
    for name in ("he355_rotate_hoisted_plain_sum_lazy", "he355_plain_extend_special"):
        assert name in be.C_ABI_SYMBOLS and getattr(lib, name), name
    assert C.sizeof(be.HoistStats) == 8 * 8 and [k for k, _ in be.HoistStats._fields_][4] == "mod_downs"  # one reserved word taken, the size kept


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    bfv = be.Context(be.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=20, sec128=False)
    ckks = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    one = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60], sec128=False)
    Lt = ckks.L
    per, ptw = 2 * Lt * N, (Lt + 1) * N
    src = np.full(4 * per, FILL, dtype=np.uint64)
    dst = np.full(4 * per, FILL, dtype=np.uint64)
    plain = np.full(3 * Lt * N, FILL, dtype=np.uint64)
    plain_qp = np.full(3 * ptw, FILL, dtype=np.uint64)
    at = lambda arr, words=0: C.c_void_p(arr.ctypes.data + 8 * int(words))
    i32s = lambda v: (C.c_int32 * max(1, len(v)))(*v)

    def lazy(h=ckks.h, L=Lt, n=4, i=at(src), s=(1, 0, -2), p=at(plain_qp), o=at(dst), ns=None):
        return lib.he355_rotate_hoisted_plain_sum_lazy(h, L, n, i, i32s(s) if s is not None else None, len(s) if ns is None else ns, p, o)

    def ext(h=ckks.h, L=Lt, n=3, i=at(plain), o=at(plain_qp), m=None):
        return lib.he355_plain_extend_special(h, L, n, i, o, m)

    bad = {
        "L 0": lambda: lazy(L=0), "L past the top": lambda: lazy(L=Lt + 1), "K < 2": lambda: lazy(h=one.h, L=1),
        "step N / 2": lambda: lazy(s=(N // 2, 0, 1)), "step -N / 2": lambda: lazy(s=(-N // 2,)),
        "null plaintexts": lambda: lazy(p=None), "null steps": lambda: lazy(s=None, ns=3),
        "span": lambda: lazy(n=1 << 60), "wraps": lambda: lazy(n=2, i=C.c_void_p(2 ** 64 - 4096), o=C.c_void_p(0x1000)),
        "out at in": lambda: lazy(o=at(src)), "out one word inside in": lambda: lazy(o=at(src, 4 * per - 1)),
        "out over the plaintexts": lambda: lazy(n=1, o=at(plain_qp)),
        "out one word inside the special row of the last plaintext": lambda: lazy(n=1, o=at(plain_qp, 3 * ptw - 1)),
        "n == 0, L 0": lambda: lazy(L=0, n=0), "n_steps == 0, L past the top": lambda: lazy(L=Lt + 1, s=()),
        "extend, L 0": lambda: ext(L=0), "extend, L past the top": lambda: ext(L=Lt + 1), "extend, K < 2": lambda: ext(h=one.h, L=1),
        "extend, null source": lambda: ext(i=None), "extend, null destination": lambda: ext(o=None),
        "extend, span": lambda: ext(n=1 << 60, i=C.c_void_p(0x1000), o=C.c_void_p(1 << 62)),
        "extend, span of the output": lambda: ext(n=(1 << 60) // ptw + 1, i=C.c_void_p(0x1000), o=C.c_void_p(1 << 62)),
        "extend, wraps": lambda: ext(n=2, i=C.c_void_p(2 ** 64 - 4096), o=C.c_void_p(0x1000)),
        "extend, in place": lambda: ext(i=at(plain_qp)), "extend, destination one word inside the source": lambda: ext(o=at(plain, 3 * Lt * N - 1)),
        "extend, source one word inside the destination": lambda: ext(i=at(plain_qp, 3 * ptw - 1)),
        "extend, n == 0, L 0": lambda: ext(L=0, n=0),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        want = b"he355_plain_extend_special: " if name.startswith("extend") else b"he355_rotate_hoisted_plain_sum_lazy: "
        assert msg.startswith(want) and len(msg) > len(want), (name, msg)
    # accepted by the host: there is no device behind these contexts, and no CPU fallback
    good = {
        "sum": lambda: lazy(), "sum on NTT-form BFV": lambda: lazy(h=bfv.h), "lower level": lambda: lazy(L=1), "the identity alone": lambda: lazy(s=(0,)),
        "out right behind in": lambda: lazy(o=at(src, 4 * per)), "steps at the edge": lambda: lazy(s=(N // 2 - 1, -(N // 2 - 1))),
        "extend": lambda: ext(), "extend on BFV": lambda: ext(h=bfv.h), "extend, L = 1": lambda: ext(L=1),
        "extend with the check": lambda: ext(m=at(dst)),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    # right behind the plaintexts / the source: accepted too (slabs of their own, so that the pointer stays inside an allocation)
    big = np.full(3 * ptw + per, FILL, dtype=np.uint64)
    assert lazy(n=1, p=at(big), o=at(big, 3 * ptw)) == be.E_DEVICE
    assert ext(i=at(big), o=at(big, Lt * N), n=1) == be.E_DEVICE
    # nothing to do: success, whatever the pointers are, and no device is asked for
    assert lazy(n=0, i=None, p=None, o=None) == be.OK
    assert lazy(s=(), p=None, o=at(src)) == be.OK
    assert ext(n=0, i=None, o=None) == be.OK
    for c in (bfv, ckks, one):
        c.close()
    assert (src == FILL).all() and (dst == FILL).all() and (plain == FILL).all() and (plain_qp == FILL).all() and (big == FILL).all()


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "rotate_hoisted_lazy_args_main.cpp", "rotate_hoisted_lazy_args ok")
