"""The refusals of he355_ckks_mod_raise and he355_ckks_lift_centred that need no device (csrc/raise_args.h), through the C ABI on contexts
without one: every bad argument is HE355_E_INVALID_ARGS with a message that names the call, decided on the host before a device is asked for
-- valid arguments then fail with HE355_E_DEVICE (no CPU fallback) -- and no buffer is touched, nothing is allocated (he355_alloc_stats of the
process is unchanged):

* a BFV context; L_in and L_to of 0 and L_top + 1; sizes 0 and 4; null d_in, null d_out; n past 2^60 words, a slab that wraps; d_out
  overlapping d_in -- one word inside it, and inside the rows of d_in the call ignores; right behind d_in is accepted; a slab that starts
  on an odd word (the kernels move 16 bytes at a time);
* n == 0 succeeds without a device;
* he355_raise_stats_t is 64 bytes; the three symbols are exported, declared in include/he355.h and bound.
And the checks themselves under the sanitizers: tests/ckks_mod_raise_args_main.cpp, a stand-alone program compiled with
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
NAMES = ("he355_ckks_mod_raise", "he355_ckks_lift_centred", "he355_raise_stats")


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
    for m in ("ckks_mod_raise", "ckks_lift_centred", "raise_stats"):
        assert hasattr(be.Context, m), m
    assert C.sizeof(be.RaiseStats) == 64
    assert [k for k, _ in be.RaiseStats._fields_][:5] == ["calls", "chunks", "fused_launches", "streaming_launches", "split_launches"]
    assert "he355_raise_stats_t" in header and "/* 64 bytes */" in header


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    before = alloc_totals(be)
    bfv = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    ckks = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    Lt = ckks.L
    words = 2 * 2 * Lt * N  # n = 2, size = 2 at the top level
    src = np.full(words, FILL, dtype=np.uint64)
    dst = np.full(words, FILL, dtype=np.uint64)
    at = lambda arr, w=0: arr.ctypes.data + 8 * int(w)
    vp = lambda p: C.c_void_p(p) if p else None

    def up(h=ckks.h, L_in=1, L_to=Lt, size=2, n=2, i=at(src), o=at(dst)):
        return lib.he355_ckks_mod_raise(h, L_in, L_to, size, n, vp(i), vp(o))

    w1, w5 = 2 * 2 * N, 2 * 2 * Lt * N
    bad = {
        "BFV": lambda: up(h=bfv.h, L_to=2), "L_in 0": lambda: up(L_in=0), "L_in past the top": lambda: up(L_in=Lt + 1), "L_to 0": lambda: up(L_to=0),
        "L_to past the top": lambda: up(L_to=Lt + 1), "size 0": lambda: up(size=0), "size 4": lambda: up(size=4), "null d_in": lambda: up(i=None),
        "null d_out": lambda: up(o=None), "span": lambda: up(n=1 << 60), "wraps": lambda: up(i=2 ** 64 - 4096, o=0x1000), "out at in": lambda: up(o=at(src)),
        "out one word inside in": lambda: up(L_to=2, o=at(src, w1 - 1)), "out inside the ignored rows": lambda: up(L_in=Lt, L_to=1, o=at(src, w5 - 1)),
        "out at the first ignored row": lambda: up(L_in=Lt, L_to=1, o=at(src, N)), "n == 0, L_in 0": lambda: up(L_in=0, n=0), "n == 0, BFV": lambda: up(h=bfv.h, n=0),
        "d_in on an odd word": lambda: up(L_to=2, i=at(src, 1)), "d_out on an odd word": lambda: up(L_to=2, o=at(dst, 1)),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        assert msg.startswith(b"he355_ckks_mod_raise: ") and len(msg) > 22, (name, msg)
    good = {
        "1 -> top": lambda: up(), "top -> top": lambda: up(L_in=Lt), "top -> 1": lambda: up(L_in=Lt, L_to=1), "size 1": lambda: up(size=1), "size 3, n 1": lambda: up(size=3, n=1),
        "out right behind in": lambda: up(L_to=2, o=at(src, w1)),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    assert up(n=0, i=None, o=None) == be.OK

    def lift(h=ckks.h, L_to=Lt, n=2, i=at(src), o=at(dst)):
        return lib.he355_ckks_lift_centred(h, L_to, n, vp(i), vp(o))

    bad = {
        "BFV": lambda: lift(h=bfv.h, L_to=2), "L_to 0": lambda: lift(L_to=0), "L_to past the top": lambda: lift(L_to=Lt + 1), "null d_coeff": lambda: lift(i=None),
        "null d_out": lambda: lift(o=None), "span": lambda: lift(n=1 << 60), "wraps": lambda: lift(i=2 ** 64 - 4096, o=0x1000), "out at in": lambda: lift(o=at(src)),
        "out one word inside in": lambda: lift(o=at(src, 2 * N - 1)), "n == 0, L_to 0": lambda: lift(L_to=0, n=0),
        "d_coeff on an odd word": lambda: lift(L_to=2, i=at(src, 1)), "d_out on an odd word": lambda: lift(L_to=2, o=at(dst, 1)),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        assert msg.startswith(b"he355_ckks_lift_centred: ") and len(msg) > 25, (name, msg)
    for name, f in {"lift": lambda: lift(), "to 1": lambda: lift(L_to=1), "out right behind in": lambda: lift(o=at(src, 2 * N))}.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    assert lift(n=0, i=None, o=None) == be.OK
    st = be.RaiseStats()
    assert lib.he355_raise_stats(ckks.h, C.byref(st), 0) == be.E_DEVICE  # (counters live with the device)
    assert lib.he355_raise_stats(ckks.h, None, 0) == be.E_INVALID_ARGS
    for c in (bfv, ckks):
        c.close()
    assert (src == FILL).all() and (dst == FILL).all()
    assert alloc_totals(be) == before


def test_the_checks_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "ckks_mod_raise_args_main.cpp", "ckks_mod_raise_args ok")
