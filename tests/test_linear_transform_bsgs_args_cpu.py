"""The refusals of he355_linear_transform_bsgs that need no device (csrc/hoist_args.h), through the C ABI on contexts without one: every bad
argument is HE355_E_INVALID_ARGS with a message that names the call, decided on the host before a device is asked for -- valid arguments
then fail with HE355_E_DEVICE (no CPU fallback) -- and no buffer is touched:

* L of 0 and L_top + 1; a chain without a special prime (K < 2); a baby or giant step of +-N / 2; null step lists, null plaintexts, null
  d_in and d_out;
* more than 2^20 (giant, baby) pairs; a mask that sets no term;
* n 2 L N past 2^60 words, a slab that wraps the address space;
* d_out overlapping d_in and d_plain_qp -- one word inside the special-prime row of the last plaintext; right behind is accepted;
* n == 0, n_baby == 0 and n_giant == 0 return success without a device and touch nothing; a bad level is refused all the same;
* both symbols are exported, declared in include/he355.h and bound; he355_hoist_stats_t keeps its 64 bytes and its first five fields, one
  reserved word is inner_sums; he355_linear_transform_bsgs_scratch_bytes needs no device.
And the checks themselves under the sanitizers: tests/linear_transform_bsgs_args_main.cpp, a stand-alone program compiled with
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
NAMES = ("he355_linear_transform_bsgs", "he355_linear_transform_bsgs_scratch_bytes")


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def test_the_c_abi_has_the_call(be):
    lib = be.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "he355.h")).read()
    for name in NAMES:
        assert name in be.C_ABI_SYMBOLS and getattr(lib, name), name
        assert name + "(" in header, name
    assert hasattr(be.Context, "linear_transform_bsgs") and hasattr(be.Context, "linear_transform_bsgs_scratch_bytes")
    fields = [k for k, _ in be.HoistStats._fields_]
    assert C.sizeof(be.HoistStats) == 64
    assert fields[:6] == ["digit_lifts", "key_products", "keys_permuted", "key_bytes", "mod_downs", "inner_sums"] and fields[4] == "mod_downs"


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    bfv = be.Context(be.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=20, sec128=False)
    ckks = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    one = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60], sec128=False)
    Lt = ckks.L
    per, ptw = 2 * Lt * N, (Lt + 1) * N
    src = np.full(4 * per, FILL, dtype=np.uint64)
    dst = np.full(4 * per, FILL, dtype=np.uint64)
    plain_qp = np.full(6 * ptw, FILL, dtype=np.uint64)
    at = lambda arr, words=0: C.c_void_p(arr.ctypes.data + 8 * int(words))
    i32s = lambda v: (C.c_int32 * max(1, len(v)))(*v)
    u8s = lambda v: (C.c_uint8 * max(1, len(v)))(*v)

    def call(h=ckks.h, L=Lt, n=4, i=at(src), b=(0, 1, -2), g=(0, 3), p=at(plain_qp), m=None, o=at(dst), nb=None, ng=None):
        return lib.he355_linear_transform_bsgs(h, L, n, i, i32s(b) if b is not None else None, len(b) if nb is None else nb, i32s(g) if g is not None else None,
                                               len(g) if ng is None else ng, p, u8s(m) if m is not None else None, o)

    bad = {
        "L 0": lambda: call(L=0), "L past the top": lambda: call(L=Lt + 1), "K < 2": lambda: call(h=one.h, L=1),
        "baby step N / 2": lambda: call(b=(N // 2, 0, 1)), "baby step -N / 2": lambda: call(b=(0, 1, -N // 2)),
        "giant step N / 2": lambda: call(g=(0, N // 2)), "giant step -N / 2": lambda: call(g=(-N // 2, 0)),
        "null baby steps": lambda: call(b=None, nb=3), "null giant steps": lambda: call(g=None, ng=2), "null plaintexts": lambda: call(p=None),
        "null d_in": lambda: call(i=None), "null d_out": lambda: call(o=None),
        "too many pairs": lambda: call(nb=(1 << 10) + 1, ng=1 << 10), "too many pairs, wrapping": lambda: call(nb=1 << 32, ng=1 << 32),
        "a mask with no term": lambda: call(m=(0,) * 6),
        "span": lambda: call(n=1 << 60), "wraps": lambda: call(n=2, i=C.c_void_p(2 ** 64 - 4096), o=C.c_void_p(0x1000)),
        "out at in": lambda: call(o=at(src)), "out one word inside in": lambda: call(o=at(src, 4 * per - 1)),
        "out over the plaintexts": lambda: call(n=1, o=at(plain_qp)),
        "out one word inside the special row of the last plaintext": lambda: call(n=1, o=at(plain_qp, 6 * ptw - 1)),
        "out inside a masked plaintext": lambda: call(n=1, m=(1, 1, 1, 1, 1, 0), o=at(plain_qp, 6 * ptw - 1)),
        "n == 0, L 0": lambda: call(L=0, n=0), "n_baby == 0, L past the top": lambda: call(L=Lt + 1, b=()), "n_giant == 0, L 0": lambda: call(L=0, g=()),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        want = b"he355_linear_transform_bsgs: "
        assert msg.startswith(want) and len(msg) > len(want), (name, msg)
    # accepted by the host: there is no device behind these contexts, and no CPU fallback
    good = {
        "transform": lambda: call(), "on NTT-form BFV": lambda: call(h=bfv.h), "lower level": lambda: call(L=1), "the identity alone": lambda: call(b=(0,), g=(0,)),
        "a mask": lambda: call(m=(1, 0, 1, 0, 0, 0)), "out right behind in": lambda: call(o=at(src, 4 * per)),
        "steps at the edge": lambda: call(b=(N // 2 - 1, -(N // 2 - 1)), g=(N // 2 - 1,)),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    # right behind the plaintexts: accepted too (a slab of its own, so that the pointer stays inside an allocation)
    big = np.full(6 * ptw + per, FILL, dtype=np.uint64)
    assert call(n=1, p=at(big), o=at(big, 6 * ptw)) == be.E_DEVICE
    # nothing to do: success, whatever the pointers are, and no device is asked for
    assert call(n=0, i=None, p=None, o=None) == be.OK
    assert call(b=(), p=None, o=at(src)) == be.OK
    assert call(g=(), p=None, o=at(src)) == be.OK
    # the scratch bound needs no device: (n_baby + 2) blocks of min(chunk, n) extended ciphertexts at least, nothing for an empty call
    sb = ckks.linear_transform_bsgs_scratch_bytes(Lt, 4, 3)
    assert sb >= (3 + 2) * 4 * 2 * (Lt + 1) * N * 8
    assert ckks.linear_transform_bsgs_scratch_bytes(Lt, 0, 3) == 0 and ckks.linear_transform_bsgs_scratch_bytes(Lt, 4, 0) == 0
    assert ckks.linear_transform_bsgs_scratch_bytes(Lt + 1, 4, 3) == 0
    # more baby steps than the call takes: 0, not a product that wrapped into a small bound; a huge batch is cut by the chunk; the bound grows with n_baby
    assert ckks.linear_transform_bsgs_scratch_bytes(Lt, 4, (1 << 20) + 1) == 0 and ckks.linear_transform_bsgs_scratch_bytes(Lt, 4, 1 << 63) == 0
    assert ckks.linear_transform_bsgs_scratch_bytes(Lt, 1 << 63, 1 << 20) >= (1 << 20) * 1024 * 2 * (Lt + 1) * N * 8
    assert ckks.linear_transform_bsgs_scratch_bytes(Lt, 4, 4) > sb
    for c in (bfv, ckks, one):
        c.close()
    assert (src == FILL).all() and (dst == FILL).all() and (plain_qp == FILL).all() and (big == FILL).all()


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "linear_transform_bsgs_args_main.cpp", "linear_transform_bsgs_args ok")
