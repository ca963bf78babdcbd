"""The refusals of he355_bfv_merge that need no device (csrc/bfv_pir_args.h::plan_merge), through the C ABI on a context without one: every
bad argument is HE355_E_INVALID_ARGS with a message, decided on the host before a device is asked for -- valid arguments then fail with
HE355_E_DEVICE (no CPU fallback) -- and neither touches a buffer:

* a CKKS context; L of 0 and L_top + 1; a count of 0 and N + 1;
* strides under which two inputs lie at one place: a stride of 0 along an index that moves, equal strides, (2, 4) with count 3 (input 2 of
  result 0 is input 0 of result 1), (6, 4) with count 3 and n 4 (k = 2, r = 0 meets k = 0, r = 3); the neighbouring strides that do not
  collide are accepted -- (n, 1), (1, count), (n + 1, 1), (3, 2) at count 2 and n 2, (6, 4) at count 3 and n 3;
* extents whose index arithmetic would wrap: strides of 2^63 and of 2^50 ciphertexts;
* more pairs than one launch holds;
* d_out overlapping the inputs: at the first input, one word inside the last, in a gap of padded inputs; right behind the last is accepted;
* n == 0 is accepted whatever the strides and pointers are.
And the check itself under the sanitizers: tests/bfv_merge_args_main.cpp, a stand-alone program, includes the header -- which needs no HIP --
and calls plan_merge at these and further edges (strides near 2^64, spans that pass the end of the address space, the grid limit to the pair),
and reads the plans back.  Compiled with g++ -fsanitize=address,undefined, the sanitizer runtimes linked statically, and run as a child
process: exit status 0.
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


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=20, sec128=False)
    Lt = ctx.L
    per = 2 * Lt * N
    slab = np.full(24 * per, FILL, dtype=np.uint64)
    other = np.full(4 * per, FILL, dtype=np.uint64)
    base = slab.ctypes.data
    at = lambda words: C.c_void_p(base + 8 * int(words))
    p, o = at(0), other.ctypes.data_as(C.c_void_p)

    def merge(L=Lt, n=2, count=4, src=p, sk=2, sr=1, dst=o, h=None):
        return lib.he355_bfv_merge(h or ctx.h, L, n, count, src, sk, sr, dst)

    bad = {
        "L 0": lambda: merge(L=0), "L past the top": lambda: merge(L=Lt + 1),
        "count 0": lambda: merge(count=0), "count N + 1": lambda: merge(count=N + 1),
        "stride_k 0": lambda: merge(sk=0), "stride_r 0": lambda: merge(sr=0), "both 0": lambda: merge(sk=0, sr=0),
        "equal strides": lambda: merge(sk=1, sr=1),
        "(2, 4) count 3": lambda: merge(count=3, sk=2, sr=4),
        "(6, 4) count 3 n 4": lambda: merge(count=3, n=4, sk=6, sr=4),
        "(1, 3) count 4": lambda: merge(count=4, sk=1, sr=3),
        "stride 2^63": lambda: merge(sk=1 << 63, sr=1), "stride 2^50": lambda: merge(sk=1, sr=1 << 50),
        "stride_r 2^63": lambda: merge(count=1, n=3, sk=0, sr=1 << 63),
        "too many pairs": lambda: merge(n=1 << 31, count=2, sk=1 << 31, sr=1),
        "one launch": lambda: merge(n=1 << 19, count=N, sk=1 << 19, sr=1),
        "out at the first input": lambda: merge(dst=p),
        "out one word inside the last input": lambda: merge(dst=at(8 * per - 1)),
        "out in a gap": lambda: merge(count=2, n=2, sk=3, sr=1, dst=at(2 * per)),
        "count 1 over itself": lambda: merge(count=1, n=1, dst=at(N)),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        assert b"he355_bfv_merge" in msg and len(msg) > len(b"he355_bfv_merge: "), name
    # accepted by the host: there is no device behind this context, and no CPU fallback
    good = {
        "child-major": lambda: merge(), "row-major": lambda: merge(sk=1, sr=4), "padded": lambda: merge(sk=3, sr=1),
        "(3, 2) count 2 n 2": lambda: merge(count=2, sk=3, sr=2), "(6, 4) count 3 n 3": lambda: merge(count=3, n=3, sk=6, sr=4),
        "count 1, stride_k 0": lambda: merge(count=1, sk=0), "n 1, stride_r 0": lambda: merge(n=1, sk=1, sr=0),
        "count 16": lambda: merge(n=1, count=16, sk=1, sr=1),
        "out right behind the last input": lambda: merge(dst=at(8 * per)),
        "lower levels": lambda: merge(L=1),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    assert merge(n=0, sk=0, sr=0, dst=p) == be.E_DEVICE  # nothing to check at n == 0; the device is asked for and is not there
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    assert merge(L=ck.L, h=ck.h) == be.E_INVALID_ARGS
    assert b"BFV context" in lib.he355_last_error()
    ck.close()
    assert (slab == FILL).all() and (other == FILL).all()


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "bfv_merge_args_main.cpp", "bfv_merge_args ok")
