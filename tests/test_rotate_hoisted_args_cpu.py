"""The refusals of the hoisted rotations that need no device (csrc/hoist_args.h::plan_rotate_hoisted), through the C ABI on contexts without
one: every bad argument is HE355_E_INVALID_ARGS with a message, decided on the host before a device is asked for -- valid arguments then
fail with HE355_E_DEVICE (no CPU fallback) -- and neither touches a buffer:

* L of 0 and L_top + 1; a chain that cannot key-switch (K < 2); ntt_form of -1 and 2; ntt_form 0 on a CKKS context;
* an even element, an element of 2N, a step of N / 2 (no element);
* n n_elts 2 L N past 2^60 words, a slab that wraps the address space;
* d_out overlapping d_in (at it, one word inside its end, d_in inside a later block of d_out) and d_plain; right behind is accepted;
* n == 0 and n_elts == 0 return success without a device and touch nothing; a bad level is refused all the same.
("Galois key not present" is the device context's to know: tests/test_gpu_rotate_hoisted.py.)
And the check itself under the sanitizers: tests/rotate_hoisted_args_main.cpp, a stand-alone program, includes the header -- which needs no
HIP -- and calls the plan at these and further edges.  Compiled with g++ -fsanitize=address,undefined, the sanitizer runtimes linked
statically, and run as a child process: exit status 0.
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


def test_the_c_abi_has_the_hoisted_calls(be):
    lib = be.lib()
    for name in ("he355_apply_galois_hoisted", "he355_rotate_hoisted", "he355_rotate_hoisted_plain_sum", "he355_hoist_stats", "he355_hoist_release_keys"):
        assert name in be.C_ABI_SYMBOLS and getattr(lib, name), name
    ctx = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    st = be.HoistStats()
    assert lib.he355_hoist_stats(ctx.h, C.byref(st), 0) == be.E_DEVICE and b"no CPU fallback" in lib.he355_last_error()
    assert lib.he355_hoist_release_keys(ctx.h) == be.E_DEVICE
    ctx.close()


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    bfv = be.Context(be.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=20, sec128=False)
    ckks = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    one = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60], sec128=False)
    Lt = bfv.L
    per = 2 * Lt * N
    src = np.full(4 * per, FILL, dtype=np.uint64)
    dst = np.full(12 * per, FILL, dtype=np.uint64)
    plain = np.full(3 * Lt * N, FILL, dtype=np.uint64)
    at = lambda arr, words=0: C.c_void_p(arr.ctypes.data + 8 * int(words))
    u32s = lambda v: (C.c_uint32 * max(1, len(v)))(*v)
    i32s = lambda v: (C.c_int32 * max(1, len(v)))(*v)

    def elts(h=bfv.h, L=Lt, nf=0, n=4, i=at(src), e=(3, 9, 2 * N - 1), o=at(dst), ne=None):
        return lib.he355_apply_galois_hoisted(h, L, nf, n, i, u32s(e), len(e) if ne is None else ne, o)

    def steps(h=bfv.h, L=Lt, nf=0, n=4, i=at(src), s=(1, 0, -2), o=at(dst)):
        return lib.he355_rotate_hoisted(h, L, nf, n, i, i32s(s), len(s), o)

    def psum(h=ckks.h, L=Lt, n=4, i=at(src), s=(1, 0, -2), p=at(plain), o=at(dst)):
        return lib.he355_rotate_hoisted_plain_sum(h, L, n, i, i32s(s), len(s), p, o)

    bad = {
        "L 0": lambda: elts(L=0), "L past the top": lambda: elts(L=Lt + 1), "steps, L 0": lambda: steps(L=0), "plain sum, L 0": lambda: psum(L=0),
        "K < 2": lambda: elts(h=one.h, L=1, nf=1), "K < 2, steps": lambda: steps(h=one.h, L=1, nf=1), "K < 2, plain sum": lambda: psum(h=one.h, L=1),
        "ntt_form -1": lambda: elts(nf=-1), "ntt_form 2": lambda: steps(nf=2),
        "coefficient form on CKKS": lambda: elts(h=ckks.h, nf=0), "steps, coefficient form on CKKS": lambda: steps(h=ckks.h, nf=0),
        "even element": lambda: elts(e=(3, 4)), "element 0": lambda: elts(e=(0,)), "element 2N": lambda: elts(e=(2 * N,)), "element 2N + 1": lambda: elts(e=(2 * N + 1,)),
        "step N / 2": lambda: steps(s=(1, N // 2)), "step -N / 2": lambda: steps(s=(-N // 2,)), "plain sum, step N / 2": lambda: psum(s=(N // 2, 0, 1)),
        "span": lambda: elts(n=1 << 60), "span of the output": lambda: elts(n=(1 << 60) // per // 2, i=C.c_void_p(0x1000), o=C.c_void_p(1 << 62)),
        "wraps": lambda: elts(n=2, i=C.c_void_p(2 ** 64 - 4096), o=C.c_void_p(0x1000)),
        "out at in": lambda: elts(o=at(src)), "out one word inside in": lambda: elts(o=at(src, 4 * per - 1)),
        "in inside a later block of out": lambda: elts(i=at(dst, 8 * per)),
        "steps, out at in": lambda: steps(o=at(src)),
        "plain sum over in": lambda: psum(o=at(src, per)), "plain sum over the plaintexts": lambda: psum(n=1, o=at(plain, 3 * Lt * N - 1)),
        "plain sum, null plaintexts": lambda: psum(p=None),
        "n == 0, L 0": lambda: elts(L=0, n=0), "n_elts == 0, ntt_form 2": lambda: elts(nf=2, e=()),
    }
    for name, f in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        assert b"he355_" in msg and b": " in msg and len(msg) > len(b"he355_rotate_hoisted_plain_sum: "), (name, msg)
    assert lib.he355_apply_galois_hoisted(bfv.h, Lt, 0, 4, at(src), None, 3, at(dst)) == be.E_INVALID_ARGS
    # accepted by the host: there is no device behind these contexts, and no CPU fallback
    good = {
        "elements": lambda: elts(), "steps": lambda: steps(), "BFV NTT form": lambda: elts(nf=1), "CKKS": lambda: elts(h=ckks.h, nf=1),
        "lower level": lambda: steps(L=1), "the identity alone": lambda: elts(e=(1,)), "an element twice": lambda: elts(e=(3, 3, 1)),
        "out right behind in": lambda: elts(o=at(src, 4 * per)), "plain sum": lambda: psum(), "plain sum on NTT-form BFV": lambda: psum(h=bfv.h),
        "plain sum right behind the plaintexts": lambda: psum(n=1, o=at(plain, 3 * Lt * N)),
        "steps at the edge": lambda: steps(s=(N // 2 - 1, -(N // 2 - 1))),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    # nothing to do: success, whatever the pointers are, and no device is asked for
    assert elts(n=0, i=None, o=None) == be.OK
    assert elts(e=(), o=at(src)) == be.OK
    assert steps(s=(), o=at(src)) == be.OK
    assert psum(s=(), p=None, o=at(src)) == be.OK
    for c in (bfv, ckks, one):
        c.close()
    assert (src == FILL).all() and (dst == FILL).all() and (plain == FILL).all()


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "rotate_hoisted_args_main.cpp", "rotate_hoisted_args ok")
