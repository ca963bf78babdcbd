"""The refusals of he355_bfv_select that need no device (csrc/bfv_pir_args.h::plan_select), through the C ABI on a context without one: every bad
argument is HE355_E_INVALID_ARGS with a message naming the call, decided on the host before a device is asked for -- valid arguments then fail
with HE355_E_DEVICE (no CPU fallback) -- and neither touches a buffer:

* a CKKS context; L of 0 and L_top + 1; digit_bits of 0 and 64; a count of 0 and of 2^24 + 1 (2^20 and 2^24 are accepted);
* leaf strides under which two leaves lie at one place (plan_merge's rule): a stride of 0 along an index that moves, equal strides, (4, 2) with
  count 3, (4, 6) with count 3 and n 4; the neighbouring strides that do not collide are accepted -- row-major (count, 1), child-major (1, n),
  padded, (2, 3) at count 2 and n 2, (4, 6) at count 3 and n 3;
* strides that take an operand past 2^60 words: leaf strides of 2^63 and 2^50 ciphertexts, a selector stride of 2^50;
* more pairs than one launch's grid holds;
* d_out overlapping the leaves (at the first leaf, one word inside the last, in a gap of padded leaves; right behind the last is accepted) or the
  selectors (the first word; the last word of two results' bits, of one result's, of shared bits; right behind them is accepted);
* every refusal's message names the call and the reason, so that no case passes for a reason it does not mean;
* all operands with real addresses lie in ONE arena at offsets the test chooses, every d_out with its whole extent, so that no verdict
  depends on where the allocator puts an array;
* n == 0 is accepted whatever the strides and pointers are; rg_stride_r == 0 is accepted (all results share one set of bits).
And the check itself under the sanitizers: tests/bfv_select_args_main.cpp, a stand-alone program, includes the header -- which needs no HIP --
and calls plan_select at these and further edges (count 1, 2, 3, 2^k +- 1, strides near 2^64, the grid limit to the pair) and reads the level
tables, the pairs per level, the pass and the block sizes back.  Compiled with g++ -fsanitize=address,undefined, the sanitizer runtimes linked
statically, and run as a child process: exit status 0.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import sanitized_program

N, BITS = 1024, [50, 40, 50]  # a small ring: the check never looks at a word, and the buffers stay small
FILL = 0xABCD
V = 20
LT, E_TOP = 2, 5                     # the chain's data primes and E(L_top) at v = 20 (asserted below)
PER = 2 * LT * N                     # words of a ciphertext at L_top
RG = 2 * E_TOP * PER                 # words of an RGSW ciphertext
# ONE arena for every operand, so that what lies next to what is the test's choice and not the allocator's: 2 ciphertexts of room, the leaves
# (26 ciphertexts), room, the selectors (6 RGSW ciphertexts), room, the output (4 ciphertexts), room.  Every `d_out` of a case with a real
# pointer lies inside it with its whole extent (checked per case).  Module-level and never freed: freeing a block of this size would move
# glibc's mmap threshold and with it the addresses of the arrays of the tests that run after this one.
GAP = 2 * PER
OFF_LEAVES, OFF_SELS, OFF_OTHER = GAP, GAP + 26 * PER + GAP, GAP + 26 * PER + GAP + 6 * RG + GAP
ARENA = np.full(OFF_OTHER + 4 * PER + GAP, FILL, dtype=np.uint64)


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
    E, _ = ctx.bfv_gadget_count(Lt, V)
    rg = 2 * E * per  # words of one RGSW ciphertext
    assert (Lt, E, per, rg) == (LT, E_TOP, PER, RG)
    base = ARENA.ctypes.data

    class Slab:
        """a region of the arena: `off` words from its start"""

        def __init__(self, off):
            self.off = off

    leaves, sels, other = Slab(OFF_LEAVES), Slab(OFF_SELS), Slab(OFF_OTHER)
    at = lambda a, words: C.c_void_p(base + 8 * (a.off + int(words)))
    p, s, o = at(leaves, 0), at(sels, 0), at(other, 0)

    def inside(dst, n, L):
        """the output's whole extent, n ciphertexts of a valid level, lies in the arena"""
        lo = dst.value - base
        return 0 <= lo and lo + 8 * n * 2 * min(max(L, 1), Lt) * N <= ARENA.nbytes

    def select(L=Lt, v=V, n=2, count=4, ct=p, sr=4, sk=1, rgsw=s, rr=2, rj=1, dst=o, h=None):
        assert n > 4 or inside(dst, n, L), "the case's d_out leaves the arena"  # (the grid cases' n are refused as numbers)
        if 1 <= L <= Lt and 1 <= v <= 63 and 1 <= n <= 4 and 1 <= count <= 16 and max(sr, sk, rr, rj) < 64:  # operands that are read where they lie
            m = (count - 1).bit_length()
            if ct is p:
                assert (n - 1) * sr + (count - 1) * sk + 1 <= 26, "the case's leaves pass the end of their slab"
            if rgsw is s and m:
                assert ((n - 1) * rr + (m - 1) * rj + 1) * 2 * ctx.bfv_gadget_count(L, v)[0] * 2 * L * N <= 6 * rg, "the case's selectors pass the end of their slab"
        return lib.he355_bfv_select(h or ctx.h, L, v, n, count, ct, sr, sk, rgsw, rr, rj, dst)

    bad = {  # what is refused, and the words of the message that say it was refused for that reason
        "L 0": (lambda: select(L=0), "level"), "L past the top": (lambda: select(L=Lt + 1), "level"),
        "v 0": (lambda: select(v=0), "digit_bits"), "v 64": (lambda: select(v=64), "digit_bits"),
        "count 0": (lambda: select(count=0), "count must be"), "count 2^24 + 1": (lambda: select(n=1, count=(1 << 24) + 1), "count must be"),
        "stride_k 0": (lambda: select(sk=0), "stride of 0"), "stride_r 0": (lambda: select(sr=0), "stride of 0"),
        "both 0": (lambda: select(sr=0, sk=0), "stride of 0"),
        "equal strides": (lambda: select(sr=1, sk=1), "at one place"),
        "(4, 2) count 3": (lambda: select(count=3, sr=4, sk=2), "at one place"),
        "(4, 6) count 3 n 4": (lambda: select(count=3, n=4, sr=4, sk=6, rr=0), "at one place"),
        "(3, 1) count 4": (lambda: select(count=4, sr=3, sk=1), "at one place"),
        "stride 2^63": (lambda: select(sr=1, sk=1 << 63), "2^60"), "stride 2^50": (lambda: select(sr=1 << 50, sk=1), "2^60"),
        "selector stride 2^50": (lambda: select(rr=1 << 50), "2^60"),
        "selector level stride 2^63": (lambda: select(rj=1 << 63), "2^60"),
        "too many results": (lambda: select(n=1 << 31, count=2, sr=1, sk=1 << 31), "one launch"),
        "too many pairs": (lambda: select(n=1 << 12, count=1 << 20, sr=1 << 20, sk=1), "one launch"),
        "out at the first leaf": (lambda: select(dst=p), "overlaps the leaves"),
        "out one word inside the last leaf": (lambda: select(dst=at(leaves, 8 * per - 1)), "overlaps the leaves"),
        "out in a gap": (lambda: select(count=2, n=2, sr=1, sk=3, dst=at(leaves, 2 * per)), "overlaps the leaves"),
        "count 1 over itself": (lambda: select(count=1, n=1, dst=at(leaves, N)), "overlaps the leaves"),
        "out at the first selector": (lambda: select(dst=s), "overlaps the selectors"),
        "out at the last selector word": (lambda: select(dst=at(sels, 4 * rg - 1)), "overlaps the selectors"),        # n 2 x 2 bits: 4 selectors
        "out at the last word of one result's bits": (lambda: select(n=1, dst=at(sels, 2 * rg - 1)), "overlaps the selectors"),
        "out inside shared bits": (lambda: select(rr=0, dst=at(sels, rg)), "overlaps the selectors"),
    }
    for name, (f, why) in bad.items():
        assert f() == be.E_INVALID_ARGS, name
        msg = lib.he355_last_error()
        assert msg.startswith(b"he355_bfv_select: ") and why.encode() in msg, (name, msg)
    # accepted by the host: there is no device behind this context, and no CPU fallback
    good = {
        "row-major": lambda: select(), "child-major": lambda: select(sr=1, sk=2), "padded": lambda: select(sr=5, sk=1),
        "(2, 3) count 2 n 2": lambda: select(count=2, sr=2, sk=3), "(4, 6) count 3 n 3": lambda: select(count=3, n=3, sr=4, sk=6),
        "count 1, stride_k 0": lambda: select(count=1, sk=0), "n 1, stride_r 0": lambda: select(n=1, sr=0, sk=1),
        "shared bits": lambda: select(rr=0), "count 3": lambda: select(count=3), "count 5, one result": lambda: select(n=1, count=5, rj=1),
        "count 2^20": lambda: select(n=1, count=1 << 20, rgsw=C.c_void_p(1 << 40), ct=C.c_void_p(1 << 50)),
        "count 2^24, L 1": lambda: select(L=1, n=1, count=1 << 24, rgsw=C.c_void_p(1 << 40), ct=C.c_void_p(1 << 50)),
        "out right behind the last leaf": lambda: select(dst=at(leaves, 8 * per)),
        "out right behind the shared bits": lambda: select(rr=0, dst=at(sels, 2 * rg)),
        "out right behind one result's bits": lambda: select(n=1, dst=at(sels, 2 * rg)),
        "v 1": lambda: select(v=1, rgsw=C.c_void_p(1 << 40)), "v 63": lambda: select(v=63),
        "lower levels": lambda: select(L=1),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    assert select(n=0, sr=0, sk=0, dst=p) == be.E_DEVICE  # nothing to check at n == 0; the device is asked for and is not there
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    assert select(L=ck.L, h=ck.h) == be.E_INVALID_ARGS
    assert b"BFV context" in lib.he355_last_error()
    ck.close()
    assert (ARENA == FILL).all()


def test_route_counters_keep_the_struct(be):
    """the four counters come out of reserved[5]: the struct keeps its 16 words, C and Python agree"""
    assert C.sizeof(be.BfvRouteStats) == 16 * 8
    names = [k for k, _ in be.BfvRouteStats._fields_]
    assert names[11:15] == ["select_cols", "select_stream", "select_tail_fused", "select_tail_routed"] and names[15] == "reserved"


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "bfv_select_args_main.cpp", "bfv_select_args ok")
