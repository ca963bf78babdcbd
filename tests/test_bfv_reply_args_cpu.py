"""The refusals of he355_bfv_reply_compress and he355_bfv_reply_decrypt that need no device (csrc/bfv_pir_args.h::plan_reply), through the C
ABI on a context without one: every bad argument is HE355_E_INVALID_ARGS with a message that names the call, decided on the host before a
device is asked for -- the neighbouring good arguments then fail with HE355_E_DEVICE (no CPU fallback) -- and neither touches a buffer:

* a CKKS context; L of 0 and L_top + 1;
* widths outside the rule: k0 below 2, k0 above k1, k1 one above the chain's limit (47 at N = 4096 under a 60-bit prime); the limit itself,
  (2, 2) and the safe pair are accepted;
* a d_bytes off an 8-byte boundary, a stride short of a reply, a stride that is no multiple of 8;
* (n - 1) stride + the reply size at 2^63 and above; one word short of it is accepted as far as the host can tell;
* more replies than one launch's grid holds;
* every overlap of output and input: the replies over the ciphertexts (first word, last word; right behind is accepted), the plaintexts over
  the replies, a budget output over the replies, over the plaintexts, over the other budget output;
* n == 0 is accepted whatever the pointers are.
The host-only calls: he355_bfv_reply_bytes (0 for a CKKS context and for refused widths) and he355_bfv_reply_safe_bits (0 under a 35-bit first
prime, the widths still written).
And the check itself under the sanitizers: tests/bfv_reply_args_main.cpp, a stand-alone program, calls plan_reply at these and further edges
(strides near 2^63 and 2^64, spans that pass the end of the address space), compiled with g++ -fsanitize=address,undefined and run as a
child process: exit status 0.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import sanitized_program

N, BITS = 4096, [60, 40, 40, 60]
FILL = 0xABCD
NEW = ["he355_bfv_reply_bytes", "he355_bfv_reply_safe_bits", "he355_bfv_reply_compress", "he355_bfv_reply_decrypt"]


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def test_symbols_exported_and_declared(be):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "he355.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
        assert hasattr(be.Context, s[len("he355_"):])


def test_host_only_calls(be):
    for n_, bits, want, size in ((8192, [60, 40, 60], (22, 35, True), 58368), (32768, [60, 40, 40, 60], (22, 37, True), 241664),
                                 (1024, [50, 40, 50], (22, 32, True), 6912), (1024, [35, 40, 60], (22, 32, False), 0)):
        ctx = be.Context(be.SCHEME_BFV, n_, bit_sizes=bits, plain_bits=20, sec128=False)
        assert ctx.bfv_reply_safe_bits() == want
        assert ctx.bfv_reply_bytes(want[0], want[1]) == size
        assert ctx.bfv_reply_bytes(2, 2) == n_ // 2 and ctx.bfv_reply_bytes(1, 2) == 0 and ctx.bfv_reply_bytes(3, 2) == 0 and ctx.bfv_reply_bytes(2, 63) == 0
        ctx.close()
    ctx = be.Context(be.SCHEME_BFV, 8192, bit_sizes=[60, 40, 60], plain_bits=20, sec128=False)
    assert ctx.bfv_reply_bytes(2, 46) == 8192 * 48 // 8 and ctx.bfv_reply_bytes(2, 47) == 0  # the limit the header states
    assert ctx.bfv_reply_bytes(22, 35) < 2 * 8192 * 8
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    assert ck.bfv_reply_bytes(22, 34) == 0 and ck.bfv_reply_safe_bits() == (0, 0, False)
    ck.close()


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=20, sec128=False)
    Lt = ctx.L
    k0, k1, ok = ctx.bfv_reply_safe_bits()
    assert (k0, k1, ok) == (22, 34, True)
    B = ctx.bfv_reply_bytes(k0, k1)
    assert B == N * 56 // 8
    per = 2 * Lt * N
    cts = np.full(4 * per, FILL, dtype=np.uint64)
    byt = np.full(4 * (B // 8 + 3), FILL, dtype=np.uint64)
    stat = np.full(8, FILL, dtype=np.uint64)
    pc, pb, ps = cts.ctypes.data, byt.ctypes.data, stat.ctypes.data
    assert pb % 8 == 0
    vp = C.c_void_p

    def comp(L=Lt, a=k0, b=k1, n=2, dst=pb, stride=B, src=pc, h=None):
        return lib.he355_bfv_reply_compress(h or ctx.h, L, a, b, n, vp(src), vp(dst), stride)

    def dec(a=k0, b=k1, n=2, src=pb, stride=B, dst=pc, bud=None, bits=None, h=None):
        return lib.he355_bfv_reply_decrypt(h or ctx.h, a, b, n, vp(src), stride, vp(dst), vp(bud) if bud else None, vp(bits) if bits else None)

    NMAX = (2 ** 31 - 1) // (N // 256)
    bad = {
        "he355_bfv_reply_compress": {
            "L 0": lambda: comp(L=0), "L past the top": lambda: comp(L=Lt + 1), "L negative": lambda: comp(L=-1),
            "k0 1": lambda: comp(a=1), "k0 above k1": lambda: comp(a=23, b=22), "k1 past the limit": lambda: comp(a=2, b=48),
            "k1 64": lambda: comp(a=2, b=64), "k0 negative": lambda: comp(a=-5),
            "d_bytes off a word": lambda: comp(dst=pb + 4), "stride short": lambda: comp(stride=B - 8), "stride odd": lambda: comp(stride=B + 4),
            "stride 0, n 1": lambda: comp(n=1, stride=0),
            "span 2^63": lambda: comp(n=3, stride=1 << 62), "span reaches 2^63": lambda: comp(stride=(1 << 63) - B),
            "stride 2^64 - 8": lambda: comp(stride=2 ** 64 - 8),
            "one launch": lambda: comp(n=NMAX + 1, a=2, b=2, stride=N // 2), "n 2^40": lambda: comp(n=1 << 40),
            "replies on the ciphertexts": lambda: comp(dst=pc), "replies on the last ciphertext word": lambda: comp(dst=pc + 8 * 2 * per - 8),
            "ciphertexts on the last reply word": lambda: comp(src=pb + 2 * B - 8),
        },
        "he355_bfv_reply_decrypt": {
            "k0 1": lambda: dec(a=1), "k0 above k1": lambda: dec(a=23, b=22), "k1 past the limit": lambda: dec(a=2, b=48),
            "d_bytes off a word": lambda: dec(src=pb + 4), "stride short": lambda: dec(stride=B - 8), "stride odd": lambda: dec(stride=B + 4),
            "span 2^63": lambda: dec(n=3, stride=1 << 62), "one launch": lambda: dec(n=NMAX + 1, a=2, b=2, stride=N // 2),
            "plaintexts on the replies": lambda: dec(dst=pb), "plaintexts on the last reply word": lambda: dec(dst=pb + 2 * B - 8),
            "budget on the replies": lambda: dec(bud=pb + 8), "bits on the plaintexts": lambda: dec(bits=pc + 8 * 2 * N - 4),
            "budget on bits": lambda: dec(bud=ps, bits=ps + 4),
        },
    }
    for call, cases in bad.items():
        for name, f in cases.items():
            assert f() == be.E_INVALID_ARGS, (call, name)
            msg = lib.he355_last_error()
            assert call.encode() in msg and len(msg) > len(call) + 2, (call, name, msg)
    # accepted by the host: there is no device behind this context, and no CPU fallback
    good = {
        "compress": comp, "L 1": lambda: comp(L=1), "(2, 2)": lambda: comp(a=2, b=2, stride=N // 2), "the limit": lambda: comp(a=2, b=47),
        "k0 = k1 = the limit": lambda: comp(a=47, b=47, n=1, stride=2 * 47 * N // 8), "padded stride": lambda: comp(stride=B + 24),
        "one word short of 2^63": lambda: comp(stride=(1 << 63) - B - 8, dst=0x1000, src=(1 << 63) + 0x10000), "one launch": lambda: comp(n=NMAX, a=2, b=2, stride=N // 2, L=1, dst=0x1000, src=1 << 62),
        "replies right behind the ciphertexts": lambda: comp(dst=pc + 8 * 2 * per), "ciphertexts right behind the replies": lambda: comp(src=pb + 2 * B),
        "n 0": lambda: comp(n=0, dst=pc),
        "decrypt": dec, "decrypt with outputs": lambda: dec(bud=ps, bits=ps + 8), "bits only": lambda: dec(bits=ps),
        "plaintexts right behind the replies": lambda: dec(dst=pb + 2 * B), "bits right behind the plaintexts": lambda: dec(bits=pc + 8 * 2 * N),
        "decrypt n 0": lambda: dec(n=0, dst=pb, bud=pb, bits=pb),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    for f in (lambda: comp(L=ck.L, h=ck.h), lambda: dec(h=ck.h)):
        assert f() == be.E_INVALID_ARGS
        assert b"BFV context" in lib.he355_last_error()
    ck.close()
    assert (cts == FILL).all() and (byt == FILL).all() and (stat == FILL).all()


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "bfv_reply_args_main.cpp", "bfv_reply_args ok")
