"""The refusals of the seeded calls that need no device (csrc/bfv_pir_args.h: plan_seeded_encrypt, plan_seeded_selector, plan_seeded_restore,
plan_keygen_galois_seeded, plan_set_galois_key_seeded), through the C ABI on a context without one: every bad argument is HE355_E_INVALID_ARGS
with a message that names the call, decided on the host before a device is asked for -- the neighbouring good arguments then fail with
HE355_E_DEVICE (no CPU fallback) -- and neither touches a buffer:

* a CKKS context; L of 0 and L_top + 1; ntt_form 2 and -1;
* a_seed == noise_seed (the three client calls);
* first_index + n one above 2^40 and wrapping 2^64; exactly 2^40 is accepted;
* more ciphertexts than one launch's grid holds (and one fewer, accepted); a slab past 2^60 words;
* every overlap of output and input: c0 on the plaintexts (first word, last word; right behind is accepted), the restored ciphertexts on c0,
  c0 on the selectors;
* he355_bfv_selector_encrypt's own rules: n_sel 0, count 0 and N + 1, slots past count, digit_bits 0 and 64;
* Galois elements 0, 1, 2, even, 2N and 2N + 1; null key halves;
* n == 0 is accepted whatever the pointers are.
The missing secret key needs a device behind the context: tests/test_gpu_bfv_seeded.py.
And the checks themselves under the sanitizers: tests/bfv_seeded_args_main.cpp, a stand-alone program, calls the plans at these and further
edges (spans that pass the end of the address space, counts near 2^64), compiled with g++ -fsanitize=address,undefined and run as a child
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
NEW = ["he355_bfv_seeded_encrypt", "he355_bfv_seeded_selector_encrypt", "he355_bfv_seeded_restore", "he355_keygen_galois_seeded",
       "he355_set_galois_key_seeded"]
TOP = 1 << 40


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
    for words in ("a_seed IS PUBLIC", "noise_seed IS SECRET", "NOT A CRYPTOGRAPHIC XOF"):  # the security caveats, in capitals
        assert words in hdr, words


def test_refusals_are_decided_on_the_host(be):
    lib = be.lib()
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=20, sec128=False)
    Lt, K = ctx.L, ctx.K
    c0 = np.full(4 * Lt * N, FILL, dtype=np.uint64)
    out = np.full(4 * 2 * Lt * N, FILL, dtype=np.uint64)
    pl = np.full(4 * N, FILL, dtype=np.uint64)
    kb = np.full(Lt * K * N, FILL, dtype=np.uint64)
    p0, po, pp, pk = c0.ctypes.data, out.ctypes.data, pl.ctypes.data, kb.ctypes.data
    vp = C.c_void_p
    A, E = 11, 12

    def enc(L=Lt, n=2, plain=pp, a=A, e=E, first=0, dst=p0, h=None):
        return lib.he355_bfv_seeded_encrypt(h or ctx.h, L, n, vp(plain) if plain else None, a, e, first, vp(dst))

    def sel(L=Lt, v=16, n=2, n_sel=2, slot=0, count=64, s=pp, a=A, e=E, first=0, dst=p0, h=None):
        return lib.he355_bfv_seeded_selector_encrypt(h or ctx.h, L, v, n, n_sel, slot, count, vp(s), a, e, first, vp(dst))

    def res(L=Lt, form=0, n=2, src=p0, a=A, first=0, dst=po, h=None):
        return lib.he355_bfv_seeded_restore(h or ctx.h, L, form, n, vp(src), a, first, vp(dst))

    def kg(elt=3, a=A, e=E, dst=pk, h=None):
        return lib.he355_keygen_galois_seeded(h or ctx.h, elt, a, e, vp(dst))

    def sk(elt=3, src=pk, a=A, h=None):
        return lib.he355_set_galois_key_seeded(h or ctx.h, elt, C.cast(vp(src), C.POINTER(C.c_uint64)) if src else None, a)

    NMAX = (2 ** 31 - 1) // (Lt * (N // 512))
    RMAX = (2 ** 31 - 1) // (2 * Lt * (N // 512))
    E10 = 4 + 3 + 3  # E(L_top) at 16 bits
    bad = {
        "he355_bfv_seeded_encrypt": {
            "L 0": lambda: enc(L=0), "L past the top": lambda: enc(L=Lt + 1), "L negative": lambda: enc(L=-1),
            "equal seeds": lambda: enc(a=7, e=7), "equal seeds 0": lambda: enc(a=0, e=0),
            "index above 2^40": lambda: enc(first=TOP - 1), "index at 2^40, n 1": lambda: enc(n=1, first=TOP), "index wraps": lambda: enc(first=2 ** 64 - 1),
            "one launch": lambda: enc(n=NMAX + 1, plain=None, dst=0x1000), "2^60 words": lambda: enc(n=1 << 50, plain=None, dst=0x1000),
            "c0 on the plaintexts": lambda: enc(dst=pp), "plaintexts on the last c0 word": lambda: enc(plain=p0 + 8 * 2 * Lt * N - 8),
            "c0 on the last plaintext word": lambda: enc(dst=pp + 8 * 2 * N - 8),
        },
        "he355_bfv_seeded_selector_encrypt": {
            "L 0": lambda: sel(L=0), "L past the top": lambda: sel(L=Lt + 1), "digit_bits 0": lambda: sel(v=0), "digit_bits 64": lambda: sel(v=64),
            "n_sel 0": lambda: sel(n_sel=0), "count 0": lambda: sel(count=0), "count N + 1": lambda: sel(count=N + 1),
            "slots past count": lambda: sel(slot=64 - 2 * E10 + 1), "equal seeds": lambda: sel(a=9, e=9),
            "index above 2^40": lambda: sel(first=TOP - 1), "index wraps": lambda: sel(first=2 ** 64 - 2),
            "one launch": lambda: sel(n=NMAX + 1, s=1 << 62, dst=0x1000), "c0 on the selectors": lambda: sel(dst=pp), "c0 on the last selector": lambda: sel(dst=pp + 8 * 3),
        },
        "he355_bfv_seeded_restore": {
            "L 0": lambda: res(L=0), "L past the top": lambda: res(L=Lt + 1), "ntt_form 2": lambda: res(form=2), "ntt_form -1": lambda: res(form=-1),
            "index above 2^40": lambda: res(first=TOP - 1), "index wraps": lambda: res(first=2 ** 64 - 1),
            "one launch": lambda: res(n=RMAX + 1, src=1 << 62, dst=0x1000), "2^60 words": lambda: res(n=1 << 50, src=1 << 62, dst=0x1000),
            "out on c0": lambda: res(dst=p0), "c0 on the last output word": lambda: res(src=po + 8 * 4 * Lt * N - 8),
            "out on the last c0 word": lambda: res(dst=p0 + 8 * 2 * Lt * N - 8),
        },
        "he355_keygen_galois_seeded": {
            "elt 0": lambda: kg(elt=0), "elt 1": lambda: kg(elt=1), "elt even": lambda: kg(elt=4), "elt 2N": lambda: kg(elt=2 * N),
            "elt 2N + 1": lambda: kg(elt=2 * N + 1), "equal seeds": lambda: kg(a=5, e=5),
        },
        "he355_set_galois_key_seeded": {
            "elt 1": lambda: sk(elt=1), "elt 2": lambda: sk(elt=2), "elt 2N + 1": lambda: sk(elt=2 * N + 1), "null halves": lambda: sk(src=None),
        },
    }
    for call, cases in bad.items():
        for name, f in cases.items():
            assert f() == be.E_INVALID_ARGS, (call, name, lib.he355_last_error())
            msg = lib.he355_last_error()
            assert call.encode() in msg and len(msg) > len(call) + 2, (call, name, msg)
    # accepted by the host: there is no device behind this context, and no CPU fallback
    good = {
        "encrypt": enc, "zeros": lambda: enc(plain=None), "L 1": lambda: enc(L=1), "seeds one apart": lambda: enc(a=7, e=8),
        "index reaches 2^40": lambda: enc(first=TOP - 2), "one launch": lambda: enc(n=NMAX, plain=None, dst=0x1000),
        "plaintexts right behind c0": lambda: enc(plain=p0 + 8 * 2 * Lt * N), "c0 right behind the plaintexts": lambda: enc(dst=pp + 8 * 2 * N),
        "n 0": lambda: enc(n=0, dst=pp, first=TOP),
        "selector": sel, "slots reach count": lambda: sel(slot=64 - 2 * E10), "selector index reaches 2^40": lambda: sel(first=TOP - 2),
        "c0 right behind the selectors": lambda: sel(dst=pp + 8 * 4), "selector n 0": lambda: sel(n=0, dst=pp),
        "restore": res, "ntt form": lambda: res(form=1), "restore L 1": lambda: res(L=1), "restore index reaches 2^40": lambda: res(first=TOP - 2),
        "restore one launch": lambda: res(n=RMAX, src=1 << 62, dst=0x1000), "c0 right behind the output": lambda: res(src=po + 8 * 4 * Lt * N),
        "out right behind c0": lambda: res(dst=p0 + 8 * 2 * Lt * N), "restore n 0": lambda: res(n=0, dst=p0),
        "keygen": kg, "keygen elt 2N - 1": lambda: kg(elt=2 * N - 1), "set": sk, "set elt 2N - 1": lambda: sk(elt=2 * N - 1),
    }
    for name, f in good.items():
        assert f() == be.E_DEVICE, (name, lib.he355_last_error())
        assert b"no CPU fallback" in lib.he355_last_error(), name
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    for f in (lambda: enc(L=ck.L, h=ck.h), lambda: sel(L=ck.L, h=ck.h), lambda: res(L=ck.L, h=ck.h), lambda: kg(h=ck.h), lambda: sk(h=ck.h)):
        assert f() == be.E_INVALID_ARGS
        assert b"BFV context" in lib.he355_last_error()
    ck.close()
    assert (c0 == FILL).all() and (out == FILL).all() and (pl == FILL).all() and (kb == FILL).all()


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "bfv_seeded_args_main.cpp", "bfv_seeded_args ok")
