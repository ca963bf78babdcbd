"""The arithmetic of the PIR database codec on the CPU (tests/csim/sim_bfv_bytes.cpp runs csrc/bfv_bytes_core.h -- a field cut out of aligned
64-bit words at any byte address, one packed output word, the field count: the functions the HIP kernels k_bfv_unpack, k_bfv_pack and
k_bfv_bytes_cols_fwd compile -- and the centred lift of csrc/bfv_level_core.h the fused kernel applies to a field) against Python integers:

* extraction against int.from_bytes(bytes, "little") arithmetic for every w in 1..63, address offsets 0..7 and B in {1, 7, 8, 9, Bmax - 1,
  Bmax} at N = 64 and N = 1024 (B above Bmax does not exist and is left out: at N = 64, w = 1 that is B = 9).  The bytes after B are 0xFF
  filler, and so are the bytes before the start when the offset is non-zero: they must never show in a field; the last byte's top bit is
  set, so the last field is seen to be zero-extended rather than cut short;
* pack(unpack(x)) == x on the first B bytes, the tail bytes of the last word zero; the same with junk above bit w of every coefficient;
* the field count, ceil(8 B / w), is where the coefficients turn to zero;
* the lifted value of a field equals bfv_gpu_helpers.lift's rule under each prime, in both builds of the u64 engine (the codec itself does
  not depend on the form of the engine and is run in the Shoup build);
* tests/bfv_bytes_guard_main.cpp, a stand-alone program that includes bfv_bytes_core.h, puts each byte slab at the very end of a heap block
  whose size is rounded up to 8 and runs extraction and packing over the same grid: compiled with g++ -fsanitize=address,undefined and run
  as a child process, exit status 0.  That is what holds "no word past the one with the last valid byte is read";
* the library without a device: the four entry points exist and are declared, he355_bfv_bytes_per_plain gives (floor(N w / 8), w) and 0 for
  a CKKS context, and every refusal is decided on the host, before any device is asked for (valid arguments then fail with HE355_E_DEVICE).
No GPU."""
import ctypes as C
import importlib
import os
import subprocess
import types

import numpy as np
import pytest

import bfv_bytes_ref
import bfv_gpu_helpers
import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u64p = C.POINTER(C.c_uint64)
NS = [64, 1024]


def declare(L):
    L.sim_bfvbytes_max.argtypes = [C.c_uint64, C.c_int]
    L.sim_bfvbytes_max.restype = C.c_uint64
    L.sim_bfvbytes_fields.argtypes = [C.c_uint64, C.c_int]
    L.sim_bfvbytes_fields.restype = C.c_uint64
    L.sim_bfvbytes_words.argtypes = [C.c_uint64]
    L.sim_bfvbytes_words.restype = C.c_uint64
    L.sim_bfvbytes_unpack.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, u64p]
    L.sim_bfvbytes_unpack.restype = None
    L.sim_bfvbytes_pack_word.argtypes = [u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.sim_bfvbytes_pack_word.restype = C.c_uint64
    L.sim_bfvbytes_lift.argtypes = [C.c_uint64] * 3
    L.sim_bfvbytes_lift.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def sim():
    return declare(csim_lib.load(fold=False))


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def sizes(N, w):
    Bmax = N * w // 8
    return sorted({B for B in (1, 7, 8, 9, Bmax - 1, Bmax) if 1 <= B <= Bmax})


def py_fields(data, w, N):
    """coefficient e = (v >> (e w)) & (2^w - 1) of v = int.from_bytes(data, "little"), 64 fields per long shift"""
    v = int.from_bytes(data, "little")
    mask, out = (1 << w) - 1, []
    for e0 in range(0, N, 64):
        chunk = (v >> (e0 * w)) & ((1 << (64 * w)) - 1)
        out += [(chunk >> (i * w)) & mask for i in range(min(64, N - e0))]
    return out


def slab(rng, off, B):
    """(array, data, address): B random bytes `off` bytes into an 8-byte aligned slab, 0xFF before them and for 24 bytes after them"""
    raw = np.full(off + B + 24 + 8, 0xFF, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 8
    a = raw[skew:]
    assert a.ctypes.data % 8 == 0
    data = rng.integers(0, 256, B, dtype=np.uint8)
    data[B - 1] |= 0x80
    a[off:off + B] = data
    return raw, data.tobytes(), a.ctypes.data + off


def test_np_reference_against_python_integers():
    rng = np.random.default_rng(90)
    for w, N, B in ((19, 64, 152), (19, 64, 9), (16, 32, 63), (21, 32, 84), (63, 16, 126), (1, 64, 8)):
        data = rng.integers(0, 256, (2, B), dtype=np.uint8)
        got = bfv_bytes_ref.np_fields(data, w, N)
        for j in range(2):
            v = int.from_bytes(data[j].tobytes(), "little")
            assert [int(x) for x in got[j]] == [(v >> (e * w)) & ((1 << w) - 1) for e in range(N)], (w, N, B)


def test_py_reference_on_a_small_case():
    assert py_fields(bytes([0xAB, 0xCD, 0x0F]), 4, 8) == [0xB, 0xA, 0xD, 0xC, 0xF, 0, 0, 0]
    assert py_fields(bytes([0xFF, 0x01]), 3, 6) == [7, 7, 7, 0, 0, 0]


@pytest.mark.parametrize("N", NS)
def test_extraction_and_packing_against_python_integers(sim, N):
    rng = np.random.default_rng(811 + N)
    out = (C.c_uint64 * N)()
    for w in range(1, 64):
        Bmax = N * w // 8
        assert sim.sim_bfvbytes_max(N, w) == Bmax
        for B in sizes(N, w):
            fields = -(-8 * B // w)
            assert sim.sim_bfvbytes_fields(B, w) == fields and fields <= N
            W = -(-B // 8)
            assert sim.sim_bfvbytes_words(B) == W
            for off in range(8):
                what = (N, w, B, off)
                keep, data, addr = slab(rng, off, B)
                sim.sim_bfvbytes_unpack(C.c_void_p(addr), B, w, N, out)
                got = list(out)
                assert got == py_fields(data, w, N), what
                assert all(x == 0 for x in got[fields:]) and (B == 1 or got[fields - 1] != 0), what  # (the last byte's top bit is set)
                # the inverse, from clean coefficients and from words with junk above bit w
                junk = [int(x) | ((int(j) << w) & (2 ** 64 - 1)) for x, j in zip(got, rng.integers(0, 2 ** 63, N, dtype=np.uint64))]
                for coef in (got, junk):
                    arr = (C.c_uint64 * N)(*coef)
                    words = [sim.sim_bfvbytes_pack_word(arr, N, k, B, w) for k in range(W)]
                    packed = b"".join(int(x).to_bytes(8, "little") for x in words)
                    assert packed[:B] == data and packed[B:] == bytes(8 * W - B), what
                    masked = sum((c & ((1 << w) - 1)) << (e * w) for e, c in enumerate(coef)) & ((1 << (8 * B)) - 1)
                    assert int.from_bytes(packed, "little") == masked, what
                del keep


def test_packing_keeps_the_low_bits_of_a_coefficient_cut_by_the_last_byte(sim):
    """coefficients that say more than 8 B bits hold: the inverse keeps the low 8 B bits, whatever lies above"""
    N, rng = 64, np.random.default_rng(812)
    for w in (3, 19, 21, 63):
        for B in sizes(N, w):
            coef = [int(x) for x in rng.integers(0, 2 ** 64, N, dtype=np.uint64)]
            arr = (C.c_uint64 * N)(*coef)
            W = -(-B // 8)
            got = sum(sim.sim_bfvbytes_pack_word(arr, N, k, B, w) << (64 * k) for k in range(W))
            want = 0
            for e, c in enumerate(coef):
                want |= (c & ((1 << w) - 1)) << (e * w)
            assert got == want & ((1 << (8 * B)) - 1), (w, B)


@pytest.mark.parametrize("fold", [False, True], ids=["shoup", "fold"])
def test_centred_lift_of_fields(be, fold):
    L = declare(csim_lib.load(fold=fold))
    bits = [60, 40, 40, 60] if fold else [50, 40, 50]
    ctx = be.Context(be.SCHEME_BFV, 1024, bit_sizes=bits, plain_bits=20, sec128=False)
    moduli = [int(q) for q in ctx.moduli[:ctx.L]]
    ctx.close()
    for t in (2, 3, 65537, 786433, 1032193, 2 ** 20, 2 ** 20 - 1, 2 ** 22 - 3):
        w = t.bit_length() - 1
        half = (t + 1) // 2
        fields = np.array(sorted({v for v in (0, 1, half - 1, half, 2 ** w - 1, 2 ** w // 2) if 0 <= v < 2 ** w}), dtype=np.uint64)
        want = bfv_gpu_helpers.lift(types.SimpleNamespace(t=t, moduli=moduli), fields, len(moduli))
        for i, q in enumerate(moduli):
            assert [L.sim_bfvbytes_lift(int(f), t, q) for f in fields] == [int(x) for x in want[i]], (t, q)


def test_guard_program_under_the_address_sanitizer(tmp_path):
    exe = str(tmp_path / "bfv_bytes_guard")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mfma", "-ffp-contract=off", "-DHE355_U64_FOLD=0", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "bfv_bytes_guard_main.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bfv_bytes guard ok" in r.stdout


# ---- the library without a device ----------------------------------------------------------------------------------------------
NEW = ["he355_bfv_bytes_per_plain", "he355_bfv_unpack_bytes", "he355_bfv_unpack_bytes_ntt", "he355_bfv_pack_bytes"]
CHAINS = {"n1024": (1024, [50, 40, 50], 20), "n4096_d3": (4096, [60, 40, 40, 60], 20), "w16": (2048, [60, 40, 60], 17), "w21": (2048, [60, 40, 60], 22)}


@pytest.fixture(scope="module")
def newlib(be):
    lib = C.CDLL(be.LIB_PATH)
    for s in NEW:
        getattr(lib, s)  # AttributeError without the feature
    return be.lib()


def test_symbols_exported_and_declared(be, newlib):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
        assert hasattr(be.Context, s[len("he355_"):])


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_bytes_per_plain(be, newlib, chain):
    N, bits, pb = CHAINS[chain]
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    w = ctx.t.bit_length() - 1
    assert w == pb - 1 and ctx.bfv_bytes_per_plain() == (N * w // 8, w)
    assert newlib.he355_bfv_bytes_per_plain(ctx.h, None) == N * w // 8  # the width is optional
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    assert ck.bfv_bytes_per_plain() == (0, 0)
    ck.close()


def test_refusals_are_decided_on_the_host(be, newlib):
    N, L = 4096, newlib
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    Lt = ctx.L
    Bmax, w = ctx.bfv_bytes_per_plain()
    pl = np.full(2 * Lt * N + 2 * N, 0xABCD, dtype=np.uint64)
    by = np.full(2 * (Bmax + 16) // 8 + 2, 0xABCD, dtype=np.uint64)
    p, b = pl.ctypes.data_as(C.c_void_p), by.ctypes.data_as(C.c_void_p)
    assert b.value % 8 == 0 and p.value % 16 == 0
    S = (Bmax + 7) // 8 * 8
    at = lambda base, nbytes: C.c_void_p(base.value + nbytes)
    un = lambda n=2, src=b, stride=Bmax, B=Bmax, dst=p: L.he355_bfv_unpack_bytes(ctx.h, n, src, stride, B, dst)
    nt = lambda n=2, src=b, stride=Bmax, B=Bmax, dst=p, Lo=Lt: L.he355_bfv_unpack_bytes_ntt(ctx.h, Lo, n, src, stride, B, dst)
    pk = lambda n=2, src=p, stride=S, B=Bmax, dst=b: L.he355_bfv_pack_bytes(ctx.h, n, src, B, stride, dst)
    NMAX = (2 ** 31 - 1) // (N // 256)  # one launch's grid; the slabs of such a call are never touched here
    bad = []
    for f in (un, nt, pk):
        bad += [lambda f=f: f(B=0), lambda f=f: f(B=Bmax + 1), lambda f=f: f(B=9, stride=8), lambda f=f: f(n=NMAX + 1),
                lambda f=f: f(n=2 ** 40), lambda f=f: f(n=3, stride=2 ** 63), lambda f=f: f(stride=2 ** 63 - 8)]  # ((n - 1) stride wraps / reaches 2^63)
    bad += [lambda: nt(Lo=0), lambda: nt(Lo=Lt + 1), lambda: nt(Lo=-1)]
    bad += [lambda: un(dst=at(p, 8))]  # unpack stores two coefficients at once: a 16-byte aligned output
    bad += [lambda: pk(dst=at(b, 4)), lambda: pk(stride=S + 4), lambda: pk(B=9, stride=8), lambda: pk(B=9, stride=12)]
    # overlaps: the bytes inside the words, the words inside the bytes, the last byte / the first byte of the one on the other
    bad += [lambda: un(n=1, src=at(p, 8 * N - 1), B=1, stride=1), lambda: un(n=1, src=at(p, 3)), lambda: un(n=2, src=at(p, 8 * 2 * N - Bmax - 1), stride=Bmax, B=1),
            lambda: nt(n=1, src=at(p, 8 * Lt * N - 1), B=1, stride=1), lambda: pk(n=1, dst=at(p, 8 * N - 8), B=8, stride=8), lambda: pk(n=1, dst=p)]
    for k, f in enumerate(bad):
        assert f() == be.E_INVALID_ARGS, k
        assert len(L.he355_last_error()) > 0
    # valid arguments: there is no device behind this context, and no CPU fallback; the neighbours of every overlap edge are valid
    good = [un, nt, pk, lambda: un(n=NMAX, B=1, stride=1, src=at(p, 8 * NMAX * N)), lambda: un(src=at(b, 3), stride=Bmax + 5),
            lambda: un(n=1, src=at(p, 8 * N), B=1, stride=1), lambda: nt(n=1, src=at(p, 8 * Lt * N), B=1, stride=1),
            lambda: un(n=1, src=at(p, 8 * N + 5), B=3, stride=3),
            lambda: pk(n=1, dst=at(p, 8 * N), B=8, stride=8), lambda: pk(B=9, stride=16), lambda: nt(Lo=1)]
    for k, f in enumerate(good):
        assert f() == be.E_DEVICE, (k, L.he355_last_error())
        assert b"no CPU fallback" in L.he355_last_error()
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False)
    for f in (lambda: L.he355_bfv_unpack_bytes(ck.h, 1, b, Bmax, Bmax, p), lambda: L.he355_bfv_unpack_bytes_ntt(ck.h, 1, 1, b, Bmax, Bmax, p),
              lambda: L.he355_bfv_pack_bytes(ck.h, 1, p, Bmax, S, b)):
        assert f() == be.E_INVALID_ARGS
        assert b"BFV context" in L.he355_last_error()
    ck.close()
    assert (pl == 0xABCD).all() and (by == 0xABCD).all()
