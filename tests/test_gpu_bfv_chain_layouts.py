"""The BFV PIR calls on chains whose engine layout no other module reaches, bit-exact (np.array_equal, no tolerance) against references that
use no device (bfv_ring_ref.py, bfv_gadget_ref.py, bfv_selector_ref.py, bfv_select_ref.py, bfv_expand_ref.py, bfv_merge_ref.py,
bfv_reply_ref.py; held to Python integers on the N = 1024 versions of these chains in test_bfv_ring_ref_cpu.py).  Every other PIR module runs
chains of ONE shape: prime 0 and the key prime in the u64 engine, every other data prime a 40-bit fp64 prime, the u64 form fold with 60-bit
primes or Shoup with 50-bit ones.  The kernels branch on the engine per output prime inside their digit loops, and index the gadget tables
(off_i, E_i) per source prime; here those run on (plain_bits 20 everywhere):

    f64_first       (2048, {40, 60, 60})      fp64 prime 0, a u64 last data prime; fold form.  Reply: top width 28, the safe pair refused
    u64_only        (2048, {60, 60, 60})      no fp64 prime: a u64 digit under another u64 prime, the 256-term run on every prime; fold form
    f64_only        (2048, {42, 38, 45, 44})  no u64 prime at all, the key prime included; L = 3.  Reply: top width 30, the safe pair refused
    shoup_60        (2048, {60, 50, 40, 60})  60-bit primes in the Shoup form (one 50-bit prime selects it), a u64 prime in the middle
    f64_first_1024  (1024, {45, 55, 50})      the ring without a column pass (streaming cuts, the routed digits / bytes / tail), fp64 prime 0

N = 2048 (LOGN1 = 1) is the smallest ring with a column pass; test_gpu_bfv_large_rings.py owns LOGN1 >= 3.  The engines are asserted by the
prime-size rule (below 2^47: fp64) and the form by the rule of he_params.cpp (fold iff every chain prime >= 2^47 is 2^60 - c, c < 2^26).

Operands are `edged` (all-0, all-(q - 1), alternating rows among uniform ones) and, for the gadget cuts, one PLANTED ciphertext: for every
ordered pair of data primes q_j < q_i residue i holds q_j - 1, q_j, q_j + 1, q_i - 1 at four neighbouring columns of each of its N / 1024
column-source groups (columns 0..3 for the first such j, 1020..1023 for the second), so that with v = 63 (the digit is the residue) the
d >= q_j reduction of a digit under another prime runs on both sides of its edge in prime j's engine.  Every output lies between a ring's worth
of sentinel words, every operand is read back, and he355_bfv_route_stats is reset before each call and asserted after it (printed:
`routes <layout> <case>`).  A mismatch names (layout, call, output prime j, source prime i, digit g).  The thresholds the shapes come from:
the column pass from n size L >= 64 residue polynomials (256 blocks), own_cols from slots L >= 32, a pool block of 4096 digit polynomials.
Lt = the chain's data level.

 1. gadget_decompose_ntt, v in {20, 45, 63}, sizes 2 and 3, the planted ciphertext in every batch: at the threshold (64: cut_cols), above it
    (66 / 72), one short of it (63: cut_stream) and 60; at N = 1024 the streaming cut.  gadget_decompose (coefficient form) once per layout.
 2. decompose_ntt at (L, L_out) in {(Lt, Lt), (1, Lt), (Lt, 1)}, sizes 2 and 3, n = 3: digits_fused / digits_routed; decompose then compose
    gives the ciphertext back.
 3. unpack_bytes_ntt: 3 records from byte 5 at stride B + 3, the first all 0, the last all 0xFF, L_out in {Lt, 1}: bytes_fused / bytes_routed.
 4. external_product, v = 20, L = Lt, every result: (a) n = 4 above the column threshold, a selector row per result; (b) child-major with one
    shared row; (c) 3 x 3 streaming; (d) ONE result over enough contiguous rows for the column pass (mac_plain); (e) one result, inner = 3.
    u64_only: L = 2, v = 4, n = 2, inner = 5 -- 300 terms, above the 256-term run of BOTH primes, one pass, against the reference and the
    composition on the device.  shoup_60: L = 3, v = 4, inner = 4 -- 304 terms, above the 60-bit prime's run only (the others: 2^16).
 5. rgsw_from_bfv, (v, key_bits) = (20, 20) and (63, 4), a uniform key: slots above the own_cols threshold (unit strides, and child-major
    behind two leading children) and below it.
 6. selector_encrypt, rgsw_encrypt and rgsw_encrypt_secret against encrypt_zero plus the numpy plant (k_bfv_secret_plain and the plant
    kernels with q_0 on each engine).
 7. select, counts 4 and 3 (a node without a partner: k_bfv_select_copy), n above and below the column threshold, per-result and shared
    selectors, against the fold of external_product_ref over bfv_select_ref's level table.
 8. expand and merge, count = 4, n = 2, L = Lt, keys from oracle.keygen_galois (f64_only: an fp64 key prime); he355_path_stats printed.
 9. reply_compress against np_compress: widths (2, 2), (top, top) and the safe pair where accepted; at L = 1 and from Lt against to_level.
10. reply_decrypt: random bytes, all ones, all zeros; the oracle's key and the constant keys +1, -1; with and without budget outputs.
11. f64_first, f64_only: the safe widths are refused by compress and decrypt, outputs untouched; bfv_reply_bytes of them is 0.

Four further layouts take their moduli from tests/golden/explicit_moduli.json (tests/explicit_moduli.py), not from the prime-size rule, and
their plain modulus with them; the cases above run on them unchanged, and the asserts that pin bit lengths and a 20-bit t are replaced by the
fixture's own primes and t:

    aux46               t = 256       the two largest 46-bit primes as data primes: the device's auxiliary base has to leave them out
    shoup_by_one_low60  t = 2^32 - 5  the Shoup form by one prime 2^59 + (small), whose 128-bit sums take 1023 terms; a 31-bit byte field
    mac_337             t = 2^16      prime 0 near 2^59.8: 337-term runs, no power of two; t a power of two (w = 16)
    tiny                batching t    {60, 14, 16, 31}-bit data primes, L = 4, a 32-bit batching t above three of its primes

In case 4 the over-the-run shapes are sized so that the 337-term and the 1023-term prime fold inside a result: mac_337 L = 2, v = 4,
inner = 7 (350 terms); shoup_by_one_low60 L = 3, v = 4, inner = 12 (1080 terms, above all three runs, the cut through the column pass).
12. tiny: bfv_seeded_encrypt and bfv_seeded_restore against tests/bfv_seeded_ref.py (a 14-bit prime under the uniform sampler's limit).

n16384_shoup is shoup_60 at N = 16384 (LOGN1 = 4; tests/shoup_rings.py): every case above once in the Shoup build's instantiations of
the large ring, the planted ciphertext included.

Not run: the other layouts at N >= 8192, and two passes through the pool block on them."""

import numpy as np
import pytest

import bfv_gadget_ref as gad
import bfv_seeded_ref as seeded
import explicit_moduli as xm
import bfv_reply_ref as rep
import bfv_ring_ref as ring
import bfv_select_ref as tree
import bfv_selector_ref as sel
import shoup_rings as shoup
from bfv_expand_ref import children, expand_levels
from bfv_gpu_helpers import SENT, At, be, edged, ep_composition, expand_keys, inner_of, pair, rand_cts, refused, sentinelled, to_level  # noqa: F401 (be: the fixture)
from bfv_merge_ref import merge_levels

pytestmark = pytest.mark.gpu

# id -> (N, bit sizes, plain bits), the form of the u64 engine, the largest accepted reply width, whether the safe pair is accepted
LAYOUTS = {
    "f64_first": ((2048, [40, 60, 60], 20), "fold", 28, False),
    "u64_only": ((2048, [60, 60, 60], 20), "fold", 48, True),
    "f64_only": ((2048, [42, 38, 45, 44], 20), None, 30, False),
    "shoup_60": ((2048, [60, 50, 40, 60], 20), "shoup", 48, True),
    "f64_first_1024": ((1024, [45, 55, 50], 20), "shoup", 34, True),
    # shoup_60 at LOGN1 = 4 (tests/shoup_rings.py): every call of this module once in the Shoup build's N = 16384 instantiations
    "n16384_shoup": (shoup.spec("n16384_60_50_40_60_shoup"), "shoup", 45, True),
}
SHOUP_RINGS = {"n16384_shoup": "n16384_60_50_40_60_shoup"}  # layout: its entry of shoup_rings.RINGS
# the layouts of explicit moduli: ((N, primes, t), form, top width, safe pair accepted) -- the last two by bfv_reply_ref's own rule
EXPLICIT = {"aux46": "aux46_t256", "shoup_by_one_low60": "shoup_by_one_low60_t4294967291", "mac_337": "mac_337_t65536", "tiny": None}
_FIX = xm.load()
for _cid, _fid in EXPLICIT.items():
    if _fid is None:
        _fid = next(k for k, c in _FIX.items() if c.get("chain") == _cid and c.get("batching") and c["N"] == 2048)
        EXPLICIT[_cid] = _fid
    _c = _FIX[_fid]
    assert _c["N"] == 2048
    LAYOUTS[_cid] = ((_c["N"], _c["primes"], _c["t"]), xm.form_of(_c["primes"]), rep.max_width(_c["N"], _c["primes"][0]),
                     rep.accepted(_c["N"], _c["primes"][0], *rep.safe_bits(_c["N"], _c["t"])))
assert [LAYOUTS[k][0][2] for k in EXPLICIT] == [256, 2 ** 32 - 5, 2 ** 16, _FIX[EXPLICIT["tiny"]]["t"]] and (LAYOUTS["tiny"][0][2] - 1) % 4096 == 0
assert [LAYOUTS[k][1] for k in EXPLICIT] == ["fold", "shoup", "shoup", "fold"]
IDS = list(LAYOUTS)
V = 20
PAD = 24  # bytes between two replies


def form_of(moduli):
    """the rule of he_params.cpp over the whole chain, the key prime included; None where no prime belongs to the u64 engine"""
    wide = [q for q in moduli if q >= 2 ** 47]
    if not wide:
        return None
    return "fold" if all(0 < 2 ** 60 - q < 2 ** 26 for q in wide) else "shoup"


_PAIRS = {}


def layout_pair(be, oracle, cid):
    """(g, o, N, sk, pk) of one layout, made once for the module"""
    if cid not in _PAIRS:
        chain, form, top, safe = LAYOUTS[cid]
        g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
        if cid in EXPLICIT:
            assert o.moduli == g.moduli == chain[1] == _FIX[EXPLICIT[cid]]["primes"] and o.t == g.t == chain[2] and g.L == len(chain[1]) - 1
            assert g.fp64 == [xm.is_f64(q) for q in chain[1]], "the engines, by the prime itself"
            assert set(g.bfv_aux_base()).isdisjoint(chain[1])
        else:
            assert [q.bit_length() for q in o.moduli] == chain[1] and g.L == len(chain[1]) - 1 and o.t.bit_length() == 20
            assert [q < 2 ** 47 for q in o.moduli] == [b < 47 for b in chain[1]], "the engines, by the prime-size rule"
        assert form_of(o.moduli) == form
        if cid in SHOUP_RINGS:
            shoup.check_device(SHOUP_RINGS[cid], g)
            shoup.check(SHOUP_RINGS[cid], o.moduli, g.t)
        q0 = int(o.moduli[0])
        assert rep.max_width(N, q0) == top and rep.accepted(N, q0, *rep.safe_bits(N, o.t)) == safe
        _PAIRS[cid] = (g, o, N, sk, pk)
    return _PAIRS[cid]


def begin(g):
    g.bfv_route_stats(reset=True)


def routed(g, cid, case, want):
    """the counters since begin(), printed, and nothing but `want` counted"""
    got = {k: c for k, c in g.bfv_route_stats().items() if c}
    print(f"routes {cid} {case}: " + ", ".join(f"{k} = {c}" for k, c in got.items()))
    assert got == want, (cid, case, got)


def same(got, want, cid, call, what, moduli=None, v=None):
    """np.array_equal, and where it fails the first differing word by name: arrays [..][L][N], axis -2 the output prime j; with (moduli, v)
    axis -3 is a digit polynomial k E + off_i + g of the width-v table"""
    assert got.shape == want.shape, (cid, call, what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    at = tuple(int(a) for a in np.argwhere(got != want)[0])
    msg = f"layout {cid}, {call}, {what}: {int((got != want).sum())} words differ, first at {at}: output prime j = {at[-2]}"
    if moduli is not None:
        E, off = gad.table(moduli, v)
        f = at[-3] % off[-1]
        i = max(i for i in range(len(moduli)) if off[i] <= f)
        msg += f", polynomial k = {at[-3] // off[-1]}, source prime i = {i}, digit g = {f - off[i]} (v = {v})"
    pytest.fail(msg + f": got {int(got[at])}, want {int(want[at])}")


def planted(o, rng, L, size, N):
    """[size][L][N]: uniform, and for every ordered pair q_j < q_i of the first L primes residue i holds q_j - 1, q_j, q_j + 1, q_i - 1 at four
    neighbouring columns of each group of 1024 coefficients: columns 0..3 for the first j, 1020..1023 for the second, 512..515 for a third"""
    c = o.random_poly(rng, L, size)
    qs = [int(q) for q in o.moduli[:L]]
    pairs = 0
    for i, qi in enumerate(qs):
        below = [qj for qj in qs if qj < qi]
        assert len(below) <= 3
        for p, qj in enumerate(below):
            assert qj + 1 < qi
            for grp in range(N // 1024):
                at = grp * 1024 + (0, 1020, 512)[p]
                c[:, i, at:at + 4] = np.array([qj - 1, qj, qj + 1, qi - 1], dtype=np.uint64)
            pairs += 1
    assert pairs == L * (L - 1) // 2
    return c


def batch(o, rng, n, L, size, N):
    """n edged ciphertexts, the planted one at index 2 (edged writes 0, 1 and n - 1)"""
    assert n >= 4
    x = edged(o, rng, n, L, size)
    x[2] = planted(o, rng, L, size, N)
    return x


# ---- 1. he355_bfv_gadget_decompose_ntt, he355_bfv_gadget_decompose -------------------------------------------------------------------------
def gadget_shapes(N, Lt):
    """(L, size, n, counter)"""
    if N == 1024:
        return [(Lt, 2, 4, "cut_stream"), (Lt, 3, 4, "cut_stream"), (1, 2, 4, "cut_stream"), (Lt, 2, 16, "cut_stream")]
    if Lt == 2:
        return [(2, 2, 16, "cut_cols"), (2, 3, 11, "cut_cols"), (1, 3, 21, "cut_stream"), (2, 3, 10, "cut_stream")]
    return [(2, 2, 16, "cut_cols"), (3, 2, 11, "cut_cols"), (3, 3, 8, "cut_cols"), (3, 3, 7, "cut_stream")]


@pytest.mark.parametrize("v", [20, 45, 63])
@pytest.mark.parametrize("cid", IDS)
def test_gadget_decompose_ntt(be, oracle, cid, v):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(503 + v)
    shapes = gadget_shapes(N, g.L)
    if N > 1024:
        sizes = sorted(n * size * L for L, size, n, _ in shapes)
        assert 64 in sizes and 63 in sizes and {2, 3} == {s for _, s, _, c in shapes if c == "cut_cols"}
    for L, size, n, counter in shapes:
        assert (N > 1024 and n * size * L >= 64) == (counter == "cut_cols")
        what = f"v = {v}, L = {L}, size = {size}, n = {n}"
        total, per = g.bfv_gadget_count(L, v)
        assert (per, total) == (gad.table(o.moduli[:L], v)[0], gad.table(o.moduli[:L], v)[1][-1])
        F = size * total
        x = batch(o, rng, n, L, size, N)
        dx = g.to_device(x)
        buf = sentinelled(g, n * F * L * N, N)
        begin(g)
        g.bfv_gadget_decompose_ntt(L, v, size, n, dx, At(buf, N))
        got = inner_of(buf, N, what).reshape(n, F, L, N)
        routed(g, cid, f"gadget_decompose_ntt {what}", {counter: 1})
        same(got, ring.gadget_ntt_ref(o, x, v), cid, "gadget_decompose_ntt", what, o.moduli[:L], v)
        assert np.array_equal(dx.download(x.shape), x), (cid, what, "input")
        dx.free()
        buf.free()


@pytest.mark.parametrize("cid", IDS)
def test_gadget_decompose_coefficient_form(be, oracle, cid):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(504)
    L, n = g.L, 4
    for v, size in ((20, 2), (63, 3), (45, 2)):
        what = f"v = {v}, size = {size}"
        F = size * g.bfv_gadget_count(L, v)[0]
        x = batch(o, rng, n, L, size, N)
        dx = g.to_device(x)
        buf = sentinelled(g, n * F * N, N)
        begin(g)
        g.bfv_gadget_decompose(L, v, size, n, dx, At(buf, N))
        got = inner_of(buf, N, what).reshape(n, F, N)
        routed(g, cid, f"gadget_decompose {what}", {})
        assert np.array_equal(got, gad.np_digits(x, o.moduli, v)), (cid, "gadget_decompose", what)
        assert np.array_equal(dx.download(x.shape), x), (cid, what, "input")
        dx.free()
        buf.free()


# ---- 2. he355_bfv_decompose_ntt, he355_bfv_decompose / he355_bfv_compose -----------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_decompose_ntt(be, oracle, cid):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(501)
    Lt, n = g.L, 3
    w = o.t.bit_length() - 1
    counter = "digits_fused" if N > 1024 else "digits_routed"
    for L, L_out in ((Lt, Lt), (1, Lt), (Lt, 1)):
        total = g.bfv_digit_count(L)[0]
        assert total == gad.table(o.moduli[:L], w)[1][-1]
        for size in (2, 3):
            what = f"L = {L}, L_out = {L_out}, size = {size}"
            F = size * total
            x = edged(o, rng, n, L, size)
            dx = g.to_device(x)
            buf = sentinelled(g, n * F * L_out * N, N)
            begin(g)
            g.bfv_decompose_ntt(L, size, n, dx, L_out, At(buf, N))
            got = inner_of(buf, N, what).reshape(n, F, L_out, N)
            routed(g, cid, f"decompose_ntt {what}", {counter: 1})
            same(got, ring.decompose_ntt_ref(o, x, L_out), cid, "decompose_ntt", what, o.moduli[:L], w)
            assert np.array_equal(dx.download(x.shape), x), (cid, what, "input")
            buf.free()
            if L_out == Lt:  # the streaming pair: the digits mod t, and back
                dig, back = sentinelled(g, n * F * N, N), sentinelled(g, n * size * L * N, N)
                begin(g)
                g.bfv_decompose(L, size, n, dx, At(dig, N))
                g.bfv_compose(L, size, n, At(dig, N), At(back, N))
                routed(g, cid, f"decompose + compose {what}", {})
                assert np.array_equal(inner_of(dig, N, what).reshape(n, F, N), gad.np_digits(x, o.moduli, w)), (cid, "decompose", what)
                same(inner_of(back, N, what).reshape(x.shape), x, cid, "compose", what)
                dig.free()
                back.free()
            dx.free()


# ---- 3. he355_bfv_unpack_bytes_ntt ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_unpack_bytes_ntt(be, oracle, cid):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(502)
    n, base = 3, 5
    B, w = g.bfv_bytes_per_plain()
    assert w == o.t.bit_length() - 1 and B == N * w // 8
    stride = B + 3
    data = rng.integers(0, 256, (n, B), dtype=np.uint8)
    data[0], data[n - 1] = 0, 0xFF
    img = np.full((base + (n - 1) * stride + B + 16 + 7) // 8 * 8, 0xA5, dtype=np.uint8)  # the filler before, between and after
    for j in range(n):
        img[base + j * stride: base + j * stride + B] = data[j]
    src = g.to_device(img.view(np.uint64))
    counter = "bytes_fused" if N > 1024 else "bytes_routed"
    for L_out in (g.L, 1):
        buf = sentinelled(g, n * L_out * N, N)
        begin(g)
        g.bfv_unpack_bytes_ntt(L_out, n, src, base, stride, B, At(buf, N))
        got = inner_of(buf, N, L_out).reshape(n, L_out, N)
        routed(g, cid, f"unpack_bytes_ntt L_out = {L_out}", {counter: 1})
        same(got, ring.unpack_bytes_ntt_ref(o, data, L_out), cid, "unpack_bytes_ntt", f"L_out = {L_out}")
        buf.free()
    assert np.array_equal(src.download().view(np.uint8), img), (cid, "input")
    src.free()


# ---- 4. he355_bfv_external_product ---------------------------------------------------------------------------------------------------------
def ep_case(g, o, rng, cid, L, v, n, inner, shared, child_major, N, case, want, composed=False):
    """one call, every result against external_product_ref; composed: against the composition on the device as well"""
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    n_rg = inner if shared else n * inner
    rg = g.alloc(n_rg * rows * per)
    g.fill_uniform(rg, n_rg * rows * 2 * L, list(range(L)), 5000 + n * 10 + inner)
    rg_h = rg.download((n_rg, rows, 2, L, N))
    x = edged(o, rng, n * inner, L)
    dx = g.to_device(x)
    sr, sk = (1, n) if child_major else (inner, 1)
    gr = 0 if shared else inner
    buf = sentinelled(g, n * per, N)
    begin(g)
    g.bfv_external_product(L, v, n, inner, dx, sr, sk, rg, gr, 1, At(buf, N))
    got = inner_of(buf, N, case).reshape(n, 2, L, N)
    routed(g, cid, f"external_product {case}", want)
    digits = ring.gadget_ntt_ref(o, x, v)  # the digits of every ciphertext once
    for r in range(n):
        at = [r * sr + k * sk for k in range(inner)]
        rows_r = rg_h[:inner] if shared else rg_h[r * inner:(r + 1) * inner]
        same(got[r], ring.external_product_ref(o, x[at], rows_r, v, digits[at]), cid, "external_product", f"{case}, result {r}")
    if composed:
        comp = ep_composition(g, L, v, n, inner, x, lambda r, k: r * sr + k * sk, rg, gr, rows, N)
        same(got, comp, cid, "external_product", f"{case}, the composition")
    assert np.array_equal(dx.download(x.shape), x), (cid, case, "ciphertexts")
    assert np.array_equal(rg.download(rg_h.shape), rg_h), (cid, case, "RGSW")
    for b in (rg, dx, buf):
        b.free()


@pytest.mark.parametrize("cid", IDS)
def test_external_product_many_results(be, oracle, cid):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(505)
    L = g.L
    inner = {4: 2, 3: 3, 2: 4}[L]
    n_c = 3 if L < 4 else 2  # (c): 3 x 3 below four data primes, as ever; 2 x 3 at four
    assert 4 * inner * L >= 32 > n_c * 3 * L  # 4 x inner x 2 x L x 4 blocks reach the column pass, (c) does not
    cut = "cut_cols" if N > 1024 else "cut_stream"
    cols, stream = {cut: 1, "mac_gadget": 1, "passes": 1}, {"cut_stream": 1, "mac_gadget": 1, "passes": 1}
    ep_case(g, o, rng, cid, L, V, 4, inner, False, False, N, f"(a) n = 4, inner = {inner}, a selector row per result", cols)
    ep_case(g, o, rng, cid, L, V, 4, inner, True, True, N, f"(b) n = 4, inner = {inner}, child-major, one selector row", cols)
    ep_case(g, o, rng, cid, L, V, n_c, 3, False, False, N, f"(c) n = {n_c}, inner = 3", stream)


@pytest.mark.parametrize("cid", IDS)
def test_external_product_one_result(be, oracle, cid):
    """n = 1 over contiguous rows is k_bfv_plain_mac's; with inner L >= 32 the cut before it is the column pass"""
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(506)
    L = g.L
    inner = {4: 8, 3: 11, 2: 16}[L]
    assert inner * L >= 32 > (inner - 1) * L and 3 * L < 32
    cut = "cut_cols" if N > 1024 else "cut_stream"
    ep_case(g, o, rng, cid, L, V, 1, inner, False, False, N, f"(d) n = 1, inner = {inner}", {cut: 1, "mac_plain": 1, "passes": 1})
    ep_case(g, o, rng, cid, L, V, 1, 3, False, False, N, "(e) n = 1, inner = 3", {"cut_stream": 1, "mac_plain": 1, "passes": 1})


def mac_run(q):
    """the terms a 128-bit accumulator holds under q, capped as bfv_mac_core.h caps them"""
    return min(2 ** 16, (2 ** 128 - 1) // (q - 1) ** 2)


@pytest.mark.parametrize("cid,L,inner,over", [("u64_only", 2, 5, (256, 256)), ("shoup_60", 3, 4, (256, None, None)),
                                              ("mac_337", 2, 7, (337, None)), ("shoup_by_one_low60", 3, 12, (256, 256, 1023))])
def test_external_product_more_terms_than_a_run(be, oracle, cid, L, inner, over):
    """v = 4, n = 2.  u64_only: 2E = 2 (15 + 15) = 60 rows, inner = 5 is 300 terms, above the 256-term run of BOTH 60-bit primes (a fold
    inside every result, under every prime).  shoup_60: 2E = 2 (15 + 13 + 10) = 76 rows, inner = 4 is 304 terms, above the run of the 60-bit
    prime alone -- the 50- and 40-bit primes' runs are capped at 2^16.  mac_337: 2E = 2 (15 + 10) = 50 rows, inner = 7 is 350 terms, above the 337
    terms of prime 0 (the 40-bit prime: 2^16).  shoup_by_one_low60: 2E = 90 rows, inner = 12 is 1080 terms, above the 1023 terms of the prime
    2^59 + (small) and four runs of the other two; its 72 residue polynomials take the column cut.  over: the run of each prime that folds
    inside a result.  One pass through the pool block each"""
    g, o, N, *_ = layout_pair(be, oracle, cid)
    v, n = 4, 2
    assert g.L == L
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    terms = inner * rows
    assert rows == 2 * sum(-(-q.bit_length() // v) for q in o.moduli[:L])
    assert terms == {"u64_only": 300, "shoup_60": 304, "mac_337": 350, "shoup_by_one_low60": 1080}[cid]
    for j, q in enumerate(o.moduli[:L]):
        if over[j]:
            assert q.bit_length() == 60 and terms > (2 ** 128 - 1) // (q - 1) ** 2 == over[j] == mac_run(q), j
        else:
            assert q.bit_length() < 60 and mac_run(q) == 2 ** 16 > terms, j
    assert 4096 // terms >= n  # one pass
    if cid in EXPLICIT and n * inner * L >= 32:
        cut = "cut_cols"
    else:
        assert n * inner * L < 32  # the streaming cut
        cut = "cut_stream"
    ep_case(g, o, np.random.default_rng(507), cid, L, v, n, inner, False, False, N, f"L = {L}, v = 4, n = 2, inner = {inner}: {terms} terms",
            {cut: 1, "mac_gadget": 1, "passes": 1}, composed=True)


# ---- 5. he355_bfv_rgsw_from_bfv ------------------------------------------------------------------------------------------------------------
def from_bfv_call(g, o, cid, L, v, kv, n, n_sel, dx, x, lead, child_major, key, refs, N, case, want):
    """one call on the slab x (already on the device); refs(c) = (row k = 0, row k = 1) of slab entry c by the oracle, made once"""
    E = g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    S = n_sel * E
    if child_major:  # the strides of an expansion: d_ct points behind `lead` leading children
        sr, sk, order = 1, n, [(lead + s) * n + r for r in range(n) for s in range(S)]
    else:
        sr, sk, order, lead = S, 1, list(range(n * S)), 0
    buf = sentinelled(g, n * n_sel * 2 * E * per, N)
    begin(g)
    g.bfv_rgsw_from_bfv(L, v, kv, n, n_sel, At(dx, lead * n * per), sr, sk, key, At(buf, N))
    got = inner_of(buf, N, case).reshape(n * n_sel, 2 * E, 2, L, N)
    routed(g, cid, f"rgsw_from_bfv {case}", want)
    k0, k1 = zip(*(refs(c) for c in order))
    same(got, sel.np_rows(np.stack(k0), np.stack(k1), E), cid, "rgsw_from_bfv", f"{case} (axis 1: row k E + f of [RGSW][2E][2][L][N])")
    assert np.array_equal(dx.download(x.shape), x), (cid, case, "ciphertexts")
    buf.free()


@pytest.mark.parametrize("v,kv", [(20, 20), (63, 4)])
@pytest.mark.parametrize("cid", IDS)
def test_rgsw_from_bfv(be, oracle, cid, v, kv):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(508 + v)
    L, lead, n = g.L, 2, 2
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    assert E == gad.table(o.moduli[:L], v)[1][-1] and rows == 2 * gad.table(o.moduli[:L], kv)[1][-1]
    n_sel = -(-32 // (n * E * L))
    S = n_sel * E
    assert n * S * L >= 32 > E * L and n * (S - E) * L < 32 and 4096 // rows >= n * S  # slots x 2 L x 4 blocks: the column pass from 256 on; one pass
    key = g.alloc(rows * 2 * L * N)
    g.fill_uniform(key, rows * 2 * L, list(range(L)), 6000 + v)
    key_h = key.download((rows, 2, L, N))
    x = edged(o, rng, (lead + S) * n, L)
    dx = g.to_device(x)
    memo = {}

    def refs(c):
        if c not in memo:
            memo[c] = ring.rgsw_from_bfv_rows(o, x[c], key_h, kv)
        return memo[c]

    above = {"own_cols" if N > 1024 else "own_stream": 1, "passes": 1}
    what = f"(v, key_bits) = ({v}, {kv})"
    from_bfv_call(g, o, cid, L, v, kv, n, n_sel, dx, x, lead, False, key, refs, N, f"{what}, n = {n}, n_sel = {n_sel}", above)
    from_bfv_call(g, o, cid, L, v, kv, n, n_sel, dx, x, lead, True, key, refs, N, f"{what}, n = {n}, n_sel = {n_sel}, child-major behind {lead} children", above)
    from_bfv_call(g, o, cid, L, v, kv, 1, 1, dx, x, lead, False, key, refs, N, f"{what}, n = 1, n_sel = 1", {"own_stream": 1, "passes": 1})
    assert np.array_equal(key.download(key_h.shape), key_h), (cid, "key")
    key.free()
    dx.free()


# ---- 6. he355_bfv_selector_encrypt, he355_bfv_rgsw_encrypt, he355_bfv_rgsw_encrypt_secret --------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_selector_encrypt(be, oracle, cid):
    g, o, N, sk, pk = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(509)
    t, L, n, seed, first = o.t, g.L, 2, 111, 9
    zero = g.alloc(n * 2 * L * N)
    g.encrypt_zero(n, seed, first, zero)
    z = zero.download((n, 2, L, N))
    zero.free()
    for v, n_sel, first_slot in ((20, 2, 5), (63, 3, 0)):
        E = g.bfv_gadget_count(L, v)[0]
        for count in (first_slot + n_sel * E, N):
            what = f"v = {v}, n_sel = {n_sel}, first_slot = {first_slot}, count = {count}"
            sels = rng.integers(0, t, (n, n_sel), dtype=np.uint64)
            sels[0, 0], sels[1, n_sel - 1], sels[1, 0] = t - 1, (t + 1) // 2, 1
            ds = g.to_device(sels)
            buf = sentinelled(g, n * 2 * L * N, N)
            begin(g)
            g.bfv_selector_encrypt(L, v, n, n_sel, first_slot, count, ds, seed, first, At(buf, N))
            got = inner_of(buf, N, what).reshape(n, 2, L, N)
            routed(g, cid, f"selector_encrypt {what}", {})
            same(got, sel.np_pack(z, sels, o.moduli, t, v, first_slot, count), cid, "selector_encrypt", what)
            assert np.array_equal(ds.download((n, n_sel)), sels), (cid, what, "selectors")
            ds.free()
            buf.free()


@pytest.mark.parametrize("cid", IDS)
def test_rgsw_encrypt_and_rgsw_encrypt_secret(be, oracle, cid):
    g, o, N, sk, pk = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(510)
    t, L, v, seed, first = o.t, g.L, V, 97, 7
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    q0 = int(o.moduli[0])
    s = o.intt(0, np.ascontiguousarray(np.asarray(sk, dtype=np.uint64).reshape(-1, N)[0]))  # the key's coefficients under prime 0: 0, 1, q_0 - 1
    assert set(np.unique(s).tolist()) == {0, 1, q0 - 1}
    m = rng.integers(0, t, (3, N), dtype=np.uint64)
    m[0, :4] = [t // 2, (t + 1) // 2, t - 1, 0]
    m[1] = 0
    m[1, N - 1] = t - 1
    m[2] = np.where(s == np.uint64(q0 - 1), np.uint64(t - 1), s)  # s mod t
    n = 3
    zero = g.alloc(n * rows * 2 * L * N)
    g.encrypt_zero(n * rows, seed, first, zero)
    z = zero.download((n, rows, 2, L, N))
    zero.free()
    want = np.stack([ring.ntt_all(o, gad.np_plant(z[r], m[r], o.moduli, t, v)) for r in range(n)])
    dm = g.to_device(m)
    buf = sentinelled(g, n * rows * 2 * L * N, N)
    begin(g)
    g.bfv_rgsw_encrypt(L, v, n, dm, seed, first, At(buf, N))
    got = inner_of(buf, N, "rgsw_encrypt").reshape(want.shape)
    routed(g, cid, "rgsw_encrypt", {})
    same(got, want, cid, "rgsw_encrypt", f"v = {v}, n = {n} (axis 1: row k E + off_i + g)")
    assert np.array_equal(dm.download(m.shape), m), (cid, "plaintexts")
    dm.free()
    buf.free()
    # RGSW(s): row f is encrypt_zero(seed, first + f), so it equals RGSW number 0 of a batch planted with s mod t at the same indices
    one = ring.ntt_all(o, gad.np_plant(z[0], m[2], o.moduli, t, v))
    buf = sentinelled(g, rows * 2 * L * N, N)
    begin(g)
    g.bfv_rgsw_encrypt_secret(L, v, seed, first, At(buf, N))
    got = inner_of(buf, N, "rgsw_encrypt_secret").reshape(one.shape)
    routed(g, cid, "rgsw_encrypt_secret", {})
    same(got, one, cid, "rgsw_encrypt_secret", f"key_bits = {v} (axis 0: row k E + off_i + g)")
    buf.free()


# ---- 7. he355_bfv_select -------------------------------------------------------------------------------------------------------------------
def select_ref(o, leaves, rg, v):
    """one result: leaves [count][2][L][N], rg [depth][2E][2][L][N] -> [2][L][N]; level j: node' = even + RGSW_j [.] (odd - even)"""
    nodes = list(leaves)
    table = tree.level_table(len(nodes))
    for j in range(len(table) - 1):
        assert len(nodes) == table[j]
        nxt = []
        for p in range(table[j] // 2):
            even, odd = nodes[2 * p], nodes[2 * p + 1]
            nxt.append(o.add(even, ring.external_product_ref(o, o.sub(odd, even)[None], rg[j][None], v)))
        if table[j] & 1:
            nxt.append(nodes[-1])
        nodes = nxt
    assert len(nodes) == 1
    return nodes[0]


@pytest.mark.parametrize("cid", IDS)
def test_select(be, oracle, cid):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(511)
    L, v = g.L, V
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    hi4, hi3 = -(-32 // (2 * L)), -(-32 // L)  # count 4: 2 n pairs at level 0; count 3: n pairs
    assert hi4 * 2 * L >= 32 > hi4 * L and hi3 * L >= 32 > 4 * L  # pairs x 2 L x 4 blocks: the column pass from 256 on
    # (count, n, one set of selectors, levels that take the column pass at N >= 2048): count 4 has 2 n pairs, then n; count 3 has n, then n
    for count, n, shared, cols in ((4, hi4, False, 1), (3, 2, False, 0), (3, hi3, True, 2), (4, 2, True, 0)):
        m = tree.depth(count)
        assert m == 2 and [n * p for p in tree.pairs_per_level(count)] == ([2 * n, n] if count == 4 else [n, n])
        if N > 1024:
            want = {"passes": 2, "select_cols": cols, "select_stream": 2 - cols, "mac_gadget": 2, "select_tail_fused": 2}
            want = {k: c for k, c in want.items() if c}
        else:
            want = {"passes": 2, "select_stream": 2, "mac_gadget": 2, "select_tail_routed": 2}
        what = f"count = {count}, n = {n}, " + ("one set of selectors" if shared else "selectors per result")
        rr, rj = (0, 1) if shared else (m, 1)
        n_rg = m if shared else n * m
        rg = g.alloc(n_rg * rows * per)
        g.fill_uniform(rg, n_rg * rows * 2 * L, list(range(L)), 7000 + 16 * n + count)
        rg_h = rg.download((n_rg, rows, 2, L, N))
        x = edged(o, rng, n * count, L)  # row-major: leaf k of result r at r count + k
        dx = g.to_device(x)
        buf = sentinelled(g, n * per, N)
        begin(g)
        g.bfv_select(L, v, n, count, dx, count, 1, rg, rr, rj, At(buf, N))
        got = inner_of(buf, N, what).reshape(n, 2, L, N)
        routed(g, cid, f"select {what}", want)
        for r in range(n):
            ref = select_ref(o, x[r * count:(r + 1) * count], rg_h[:m] if shared else rg_h[r * m:(r + 1) * m], v)
            same(got[r], ref, cid, "select", f"{what}, result {r}")
        assert np.array_equal(dx.download(x.shape), x), (cid, what, "leaves")
        assert np.array_equal(rg.download(rg_h.shape), rg_h), (cid, what, "selectors")
        for b in (rg, dx, buf):
            b.free()


# ---- 8. he355_bfv_expand, he355_bfv_merge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_expand_and_merge(be, oracle, cid):
    g, o, N, sk, pk = layout_pair(be, oracle, cid)
    rng = np.random.default_rng(512)
    L, n, count = g.L, 2, 4
    per = 2 * L * N
    gks = expand_keys(g, o, sk, count, 190)
    assert list(gks) == [N + 1, N // 2 + 1]
    q = np.stack([o.encrypt(pk, rng.integers(0, o.t, N, dtype=np.uint64), 191), edged(o, rng, 3, L)[1]])
    dq = g.to_device(q)
    buf = sentinelled(g, count * n * per, N)
    begin(g)
    g.path_stats(reset=True)
    g.bfv_expand(L, n, dq, count, At(buf, N))
    got = inner_of(buf, N, "expand").reshape(count, n, 2, L, N)  # child k of query r at k n + r
    print(f"paths {cid} expand count = {count}, n = {n}: " + ", ".join(f"{k} = {c}" for k, c in g.path_stats().items() if c))
    routed(g, cid, "expand", {})
    for r in range(n):
        kids = children(expand_levels(o, q[r], 2, gks, L), count)
        for k in range(count):
            same(got[k, r], kids[k], cid, "expand", f"child {k} of query {r}")
    assert np.array_equal(dq.download(q.shape), q), (cid, "queries")
    dq.free()
    buf.free()
    # merge: input k of result r at k n + r; result 0 real encryptions, result 1 edged
    x = np.empty((count, n, 2, L, N), dtype=np.uint64)
    for k in range(count):
        x[k, 0] = o.encrypt(pk, rng.integers(0, o.t, N, dtype=np.uint64), 200 + k)
    x[:, 1] = edged(o, rng, count, L)
    for c in (count, 3):
        din = g.to_device(np.ascontiguousarray(x[:c]))
        buf = sentinelled(g, n * per, N)
        begin(g)
        g.path_stats(reset=True)
        g.bfv_merge(L, n, c, din, n, 1, At(buf, N))
        got = inner_of(buf, N, "merge").reshape(n, 2, L, N)
        print(f"paths {cid} merge count = {c}, n = {n}: " + ", ".join(f"{k} = {v}" for k, v in g.path_stats().items() if v))
        routed(g, cid, f"merge count = {c}", {})
        for r in range(n):
            same(got[r], merge_levels(o, list(x[:c, r]), c, gks, L), cid, "merge", f"count = {c}, result {r}")
        assert np.array_equal(din.download(x[:c].shape), x[:c]), (cid, "merge inputs")
        din.free()
        buf.free()


# ---- 9 - 11. he355_bfv_reply_compress, he355_bfv_reply_decrypt ----------------------------------------------------------------------------
def widths_of(g, cid, N):
    """(2, 2), (top, top) and the safe pair where the chain's first prime holds it"""
    q = int(g.moduli[0])
    top, safe = LAYOUTS[cid][2:]
    k0, k1, ok = g.bfv_reply_safe_bits()
    tb = 20 if cid not in EXPLICIT else g.t.bit_length()  # bitlen(t) + 2, and log2 N more
    assert (k0, k1) == rep.safe_bits(N, g.t) == (tb + 2, tb + 2 + N.bit_length() - 1) and ok == safe == rep.accepted(N, q, k0, k1)
    assert top == rep.max_width(N, q) and not rep.accepted(N, q, 2, top + 1) and g.bfv_reply_bytes(2, top + 1) == 0
    out = [(2, 2), (top, top)] + ([(k0, k1)] if ok else [])
    assert all(rep.accepted(N, q, *w) for w in out)
    return out


def as_words(data, stride):
    """[n][B] uint8 -> the uint64 words of n replies `stride` bytes apart, the gaps filled with the sentinel"""
    n, B = data.shape
    h = np.full((n, stride // 8), SENT, dtype=np.uint64)
    h.view(np.uint8).reshape(n, stride)[:, :B] = data
    return h.reshape(-1)


def check_compress(g, cid, N, L, ct, want_low, q, k0, k1):
    n = ct.shape[0]
    what = f"L = {L}, widths ({k0}, {k1})"
    B = g.bfv_reply_bytes(k0, k1)
    assert B == rep.reply_bytes(N, k0, k1)
    stride = B + PAD
    din = g.to_device(ct)
    buf = sentinelled(g, n * stride // 8, N)
    begin(g)
    g.bfv_reply_compress(L, k0, k1, n, din, buf, stride, byte_offset=8 * N)
    got = inner_of(buf, N, what).view(np.uint8).reshape(n, stride)
    routed(g, cid, f"reply_compress {what}", {})
    assert np.array_equal(got[:, :B], rep.np_compress(want_low, q, k0, k1)), (cid, "reply_compress", what, "prime 0")
    assert (got[:, B:].reshape(-1).view(np.uint64) == SENT).all(), (cid, what, "gaps")
    assert np.array_equal(din.download(ct.shape), ct), (cid, what, "operands")
    din.free()
    buf.free()


@pytest.mark.parametrize("cid", IDS)
def test_reply_compress(be, oracle, cid):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    q = int(g.moduli[0])
    rng = np.random.default_rng(513)
    x = np.concatenate((edged(o, rng, 3, g.L), rand_cts(o, rng, 2, g.L)))
    low = np.stack([to_level(o, c, 1) for c in x])
    at1 = np.concatenate((edged(o, rng, 3, 1), rand_cts(o, rng, 2, 1)))
    for k0, k1 in widths_of(g, cid, N):
        check_compress(g, cid, N, 1, at1, at1, q, k0, k1)
        check_compress(g, cid, N, g.L, x, low, q, k0, k1)


def product_ref(o, lifted, sk0, q):
    """[n][N] residues mod q_0 -> the residues of their negacyclic products with the key whose NTT form at prime 0 is sk0"""
    s = sk0.astype(object)
    return np.stack([o.intt(0, (o.ntt(0, row).astype(object) * s % q).astype(np.uint64)) for row in lifted])


def decrypt_ref(o, data, N, k0, k1, q, t, sk0):
    y0, y1 = rep.np_unpack(data, N, k0, k1)
    return rep.np_finish(y0, product_ref(o, rep.np_lift(y1, k1, q), sk0, q), k0, k1, q, t)


@pytest.mark.parametrize("key", ["oracle", "+1", "-1"])
@pytest.mark.parametrize("cid", IDS)
def test_reply_decrypt(be, oracle, cid, key):
    g, o, N, sk, _ = layout_pair(be, oracle, cid)
    q, t, n = int(g.moduli[0]), g.t, 5
    keys = {"oracle": sk, "+1": np.ones((g.K, N), dtype=np.uint64), "-1": np.stack([np.full(N, int(p) - 1, dtype=np.uint64) for p in g.moduli])}
    rng = np.random.default_rng(514 + N)
    g.set_secret_key(keys[key])
    try:
        for k0, k1 in widths_of(g, cid, N):
            what = f"key {key}, widths ({k0}, {k1})"
            B = g.bfv_reply_bytes(k0, k1)
            data = rng.integers(0, 256, (n, B), dtype=np.uint8)
            data[n - 2], data[n - 1] = 0xFF, 0
            want, budget, bits = decrypt_ref(o, data, N, k0, k1, q, t, np.asarray(keys[key], dtype=np.uint64).reshape(-1, N)[0])
            stride = B + PAD
            dby = g.to_device(as_words(data, stride))
            for with_budget in (True, False):
                out = sentinelled(g, n * N, N)
                begin(g)
                res = g.bfv_reply_decrypt(k0, k1, n, dby, stride, At(out, N), with_budget=with_budget)
                plain = inner_of(out, N, what).reshape(n, N)
                routed(g, cid, f"reply_decrypt {what}" + ("" if with_budget else ", no budget outputs"), {})
                assert np.array_equal(plain, want), (cid, "reply_decrypt", what, with_budget, "prime 0")
                if with_budget:
                    assert np.array_equal(res[0], budget) and np.array_equal(res[1], bits), (cid, what, res, budget, bits)
                else:
                    assert res is None
                out.free()
            if key != "oracle":  # the product is -+ the centred c1 itself
                y0, y1 = rep.np_unpack(data[:1], N, k0, k1)
                sign = 1 if key == "+1" else -1
                w = [sign * rep.centre(int(c), k1) for c in y1[0]]
                assert [int(c) for c in want[0]] == rep.finish([int(c) for c in y0[0]], w, k0, k1, t)[0]
            assert np.array_equal(dby.download(), as_words(data, stride)), (cid, what, "the replies are read, not written")
            dby.free()
    finally:
        g.set_secret_key(sk)


@pytest.mark.parametrize("cid", ["f64_first", "f64_only"])
def test_reply_refusals_where_the_first_prime_cannot_hold_the_safe_widths(be, oracle, cid):
    g, o, N, *_ = layout_pair(be, oracle, cid)
    q = int(g.moduli[0])
    k0, k1, ok = g.bfv_reply_safe_bits()
    assert (k0, k1) == rep.safe_bits(N, g.t) == (22, 33) and not ok and not rep.accepted(N, q, k0, k1)
    assert g.bfv_reply_bytes(k0, k1) == 0  # the contract of a refused pair; it would be rep.reply_bytes long
    B = rep.reply_bytes(N, k0, k1)
    assert B == N * 55 // 8
    x = rand_cts(o, np.random.default_rng(515), 2, g.L)
    dx = g.to_device(x)
    by = g.to_device(np.full(2 * B // 8 + 2 * N, SENT, dtype=np.uint64))
    pl = g.to_device(np.full(2 * N + 2, SENT, dtype=np.uint64))
    begin(g)
    refused(be, lambda: g.bfv_reply_compress(g.L, k0, k1, 2, dx, by, B))
    refused(be, lambda: g.bfv_reply_compress(1, k0, k1, 2, dx, by, B))
    refused(be, lambda: g.bfv_reply_decrypt(k0, k1, 2, by, B, pl))
    refused(be, lambda: g.bfv_reply_decrypt(k0, k1, 2, by, B, pl, with_budget=True))
    routed(g, cid, "reply refusals", {})
    assert (by.download() == SENT).all() and (pl.download() == SENT).all(), (cid, "outputs")
    assert np.array_equal(dx.download(x.shape), x), (cid, "operands")
    for b in (dx, by, pl):
        b.free()


# ---- 12. he355_bfv_seeded_encrypt, he355_bfv_seeded_restore on the small primes ------------------------------------------------------------
def test_seeded_encrypt_and_restore_on_tiny(be, oracle):
    """the uniform half drawn under 14-, 16- and 31-bit primes (bfv_seeded_limit: the rejection bound of each) and the secret-key
    product under them, against the definition in numpy and Python integers"""
    cid = "tiny"
    g, o, N, sk, pk = layout_pair(be, oracle, cid)
    assert [q.bit_length() for q in o.moduli[:g.L]] == [60, 14, 16, 31]
    rng = np.random.default_rng(516)
    n, a_seed, e_seed, first = 5, 0xA5EED, 0x5EC4E7, 70
    t = o.t
    m = rng.integers(0, t, (n, N), dtype=np.uint64)
    m[0, :5] = [0, 1, t // 2, t // 2 + 1, t - 1]
    m[n - 1] = t - 1
    dp = g.to_device(m)
    for L in (g.L, 1):
        per = L * N
        buf = sentinelled(g, n * per, N)
        begin(g)
        g.bfv_seeded_encrypt(L, n, dp, a_seed, e_seed, first, At(buf, N))
        c0 = inner_of(buf, N, ("seeded_encrypt", L)).reshape(n, L, N)
        routed(g, cid, f"seeded_encrypt L = {L}", {})
        for r in range(n):
            same(c0[r], seeded.encrypt(o, sk, L, m[r:r + 1], a_seed, e_seed, first + r)[0], cid, "seeded_encrypt", f"L = {L}, row {r}")
        dc = g.to_device(c0)
        for form in (0, 1):
            out = sentinelled(g, n * 2 * per, N)
            g.bfv_seeded_restore(L, form, n, dc, a_seed, first, At(out, N))
            got = inner_of(out, N, ("seeded_restore", L, form)).reshape(n, 2, L, N)
            for r in range(n):
                same(got[r], seeded.restore(o, L, form, c0[r:r + 1], a_seed, first + r)[0], cid, "seeded_restore", f"L = {L}, form {form}, row {r}")
            out.free()
        if L == g.L:  # and it decrypts
            out = g.alloc(n * 2 * per)
            g.bfv_seeded_restore(L, 0, n, dc, a_seed, first, out)
            dec = g.alloc(n * N)
            g.decrypt(L, 2, n, out, dec)
            assert np.array_equal(dec.download((n, N)), m), (cid, "decrypt of the restored ciphertexts")
            out.free()
            dec.free()
        assert np.array_equal(dp.download((n, N)), m), (cid, "plaintexts")
        buf.free()
        dc.free()
    dp.free()
