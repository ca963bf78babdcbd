// bfv_pir_args.h -- the argument checks of the BFV PIR calls that need no device (monomial multiply, expansion, merge, decomposition, the external
// product, the selection tree and its selectors, database bytes, reply compression, seeded queries and keys), each made ONCE per call: the C ABI function (bfv_pir.inc) runs the check before it asks for a
// device -- a refusal is HE355_E_INVALID_ARGS whether a device exists or not -- and keeps what the check worked out (the digit tables, F,
// rows, terms, pass, the field width) as its plan.  What needs the device or its state (keys present, the Galois keys, the
// key-switch tables) is checked after that, in the same function.  Host-only on purpose: no HIP header, so tests/bfv_pir_args_main.cpp runs every check at its edges
// under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <array>
#include <stdexcept>
#include <string>

#include "bfv_bytes_core.h"
#include "bfv_digits_core.h"
#include "bfv_gadget_core.h"
#include "bfv_reply_core.h"
#include "bfv_seeded_core.h"
#include "he_params.h"

namespace he355 {

// do the u64 ranges [p, p + np) and [q, q + nq) share an element?
inline bool ranges_overlap(const u64 *p, size_t np, const u64 *q, size_t nq) { return np && nq && p < q + nq && q < p + np; }
// [base, base + bytes) as integers: a span of up to 2^60 words behind any address may pass the end of the address space, where no pointer may be
// formed, and such a range is refused
struct AddrRange {
    unsigned long long lo, hi;
    bool overlaps(const AddrRange &o) const { return lo < hi && o.lo < o.hi && lo < o.hi && o.lo < hi; }
};
inline AddrRange byte_range(const std::string &w, const void *base, unsigned long long bytes)
{
    const unsigned long long lo = (unsigned long long)base;
    if (lo + bytes < lo) throw std::invalid_argument(w + ": a range wraps the address space");
    return {lo, lo + bytes};
}
inline AddrRange word_range(const std::string &w, const u64 *base, u64 words) { return byte_range(w, base, 8 * (unsigned long long)words); }
inline void check_size(int size, int lo, int hi) // "ciphertext size must be 1..3" / "... 2 or 3"
{
    if (size < lo || size > hi) throw std::invalid_argument("ciphertext size must be " + std::to_string(lo) + (hi == lo + 1 ? " or " : "..") + std::to_string(hi));
}
inline void check_level(const Params &p, const std::string &w, int L)
{
    if (L < 1 || (size_t)L > p.Ltop) throw std::invalid_argument(w + ": level out of range");
}
// the first L primes of the chain (1 <= L <= L_top), as the table builders take them
inline std::array<u64, kMaxPrimes> level_primes(const Params &p, int L)
{
    std::array<u64, kMaxPrimes> q{};
    for (int i = 0; i < L; ++i) q[i] = p.primes[i].q;
    return q;
}

// ---- monomial multiply and oblivious query expansion ------------------------------------------------------------------------------
inline void check_monomial_args(const Params &p, int L, int size, u32 e)
{
    check_level(p, "he355_bfv_multiply_monomial", L);
    check_size(size, 1, 3);
    if (e >= 2 * p.N) throw std::invalid_argument("he355_bfv_multiply_monomial: the exponent must be below 2N (X^N = -1)");
}
// levels of the expansion tree of `count` children, ceil(log2 count); level j uses the Galois element N / 2^j + 1
inline int expand_depth(u64 count)
{
    int d = 0;
    while (((u64)1 << d) < count) ++d;
    return d;
}
struct BfvExpandPlan {
    int depth;
};
inline BfvExpandPlan plan_expand(const Params &p, int L, u64 count)
{
    check_level(p, "he355_bfv_expand", L);
    if (count < 1 || count > p.N) throw std::invalid_argument("he355_bfv_expand: count must be in 1..N");
    return {expand_depth(count)};
}

// ---- ciphertext decomposition for recursive (two-dimensional) PIR, and the gadget cut ----------------------------------------------
// the digit table of level L and F = size D(L), the polynomials one ciphertext is cut into
struct BfvDigitPlan {
    BfvDigitTab tab;
    u64 F;
};
inline BfvDigitTab digit_table(const Params &p, int L) { return bfv_digit_table(level_primes(p, L).data(), L, p.plain_modulus); }
// `ct` [n][size][L][N], `plain` [n][F][N] (!ntt) or [n][F][L_out][N] (ntt: 1 <= L_out <= L_top): the two may not overlap, whichever is written
inline BfvDigitPlan plan_digits(const Params &p, const char *what, int L, int size, u64 n, const u64 *ct, const u64 *plain, bool ntt = false, int L_out = 0)
{
    const std::string w(what);
    check_level(p, w, L);
    if (L_out < (ntt ? 1 : 0) || (size_t)L_out > p.Ltop) throw std::invalid_argument(w + ": level out of range");
    check_size(size, 1, 3);
    if (p.plain_modulus < 2) throw std::invalid_argument(w + ": the plain modulus must be at least 2");
    const BfvDigitTab tab = digit_table(p, L);
    const u64 F = (u64)size * tab.total;
    if (n > 0xffffffffull / F) throw std::invalid_argument(w + ": too many plaintexts for one call (n F must be below 2^32)");
    if (ranges_overlap(ct, (size_t)n * size * L * p.N, plain, (size_t)n * F * (L_out ? L_out : 1) * p.N))
        throw std::invalid_argument(w + ": the plaintexts overlap the ciphertexts");
    return {tab, F};
}
constexpr u64 kGadgetPassPolys = 4096; // digit polynomials one pass of he355_bfv_external_product holds in its pool block
inline u64 gadget_poly_blocks(const Params &p, bool cols) { return cols && p.N > 1024 ? 4 : p.N / 512; } // blocks per residue polynomial
inline BfvDigitTab gadget_table(const Params &p, const std::string &w, int L, int v)
{
    check_level(p, w, L);
    if (!bfv_gadget_width_ok(v)) throw std::invalid_argument(w + ": digit_bits must be 1..63");
    return bfv_gadget_table(level_primes(p, L).data(), L, v);
}
// `ct` [n][size][L][N] -> `digits` [n][size E][N] (ntt false) or [n][size E][L][N]
inline BfvDigitPlan plan_gadget_cut(const Params &p, const char *what, int L, int v, int size, u64 n, const u64 *ct, const u64 *digits, bool ntt)
{
    const std::string w(what);
    const BfvDigitTab tab = gadget_table(p, w, L, v);
    check_size(size, 1, 3);
    const u64 F = (u64)size * tab.total;
    if (n > 0xffffffffull / F) throw std::invalid_argument(w + ": too many digit polynomials for one call (n size E must be below 2^32)");
    if (n * size * L > 0x7fffffffull / gadget_poly_blocks(p, ntt)) throw std::invalid_argument(w + ": too many polynomials for one launch");
    if (ranges_overlap(ct, (size_t)n * size * L * p.N, digits, (size_t)n * F * (ntt ? L : 1) * p.N)) throw std::invalid_argument(w + ": the digits overlap the ciphertexts");
    return {tab, F};
}

// ---- the external product RGSW x ciphertext ----------------------------------------------------------------------------------------
// the gadget table of level L and the rows n 2 E(L) of the batch, each an encryption of zero plus its planted term
struct BfvRgswPlan {
    BfvDigitTab tab;
    u64 rows;
};
inline BfvRgswPlan plan_rgsw(const Params &p, int L, int v, u64 n, const u64 *plain, const u64 *out)
{
    const std::string w("he355_bfv_rgsw_encrypt");
    const BfvDigitTab tab = gadget_table(p, w, L, v);
    if (p.plain_modulus < 2) throw std::invalid_argument(w + ": the plain modulus must be at least 2");
    const u64 per = 2 * (u64)tab.total * 2 * L; // residue polynomials of one RGSW ciphertext
    if (n > 0x7fffffffull / (per * (p.N / 512))) throw std::invalid_argument(w + ": too many RGSW ciphertexts for one launch");
    if (ranges_overlap(plain, (size_t)n * p.N, out, (size_t)n * per * p.N)) throw std::invalid_argument(w + ": `d_rgsw` overlaps the plaintexts");
    return {tab, n * 2 * tab.total};
}
// the words from the first operand of a batch to the end of the last one it touches, ((n - 1) stride_r + (inner - 1) stride_k + 1) items of
// `item_words` each, formed in 128 bits and refused where they cannot lie in one address space
inline size_t gadget_span_words(const std::string &w, u64 n, u64 inner, u64 stride_r, u64 stride_k, u64 item_words)
{
    const u128 items = (u128)(n - 1) * stride_r + (u128)(inner - 1) * stride_k + 1;
    if (items > ((u128)1 << 60) || items * item_words > ((u128)1 << 60)) throw std::invalid_argument(w + ": a stride takes the operands past 2^60 words");
    return (size_t)(items * item_words);
}
// rows = 2 E(L) of one RGSW ciphertext, terms = inner rows digit polynomials per result, pass = results per pass (bfv_gadget_pass; 0 when n is)
struct BfvExternalPlan {
    BfvDigitTab tab;
    u32 rows;
    u64 terms, pass;
};
inline BfvExternalPlan plan_external_product(const Params &p, int L, int v, u64 n, u64 inner, const u64 *ct, u64 ct_stride_r, u64 ct_stride_k, const u64 *rgsw, u64 rg_stride_r,
                                             u64 rg_stride_k, const u64 *out)
{
    const std::string w("he355_bfv_external_product");
    const BfvDigitTab tab = gadget_table(p, w, L, v);
    const u64 rows = 2 * (u64)tab.total;
    if (inner < 1 || inner > 0x7fffffffull / rows) throw std::invalid_argument(w + ": inner must be at least 1 and inner 2 E(L) below 2^31");
    const u64 terms = inner * rows, pass = bfv_gadget_pass(terms, n, kGadgetPassPolys);
    const BfvExternalPlan plan{tab, (u32)rows, terms, pass};
    if (!n) return plan;
    if (n > 0x7fffffffull || pass * inner * 2 * L > 0x7fffffffull / gadget_poly_blocks(p, true) || pass * L > 0x7fffffffull / (p.N / 512))
        throw std::invalid_argument(w + ": too many polynomials for one launch");
    const size_t ctn = 2 * (size_t)L * p.N;
    if (ranges_overlap(out, n * ctn, ct, gadget_span_words(w, n, inner, ct_stride_r, ct_stride_k, ctn))) throw std::invalid_argument(w + ": `d_out` overlaps the ciphertexts");
    if (ranges_overlap(out, n * ctn, rgsw, gadget_span_words(w, n, inner, rg_stride_r, rg_stride_k, rows * ctn))) throw std::invalid_argument(w + ": `d_out` overlaps the RGSW ciphertexts");
    return plan;
}

// ---- ciphertext merge (he355_bfv_merge) ------------------------------------------------------------------------------------------------
// the merge, the expansion's transpose: input k < count of result r < n is ciphertext k stride_k + r stride_r of `in`, `out` is [n][2][L][N].
// depth: the levels; half = 2^(depth-1) n, the pairs of the first level (0 at depth 0); scratch_cts: the pool block, S and D of the first
// level and, unless that level is the last, its output (0 when n is 0 or the call only copies)
struct BfvMergePlan {
    int depth;
    u64 half, scratch_cts;
};
inline u64 gcd_u64(u64 a, u64 b)
{
    while (b) { const u64 t = a % b; a = b; b = t; }
    return a;
}
// two `noun` (item k < count of result r < n lies at k stride_k + r stride_r) at one place: a stride of 0 along an index that moves, or
// k stride_k + r stride_r = k' stride_k + r' stride_r, which has a solution exactly when the smallest one, k - k' = stride_r / g and
// r' - r = stride_k / g (g the strides' gcd), lies inside the extents
inline void check_strides_apart(const std::string &w, const char *noun, u64 n, u64 count, u64 stride_r, u64 stride_k)
{
    if ((count > 1 && !stride_k) || (n > 1 && !stride_r)) throw std::invalid_argument(w + ": a stride of 0 puts two " + noun + " at one place");
    if (count > 1 && n > 1) {
        const u64 g = gcd_u64(stride_k, stride_r);
        if (stride_r / g <= count - 1 && stride_k / g <= n - 1) throw std::invalid_argument(w + ": under these strides two " + noun + " lie at one place");
    }
}
inline BfvMergePlan plan_merge(const Params &p, int L, u64 n, u64 count, const u64 *in, u64 stride_k, u64 stride_r, const u64 *out)
{
    const std::string w("he355_bfv_merge");
    check_level(p, w, L);
    if (count < 1 || count > p.N) throw std::invalid_argument(w + ": count must be in 1..N");
    const int d = expand_depth(count);
    if (!n) return {d, 0, 0};
    check_strides_apart(w, "inputs", n, count, stride_r, stride_k);
    const size_t ctn = 2 * (size_t)L * p.N;
    const size_t span = gadget_span_words(w, n, count, stride_r, stride_k, ctn); // checked: refused where the index arithmetic would wrap
    const u64 blocks_per_ct = 2 * (u64)L * (p.N / 512);
    const u128 half = d ? (u128)n << (d - 1) : 0;
    if (n > 0x7fffffffull || half > 0x7fffffffull / blocks_per_ct) throw std::invalid_argument(w + ": too many polynomials for one launch");
    const AddrRange src = word_range(w, in, span), dst = word_range(w, out, n * ctn);
    if (dst.overlaps(src)) throw std::invalid_argument(w + ": `d_out` overlaps the inputs (it may not lie inside their span)");
    return {d, (u64)half, (u64)half * (d > 1 ? 3 : 2)};
}

// ---- the selection tree (he355_bfv_select) ----------------------------------------------------------------------------------------------
// Leaf k < count of result r < n is ciphertext r ct_stride_r + k ct_stride_k of `ct`, selector j < depth of result r the RGSW ciphertext
// r rg_stride_r + j rg_stride_j of `rgsw`, `out` is [n][2][L][N].  depth = ceil(log2 count); c[j]: the nodes per result at level j (c[0] = count,
// c[j+1] = ceil(c[j] / 2), c[depth] = 1); pairs(j) = n floor(c[j] / 2), the pairs of all results at level j (level 0 has the most); pass: pairs
// per trip through the digit slab (bfv_gadget_pass over level 0's pairs with terms = rows = 2 E(L)); slab_polys: the residue-polynomial slots
// ([N] words each) of that block, pass (rows + 2) L: the digits and, behind them, the pass's sums (N = 1024, whose tail runs once per level: the
// sums of level 0's pairs, (pass rows + 2 pairs(0)) L); node_cts: the ciphertexts of the block that
// holds the two alternating node levels, n c[1] (depth >= 2) + n c[2] (depth >= 3), at most (ceil(count/2) + ceil(count/4)) n.
constexpr u64 kSelectMaxCount = (u64)1 << 24; // leaves per result
constexpr int kSelectMaxDepth = 24;
struct BfvSelectPlan {
    BfvDigitTab tab;
    u32 rows;
    int depth;
    u64 n;
    u64 c[kSelectMaxDepth + 1];
    u64 pass, slab_polys, node_cts;
    u64 pairs(int j) const { return n * (c[j] / 2); }
};
inline BfvSelectPlan plan_select(const Params &p, int L, int v, u64 n, u64 count, const u64 *ct, u64 ct_stride_r, u64 ct_stride_k, const u64 *rgsw, u64 rg_stride_r, u64 rg_stride_j,
                                 const u64 *out)
{
    const std::string w("he355_bfv_select");
    BfvSelectPlan pl{};
    pl.tab = gadget_table(p, w, L, v);
    pl.rows = 2 * (u32)pl.tab.total;
    if (count < 1 || count > kSelectMaxCount) throw std::invalid_argument(w + ": count must be in 1..2^24");
    pl.depth = expand_depth(count);
    pl.n = n;
    pl.c[0] = count;
    for (int j = 0; j < pl.depth; ++j) pl.c[j + 1] = (pl.c[j] + 1) / 2;
    if (!n) return pl;
    check_strides_apart(w, "leaves", n, count, ct_stride_r, ct_stride_k);
    const size_t ctn = 2 * (size_t)L * p.N;
    const size_t span = gadget_span_words(w, n, count, ct_stride_r, ct_stride_k, ctn); // refused where the index arithmetic would wrap
    const size_t rspan = pl.depth ? gadget_span_words(w, n, (u64)pl.depth, rg_stride_r, rg_stride_j, pl.rows * ctn) : 0;
    // a level's pairs (count == 1: its n copies) as one streaming launch of 2 L N / 512 blocks per ciphertext: the passes launch fewer, the
    // copy of the nodes without a partner at most n of them
    const u128 units = (u128)n * (count > 1 ? count / 2 : 1);
    if (n > 0x7fffffffull || units > 0x7fffffffull / (2 * (u64)L * (p.N / 512))) throw std::invalid_argument(w + ": more pairs than one launch's grid holds");
    const AddrRange src = word_range(w, ct, span), dst = word_range(w, out, n * ctn), sel = word_range(w, rgsw, rspan);
    if (dst.overlaps(src)) throw std::invalid_argument(w + ": `d_out` overlaps the leaves (it may not lie inside their span)");
    if (dst.overlaps(sel)) throw std::invalid_argument(w + ": `d_out` overlaps the selectors");
    if (pl.depth) {
        pl.pass = bfv_gadget_pass(pl.rows, pl.pairs(0), kGadgetPassPolys);
        pl.slab_polys = (pl.pass * pl.rows + (p.N == 1024 ? pl.pairs(0) : pl.pass) * 2) * L;
        pl.node_cts = (pl.depth >= 2 ? n * pl.c[1] : 0) + (pl.depth >= 3 ? n * pl.c[2] : 0);
    }
    return pl;
}

// ---- RGSW selectors from ONE packed query ciphertext ---------------------------------------------------------------------------------
// `sel` [n][n_sel] mod t -> `out` [n][2][L][N]; depth: the levels of the expansion the query is packed for
struct BfvSelectorPlan {
    BfvDigitTab tab;
    int depth;
};
inline BfvSelectorPlan plan_selector(const Params &p, int L, int v, u64 n, u64 n_sel, u64 first_slot, u64 count, const u64 *sel, const u64 *out)
{
    const std::string w("he355_bfv_selector_encrypt");
    const BfvDigitTab tab = gadget_table(p, w, L, v);
    if (p.plain_modulus < 2) throw std::invalid_argument(w + ": the plain modulus must be at least 2");
    if (!n_sel) throw std::invalid_argument(w + ": n_sel must be at least 1");
    if (count < 1 || count > p.N) throw std::invalid_argument(w + ": count must be in 1..N");
    if ((u128)first_slot + (u128)n_sel * tab.total > count) throw std::invalid_argument(w + ": first_slot + n_sel E(L) must not exceed count");
    if (n > 0x7fffffffull / (2 * (u64)L * (p.N / 512))) throw std::invalid_argument(w + ": too many ciphertexts for one launch");
    if (ranges_overlap(sel, (size_t)(n * n_sel), out, (size_t)n * 2 * L * p.N)) throw std::invalid_argument(w + ": `d_out` overlaps the selectors");
    return {tab, expand_depth(count)};
}
// the call's own refusals; its RGSW rows are he355_bfv_rgsw_encrypt's (plan_rgsw with n = 1, once the secret's coefficients lie in their block)
inline void check_rgsw_secret_args(const Params &p, int L, int kv)
{
    const std::string w("he355_bfv_rgsw_encrypt_secret");
    if (L >= 1 && (size_t)L <= p.Ltop && !bfv_gadget_width_ok(kv)) throw std::invalid_argument(w + ": key_bits must be 1..63");
    const BfvDigitTab tab = gadget_table(p, w, L, kv);
    if (p.plain_modulus < 2) throw std::invalid_argument(w + ": the plain modulus must be at least 2");
    if (2 * (u64)tab.total * 2 * L > 0x7fffffffull / (p.N / 512)) throw std::invalid_argument(w + ": too many polynomials for one launch");
}
// slot ciphertexts at r ct_stride_r + (b E + f) ct_stride_k of `ct`, `key` [2 E_key][2][L][N] -> `out` [n][n_sel][2E][2][L][N].  tab: the selectors'
// table, ktab: the key's; rows = 2 E_key terms per slot ciphertext, C = n n_sel E slot ciphertexts, pass of them at a time (both 0 when n is)
struct BfvFromBfvPlan {
    BfvDigitTab tab, ktab;
    u32 rows;
    u64 C, pass;
};
inline BfvFromBfvPlan plan_from_bfv(const Params &p, int L, int v, int kv, u64 n, u64 n_sel, const u64 *ct, u64 ct_stride_r, u64 ct_stride_k, const u64 *key, const u64 *out)
{
    const std::string w("he355_bfv_rgsw_from_bfv");
    const BfvDigitTab tab = gadget_table(p, w, L, v);
    if (!bfv_gadget_width_ok(kv)) throw std::invalid_argument(w + ": key_bits must be 1..63");
    const BfvDigitTab kt = gadget_table(p, w, L, kv);
    const u64 rows = 2 * (u64)kt.total;
    if (!n_sel) throw std::invalid_argument(w + ": n_sel must be at least 1");
    if (!n) return {tab, kt, (u32)rows, 0, 0};
    const u128 slots = (u128)n * n_sel * tab.total; // slot ciphertexts
    if (n > 0x7fffffffull || n_sel > 0x7fffffffull || slots > 0x7fffffffull / (2 * (u64)L * 4)) throw std::invalid_argument(w + ": too many polynomials for one launch");
    const u64 C = (u64)slots, pass = bfv_gadget_pass(rows, C, kGadgetPassPolys);
    if (pass * 2 * L > 0x7fffffffull / gadget_poly_blocks(p, false) || pass * rows * L > 0x3fffffffull)
        throw std::invalid_argument(w + ": too many polynomials for one launch");
    const size_t ctn = 2 * (size_t)L * p.N, outn = (size_t)C * 2 * ctn;
    if (ranges_overlap(out, outn, ct, gadget_span_words(w, n, n_sel * tab.total, ct_stride_r, ct_stride_k, ctn))) throw std::invalid_argument(w + ": `d_rgsw` overlaps the ciphertexts");
    if (ranges_overlap(out, outn, key, (size_t)rows * ctn)) throw std::invalid_argument(w + ": `d_rgsw` overlaps the key");
    return {tab, kt, (u32)rows, C, pass};
}

// ---- a PIR database from packed bytes -------------------------------------------------------------------------------------------------
constexpr u64 kBytesChunk = 4096; // N = 1024's routed path: plaintexts per pass through its pool block (32 MiB)
struct BfvBytesPlan {
    int w; // the field width
};
// `bytes`: plaintext j at bytes + j stride, B bytes; `words`: [n][per] 64-bit words, per = N (coefficients) or L_out N (ntt: 1 <= L_out <= L_top).
// pack: the bytes are the output, whole 8-byte words of it.
inline BfvBytesPlan plan_bytes(const Params &p, const char *what, u64 n, const void *bytes, u64 stride, u64 B, const u64 *words, bool pack, bool ntt = false, int L_out = 0)
{
    const std::string s(what);
    if (L_out < (ntt ? 1 : 0) || (size_t)L_out > p.Ltop) throw std::invalid_argument(s + ": level out of range");
    if (p.plain_modulus < 2) throw std::invalid_argument(s + ": the plain modulus must be at least 2");
    const int w = bfv_bitlen(p.plain_modulus) - 1;
    if (B < 1 || B > bfv_bytes_max(p.N, w)) throw std::invalid_argument(s + ": bytes_per_plain must be 1 .. floor(N w / 8) (he355_bfv_bytes_per_plain)");
    if (stride < B) throw std::invalid_argument(s + ": stride_bytes must be at least bytes_per_plain");
    const u64 tail = pack ? 8 * bfv_bytes_words(B) : B; // the bytes of the last plaintext the call touches
    // (n - 1) stride + tail stays below 2^63: neither the range below nor a kernel's j * stride can wrap
    if (n > 1 && n - 1 > (((u64)1 << 63) - tail) / stride) throw std::invalid_argument(s + ": (n - 1) stride_bytes must be below 2^63");
    if (!pack && !L_out && ((unsigned long long)words & 15)) throw std::invalid_argument(s + ": d_plain must be 16-byte aligned");
    if (pack && (((unsigned long long)bytes & 7) || (stride & 7) || stride < tail))
        throw std::invalid_argument(s + ": d_bytes must be 8-byte aligned and stride_bytes a multiple of 8, at least 8 ceil(bytes_per_plain / 8)");
    if (n > 0x7fffffffull / (p.N / 256)) throw std::invalid_argument(s + ": too many plaintexts for one launch (n N / 256 must be below 2^31)");
    if (n) {
        const AddrRange br = byte_range(s, bytes, (n - 1) * stride + tail), wr = word_range(s, words, n * (L_out ? (u64)L_out : 1) * p.N);
        if (br.overlaps(wr)) throw std::invalid_argument(s + ": the bytes overlap the plaintexts");
    }
    return {w};
}

// ---- reply compression (he355_bfv_reply_compress, he355_bfv_reply_decrypt) -----------------------------------------------------------------
// reply j: `bytes` whole words at bytes + j stride; `words`: the other side, [n][per] 64-bit words -- the ciphertexts [n][2][L][N]
// (per = 2 L N, read) or the plaintexts [n][N] (per = N, written); `stats`: decrypt's int32 outputs [n], either may be null.
struct BfvReplyPlan {
    u64 bytes; // of one reply, N (k0 + k1) / 8
};
inline void check_reply_widths(const Params &p, const std::string &s, int k0, int k1)
{
    if (!bfv_reply_widths_ok(p.N, p.primes[0].q, k0, k1))
        throw std::invalid_argument(s + ": the widths must satisfy 2 <= k0 <= k1 and N 2^(k1 - 1) <= (q_0 - 1) / 2");
}
inline BfvReplyPlan plan_reply(const Params &p, const char *what, int L, int k0, int k1, u64 n, const void *bytes, u64 stride, const u64 *words, u64 per,
                               bool decrypt = false, const int32_t *stat_a = nullptr, const int32_t *stat_b = nullptr)
{
    const std::string s(what);
    check_level(p, s, L);
    if (p.plain_modulus < 2) throw std::invalid_argument(s + ": the plain modulus must be at least 2");
    check_reply_widths(p, s, k0, k1);
    const u64 B = bfv_reply_size(p.N, k0, k1);
    if (((unsigned long long)bytes & 7) || (stride & 7) || stride < B)
        throw std::invalid_argument(s + ": d_bytes must be 8-byte aligned and stride_bytes a multiple of 8, at least the reply size (he355_bfv_reply_bytes)");
    // (n - 1) stride + B stays below 2^63: neither the range below nor a kernel's j * stride can wrap
    if (n > 1 && n - 1 > (((u64)1 << 63) - 1 - B) / stride) throw std::invalid_argument(s + ": (n - 1) stride_bytes + the reply size must be below 2^63");
    // the largest grid: a block per 256 coefficients (the client's kernels, the switch to L = 1) or per 256 words of a reply (the packing)
    const u64 blocks = std::max<u64>(p.N / 256, (B / 8 + 255) / 256);
    if (n > 0x7fffffffull / blocks) throw std::invalid_argument(s + ": too many replies for one launch (its grid must stay below 2^31 blocks)");
    if (n) {
        const AddrRange br = byte_range(s, bytes, (n - 1) * stride + B), wr = word_range(s, words, n * per);
        if (br.overlaps(wr)) throw std::invalid_argument(s + ": the replies overlap the " + (decrypt ? "plaintexts" : "ciphertexts"));
        for (const int32_t *st : {stat_a, stat_b}) {
            if (!st) continue;
            const AddrRange sr = byte_range(s, st, 4 * n);
            if (sr.overlaps(br) || sr.overlaps(wr)) throw std::invalid_argument(s + ": a budget output overlaps the replies or the plaintexts");
        }
        if (stat_a && stat_b && byte_range(s, stat_a, 4 * n).overlaps(byte_range(s, stat_b, 4 * n))) throw std::invalid_argument(s + ": the two budget outputs overlap");
    }
    return {B};
}

// ---- seeded queries and Galois keys (he355_bfv_seeded_*, he355_keygen_galois_seeded, he355_set_galois_key_seeded) ----------------------------
// ciphertext r of a call is seeded ciphertext first_index + r; `c0` is [n][L][N], the restored ciphertexts [n][2][L][N]
inline void check_seeded_seeds(const std::string &w, u64 a_seed, u64 noise_seed)
{
    // splitmix64 is a bijection: with one seed for both, the published seed would give the error away
    if (a_seed == noise_seed) throw std::invalid_argument(w + ": a_seed (public) and noise_seed (secret) must differ");
}
inline void check_seeded_index(const std::string &w, u64 first_index, u64 n)
{
    if (first_index + n < first_index || first_index + n > kBfvSeededMaxIndex) throw std::invalid_argument(w + ": first_index + n must not exceed 2^40");
}
// `polys_per_ct` residue polynomials per ciphertext in the call's largest slab: its words stay below 2^60 and a streaming launch over it
// (a block per 512 words) below 2^31 blocks; the transforms' grids are smaller
inline void check_seeded_size(const Params &p, const std::string &w, u64 n, u64 polys_per_ct)
{
    if ((u128)n * polys_per_ct * p.N > ((u128)1 << 60)) throw std::invalid_argument(w + ": the ciphertexts span more than 2^60 words");
    if (n > 0x7fffffffull / (polys_per_ct * (p.N / 512))) throw std::invalid_argument(w + ": too many ciphertexts for one launch (its grid must stay below 2^31 blocks)");
}
inline void check_galois_elt(const Params &p, const std::string &w, uint32_t elt)
{
    if (!(elt & 1) || elt < 3 || elt >= 2 * p.N) throw std::invalid_argument(w + ": Galois element is not valid (odd, 3 .. 2N - 1)");
    if (p.K < 2) throw std::invalid_argument(w + ": encryption parameters do not support key switching");
}
inline void plan_seeded_encrypt(const Params &p, int L, u64 n, const u64 *plain, u64 a_seed, u64 noise_seed, u64 first_index, const u64 *c0)
{
    const std::string w("he355_bfv_seeded_encrypt");
    check_level(p, w, L);
    if (p.plain_modulus < 2) throw std::invalid_argument(w + ": the plain modulus must be at least 2");
    check_seeded_seeds(w, a_seed, noise_seed);
    check_seeded_index(w, first_index, n);
    check_seeded_size(p, w, n, (u64)L);
    if (!n) return;
    const AddrRange dst = word_range(w, c0, n * L * p.N); // (refused where it wraps the address space, with or without plaintexts)
    if (plain && dst.overlaps(word_range(w, plain, n * p.N))) throw std::invalid_argument(w + ": `d_c0` overlaps the plaintexts");
}
inline void plan_seeded_restore(const Params &p, int L, int ntt_form, u64 n, const u64 *c0, u64 first_index, const u64 *out)
{
    const std::string w("he355_bfv_seeded_restore");
    check_level(p, w, L);
    if (ntt_form != 0 && ntt_form != 1) throw std::invalid_argument(w + ": ntt_form must be 0 or 1");
    check_seeded_index(w, first_index, n);
    check_seeded_size(p, w, n, 2 * (u64)L);
    if (n && word_range(w, out, n * 2 * L * p.N).overlaps(word_range(w, c0, n * L * p.N))) throw std::invalid_argument(w + ": `d_out` overlaps `d_c0`");
}
// he355_bfv_selector_encrypt's rules (plan_selector) on a `c0` of [n][L][N], and the seeded ones
inline BfvSelectorPlan plan_seeded_selector(const Params &p, int L, int v, u64 n, u64 n_sel, u64 first_slot, u64 count, const u64 *sel, u64 a_seed, u64 noise_seed,
                                            u64 first_index, const u64 *c0)
{
    const std::string w("he355_bfv_seeded_selector_encrypt");
    const BfvDigitTab tab = gadget_table(p, w, L, v);
    if (p.plain_modulus < 2) throw std::invalid_argument(w + ": the plain modulus must be at least 2");
    if (!n_sel) throw std::invalid_argument(w + ": n_sel must be at least 1");
    if (count < 1 || count > p.N) throw std::invalid_argument(w + ": count must be in 1..N");
    if ((u128)first_slot + (u128)n_sel * tab.total > count) throw std::invalid_argument(w + ": first_slot + n_sel E(L) must not exceed count");
    check_seeded_seeds(w, a_seed, noise_seed);
    check_seeded_index(w, first_index, n);
    check_seeded_size(p, w, n, (u64)L);
    if (n && word_range(w, c0, n * L * p.N).overlaps(word_range(w, sel, n * n_sel))) throw std::invalid_argument(w + ": `d_c0` overlaps the selectors");
    return {tab, expand_depth(count)};
}
inline void plan_keygen_galois_seeded(const Params &p, uint32_t elt, u64 a_seed, u64 noise_seed)
{
    const std::string w("he355_keygen_galois_seeded");
    check_galois_elt(p, w, elt);
    check_seeded_seeds(w, a_seed, noise_seed);
}
inline void plan_set_galois_key_seeded(const Params &p, uint32_t elt, const u64 *h_b)
{
    const std::string w("he355_set_galois_key_seeded");
    check_galois_elt(p, w, elt);
    if (!h_b) throw std::invalid_argument(w + ": null key halves");
}

} // namespace he355
