// bfv_pir_args_main.cpp -- TEST-ONLY, stand-alone.  Runs every argument check of csrc/bfv_pir_args.h (the device-free checks of the BFV PIR
// calls, and the plans they return) at the accepted and refused edge arguments of the CPU tests -- levels and widths at and past their
// ends, n F at 2^32, grids at 2^31, strides that take a span past 2^60 words or wrap 64 bits, overlaps one word inside and right behind --
// compiled with -fsanitize=address,undefined (tests/test_bfv_pir_args_cpu.py).  The checks do arithmetic on counts, strides and addresses
// the caller chose: none of it may overflow a signed type, shift out of range or form a pointer outside its slab before the refusal.
// Prints "bfv_pir_args ok" and exits 0, or names the first case that went the other way.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/bfv_pir_args.h"
#include "args_main_common.h"

using namespace he355;

int main()
{
    const size_t N = 4096;
    const int v = 20;
    std::unique_ptr<Params> pp(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    const Params &P = *pp;
    const int Lt = (int)P.Ltop;
    const u64 E = bfv_gadget_table(level_primes(P, Lt).data(), Lt, v).total, D = digit_table(P, Lt).total;
    const size_t per = 2 * (size_t)Lt * N;
    std::vector<u64> a(4 * E * per + N), b(6 * E * per), k(2 * 60 * 2 * N); // (k: the key at key_bits = 1, 60 digits, still fits)
    const u64 *pa = a.data(), *pb = b.data(), *pk = k.data();
    // an address `words` words behind a slab's start, formed as an integer: the callers' pointers are only numbers to the checks
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };

    // ---- monomial, expansion ---------------------------------------------------------------------------------------------------------
    for (int L : {0, Lt + 1, -1}) BAD("monomial", check_monomial_args(P, L, 2, 1));
    BAD("monomial", check_monomial_args(P, Lt, 0, 1));
    BAD("monomial", check_monomial_args(P, Lt, 4, 1));
    BAD("monomial", check_monomial_args(P, Lt, 2, (u32)(2 * N)));
    BAD("monomial", check_monomial_args(P, Lt, 2, 0xffffffffu));
    GOOD("monomial", check_monomial_args(P, Lt, 3, (u32)(2 * N - 1)));
    GOOD("monomial", check_monomial_args(P, 1, 1, 0));
    for (int L : {0, Lt + 1, -1}) BAD("expand", plan_expand(P, L, 4));
    BAD("expand", plan_expand(P, Lt, 0));
    BAD("expand", plan_expand(P, Lt, N + 1));
    BAD("expand", plan_expand(P, Lt, ~(u64)0));
    GOOD("expand", if (plan_expand(P, Lt, 1).depth != 0 || plan_expand(P, 1, 5).depth != 3 || plan_expand(P, Lt, N).depth != 12) throw std::invalid_argument("depth"));

    // ---- digits ----------------------------------------------------------------------------------------------------------------------
    for (int L : {0, Lt + 1, -1}) BAD("digits", plan_digits(P, "d", L, 2, 1, pa, pb));
    for (int Lo : {0, Lt + 1, -1}) BAD("digits", plan_digits(P, "d", Lt, 2, 1, pa, pb, true, Lo));
    BAD("digits", plan_digits(P, "d", Lt, 2, 1, pa, pb, false, -1));
    BAD("digits", plan_digits(P, "d", Lt, 0, 1, pa, pb));
    BAD("digits", plan_digits(P, "d", Lt, 4, 1, pa, pb));
    BAD("digits", plan_digits(P, "d", Lt, 2, (u64)1 << 32, pa, pb));              // n F at 2^32
    BAD("digits", plan_digits(P, "d", Lt, 1, 0xffffffffull / D + 1, pa, pb));
    BAD("digits", plan_digits(P, "d", Lt, 2, 1, pb, pb));                         // the same slab
    BAD("digits", plan_digits(P, "d", Lt, 2, 1, at(pb, 2 * D * N - 1), pb));      // the last word of the plaintexts
    BAD("digits", plan_digits(P, "d", Lt, 2, 1, at(pb, 2 * D * Lt * N - 1), pb, true, Lt));
    GOOD("digits", plan_digits(P, "d", Lt, 2, 1, at(pb, 2 * D * N), pb));
    GOOD("digits", plan_digits(P, "d", Lt, 2, 1, at(pb, 2 * D * Lt * N), pb, true, Lt));
    GOOD("digits", if (plan_digits(P, "d", Lt, 3, 1, pa, pb, true, 1).F != 3 * D) throw std::invalid_argument("F"));
    GOOD("digits", plan_digits(P, "d", 1, 1, 0, pa, pa));                          // nothing to overlap

    // ---- gadget cut, RGSW encryption, external product ----------------------------------------------------------------------------------
    for (bool ntt : {false, true}) {
        for (int L : {0, Lt + 1, -1}) BAD("cut", plan_gadget_cut(P, "g", L, v, 2, 1, pa, pb, ntt));
        for (int w : {0, 64, -1}) BAD("cut", plan_gadget_cut(P, "g", Lt, w, 2, 1, pa, pb, ntt));
        BAD("cut", plan_gadget_cut(P, "g", Lt, v, 0, 1, pa, pb, ntt));
        BAD("cut", plan_gadget_cut(P, "g", Lt, v, 4, 1, pa, pb, ntt));
        BAD("cut", plan_gadget_cut(P, "g", Lt, v, 2, (u64)1 << 32, pa, pb, ntt)); // n size E at 2^32
        BAD("cut", plan_gadget_cut(P, "g", Lt, 63, 2, (u64)1 << 28, pa, pb, ntt)); // the grid of one launch
        BAD("cut", plan_gadget_cut(P, "g", Lt, v, 2, 1, pb, pb, ntt));
        BAD("cut", plan_gadget_cut(P, "g", Lt, v, 2, 1, at(pb, N), pb, ntt));
        for (int lv : {1, Lt}) {
            const u64 e = bfv_gadget_table(level_primes(P, lv).data(), lv, v).total, end = 2 * e * (ntt ? lv : 1) * N;
            BAD("cut", plan_gadget_cut(P, "g", lv, v, 2, 1, at(pb, end - 1), pb, ntt));
            GOOD("cut", plan_gadget_cut(P, "g", lv, v, 2, 1, at(pb, end), pb, ntt));
        }
        GOOD("cut", if (plan_gadget_cut(P, "g", Lt, v, 3, 1, pa, pb, ntt).F != 3 * E) throw std::invalid_argument("F"));
    }
    for (int L : {0, Lt + 1, -1}) BAD("rgsw", plan_rgsw(P, L, v, 1, pa, pb));
    for (int w : {0, 64, -1}) BAD("rgsw", plan_rgsw(P, Lt, w, 1, pa, pb));
    BAD("rgsw", plan_rgsw(P, Lt, v, 1, pb, pb));
    BAD("rgsw", plan_rgsw(P, Lt, v, 1, at(pb, 2 * E * per - N), pb));
    BAD("rgsw", plan_rgsw(P, Lt, v, (u64)1 << 31, pa, pb));
    BAD("rgsw", plan_rgsw(P, Lt, v, ~(u64)0, pa, pb));
    GOOD("rgsw", if (plan_rgsw(P, Lt, v, 1, pa, pb).rows != 2 * E) throw std::invalid_argument("rows"));
    GOOD("rgsw", plan_rgsw(P, 1, v, 1, at(pb, 2 * E * per), pb));
    auto ep = [&](int L, int w, u64 n, u64 inner, const u64 *ct, u64 sr, u64 sk, const u64 *rg, u64 gr, u64 gk, const u64 *dst) {
        return plan_external_product(P, L, w, n, inner, ct, sr, sk, rg, gr, gk, dst);
    };
    const u64 *ct1 = at(pa, per);
    for (int L : {0, Lt + 1, -1}) BAD("ep", ep(L, v, 1, 1, ct1, 1, 1, pb, 0, 1, pa));
    for (int w : {0, 64, -1}) BAD("ep", ep(Lt, w, 1, 1, ct1, 1, 1, pb, 0, 1, pa));
    BAD("ep", ep(Lt, v, 1, 0, ct1, 1, 1, pb, 0, 1, pa));
    BAD("ep", ep(Lt, v, 0, 0, ct1, 1, 1, pb, 0, 1, pa));                           // n == 0 is still checked
    BAD("ep", ep(Lt, v, 1, ((u64)1 << 31) / (2 * E) + 1, ct1, 1, 1, pb, 0, 1, pa)); // inner 2E at 2^31
    BAD("ep", ep(Lt, v, 1, (u64)1 << 62, ct1, 1, 1, pb, 0, 1, pa));
    BAD("ep", ep(Lt, v, (u64)1 << 31, 1, ct1, 1, 1, pb, 0, 1, pa));                // the grid
    BAD("ep", ep(Lt, 63, (u64)1 << 29, 1, ct1, 1, 1, pb, 0, 1, pa));
    BAD("ep", ep(Lt, v, 2, 1, ct1, (u64)1 << 50, 1, pb, 0, 1, pa));                // strides that take a span past 2^60 words
    BAD("ep", ep(Lt, v, 2, 1, ct1, 1, 1, pb, (u64)1 << 63, 1, pa));
    BAD("ep", ep(Lt, v, 1, 2, ct1, 1, (u64)1 << 60, pb, 0, 1, pa));
    BAD("ep", ep(Lt, v, 2, 2, ct1, ~(u64)0, ~(u64)0, pb, 0, 1, pa));
    BAD("ep", ep(Lt, v, 1, 1, ct1, 1, 1, pb, 0, 1, ct1));                          // the output on / inside the ciphertext
    BAD("ep", ep(Lt, v, 1, 1, ct1, 1, 1, pb, 0, 1, at(pa, 2 * per - 1)));
    BAD("ep", ep(Lt, v, 1, 1, ct1, 1, 1, pb, 0, 1, at(pb, 2 * E * per - per)));    // ... inside the RGSW rows
    BAD("ep", ep(Lt, v, 2, 1, ct1, 1, 1, pb, 1, 1, at(pb, 2 * E * per)));          // the second selector row is read too
    BAD("ep", ep(Lt, v, 1, 2, pa, 1, 3, pb, 0, 1, at(pa, 3 * per)));               // ciphertext (0, 1) at stride 3
    GOOD("ep", ep(Lt, v, 1, 2, pa, 1, 2, pb, 0, 1, at(pa, 3 * per)));              // right behind it at stride 2
    GOOD("ep", ep(Lt, v, 1, 1, ct1, 1, 1, pb, 0, 1, at(pb, 2 * E * per)));         // right behind the one selector row
    GOOD("ep", ep(1, 63, 1, 1, ct1, 1, 1, pb, 0, 1, pa));
    GOOD("ep", const BfvExternalPlan pl = ep(Lt, v, 0, 1, ct1, 1, 1, pb, 0, 1, pa); if (pl.pass != 0 || pl.terms != 2 * E) throw std::invalid_argument("plan"));
    GOOD("ep", const BfvExternalPlan pl = ep(Lt, v, 3, 2, pa, 2, 1, pb, 0, 1, at(pa, 6 * per));
         if (pl.rows != 2 * E || pl.terms != 4 * E || pl.pass != bfv_gadget_pass(4 * E, 3, kGadgetPassPolys)) throw std::invalid_argument("plan"));

    // ---- selectors ---------------------------------------------------------------------------------------------------------------------
    auto se = [&](int L, int w, u64 n, u64 n_sel, u64 first, u64 count, const u64 *sel, const u64 *dst) { return plan_selector(P, L, w, n, n_sel, first, count, sel, dst); };
    auto fb = [&](int L, int w, int kw, u64 n, u64 n_sel, const u64 *ct, u64 sr, u64 sk, const u64 *key, const u64 *dst) {
        return plan_from_bfv(P, L, w, kw, n, n_sel, ct, sr, sk, key, dst);
    };
    for (int L : {0, Lt + 1, -1}) {
        BAD("selector", se(L, v, 1, 2, 3, 64, pa, pb));
        BAD("secret", check_rgsw_secret_args(P, L, v));
        BAD("from_bfv", fb(L, v, v, 1, 2, pa, 1, 1, pk, pb));
    }
    for (int w : {0, 64, -1}) {
        BAD("selector", se(Lt, w, 1, 2, 3, 64, pa, pb));
        BAD("secret", check_rgsw_secret_args(P, Lt, w));
        BAD("from_bfv", fb(Lt, w, v, 1, 2, pa, 1, 1, pk, pb));
        BAD("from_bfv", fb(Lt, v, w, 1, 2, pa, 1, 1, pk, pb));
    }
    BAD("selector", se(Lt, v, 1, 0, 3, 64, pa, pb));
    BAD("selector", se(Lt, v, 0, 0, 3, 64, pa, pb));
    BAD("selector", se(Lt, v, 1, 2, 3, 0, pa, pb));
    BAD("selector", se(Lt, v, 1, 1, 3, N + 1, pa, pb));
    BAD("selector", se(Lt, v, 1, 2, 3, (u64)1 << 63, pa, pb));
    BAD("selector", se(Lt, v, 1, 2, 64 - 2 * E + 1, 64, pa, pb));
    BAD("selector", se(Lt, v, 1, (u64)1 << 62, 3, 64, pa, pb));
    BAD("selector", se(Lt, v, 1, 2, ~(u64)0, 64, pa, pb));
    BAD("selector", se(Lt, v, 1, 2, 0, 2 * E - 1, pa, pb));
    BAD("selector", se(Lt, v, (u64)1 << 31, 2, 3, 64, pa, pb));
    BAD("selector", se(Lt, v, 1, 2, 3, 64, pb, pb));
    BAD("selector", se(Lt, v, 1, 2, 3, 64, at(pb, per - 1), pb));
    BAD("selector", se(Lt, v, 2, 2, 3, 64, at(pb, 2 * per - 1), pb));
    GOOD("selector", if (se(Lt, v, 1, 2, 3, 64, pa, pb).depth != 6) throw std::invalid_argument("depth"));
    GOOD("selector", se(1, 63, 1, 64, 0, 64, pa, pb));
    GOOD("selector", se(Lt, v, 1, 2, N - 2 * E, N, pa, pb));
    GOOD("selector", se(Lt, v, 1, 2, 3, 3 + 2 * E, pa, pb));
    GOOD("selector", se(Lt, v, 0, 2, 3, 64, pa, pb));
    GOOD("selector", se(Lt, v, 1, 2, 3, 64, at(pb, per), pb));
    GOOD("secret", check_rgsw_secret_args(P, Lt, v));
    GOOD("secret", check_rgsw_secret_args(P, 1, 1));
    BAD("from_bfv", fb(Lt, v, v, 1, 0, pa, 1, 1, pk, pb));
    BAD("from_bfv", fb(Lt, v, v, 0, 0, pa, 1, 1, pk, pb));
    BAD("from_bfv", fb(Lt, v, v, (u64)1 << 31, 2, pa, 1, 1, pk, pb));                // the grid
    BAD("from_bfv", fb(Lt, v, v, 1, (u64)1 << 31, pa, 1, 1, pk, pb));
    BAD("from_bfv", fb(Lt, v, v, (u64)1 << 20, (u64)1 << 20, pa, 1, 1, pk, pb));
    BAD("from_bfv", fb(Lt, v, v, 2, 2, pa, (u64)1 << 60, 1, pk, pb));                // strides that take a span past 2^60 words
    BAD("from_bfv", fb(Lt, v, v, 1, 2, pa, 1, (u64)1 << 60, pk, pb));
    BAD("from_bfv", fb(Lt, v, v, 2, 2, pa, (u64)1 << 63, 1, pk, pb));
    BAD("from_bfv", fb(Lt, v, v, 1, 2, pb, 1, 1, pk, pb));                           // the output on the ciphertexts
    BAD("from_bfv", fb(Lt, v, v, 1, 2, at(pb, 4 * E * per - 1), 1, 1, pk, pb));
    BAD("from_bfv", fb(Lt, v, v, 1, 2, pa, 1, 1, pk, at(pa, 2 * E * per - 1)));
    BAD("from_bfv", fb(Lt, v, v, 1, 1, pa, 1, 2, pk, at(pa, (2 * E - 2) * per)));    // the last one at stride 2
    BAD("from_bfv", fb(Lt, v, v, 1, 2, pa, 1, 1, pb, pb));                           // ... on the key
    BAD("from_bfv", fb(Lt, v, v, 1, 2, pa, 1, 1, at(pb, 4 * E * per - 1), pb));
    BAD("from_bfv", fb(Lt, v, v, 1, 2, pa, 1, 1, pk, at(pk, 2 * E * per - 1)));
    GOOD("from_bfv", const BfvFromBfvPlan pl = fb(Lt, v, v, 1, 2, pa, 1, 1, pk, pb);
         if (pl.rows != 2 * E || pl.C != 2 * E || pl.pass != bfv_gadget_pass(2 * E, 2 * E, kGadgetPassPolys) || pl.ktab.total != E) throw std::invalid_argument("plan"));
    GOOD("from_bfv", fb(1, 63, 1, 1, 2, pa, 1, 1, pk, pb));
    GOOD("from_bfv", const BfvFromBfvPlan pl = fb(Lt, v, v, 0, 2, pa, 1, 1, pk, pb); if (pl.C || pl.pass) throw std::invalid_argument("plan"));
    GOOD("from_bfv", fb(Lt, v, v, 1, 1, pa, 1, 2, pk, at(pa, (2 * E - 1) * per)));
    GOOD("from_bfv", fb(Lt, v, v, 1, 2, at(pb, 4 * E * per), 1, 1, pk, pb));

    // ---- database bytes ----------------------------------------------------------------------------------------------------------------
    const int w = bfv_bitlen(P.plain_modulus) - 1;
    const u64 Bmax = bfv_bytes_max(N, w), S = (Bmax + 7) / 8 * 8, NMAX = 0x7fffffffull / (N / 256);
    auto byte_at = [](const u64 *base, u64 bytes) { return (const void *)((unsigned long long)base + bytes); };
    auto un = [&](u64 n, const void *src, u64 stride, u64 B, const u64 *dst) { return plan_bytes(P, "b", n, src, stride, B, dst, false); };
    auto nt = [&](u64 n, const void *src, u64 stride, u64 B, const u64 *dst, int Lo) { return plan_bytes(P, "b", n, src, stride, B, dst, false, true, Lo); };
    auto pk8 = [&](u64 n, const u64 *src, u64 stride, u64 B, const void *dst) { return plan_bytes(P, "b", n, dst, stride, B, src, true); };
    for (int form = 0; form < 3; ++form) {
        auto f = [&](u64 n, u64 stride, u64 B) {
            if (form == 0) un(n, pb, stride, B, pa);
            else if (form == 1) nt(n, pb, stride, B, pa, Lt);
            else pk8(n, pa, stride == Bmax ? S : stride, B, pb);
        };
        BAD("bytes", f(2, Bmax, 0));
        BAD("bytes", f(2, Bmax, Bmax + 1));
        BAD("bytes", f(2, 8, 9));
        BAD("bytes", f(NMAX + 1, Bmax, Bmax));
        BAD("bytes", f((u64)1 << 40, Bmax, Bmax));
        BAD("bytes", f(3, (u64)1 << 63, Bmax));                                     // (n - 1) stride wraps / reaches 2^63
        BAD("bytes", f(2, ((u64)1 << 63) - 8, Bmax));
        GOOD("bytes", f(2, Bmax, Bmax));
    }
    for (int Lo : {0, Lt + 1, -1}) BAD("bytes", nt(2, pb, Bmax, Bmax, pa, Lo));
    BAD("bytes", un(2, pb, Bmax, Bmax, at(pa, 1)));                                 // a 16-byte aligned output
    BAD("bytes", pk8(2, pa, S, Bmax, byte_at(pb, 4)));
    BAD("bytes", pk8(2, pa, S + 4, Bmax, pb));
    BAD("bytes", pk8(2, pa, 8, 9, pb));
    BAD("bytes", pk8(2, pa, 12, 9, pb));
    BAD("bytes", un(1, byte_at(pa, 8 * N - 1), 1, 1, pa));                          // the bytes inside the words, last byte / first byte
    BAD("bytes", un(1, byte_at(pa, 3), Bmax, Bmax, pa));
    BAD("bytes", nt(1, byte_at(pa, 8 * Lt * N - 1), 1, 1, pa, Lt));
    BAD("bytes", pk8(1, pa, 8, 8, byte_at(pa, 8 * N - 8)));
    BAD("bytes", pk8(1, pa, S, Bmax, pa));
    GOOD("bytes", un(NMAX, byte_at(pa, 8 * NMAX * N), 1, 1, pa));                   // the largest grid, the bytes right behind its words
    GOOD("bytes", un(2, byte_at(pb, 3), Bmax + 5, Bmax, pa));
    GOOD("bytes", un(1, byte_at(pa, 8 * N), 1, 1, pa));
    GOOD("bytes", nt(1, byte_at(pa, 8 * Lt * N), 1, 1, pa, Lt));
    GOOD("bytes", un(1, byte_at(pa, 8 * N + 5), 3, 3, pa));
    GOOD("bytes", pk8(1, pa, 8, 8, byte_at(pa, 8 * N)));
    GOOD("bytes", pk8(2, pa, 16, 9, pb));
    GOOD("bytes", if (nt(2, pb, Bmax, Bmax, pa, 1).w != w) throw std::invalid_argument("w"));

    if (failures) return 1;
    std::printf("bfv_pir_args ok\n");
    return 0;
}
