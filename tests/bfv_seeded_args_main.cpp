// bfv_seeded_args_main.cpp -- TEST-ONLY, stand-alone.  Runs the device-free checks of the seeded calls (csrc/bfv_pir_args.h: plan_seeded_encrypt,
// plan_seeded_selector, plan_seeded_restore, plan_keygen_galois_seeded, plan_set_galois_key_seeded) at accepted and refused edge arguments --
// levels at and past their ends, ntt_form outside {0, 1}, equal seeds, first_index + n at 2^40, above it and wrapping 2^64, slabs past 2^60
// words, grids at 2^31, spans that pass the end of the address space, overlaps one word inside and right behind, the selector rules, Galois
// elements at their ends -- compiled with -fsanitize=address,undefined (tests/test_bfv_seeded_args_cpu.py).  The checks do arithmetic on counts,
// indices and addresses the caller chose: none of it may overflow a signed type, shift out of range or form a pointer outside its slab before
// the refusal.  Prints "bfv_seeded_args ok" and exits 0, or names the first case that went the other way.
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
    std::unique_ptr<Params> pp(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    const Params &P = *pp;
    const int Lt = (int)P.Ltop;
    std::vector<u64> c0v(4 * (size_t)Lt * N), outv(4 * 2 * (size_t)Lt * N), plv(4 * N);
    const u64 *c0 = c0v.data(), *out = outv.data(), *pl = plv.data();
    auto wat = [](const void *base, u64 bytes) { return (const u64 *)((unsigned long long)base + bytes); };
    const u64 *low = (const u64 *)0x1000, *mid = (const u64 *)0x4000000000000000ull, *high = (const u64 *)0xfffffffffffff000ull;
    const u64 A = 11, E = 12, TOP = (u64)1 << 40;
    auto enc = [&](int L, u64 n, const u64 *plain, u64 a, u64 e, u64 first, const u64 *dst) { plan_seeded_encrypt(P, L, n, plain, a, e, first, dst); };
    auto res = [&](int L, int form, u64 n, const u64 *src, u64 first, const u64 *dst) { plan_seeded_restore(P, L, form, n, src, first, dst); };
    auto sel = [&](int L, int v, u64 n, u64 n_sel, u64 slot, u64 count, const u64 *s, u64 a, u64 e, u64 first, const u64 *dst) {
        return plan_seeded_selector(P, L, v, n, n_sel, slot, count, s, a, e, first, dst);
    };
    // ---- encrypt -------------------------------------------------------------------------------------------------------------------------
    GOOD("encrypt", enc(Lt, 4, pl, A, E, 0, c0));
    GOOD("encrypt", enc(1, 4, nullptr, A, E, 0, c0));
    for (int L : {0, Lt + 1, -1, 1 << 30}) BAD("encrypt", enc(L, 1, pl, A, E, 0, c0));
    BAD("encrypt", enc(Lt, 1, pl, A, A, 0, c0));
    BAD("encrypt", enc(Lt, 1, pl, 0, 0, 0, c0));
    GOOD("encrypt", enc(Lt, 1, pl, A, A + 1, 0, c0));
    // first_index + n
    GOOD("encrypt", enc(Lt, 4, pl, A, E, TOP - 4, c0));
    BAD("encrypt", enc(Lt, 4, pl, A, E, TOP - 3, c0));
    BAD("encrypt", enc(Lt, 1, pl, A, E, TOP, c0));
    GOOD("encrypt", enc(Lt, 0, pl, A, E, TOP, c0));
    BAD("encrypt", enc(Lt, 0, pl, A, E, TOP + 1, c0));
    BAD("encrypt", enc(Lt, 2, pl, A, E, ~(u64)0 - 1, c0));   // wraps to 0
    BAD("encrypt", enc(Lt, 1, pl, A, E, ~(u64)0, c0));
    BAD("encrypt", enc(Lt, ~(u64)0, pl, A, E, 1, c0));
    // one launch, 2^60 words
    const u64 nmax = 0x7fffffffull / ((u64)Lt * (N / 512));
    GOOD("encrypt", enc(Lt, nmax, nullptr, A, E, 0, low));
    BAD("encrypt", enc(Lt, nmax + 1, nullptr, A, E, 0, low));
    BAD("encrypt", enc(1, (u64)1 << 39, nullptr, A, E, 0, low));
    BAD("encrypt", enc(Lt, (u64)1 << 49, nullptr, A, E, 0, low));   // past 2^60 words (and past 2^40 indices)
    BAD("encrypt", enc(1, ~(u64)0, nullptr, A, E, 0, low));
    // the address space
    BAD("encrypt", enc(Lt, 1, nullptr, A, E, 0, high));
    BAD("encrypt", enc(Lt, 1, wat(high, 0), A, E, 0, c0));
    GOOD("encrypt", enc(Lt, 0, wat(high, 0), A, E, 0, high));
    GOOD("encrypt", enc(Lt, nmax, mid, A, E, 0, low));
    // overlaps
    BAD("encrypt", enc(Lt, 2, c0, A, E, 0, c0));
    BAD("encrypt", enc(Lt, 2, wat(c0, 8 * 2 * (u64)Lt * N - 8), A, E, 0, c0));   // the plaintexts start on c0's last word
    GOOD("encrypt", enc(Lt, 2, wat(c0, 8 * 2 * (u64)Lt * N), A, E, 0, c0));
    BAD("encrypt", enc(Lt, 2, pl, A, E, 0, wat(pl, 8 * 2 * N - 8)));
    GOOD("encrypt", enc(Lt, 2, pl, A, E, 0, wat(pl, 8 * 2 * N)));
    GOOD("encrypt", enc(1, 2, wat(c0, 8 * 2 * N), A, E, 0, c0));                 // lower levels write less
    // ---- restore -------------------------------------------------------------------------------------------------------------------------
    GOOD("restore", res(Lt, 0, 4, c0, 0, out));
    GOOD("restore", res(1, 1, 4, c0, TOP - 4, out));
    for (int L : {0, Lt + 1, -1}) BAD("restore", res(L, 0, 1, c0, 0, out));
    for (int f : {2, -1, 1 << 30, -(1 << 30)}) BAD("restore", res(Lt, f, 1, c0, 0, out));
    BAD("restore", res(Lt, 0, 4, c0, TOP - 3, out));
    BAD("restore", res(Lt, 0, 2, c0, ~(u64)0, out));
    const u64 rmax = 0x7fffffffull / (2 * (u64)Lt * (N / 512));
    GOOD("restore", res(Lt, 0, rmax, mid, 0, low));
    BAD("restore", res(Lt, 0, rmax + 1, mid, 0, low));
    BAD("restore", res(Lt, 1, (u64)1 << 50, mid, 0, low));
    BAD("restore", res(Lt, 0, 1, c0, 0, high));
    BAD("restore", res(Lt, 0, 1, high, 0, out));
    GOOD("restore", res(Lt, 0, 0, high, 0, high));
    BAD("restore", res(Lt, 0, 2, out, 0, out));
    BAD("restore", res(Lt, 0, 2, wat(out, 8 * 4 * (u64)Lt * N - 8), 0, out));    // c0 starts on the output's last word
    GOOD("restore", res(Lt, 0, 2, wat(out, 8 * 4 * (u64)Lt * N), 0, out));
    BAD("restore", res(Lt, 1, 2, c0, 0, wat(c0, 8 * 2 * (u64)Lt * N - 8)));
    GOOD("restore", res(Lt, 1, 2, c0, 0, wat(c0, 8 * 2 * (u64)Lt * N)));
    // ---- selector_encrypt ----------------------------------------------------------------------------------------------------------------
    const BfvDigitTab tab = bfv_gadget_table(level_primes(P, Lt).data(), Lt, 16);
    const u64 Et = tab.total;
    if (Et != 4 + 3 + 3) { std::printf("E(L_top) at 16 bits\n"); return 1; }
    if (sel(Lt, 16, 2, 2, 3, 64, pl, A, E, 0, c0).depth != 6) { std::printf("plan depth\n"); return 1; }
    GOOD("selector", sel(Lt, 16, 2, 2, 64 - 2 * Et, 64, pl, A, E, TOP - 2, c0));
    BAD("selector", sel(Lt, 16, 2, 2, 64 - 2 * Et + 1, 64, pl, A, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, 0, 0, 64, pl, A, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, 1, 0, 0, pl, A, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, 1, 0, N + 1, pl, A, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, ~(u64)0, 1, N, pl, A, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, 1, ~(u64)0, N, pl, A, E, 0, c0));
    for (int v : {0, 64, -1}) BAD("selector", sel(Lt, v, 2, 1, 0, 64, pl, A, E, 0, c0));
    for (int L : {0, Lt + 1}) BAD("selector", sel(L, 16, 2, 1, 0, 64, pl, A, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, 2, 0, 64, pl, E, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, 2, 0, 64, pl, A, E, TOP - 1, c0));
    BAD("selector", sel(Lt, 16, nmax + 1, 2, 0, 64, mid, A, E, 0, low));
    GOOD("selector", sel(Lt, 16, nmax, 2, 0, 64, mid, A, E, 0, low));
    BAD("selector", sel(Lt, 16, 2, 2, 0, 64, c0, A, E, 0, c0));
    BAD("selector", sel(Lt, 16, 2, 2, 0, 64, pl, A, E, 0, wat(pl, 8 * 4 - 8)));   // c0 starts on the last selector
    GOOD("selector", sel(Lt, 16, 2, 2, 0, 64, pl, A, E, 0, wat(pl, 8 * 4)));
    GOOD("selector", sel(Lt, 16, 0, 2, 0, 64, high, A, E, TOP, high));
    // ---- Galois keys ---------------------------------------------------------------------------------------------------------------------
    GOOD("keygen", plan_keygen_galois_seeded(P, 3, A, E));
    GOOD("keygen", plan_keygen_galois_seeded(P, (uint32_t)(2 * N - 1), A, E));
    for (uint32_t elt : {0u, 1u, 2u, 4u, (uint32_t)(2 * N), (uint32_t)(2 * N + 1), 0xffffffffu}) {
        BAD("keygen", plan_keygen_galois_seeded(P, elt, A, E));
        BAD("set", plan_set_galois_key_seeded(P, elt, pl));
    }
    BAD("keygen", plan_keygen_galois_seeded(P, 3, A, A));
    GOOD("set", plan_set_galois_key_seeded(P, 3, pl));
    BAD("set", plan_set_galois_key_seeded(P, 3, nullptr));
    std::unique_ptr<Params> one(Params::create(kSchemeCKKS, N, {50}, 0, false)); // one prime: no special prime, no key switching (the C ABI refuses CKKS first)
    BAD("keygen", plan_keygen_galois_seeded(*one, 3, A, E));
    BAD("set", plan_set_galois_key_seeded(*one, 3, pl));
    if (failures) return 1;
    std::printf("bfv_seeded_args ok\n");
    return 0;
}
