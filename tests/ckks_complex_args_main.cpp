// ckks_complex_args_main.cpp -- TEST-ONLY, stand-alone.  Runs the device-free checks of the five complex-slot call families (csrc/cplx_args.h;
// csrc/poly_args.h for the two that take he355_combine_scalars' and he355_ckks_eval_poly's rules under their own names) at accepted and
// refused edge arguments: the codec (a BFV context, count at and past N / 2, scales, levels, ranges, null pointers, spans and wraps, the
// empty calls), the units and the residue pairs (levels, null, parts at and past 2^126 -- the imaginary part after its division by sqrt 2 --
// and the pairs themselves against u^2 = -2), the combination (both halves of every scalar and of the constant at q - 1 and q, and the
// real call's list of refusals with two residues per term) and the evaluation (null and non-finite imaginary parts, a coefficient that is
// zero only when both parts are, a plan equal to the real call's tree).  Compiled with -fsanitize=address,undefined
// (tests/test_ckks_complex_args_cpu.py).  Prints "ckks_complex_args ok" and exits 0, or names the first case that went the other way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/poly_args.h"
#include "args_main_common.h"

using namespace he355;

int main()
{
    const size_t N = 4096;
    std::unique_ptr<Params> pb(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    std::unique_ptr<Params> pc(Params::create(kSchemeCKKS, N, {60, 40, 40, 40, 40, 60}, 0, false));
    const Params &B = *pb, &Ck = *pc;
    const int Lt = (int)Ck.Ltop; // 5
    const size_t per = 2 * (size_t)Lt * N;
    std::vector<u64> a(4 * per), b(4 * per);
    std::vector<double> dv(4 * N);
    const u64 *pa = a.data(), *po = b.data();
    const double *pv = dv.data();
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double s40 = 0x1p40;

    // ---- he355_ckks_encode_complex
    GOOD("encode", if (plan_encode_complex(Ck, 2, pv, N / 2, s40, po)) throw std::invalid_argument("empty"));
    GOOD("encode one slot", plan_encode_complex(Ck, 2, pv, 1, s40, po));
    GOOD("encode no slot", plan_encode_complex(Ck, 2, nullptr, 0, s40, po));
    GOOD("encode n == 0", if (!plan_encode_complex(Ck, 0, nullptr, 8, s40, nullptr)) throw std::invalid_argument("not empty"));
    BAD("encode on BFV", plan_encode_complex(B, 2, pv, 8, s40, po));
    BAD("encode count", plan_encode_complex(Ck, 2, pv, N / 2 + 1, s40, po));
    BAD("encode count, n == 0", plan_encode_complex(Ck, 0, nullptr, N / 2 + 1, s40, nullptr));
    for (double s : {0.0, -1.0, inf, nan}) BAD("encode scale", plan_encode_complex(Ck, 2, pv, 8, s, po));
    BAD("encode null values", plan_encode_complex(Ck, 2, nullptr, 8, s40, po));
    BAD("encode null plain", plan_encode_complex(Ck, 2, pv, 8, s40, nullptr));
    BAD("encode span", plan_encode_complex(Ck, ~(u64)0, pv, 8, s40, mid));
    BAD("encode span", plan_encode_complex(Ck, ((u64)1 << 60) / (Lt * N) + 1, pv, 8, s40, mid));
    BAD("encode plain wraps", plan_encode_complex(Ck, 2, pv, 8, s40, high));
    BAD("encode values wrap", plan_encode_complex(Ck, 2, (const double *)high, N / 2, s40, po));

    // ---- he355_ckks_decode_complex / _slots
    SlotRanges sr;
    auto dec = [&](const Params &P, int L, u64 n, const u64 *plain, double scale, const u64 *ranges, u64 nr, bool slots, const double *out) {
        return plan_decode_complex(P, slots ? "he355_ckks_decode_complex_slots" : "he355_ckks_decode_complex", L, n, plain, scale, ranges, nr, slots, out, sr);
    };
    GOOD("decode", if (dec(Ck, Lt, 2, pa, s40, nullptr, 0, false, pv) || sr.total != N / 2) throw std::invalid_argument("ranges"));
    GOOD("decode at level 1", dec(Ck, 1, 2, pa, s40, nullptr, 0, false, pv));
    GOOD("decode n == 0", if (!dec(Ck, Lt, 0, nullptr, s40, nullptr, 0, false, nullptr)) throw std::invalid_argument("not empty"));
    BAD("decode on BFV", dec(B, 2, 2, pa, s40, nullptr, 0, false, pv));
    for (int l : {0, Lt + 1, -1}) BAD("decode level", dec(Ck, l, 2, pa, s40, nullptr, 0, false, pv));
    for (double s : {0.0, -1.0, inf, nan}) BAD("decode scale", dec(Ck, Lt, 2, pa, s, nullptr, 0, false, pv));
    BAD("decode null plain", dec(Ck, Lt, 2, nullptr, s40, nullptr, 0, false, pv));
    BAD("decode null out", dec(Ck, Lt, 2, pa, s40, nullptr, 0, false, nullptr));
    BAD("decode span", dec(Ck, Lt, ((u64)1 << 60) / (Lt * N) + 1, low, s40, nullptr, 0, false, pv));
    BAD("decode plain wraps", dec(Ck, Lt, 2, high, s40, nullptr, 0, false, pv));
    BAD("decode out wraps", dec(Ck, Lt, 2, pa, s40, nullptr, 0, false, (const double *)high));
    {
        const u64 two[4] = {0, 3, N / 2 - 2, 2}, past[2] = {N / 2 - 1, 2}, first[2] = {N / 2 + 1, 0}, none[2] = {5, 0}, five[10] = {0, 1, 1, 1, 2, 1, 3, 1, 4, 1};
        GOOD("two ranges", if (dec(Ck, Lt, 2, pa, s40, two, 2, true, pv) || sr.total != 5 || sr.n != 2) throw std::invalid_argument("ranges"));
        GOOD("an empty range touches nothing", if (!dec(Ck, Lt, 2, nullptr, s40, none, 1, true, nullptr)) throw std::invalid_argument("not empty"));
        GOOD("four ranges", dec(Ck, Lt, 2, pa, s40, five, 4, true, pv));
        BAD("a range past the slots", dec(Ck, Lt, 2, pa, s40, past, 1, true, pv));
        BAD("a range that starts past the slots", dec(Ck, Lt, 2, pa, s40, first, 1, true, pv));
        BAD("five ranges", dec(Ck, Lt, 2, pa, s40, five, 5, true, pv));
        BAD("no range", dec(Ck, Lt, 2, pa, s40, two, 0, true, pv));
        BAD("null ranges", dec(Ck, Lt, 2, pa, s40, nullptr, 1, true, pv));
    }

    // ---- he355_ckks_complex_unit, he355_ckks_complex_scalar_residues
    std::vector<u64> u(Lt), r(2 * Lt);
    const std::string wu("he355_ckks_complex_unit"), ws("he355_ckks_complex_scalar_residues");
    GOOD("units", cplx_units(Ck, wu, Lt, u.data()); for (int i = 0; i < Lt; ++i) {
        const u64 q = Ck.primes[i].q;
        if (u[i] >= q || (u64)(((u128)u[i] * u[i] + 2) % q) != 0) throw std::invalid_argument("u^2 != -2");
    });
    GOOD("units on BFV", std::vector<u64> ub(3); cplx_units(B, wu, 3, ub.data()));
    for (int l : {0, Lt + 1, -1}) BAD("units level", cplx_units(Ck, wu, l, u.data()));
    BAD("units null", cplx_units(Ck, wu, Lt, nullptr));
    GOOD("a real scalar gives equal halves", cplx_scalar_residues(Ck, ws, Lt, -1.0, 0.0, r.data()); for (int i = 0; i < Lt; ++i) if (r[i] != Ck.primes[i].q - 1 || r[Lt + i] != r[i]) throw std::invalid_argument("-1"));
    GOOD("i sqrt 2 is u", cplx_scalar_residues(Ck, ws, Lt, 0.0, std::sqrt(2.0), r.data()); for (int i = 0; i < Lt; ++i) if (r[i] != u[i] || r[Lt + i] != Ck.primes[i].q - u[i]) throw std::invalid_argument("u"));
    GOOD("the halves sum to 2 A", cplx_scalar_residues(Ck, ws, Lt, 12345.0, -6789.0, r.data()); for (int i = 0; i < Lt; ++i) if ((r[i] + r[Lt + i]) % Ck.primes[i].q != 24690) throw std::invalid_argument("2 A"));
    GOOD("2^125 and 2^126 / sqrt 2", cplx_scalar_residues(Ck, ws, Lt, 0x1p125, 0x1p126, r.data()));
    for (double v : {0x1p126, -0x1p126, inf, nan}) BAD("the real part", cplx_scalar_residues(Ck, ws, Lt, v, 1.0, r.data()));
    for (double v : {0x1p127, -0x1p127, inf, nan}) BAD("the imaginary part", cplx_scalar_residues(Ck, ws, Lt, 1.0, v, r.data()));
    for (int l : {0, Lt + 1}) BAD("residues level", cplx_scalar_residues(Ck, ws, l, 1.0, 1.0, r.data()));
    BAD("residues null", cplx_scalar_residues(Ck, ws, Lt, 1.0, 1.0, nullptr));

    // ---- he355_combine_scalars_complex: L = 3, two terms at levels 3 and 5, scalars [2 terms][2][L], constant [2][L]
    const int L = 3;
    std::vector<u64> sc(2 * 2 * L), cs(2 * L);
    for (int h = 0; h < 2; ++h)
        for (int i = 0; i < L; ++i) sc[h * L + i] = sc[2 * L + h * L + i] = cs[h * L + i] = Ck.primes[i].q - 1;
    he355_term tt[2] = {{pa, 3, 0}, {pa, 5, 0}};
    auto comb = [&](const Params &P, int l, int size, u64 n, const he355_term *t, u64 nt, const u64 *s, const u64 *c, const u64 *out) {
        try {
            return plan_combine_scalars(P, l, size, n, t, nt, s, c, out, 2);
        } catch (const std::invalid_argument &e) {
            if (std::string(e.what()).rfind("he355_combine_scalars_complex: ", 0) != 0) {
                std::printf("a refusal under another call's name: %s\n", e.what());
                ++failures;
            }
            throw;
        }
    };
    GOOD("combine", if (comb(Ck, L, 2, 4, tt, 2, sc.data(), cs.data(), po)) throw std::invalid_argument("empty"));
    GOOD("combine on BFV", const u64 ones[4] = {1, B.primes[1].q - 1, 0, 1}; comb(B, 2, 2, 1, tt, 1, ones, nullptr, po));
    GOOD("a repeated pointer, size 3", comb(Ck, L, 3, 2, tt, 2, sc.data(), nullptr, po));
    for (int l : {0, Lt + 1, -1}) BAD("level", comb(Ck, l, 2, 4, tt, 2, sc.data(), cs.data(), po));
    for (int size : {1, 4, 0}) BAD("size", comb(Ck, L, size, 4, tt, 2, sc.data(), cs.data(), po));
    {
        he355_term lowt[2] = {{pa, 3, 0}, {pa, 2, 0}}, hight[2] = {{pa, Lt + 1, 0}, {pa, 3, 0}}, nullt[2] = {{pa, 3, 0}, {nullptr, 3, 0}};
        BAD("a term below the call's level", comb(Ck, L, 2, 4, lowt, 2, sc.data(), cs.data(), po));
        BAD("a term above the top", comb(Ck, L, 2, 4, hight, 2, sc.data(), cs.data(), po));
        BAD("a null term", comb(Ck, L, 2, 4, nullt, 2, sc.data(), cs.data(), po));
        GOOD("a null term, n == 0", if (!comb(Ck, L, 2, 0, nullt, 2, sc.data(), cs.data(), nullptr)) throw std::invalid_argument("not empty"));
    }
    BAD("null terms", comb(Ck, L, 2, 4, nullptr, 2, sc.data(), cs.data(), po));
    BAD("null scalars", comb(Ck, L, 2, 4, tt, 2, nullptr, cs.data(), po));
    BAD("null output", comb(Ck, L, 2, 4, tt, 2, sc.data(), cs.data(), nullptr));
    BAD("too many terms", comb(Ck, L, 2, 4, tt, ((u64)1 << 20) + 1, sc.data(), cs.data(), po));
    {
        std::vector<he355_term> many((size_t)1 << 20, he355_term{pa, 3, 0});
        std::vector<u64> ms(((size_t)1 << 20) * 2 * L, 1);
        GOOD("2^20 terms", comb(Ck, L, 2, 4, many.data(), many.size(), ms.data(), nullptr, po));
    }
    for (int h = 0; h < 2; ++h)
        for (int i = 0; i < L; ++i) { // either half of the second term's scalar and of the constant
            std::vector<u64> s2 = sc, c2 = cs;
            s2[2 * L + h * L + i] = Ck.primes[i].q;
            c2[h * L + i] = Ck.primes[i].q;
            BAD("a scalar of q", comb(Ck, L, 2, 4, tt, 2, s2.data(), cs.data(), po));
            BAD("a constant of q", comb(Ck, L, 2, 4, tt, 2, sc.data(), c2.data(), po));
            s2[2 * L + h * L + i] = ~(u64)0;
            BAD("a scalar of 2^64 - 1", comb(Ck, L, 2, 4, tt, 2, s2.data(), cs.data(), po));
        }
    GOOD("n == 0", if (!comb(Ck, L, 2, 0, nullptr, 0, nullptr, nullptr, nullptr)) throw std::invalid_argument("not empty"));
    GOOD("no term, no constant", if (!comb(Ck, L, 2, 4, nullptr, 0, nullptr, nullptr, nullptr)) throw std::invalid_argument("not empty"));
    BAD("a constant alone", comb(Ck, L, 2, 4, nullptr, 0, nullptr, cs.data(), po));
    BAD("n == 0, bad level", comb(Ck, 0, 2, 0, nullptr, 0, nullptr, nullptr, nullptr));
    {
        he355_term lt[1] = {{low, 3, 0}}, ht[1] = {{high, 3, 0}}, l5[1] = {{low, 5, 0}};
        BAD("span", comb(Ck, L, 2, ~(u64)0, lt, 1, sc.data(), nullptr, mid));
        BAD("span", comb(Ck, L, 2, ((u64)1 << 60) / (2 * L * N) + 1, lt, 1, sc.data(), nullptr, mid));
        BAD("span of a higher term", comb(Ck, L, 2, ((u64)1 << 60) / (2 * 5 * N) + 1, l5, 1, sc.data(), nullptr, mid));
        GOOD("span", comb(Ck, L, 2, ((u64)1 << 44) / (2 * L * N), lt, 1, sc.data(), nullptr, mid));
        BAD("a term wraps", comb(Ck, L, 2, 2, ht, 1, sc.data(), nullptr, low));
        BAD("out wraps", comb(Ck, L, 2, 2, lt, 1, sc.data(), nullptr, high));
    }
    {
        const u64 w3 = 2 * 2 * 3 * N, w5 = 2 * 2 * 5 * N;
        he355_term t3[1] = {{pa, 3, 0}}, t5[1] = {{pa, 5, 0}};
        BAD("out at a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, pa));
        BAD("out one word inside a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, at(pa, w3 - 1)));
        GOOD("out right behind a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, at(pa, w3)));
        BAD("out inside the ignored rows of a higher term", comb(Ck, L, 2, 2, t5, 1, sc.data(), nullptr, at(pa, w5 - 1)));
        GOOD("out right behind a higher term", comb(Ck, L, 2, 2, t5, 1, sc.data(), nullptr, at(pa, w5)));
        he355_term second[2] = {{at(po, w3), 3, 0}, {po, 3, 0}};
        BAD("the second term under out", comb(Ck, L, 2, 2, second, 2, sc.data(), nullptr, po));
    }

    // ---- he355_ckks_eval_poly_complex
    const double re3[4] = {0.5, 0.15012, 0.0, -0.0015930078125}, im3[4] = {0.1, -0.25, 0.0, 0.05}, zero4[4] = {0, 0, 0, 0};
    const double reo[4] = {0.5, 0.0, 0.0, 0.0}, imo[4] = {0.0, 0.0, 0.0, 0.25}; // degree 3 by its imaginary part alone
    auto plan = [&](const Params &P, int l, u64 n, const u64 *in, const double *cr, const double *ci, u64 nc, int lb, double si, double so, const u64 *out) {
        return plan_eval_poly(P, "he355_ckks_eval_poly_complex", l, n, in, cr, nc, lb, si, so, out, true, 1024, ci, true);
    };
    GOOD("degree 3", const PolyPlan pl = plan(Ck, Lt, 4, pa, re3, im3, 4, 1, s40, s40, po);
         const PolyPlan rl = plan_eval_poly(Ck, "he355_ckks_eval_poly", Lt, 4, pa, re3, 4, 1, s40, s40, po, true, 1024);
         if (pl.info.depth != rl.info.depth || pl.info.products != rl.info.products || pl.info.combinations != rl.info.combinations || pl.steps.size() != rl.steps.size() ||
             pl.words_per_ct != rl.words_per_ct)
             throw std::invalid_argument("the tree is not the real call's");
         for (size_t k = 0; k < pl.steps.size(); ++k) {
             const PolyStep &s = pl.steps[k], &t = rl.steps[k];
             if (s.op != t.op || s.L != t.L || s.dst != t.dst) throw std::invalid_argument("step");
             if (s.op == kPolyCombine && (!s.cplx || t.cplx || s.scalars.size() != 2 * t.scalars.size() || s.cst.size() != 2 * t.cst.size())) throw std::invalid_argument("tables");
         });
    GOOD("zero imaginary parts: both halves are the real call's residues", const PolyPlan pl = plan(Ck, Lt, 4, pa, re3, zero4, 4, 1, s40, s40, po);
         const PolyPlan rl = plan_eval_poly(Ck, "he355_ckks_eval_poly", Lt, 4, pa, re3, 4, 1, s40, s40, po, true, 1024);
         if (pl.info.min_scalar_bits != rl.info.min_scalar_bits) throw std::invalid_argument("min_scalar_bits");
         for (size_t k = 0; k < pl.steps.size(); ++k) {
             const PolyStep &s = pl.steps[k], &t = rl.steps[k];
             if (s.op != kPolyCombine) continue;
             const size_t Lc = (size_t)s.L;
             for (size_t j = 0; j < t.scalars.size(); ++j)
                 if (s.scalars[(j / Lc) * 2 * Lc + j % Lc] != t.scalars[j] || s.scalars[(j / Lc) * 2 * Lc + Lc + j % Lc] != t.scalars[j]) throw std::invalid_argument("scalar");
             for (size_t j = 0; j < t.cst.size(); ++j)
                 if (s.cst[j] != t.cst[j] || s.cst[Lc + j] != t.cst[j]) throw std::invalid_argument("constant");
         });
    GOOD("a coefficient is zero when both parts are", const PolyPlan pl = plan(Ck, Lt, 4, pa, reo, imo, 4, 1, s40, s40, po); if (pl.info.degree != 3 || pl.info.depth != 2) throw std::invalid_argument("plan"));
    GOOD("n == 0", const PolyPlan pl = plan(Ck, Lt, 0, nullptr, re3, im3, 4, 1, s40, s40, nullptr); if (!pl.empty) throw std::invalid_argument("plan"));
    BAD("BFV", plan(B, 3, 4, pa, re3, im3, 4, 1, s40, s40, po));
    for (int l : {0, Lt + 1, -1}) BAD("level", plan(Ck, l, 4, pa, re3, im3, 4, 1, s40, s40, po));
    BAD("null imaginary parts", plan(Ck, Lt, 4, pa, re3, nullptr, 4, 1, s40, s40, po));
    BAD("null real parts", plan(Ck, Lt, 4, pa, nullptr, im3, 4, 1, s40, s40, po));
    BAD("a constant polynomial", plan(Ck, Lt, 4, pa, reo, zero4, 4, 1, s40, s40, po));
    BAD("no coefficients", plan(Ck, Lt, 4, pa, re3, im3, 0, 1, s40, s40, po));
    {
        double bad[4] = {0.1, nan, 0, 0.05};
        BAD("a nan imaginary part", plan(Ck, Lt, 4, pa, re3, bad, 4, 1, s40, s40, po));
        bad[1] = inf;
        BAD("an infinite imaginary part", plan(Ck, Lt, 4, pa, re3, bad, 4, 1, s40, s40, po));
        BAD("an infinite real part", plan(Ck, Lt, 4, pa, bad, im3, 4, 1, s40, s40, po));
        bad[1] = 0x1p100; // (c T) / s = 2^140
        BAD("an imaginary scalar past 2^126", plan(Ck, Lt, 4, pa, re3, bad, 4, 1, s40, s40, po));
        std::vector<double> many(1025, 0.0);
        many[1] = 1.0;
        BAD("1025 coefficients", plan(Ck, Lt, 4, pa, many.data(), many.data(), 1025, 1, s40, s40, po));
    }
    for (int lb : {0, 7}) BAD("log_baby", plan(Ck, Lt, 4, pa, re3, im3, 4, lb, s40, s40, po));
    for (double s : {0.0, -1.0, inf, nan}) {
        BAD("in_scale", plan(Ck, Lt, 4, pa, re3, im3, 4, 1, s, s40, po));
        BAD("out_scale", plan(Ck, Lt, 4, pa, re3, im3, 4, 1, s40, s, po));
    }
    BAD("depth == L", plan(Ck, 2, 4, pa, re3, im3, 4, 1, s40, s40, po));
    GOOD("depth == L - 1", plan(Ck, 3, 4, pa, re3, im3, 4, 1, s40, s40, po));
    BAD("null input", plan(Ck, Lt, 4, nullptr, re3, im3, 4, 1, s40, s40, po));
    BAD("null output", plan(Ck, Lt, 4, pa, re3, im3, 4, 1, s40, s40, nullptr));
    BAD("span", plan(Ck, Lt, ((u64)1 << 60) / per + 1, low, re3, im3, 4, 1, s40, s40, mid));
    BAD("wraps", plan(Ck, Lt, 2, high, re3, im3, 4, 1, s40, s40, low));
    BAD("out at in", plan(Ck, Lt, 4, pa, re3, im3, 4, 1, s40, s40, pa));
    BAD("out one word inside in", plan(Ck, Lt, 4, pa, re3, im3, 4, 1, s40, s40, at(pa, 4 * per - 1)));
    GOOD("out right behind in", plan(Ck, Lt, 4, pa, re3, im3, 4, 1, s40, s40, at(pa, 4 * per)));
    if (failures) return 1;
    std::printf("ckks_complex_args ok\n");
    return 0;
}
