// ckks_eval_poly_args_main.cpp -- TEST-ONLY, stand-alone.  Runs the device-free checks of he355_combine_scalars, he355_ckks_scalar_residues and
// he355_ckks_eval_poly (csrc/poly_args.h) at accepted and refused edge arguments -- levels at and past their ends, term levels below the
// call's and above the top, sizes 1 and 4, null lists and null terms, more than 2^20 terms, scalars and constants at q - 1 and q, spans at
// and past 2^60 words and past the end of the address space, overlaps one word inside and right behind (a higher term's ignored rows count),
// the empty calls; coefficient lists, log_baby, scales, depth at and past L -- and the plan it hands on: depth, counts, powers, buffers
// inside the block.  Compiled with -fsanitize=address,undefined (tests/test_ckks_eval_poly_args_cpu.py).  Prints
// "ckks_eval_poly_args ok" and exits 0, or names the first case that went the other way.
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
    std::unique_ptr<Params> p1(Params::create(kSchemeCKKS, N, {60}, 0, false)); // K = 1: no special prime
    const Params &B = *pb, &Ck = *pc;
    const int Lt = (int)Ck.Ltop; // 5
    const size_t per = 2 * (size_t)Lt * N;
    std::vector<u64> a(4 * per), b(4 * per);
    const u64 *pa = a.data(), *po = b.data();
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;

    // ---- he355_combine_scalars: L = 3, two terms at levels 3 and 5
    const int L = 3;
    std::vector<u64> sc(2 * L), cs(L);
    for (int i = 0; i < L; ++i) sc[i] = sc[L + i] = cs[i] = Ck.primes[i].q - 1;
    he355_term tt[2] = {{pa, 3, 0}, {pa, 5, 0}};
    auto comb = [&](const Params &P, int l, int size, u64 n, const he355_term *t, u64 nt, const u64 *s, const u64 *c, const u64 *out) {
        return plan_combine_scalars(P, l, size, n, t, nt, s, c, out);
    };
    GOOD("combine", if (comb(Ck, L, 2, 4, tt, 2, sc.data(), cs.data(), po)) throw std::invalid_argument("empty"));
    {
        const u64 ones[2] = {1, B.primes[1].q - 1};
        GOOD("combine on BFV", comb(B, 2, 2, 1, tt, 1, ones, nullptr, po));
    }
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
        std::vector<u64> ms(((size_t)1 << 20) * L, 1);
        GOOD("2^20 terms", comb(Ck, L, 2, 4, many.data(), many.size(), ms.data(), nullptr, po));
    }
    for (int i = 0; i < L; ++i) {
        std::vector<u64> s2 = sc, c2 = cs;
        s2[L + i] = Ck.primes[i].q;
        c2[i] = Ck.primes[i].q;
        BAD("a scalar of q", comb(Ck, L, 2, 4, tt, 2, s2.data(), cs.data(), po));
        BAD("a constant of q", comb(Ck, L, 2, 4, tt, 2, sc.data(), c2.data(), po));
        s2[L + i] = ~(u64)0;
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
        // n = 2: term 0 spans 2 * 2 * 3 * N words, term 1 (level 5) 2 * 2 * 5 * N -- its rows 3 and 4 are never read and still count
        const u64 w3 = 2 * 2 * 3 * N, w5 = 2 * 2 * 5 * N;
        he355_term t3[1] = {{pa, 3, 0}}, t5[1] = {{pa, 5, 0}};
        BAD("out at a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, pa));
        BAD("out one word inside a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, at(pa, w3 - 1)));
        GOOD("out right behind a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, at(pa, w3)));
        BAD("out inside the ignored rows of a higher term", comb(Ck, L, 2, 2, t5, 1, sc.data(), nullptr, at(pa, w5 - 1)));
        GOOD("out right behind a higher term", comb(Ck, L, 2, 2, t5, 1, sc.data(), nullptr, at(pa, w5)));
        he355_term before[1] = {{at(po, w3 - 1), 3, 0}}, behind[1] = {{at(po, w3), 3, 0}};
        BAD("a term one word inside out", comb(Ck, L, 2, 2, before, 1, sc.data(), nullptr, po));
        GOOD("a term right behind out", comb(Ck, L, 2, 2, behind, 1, sc.data(), nullptr, po));
        he355_term second[2] = {{at(po, w3), 3, 0}, {po, 3, 0}};
        BAD("the second term under out", comb(Ck, L, 2, 2, second, 2, sc.data(), nullptr, po));
    }

    // ---- he355_ckks_scalar_residues
    {
        std::vector<u64> r(Lt);
        const std::string w("he355_ckks_scalar_residues");
        GOOD("residues", poly_scalar_residues(Ck, w, Lt, -1.0, r.data()); for (int i = 0; i < Lt; ++i) if (r[i] != Ck.primes[i].q - 1) throw std::invalid_argument("-1"));
        GOOD("2^125", poly_scalar_residues(Ck, w, Lt, 0x1p125, r.data()));
        GOOD("ties to even", poly_scalar_residues(Ck, w, 1, 2.5, r.data()); if (r[0] != 2) throw std::invalid_argument("2.5"));
        BAD("2^126", poly_scalar_residues(Ck, w, Lt, 0x1p126, r.data()));
        BAD("-2^126", poly_scalar_residues(Ck, w, Lt, -0x1p126, r.data()));
        BAD("inf", poly_scalar_residues(Ck, w, Lt, std::numeric_limits<double>::infinity(), r.data()));
        BAD("nan", poly_scalar_residues(Ck, w, Lt, std::nan(""), r.data()));
        BAD("level", poly_scalar_residues(Ck, w, 0, 1.0, r.data()));
        BAD("level", poly_scalar_residues(Ck, w, Lt + 1, 1.0, r.data()));
        BAD("null", poly_scalar_residues(Ck, w, Lt, 1.0, nullptr));
    }

    // ---- he355_ckks_eval_poly
    const double s40 = 0x1p40;
    const double c3[4] = {0.5, 0.15012, 0.0, -0.0015930078125}, c7[8] = {0, 1, 0, -0.3, 0, 0.1, 0, -0.01};
    auto plan = [&](const Params &P, int l, u64 n, const u64 *in, const double *c, u64 nc, int lb, double si, double so, const u64 *out) {
        return plan_eval_poly(P, "he355_ckks_eval_poly", l, n, in, c, nc, lb, si, so, out, true, 1024);
    };
    GOOD("degree 3", const PolyPlan pl = plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, po);
         if (pl.empty || pl.info.depth != 2 || pl.info.L_out != Lt - 2 || pl.info.degree != 3 || pl.info.products != 2 || pl.info.combinations != 2 || pl.info.rescales != 2 ||
             pl.info.adds != 1 || pl.info.powers != 1 || pl.info.power_mask[0] != 4 || pl.info.chunks != 1 || pl.info.min_scalar_bits < 20)
             throw std::invalid_argument("plan"));
    GOOD("degree 7, odd", const PolyPlan pl = plan(Ck, Lt, 4, pa, c7, 8, 1, s40, s40, po); if (pl.info.depth != 3 || pl.info.powers != 2) throw std::invalid_argument("plan"));
    GOOD("degree 7, four babies", const PolyPlan pl = plan(Ck, Lt, 4, pa, c7, 8, 2, s40, s40, po); if (pl.info.depth != 4 || pl.info.L_out != 1) throw std::invalid_argument("plan"));
    GOOD("the plan's buffers lie inside its block", const PolyPlan pl = plan(Ck, Lt, 4, pa, c7, 8, 1, s40, s40, po);
         for (const PolyBuf &bf : pl.bufs) if (bf.kind == 2 && bf.off + 2 * (u64)bf.L * N > pl.words_per_ct) throw std::invalid_argument("buffer");
         for (const PolyStep &st : pl.steps) if (st.dst < 0 || (size_t)st.dst >= pl.bufs.size() || pl.bufs[(size_t)st.dst].kind == 0) throw std::invalid_argument("step"));
    GOOD("trailing zeros are trimmed", const double z[6] = {0.5, 0.25, 0, 0, 0, 0}; const PolyPlan pl = plan(Ck, Lt, 4, pa, z, 6, 1, s40, s40, po);
         if (pl.info.degree != 1 || pl.info.depth != 1 || pl.info.products != 0) throw std::invalid_argument("plan"));
    GOOD("n == 0", const PolyPlan pl = plan(Ck, Lt, 0, nullptr, c3, 4, 1, s40, s40, nullptr); if (!pl.empty || pl.info.chunks != 0) throw std::invalid_argument("plan"));
    BAD("BFV", plan(B, 3, 4, pa, c3, 4, 1, s40, s40, po));
    BAD("K < 2", plan(*p1, 1, 4, pa, c3, 2, 1, s40, s40, po));
    for (int l : {0, Lt + 1, -1}) BAD("level", plan(Ck, l, 4, pa, c3, 4, 1, s40, s40, po));
    BAD("n == 0, bad level", plan(Ck, 0, 0, nullptr, c3, 4, 1, s40, s40, nullptr));
    {
        const double only0[3] = {1.0, 0.0, 0.0};
        BAD("a constant polynomial", plan(Ck, Lt, 4, pa, only0, 3, 1, s40, s40, po));
        BAD("no coefficients", plan(Ck, Lt, 4, pa, c3, 0, 1, s40, s40, po));
        BAD("null coefficients", plan(Ck, Lt, 4, pa, nullptr, 4, 1, s40, s40, po));
        std::vector<double> many(1025, 0.0);
        many[1] = 1.0;
        BAD("1025 coefficients", plan(Ck, Lt, 4, pa, many.data(), 1025, 1, s40, s40, po));
        GOOD("1024 coefficients, degree 1", plan(Ck, Lt, 4, pa, many.data(), 1024, 1, s40, s40, po));
        double bad[4] = {0.5, std::nan(""), 0, 1};
        BAD("a nan coefficient", plan(Ck, Lt, 4, pa, bad, 4, 1, s40, s40, po));
        bad[1] = std::numeric_limits<double>::infinity();
        BAD("an infinite coefficient", plan(Ck, Lt, 4, pa, bad, 4, 1, s40, s40, po));
        bad[1] = 0x1p100; // (c T) / s = 2^140: a scalar he355_ckks_scalar_residues refuses
        BAD("a scalar past 2^126", plan(Ck, Lt, 4, pa, bad, 4, 1, s40, s40, po));
    }
    for (int lb : {0, 7, -1}) BAD("log_baby", plan(Ck, Lt, 4, pa, c3, 4, lb, s40, s40, po));
    GOOD("log_baby 6", plan(Ck, Lt, 4, pa, c3, 4, 6, s40, s40, po));
    for (double s : {0.0, -1.0, std::numeric_limits<double>::infinity(), std::nan("")}) {
        BAD("in_scale", plan(Ck, Lt, 4, pa, c3, 4, 1, s, s40, po));
        BAD("out_scale", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s, po));
    }
    BAD("depth == L", plan(Ck, 2, 4, pa, c3, 4, 1, s40, s40, po));
    GOOD("depth == L - 1", plan(Ck, 3, 4, pa, c3, 4, 1, s40, s40, po));
    BAD("depth > L", plan(Ck, 1, 4, pa, c3, 4, 1, s40, s40, po));
    BAD("null input", plan(Ck, Lt, 4, nullptr, c3, 4, 1, s40, s40, po));
    BAD("null output", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, nullptr));
    BAD("span", plan(Ck, Lt, ~(u64)0, low, c3, 4, 1, s40, s40, mid));
    BAD("span", plan(Ck, Lt, ((u64)1 << 60) / per + 1, low, c3, 4, 1, s40, s40, mid));
    GOOD("span", plan(Ck, Lt, ((u64)1 << 44) / per, low, c3, 4, 1, s40, s40, mid));
    BAD("wraps", plan(Ck, Lt, 2, high, c3, 4, 1, s40, s40, low));
    BAD("wraps", plan(Ck, Lt, 2, low, c3, 4, 1, s40, s40, high));
    BAD("out at in", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, pa));
    BAD("out one word inside in", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, at(pa, 4 * per - 1)));
    GOOD("out right behind in", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, at(pa, 4 * per)));
    BAD("in one word inside out", plan(Ck, Lt, 4, at(po, 4 * 2 * (Lt - 2) * N - 1), c3, 4, 1, s40, s40, po)); // out is [4][2][L - depth][N]
    GOOD("in right behind out", plan(Ck, Lt, 4, at(po, 4 * 2 * (Lt - 2) * N), c3, 4, 1, s40, s40, po));
    if (failures) return 1;
    std::printf("ckks_eval_poly_args ok\n");
    return 0;
}
