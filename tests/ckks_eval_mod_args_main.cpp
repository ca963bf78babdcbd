// ckks_eval_mod_args_main.cpp -- TEST-ONLY, stand-alone.  Runs the device-free checks of he355_combine_scalars_rescale,
// he355_ckks_eval_chebyshev and he355_ckks_eval_mod (csrc/cheb_args.h over csrc/poly_args.h) at accepted and refused edge arguments -- L of
// 1 and 2, a BFV context, every refusal he355_combine_scalars has under the new name, the output's [L - 1] rows in the overlap rule (one word
// inside and right behind, a higher term's ignored rows count); coefficient lists, log_baby, scales, depth at and past L, a coefficient that
// overflows in the split, double_angles of -1, 0, 8 and 9 and depth + r at and past L -- and the plans it hands on: counts, the fused steps,
// buffers and the row block inside the pool block, the scales of the double angles.  Compiled with -fsanitize=address,undefined
// (tests/test_ckks_eval_mod_args_cpu.py).  Prints "ckks_eval_mod_args ok" and exits 0, or names the first case that went the other way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/cheb_args.h"
#include "args_main_common.h"

using namespace he355;

int main()
{
    const size_t N = 4096;
    std::unique_ptr<Params> pb(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    std::unique_ptr<Params> pc(Params::create(kSchemeCKKS, N, {60, 40, 40, 40, 40, 40, 40, 60}, 0, false));
    std::unique_ptr<Params> p1(Params::create(kSchemeCKKS, N, {60}, 0, false)); // K = 1: no special prime
    const Params &B = *pb, &Ck = *pc;
    const int Lt = (int)Ck.Ltop; // 7
    const size_t per = 2 * (size_t)Lt * N;
    std::vector<u64> a(4 * per), b(4 * per);
    const u64 *pa = a.data(), *po = b.data();
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;

    // ---- he355_combine_scalars_rescale: L = 3, two terms at levels 3 and 5
    const int L = 3;
    std::vector<u64> sc(2 * L), cs(L);
    for (int i = 0; i < L; ++i) sc[i] = sc[L + i] = cs[i] = Ck.primes[i].q - 1;
    he355_term tt[2] = {{pa, 3, 0}, {pa, 5, 0}};
    auto comb = [&](const Params &P, int l, int size, u64 n, const he355_term *t, u64 nt, const u64 *s, const u64 *c, const u64 *out) {
        return plan_combine_scalars_rescale(P, l, size, n, t, nt, s, c, out);
    };
    GOOD("fused", if (comb(Ck, L, 2, 4, tt, 2, sc.data(), cs.data(), po)) throw std::invalid_argument("empty"));
    {
        const u64 s2[4] = {Ck.primes[0].q - 1, Ck.primes[1].q - 1, 2, 0};
        GOOD("fused at L = 2", comb(Ck, 2, 2, 4, tt, 2, s2, s2, po));
    }
    GOOD("a repeated pointer, size 3", comb(Ck, L, 3, 2, tt, 2, sc.data(), nullptr, po));
    BAD("L = 1", comb(Ck, 1, 2, 4, tt, 2, sc.data(), cs.data(), po));
    BAD("L = 1, n == 0", comb(Ck, 1, 2, 0, nullptr, 0, nullptr, nullptr, nullptr));
    {
        const u64 ones[2] = {1, 1};
        BAD("BFV", comb(B, 2, 2, 1, tt, 1, ones, nullptr, po));
        BAD("BFV, n == 0", comb(B, 2, 2, 0, nullptr, 0, nullptr, nullptr, nullptr));
    }
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
    for (int i = 0; i < L; ++i) {
        std::vector<u64> s2 = sc, c2 = cs;
        s2[L + i] = Ck.primes[i].q;
        c2[i] = Ck.primes[i].q;
        BAD("a scalar of q", comb(Ck, L, 2, 4, tt, 2, s2.data(), cs.data(), po));
        BAD("a constant of q", comb(Ck, L, 2, 4, tt, 2, sc.data(), c2.data(), po));
    }
    GOOD("n == 0", if (!comb(Ck, L, 2, 0, nullptr, 0, nullptr, nullptr, nullptr)) throw std::invalid_argument("not empty"));
    GOOD("no term, no constant", if (!comb(Ck, L, 2, 4, nullptr, 0, nullptr, nullptr, nullptr)) throw std::invalid_argument("not empty"));
    BAD("a constant alone", comb(Ck, L, 2, 4, nullptr, 0, nullptr, cs.data(), po));
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
        // n = 2: term 0 spans 2 * 2 * 3 * N words, term 1 (level 5) 2 * 2 * 5 * N; the output 2 * 2 * (L - 1) * N
        const u64 w3 = 2 * 2 * 3 * N, w5 = 2 * 2 * 5 * N, wo = 2 * 2 * (L - 1) * N;
        he355_term t3[1] = {{pa, 3, 0}}, t5[1] = {{pa, 5, 0}};
        BAD("out at a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, pa));
        BAD("out one word inside a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, at(pa, w3 - 1)));
        GOOD("out right behind a term", comb(Ck, L, 2, 2, t3, 1, sc.data(), nullptr, at(pa, w3)));
        BAD("out inside the ignored rows of a higher term", comb(Ck, L, 2, 2, t5, 1, sc.data(), nullptr, at(pa, w5 - 1)));
        GOOD("out right behind a higher term", comb(Ck, L, 2, 2, t5, 1, sc.data(), nullptr, at(pa, w5)));
        he355_term before[1] = {{at(po, wo - 1), 3, 0}}, behind[1] = {{at(po, wo), 3, 0}};
        BAD("a term one word inside the [L - 1] output", comb(Ck, L, 2, 2, before, 1, sc.data(), nullptr, po));
        GOOD("a term right behind the [L - 1] output", comb(Ck, L, 2, 2, behind, 1, sc.data(), nullptr, po));
        he355_term second[2] = {{at(po, wo), 3, 0}, {po, 3, 0}};
        BAD("the second term under out", comb(Ck, L, 2, 2, second, 2, sc.data(), nullptr, po));
    }

    // ---- he355_ckks_eval_chebyshev
    const double s40 = 0x1p40;
    const double c3[4] = {0.5, 0.15012, 0.0, -0.0015930078125}, c7[8] = {0, 1, 0, -0.3, 0, 0.1, 0, -0.01};
    auto plan = [&](const Params &P, int l, u64 n, const u64 *in, const double *c, u64 nc, int lb, double si, double so, const u64 *out) {
        return plan_eval_chebyshev(P, "he355_ckks_eval_chebyshev", l, n, in, c, nc, lb, si, so, out, true, 1024);
    };
    // degree 3 at m = 2: powers T_2 (a product and a fused step); e = 2, hi = {c_2, 2 c_3} = a leaf, lo = {c_0, c_1 - c_3} a leaf: an add
    GOOD("degree 3", const PolyPlan pl = plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, po);
         if (pl.empty || pl.info.depth != 2 || pl.info.L_out != Lt - 2 || pl.info.degree != 3 || pl.info.products != 2 || pl.info.combinations != 0 || pl.info.rescales != 3 ||
             pl.info.adds != 1 || pl.info.powers != 1 || pl.info.power_mask[0] != 4 || pl.info.chunks != 1 || pl.info.reserved[0] != 0)
             throw std::invalid_argument("plan"));
    GOOD("degree 7, odd", const PolyPlan pl = plan(Ck, Lt, 4, pa, c7, 8, 1, s40, s40, po); if (pl.info.depth != 3) throw std::invalid_argument("plan"));
    GOOD("the plan's buffers and its row block lie inside its block", const PolyPlan pl = plan(Ck, Lt, 4, pa, c7, 8, 2, s40, s40, po);
         for (const PolyBuf &bf : pl.bufs) if (bf.kind == 2 && bf.off + 2 * (u64)bf.L * N > pl.row_off) throw std::invalid_argument("buffer");
         if (pl.row_off + 2 * N != pl.words_per_ct) throw std::invalid_argument("row block");
         for (const PolyStep &st : pl.steps) {
             if (st.dst < 0 || (size_t)st.dst >= pl.bufs.size() || pl.bufs[(size_t)st.dst].kind == 0) throw std::invalid_argument("step");
             if (st.op == kPolyRescale) throw std::invalid_argument("a separate rescale");
             if (st.op == kPolyFused && (pl.bufs[(size_t)st.dst].L != st.L - 1 || st.scalars.size() != st.terms.size() * (size_t)st.L)) throw std::invalid_argument("fused step");
         });
    GOOD("n == 0", const PolyPlan pl = plan(Ck, Lt, 0, nullptr, c3, 4, 1, s40, s40, nullptr); if (!pl.empty || pl.info.chunks != 0) throw std::invalid_argument("plan"));
    BAD("BFV", plan(B, 3, 4, pa, c3, 4, 1, s40, s40, po));
    BAD("K < 2", plan(*p1, 1, 4, pa, c3, 2, 1, s40, s40, po));
    for (int l : {0, Lt + 1, -1}) BAD("level", plan(Ck, l, 4, pa, c3, 4, 1, s40, s40, po));
    {
        const double only0[3] = {1.0, 0.0, 0.0};
        BAD("a constant polynomial", plan(Ck, Lt, 4, pa, only0, 3, 1, s40, s40, po));
        BAD("no coefficients", plan(Ck, Lt, 4, pa, c3, 0, 1, s40, s40, po));
        BAD("null coefficients", plan(Ck, Lt, 4, pa, nullptr, 4, 1, s40, s40, po));
        std::vector<double> many(1025, 0.0);
        many[1] = 1.0;
        BAD("1025 coefficients", plan(Ck, Lt, 4, pa, many.data(), 1025, 1, s40, s40, po));
        double bad[4] = {0.5, std::nan(""), 0, 1};
        BAD("a nan coefficient", plan(Ck, Lt, 4, pa, bad, 4, 1, s40, s40, po));
        bad[1] = std::numeric_limits<double>::infinity();
        BAD("an infinite coefficient", plan(Ck, Lt, 4, pa, bad, 4, 1, s40, s40, po));
        bad[1] = 0x1p100;
        BAD("a scalar past 2^126", plan(Ck, Lt, 4, pa, bad, 4, 1, s40, s40, po));
        const double big = std::numeric_limits<double>::max();
        const double over[4] = {0.0, -big, 0.0, big}; // every coefficient finite; hi[1] = 2.0 * c_3 is not
        BAD("2 c_3 overflows in the split", plan(Ck, Lt, 4, pa, over, 4, 1, s40, s40, po));
    }
    for (int lb : {0, 7, -1}) BAD("log_baby", plan(Ck, Lt, 4, pa, c3, 4, lb, s40, s40, po));
    for (double s : {0.0, -1.0, std::numeric_limits<double>::infinity(), std::nan("")}) {
        BAD("in_scale", plan(Ck, Lt, 4, pa, c3, 4, 1, s, s40, po));
        BAD("out_scale", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s, po));
    }
    BAD("depth == L", plan(Ck, 2, 4, pa, c3, 4, 1, s40, s40, po));
    GOOD("depth == L - 1", plan(Ck, 3, 4, pa, c3, 4, 1, s40, s40, po));
    BAD("null input", plan(Ck, Lt, 4, nullptr, c3, 4, 1, s40, s40, po));
    BAD("null output", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, nullptr));
    BAD("span", plan(Ck, Lt, ((u64)1 << 60) / per + 1, low, c3, 4, 1, s40, s40, mid));
    BAD("wraps", plan(Ck, Lt, 2, high, c3, 4, 1, s40, s40, low));
    BAD("out at in", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, pa));
    BAD("out one word inside in", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, at(pa, 4 * per - 1)));
    GOOD("out right behind in", plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, at(pa, 4 * per)));

    // ---- he355_ckks_eval_mod
    auto mod = [&](const Params &P, int l, u64 n, const u64 *in, const double *c, u64 nc, int lb, double si, double so, int r, const u64 *out) {
        return plan_eval_mod(P, "he355_ckks_eval_mod", l, n, in, c, nc, lb, si, so, r, out, true, 1024);
    };
    GOOD("r = 0 is the Chebyshev plan", const PolyPlan p0 = mod(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, 0, po), pc0 = plan(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, po);
         if (p0.steps.size() != pc0.steps.size() || p0.info.depth != pc0.info.depth || p0.info.out_scale != s40 || p0.words_per_ct != pc0.words_per_ct) throw std::invalid_argument("plan"));
    GOOD("two double angles", const PolyPlan pl = mod(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, 2, po);
         if (pl.info.depth != 4 || pl.info.L_out != Lt - 4 || pl.info.products != 4 || pl.info.combinations != 2 || pl.info.rescales != 3 || pl.info.reserved[0] != 2 ||
             std::fabs(pl.info.out_scale / s40 - 1.0) > 1e-12 || pl.bufs[(size_t)pl.steps.back().dst].kind != 1)
             throw std::invalid_argument("plan"));
    GOOD("depth + r == L - 1", mod(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, 4, po));
    BAD("depth + r == L", mod(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, 5, po));
    BAD("double_angles -1", mod(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, -1, po));
    BAD("double_angles 9", mod(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, 9, po));
    BAD("double_angles 9, n == 0", mod(Ck, Lt, 0, nullptr, c3, 4, 1, s40, s40, 9, nullptr));
    BAD("BFV", mod(B, 3, 4, pa, c3, 4, 1, s40, s40, 1, po));
    BAD("out one word inside in", mod(Ck, Lt, 4, pa, c3, 4, 1, s40, s40, 2, at(pa, 4 * per - 1)));
    BAD("in one word inside out", mod(Ck, Lt, 4, at(po, 4 * 2 * (Lt - 4) * N - 1), c3, 4, 1, s40, s40, 2, po)); // out is [4][2][L - depth - r][N]
    GOOD("in right behind out", mod(Ck, Lt, 4, at(po, 4 * 2 * (Lt - 4) * N), c3, 4, 1, s40, s40, 2, po));
    if (failures) return 1;
    std::printf("ckks_eval_mod_args ok\n");
    return 0;
}
