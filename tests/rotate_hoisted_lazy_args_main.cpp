// rotate_hoisted_lazy_args_main.cpp -- TEST-ONLY, stand-alone.  Runs the device-free checks of he355_rotate_hoisted_plain_sum_lazy
// (plan_rotate_hoisted of csrc/hoist_args.h with the [n_steps][L + 1][N] plaintext span) and of he355_plain_extend_special
// (plan_plain_extend) at accepted and refused edge arguments -- levels at and past their ends, a chain without a special prime, steps at
// +-N/2, null pointers, spans at and past 2^60 words and past the end of the address space, overlaps one word inside and right behind (the
// extra row of every plaintext counts), the empty calls -- compiled with -fsanitize=address,undefined
// (tests/test_rotate_hoisted_lazy_args_cpu.py).  Prints "rotate_hoisted_lazy_args ok" and exits 0, or names the first case that went the
// other way.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/hoist_args.h"
#include "args_main_common.h"

using namespace he355;

int main()
{
    const size_t N = 4096;
    std::unique_ptr<Params> pb(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    std::unique_ptr<Params> pc(Params::create(kSchemeCKKS, N, {60, 40, 40, 60}, 0, false));
    std::unique_ptr<Params> p1(Params::create(kSchemeCKKS, N, {60}, 0, false)); // K = 1: no special prime
    const Params &B = *pb, &Ck = *pc;
    const int Lt = (int)Ck.Ltop;
    const size_t per = 2 * (size_t)Lt * N, ptw = (size_t)(Lt + 1) * N; // words of a ciphertext and of an extended plaintext
    std::vector<u64> a(4 * per), b(4 * per), pt(3 * ptw), pn(3 * (size_t)Lt * N);
    const u64 *pa = a.data(), *po = b.data(), *pp = pt.data(), *ps = pn.data();
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;
    const int32_t s3[3] = {1, 0, -2};
    auto lazy = [&](const Params &P, int L, u64 n, const u64 *in, const int32_t *s, u64 ns, const u64 *plain, const u64 *out) {
        return plan_rotate_hoisted(P, "he355_rotate_hoisted_plain_sum_lazy", L, 1, n, in, nullptr, s, ns, plain, out, true, true);
    };

    // ---- the lazy plain sum ----
    for (int L : {0, Lt + 1, -1}) BAD("level", lazy(Ck, L, 4, pa, s3, 3, pp, po));
    BAD("K < 2", lazy(*p1, 1, 1, pa, s3, 3, pp, po));
    GOOD("CKKS", lazy(Ck, Lt, 4, pa, s3, 3, pp, po));
    GOOD("NTT-form BFV", lazy(B, Lt, 4, pa, s3, 3, pp, po));
    GOOD("lower level", lazy(Ck, 1, 4, pa, s3, 3, pp, po));
    for (int32_t s : {(int32_t)(N / 2), -(int32_t)(N / 2), (int32_t)0x7fffffff, (int32_t)0x80000000}) {
        const int32_t bad[2] = {1, s};
        BAD("step", lazy(Ck, Lt, 4, pa, bad, 2, pp, po));
    }
    {
        const int32_t edge[2] = {(int32_t)(N / 2 - 1), -(int32_t)(N / 2 - 1)};
        GOOD("steps at the edge", lazy(Ck, Lt, 4, pa, edge, 2, pp, po));
    }
    BAD("null steps", lazy(Ck, Lt, 4, pa, nullptr, 3, pp, po));
    BAD("null plaintexts", lazy(Ck, Lt, 4, pa, s3, 3, nullptr, po));
    BAD("too many steps", lazy(Ck, Lt, 1, pa, s3, ((u64)1 << 20) + 1, pp, po));
    GOOD("plan", const HoistPlan pl = lazy(Ck, Lt, 4, pa, s3, 3, pp, po);
         if (pl.keyed != 2 || pl.empty || pl.elts[0] != Ck.galois_elt_from_step(1) || pl.elts[1] != 1 || pl.elts[2] != Ck.galois_elt_from_step(-2)) throw std::invalid_argument("plan"));
    GOOD("n == 0", const HoistPlan pl = lazy(Ck, Lt, 0, nullptr, s3, 3, nullptr, nullptr); if (!pl.empty) throw std::invalid_argument("plan"));
    GOOD("n_steps == 0", const HoistPlan pl = lazy(Ck, Lt, 4, pa, nullptr, 0, nullptr, pa); if (!pl.empty) throw std::invalid_argument("plan"));
    BAD("n == 0, bad level", lazy(Ck, 0, 0, nullptr, s3, 3, nullptr, nullptr));
    BAD("span", lazy(Ck, Lt, ~(u64)0, low, s3, 3, pp, mid));
    BAD("span", lazy(Ck, Lt, ((u64)1 << 60) / per + 1, low, s3, 3, pp, mid));
    GOOD("span", lazy(Ck, Lt, ((u64)1 << 44) / per, low, s3, 3, pp, mid));
    BAD("wraps", lazy(Ck, Lt, 2, high, s3, 3, pp, low));
    BAD("wraps", lazy(Ck, Lt, 2, low, s3, 3, pp, high));
    BAD("plaintexts wrap", lazy(Ck, Lt, 1, low, s3, 3, high, mid));
    BAD("out at in", lazy(Ck, Lt, 4, pa, s3, 3, pp, pa));
    BAD("out one word inside in", lazy(Ck, Lt, 4, pa, s3, 3, pp, at(pa, 4 * per - 1)));
    GOOD("out right behind in", lazy(Ck, Lt, 4, pa, s3, 3, pp, at(pa, 4 * per)));
    BAD("out over the plaintexts", lazy(Ck, Lt, 1, pa, s3, 3, pp, pp));
    // the extra row counts: the last word of the third plaintext is 3 (L + 1) N - 1 words in, past the 3 L N of the eager call
    BAD("out one word inside the special row of the last plaintext", lazy(Ck, Lt, 1, pa, s3, 3, pp, at(pp, 3 * ptw - 1)));
    GOOD("out right behind the plaintexts", lazy(Ck, Lt, 1, pa, s3, 3, pp, at(pp, 3 * ptw)));
    BAD("plaintexts inside out", lazy(Ck, Lt, 4, pa, s3, 3, at(po, 4 * per - 1), po));
    GOOD("plaintexts right behind out", lazy(Ck, Lt, 4, pa, s3, 3, at(po, 4 * per), po));

    // ---- he355_plain_extend_special ----
    auto ext = [&](const Params &P, int L, u64 n, const u64 *src, const u64 *dst) { return plan_plain_extend(P, L, n, src, dst); };
    for (int L : {0, Lt + 1, -1}) BAD("extend, level", ext(Ck, L, 3, ps, pp));
    BAD("extend, K < 2", ext(*p1, 1, 1, ps, pp));
    GOOD("extend", if (ext(Ck, Lt, 3, ps, pp)) throw std::invalid_argument("not empty"));
    GOOD("extend, BFV, L = 1", if (ext(B, 1, 3, ps, pp)) throw std::invalid_argument("not empty"));
    GOOD("extend, n == 0", if (!ext(Ck, Lt, 0, nullptr, nullptr)) throw std::invalid_argument("empty"));
    BAD("extend, n == 0, bad level", ext(Ck, 0, 0, nullptr, nullptr));
    BAD("extend, null source", ext(Ck, Lt, 3, nullptr, pp));
    BAD("extend, null destination", ext(Ck, Lt, 3, ps, nullptr));
    BAD("extend, span", ext(Ck, Lt, ~(u64)0, low, mid));
    BAD("extend, span", ext(Ck, Lt, (u64)1 << 60, low, mid));
    BAD("extend, span of the output", ext(Ck, Lt, ((u64)1 << 60) / ptw + 1, low, mid)); // the input fits, one more row each does not
    GOOD("extend, span", if (ext(Ck, Lt, ((u64)1 << 44) / ptw, low, mid)) throw std::invalid_argument("not empty"));
    BAD("extend, wraps", ext(Ck, Lt, 2, high, low));
    BAD("extend, wraps", ext(Ck, Lt, 2, low, high));
    BAD("extend, in place", ext(Ck, Lt, 3, pp, pp));
    BAD("extend, destination one word inside the source", ext(Ck, Lt, 3, ps, at(ps, 3 * (size_t)Lt * N - 1)));
    GOOD("extend, destination right behind the source", if (ext(Ck, Lt, 3, ps, at(ps, 3 * (size_t)Lt * N))) throw std::invalid_argument("not empty"));
    BAD("extend, source one word inside the destination", ext(Ck, Lt, 3, at(pp, 3 * ptw - 1), pp));
    GOOD("extend, source right behind the destination", if (ext(Ck, Lt, 3, at(pp, 3 * ptw), pp)) throw std::invalid_argument("not empty"));
    if (failures) return 1;
    std::printf("rotate_hoisted_lazy_args ok\n");
    return 0;
}
