// rotate_hoisted_args_main.cpp -- TEST-ONLY, stand-alone.  Runs plan_rotate_hoisted of csrc/hoist_args.h (the device-free check of
// he355_apply_galois_hoisted, he355_rotate_hoisted and he355_rotate_hoisted_plain_sum, and the plan it returns) at accepted and refused edge
// arguments -- levels at and past their ends, a chain that cannot key-switch, ntt_form outside {0, 1} and 0 on a CKKS context, even elements and
// elements at 2N, steps at +-N/2, spans at and past 2^60 words and past the end of the address space, overlaps one word inside and right behind,
// the empty calls -- compiled with -fsanitize=address,undefined (tests/test_rotate_hoisted_args_cpu.py).  The check does arithmetic on counts and
// addresses the caller chose: none of it may overflow a signed type or form a pointer outside its slab before the refusal.  Prints
// "rotate_hoisted_args ok" and exits 0, or names the first case that went the other way.
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
    const int Lt = (int)B.Ltop;
    const size_t per = 2 * (size_t)Lt * N;
    std::vector<u64> a(4 * per), b(12 * per), pt(3 * (size_t)Lt * N);
    const u64 *pa = a.data(), *po = b.data(), *pp = pt.data();
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;
    const uint32_t e3[3] = {3, 9, (uint32_t)(2 * N - 1)}, ident[2] = {1, 1}, twice[3] = {3, 3, 1};
    const int32_t s3[3] = {1, 0, -2};
    const char *W = "he355_apply_galois_hoisted";
    auto elts = [&](const Params &P, int L, int nf, u64 n, const u64 *in, const uint32_t *e, u64 ne, const u64 *out) {
        return plan_rotate_hoisted(P, W, L, nf, n, in, e, nullptr, ne, nullptr, out, false);
    };
    auto steps = [&](const Params &P, int L, int nf, u64 n, const u64 *in, const int32_t *s, u64 ns, const u64 *out) {
        return plan_rotate_hoisted(P, "he355_rotate_hoisted", L, nf, n, in, nullptr, s, ns, nullptr, out, false);
    };
    auto psum = [&](const Params &P, int L, u64 n, const u64 *in, const int32_t *s, u64 ns, const u64 *plain, const u64 *out) {
        return plan_rotate_hoisted(P, "he355_rotate_hoisted_plain_sum", L, 1, n, in, nullptr, s, ns, plain, out, true);
    };

    // levels, key switching, the form
    for (int L : {0, Lt + 1, -1}) BAD("level", elts(B, L, 0, 4, pa, e3, 3, po));
    BAD("K < 2", elts(*p1, 1, 1, 1, pa, e3, 3, po));
    for (int nf : {-1, 2, 256}) BAD("ntt_form", elts(B, Lt, nf, 4, pa, e3, 3, po));
    BAD("coefficient form on CKKS", elts(Ck, Lt, 0, 4, pa, e3, 3, po));
    GOOD("CKKS", elts(Ck, Lt, 1, 4, pa, e3, 3, po));
    GOOD("BFV coefficient form", elts(B, Lt, 0, 4, pa, e3, 3, po));
    GOOD("BFV NTT form", elts(B, 1, 1, 4, pa, e3, 3, po));
    // elements and steps
    for (uint32_t e : {0u, 2u, (uint32_t)(2 * N), (uint32_t)(2 * N + 1), 0xffffffffu, 0x80000001u}) {
        const uint32_t bad[2] = {3, e};
        BAD("element", elts(B, Lt, 0, 4, pa, bad, 2, po));
    }
    for (int32_t s : {(int32_t)(N / 2), -(int32_t)(N / 2), (int32_t)0x7fffffff, (int32_t)0x80000000}) {
        const int32_t bad[2] = {1, s};
        BAD("step", steps(B, Lt, 0, 4, pa, bad, 2, po));
    }
    {
        const int32_t edge[2] = {(int32_t)(N / 2 - 1), -(int32_t)(N / 2 - 1)};
        GOOD("steps at the edge", steps(B, Lt, 0, 4, pa, edge, 2, po));
    }
    BAD("null elements", plan_rotate_hoisted(B, W, Lt, 0, 4, pa, nullptr, nullptr, 3, nullptr, po, false));
    BAD("too many elements", elts(B, Lt, 0, 1, pa, e3, ((u64)1 << 20) + 1, po));
    // the plans
    GOOD("plan", const HoistPlan pl = elts(B, Lt, 0, 4, pa, e3, 3, po); if (pl.elts.size() != 3 || pl.keyed != 3 || pl.empty || pl.elts[2] != 2 * N - 1) throw std::invalid_argument("plan"));
    GOOD("plan", const HoistPlan pl = elts(B, Lt, 0, 4, pa, ident, 2, po); if (pl.keyed != 0 || pl.empty) throw std::invalid_argument("plan"));
    GOOD("plan", const HoistPlan pl = elts(B, Lt, 0, 4, pa, twice, 3, po); if (pl.keyed != 2 || pl.elts[1] != 3) throw std::invalid_argument("plan"));
    GOOD("plan", const HoistPlan pl = steps(B, Lt, 0, 4, pa, s3, 3, po);
         if (pl.keyed != 2 || pl.elts[0] != B.galois_elt_from_step(1) || pl.elts[1] != 1 || pl.elts[2] != B.galois_elt_from_step(-2)) throw std::invalid_argument("plan"));
    // the empty calls: nothing to check behind the arguments' own ranges
    GOOD("n == 0", const HoistPlan pl = elts(B, Lt, 0, 0, nullptr, e3, 3, nullptr); if (!pl.empty) throw std::invalid_argument("plan"));
    GOOD("n_elts == 0", const HoistPlan pl = elts(B, Lt, 0, 4, pa, nullptr, 0, pa); if (!pl.empty) throw std::invalid_argument("plan"));
    GOOD("n_steps == 0", const HoistPlan pl = psum(Ck, Lt, 4, pa, nullptr, 0, nullptr, pa); if (!pl.empty) throw std::invalid_argument("plan"));
    BAD("n == 0, bad level", elts(B, 0, 0, 0, nullptr, e3, 3, nullptr));
    BAD("n == 0, bad element", const uint32_t ev[1] = {4}; elts(B, Lt, 0, 0, nullptr, ev, 1, nullptr));
    // spans: n n_elts 2 L N words, formed in 128 bits
    BAD("span", elts(B, Lt, 0, ~(u64)0, low, e3, 3, mid));
    BAD("span", elts(B, Lt, 0, (u64)1 << 60, low, e3, 3, mid));
    BAD("span", elts(B, Lt, 0, ((u64)1 << 60) / per + 1, low, ident, 1, mid));
    BAD("span of the output", elts(B, Lt, 0, ((u64)1 << 60) / per / 2, low, e3, 3, mid)); // the input fits, three times it does not
    GOOD("span", elts(B, Lt, 0, ((u64)1 << 44) / per, low, e3, 3, mid));
    BAD("wraps", elts(B, Lt, 0, 2, high, e3, 3, low));
    BAD("wraps", elts(B, Lt, 0, 2, low, e3, 3, high));
    BAD("wraps", psum(Ck, Lt, 1, low, s3, 3, high, mid));
    // overlaps
    BAD("out at in", elts(B, Lt, 0, 4, pa, e3, 3, pa));
    BAD("out one word inside in", elts(B, Lt, 0, 4, pa, e3, 3, at(pa, 4 * per - 1)));
    GOOD("out right behind in", elts(B, Lt, 0, 4, pa, e3, 3, at(pa, 4 * per)));
    BAD("in inside out", elts(B, Lt, 0, 1, at(po, 3 * per - 1), e3, 3, po));
    GOOD("in right behind out", elts(B, Lt, 0, 1, at(po, 3 * per), e3, 3, po));
    BAD("in inside out's later blocks", elts(B, Lt, 0, 4, at(po, 8 * per), e3, 3, po));
    GOOD("plain sum", psum(Ck, Lt, 4, pa, s3, 3, pp, po));
    BAD("plain sum over in", psum(Ck, Lt, 4, pa, s3, 3, pp, at(pa, per)));
    BAD("plain sum over the plaintexts", psum(Ck, Lt, 1, pa, s3, 3, pp, at(pp, 3 * (size_t)Lt * N - 1)));
    GOOD("plain sum behind the plaintexts", psum(Ck, Lt, 1, pa, s3, 3, pp, at(pp, 3 * (size_t)Lt * N)));
    BAD("plain sum, null plaintexts", psum(Ck, Lt, 4, pa, s3, 3, nullptr, po));
    BAD("plain sum, null steps", psum(Ck, Lt, 4, pa, nullptr, 3, pp, po));
    if (failures) return 1;
    std::printf("rotate_hoisted_args ok\n");
    return 0;
}
