// linear_transform_bsgs_args_main.cpp -- TEST-ONLY, stand-alone.  Runs the device-free checks of he355_linear_transform_bsgs
// (plan_linear_transform_bsgs of csrc/hoist_args.h) at accepted and refused edge arguments -- levels at and past their ends, a chain without a
// special prime, steps at +-N/2, null pointers, more than 2^20 pairs, a mask with no term, spans at and past 2^60 words and past the end of
// the address space, overlaps one word inside and right behind (the special-prime row of the last plaintext counts), the empty calls -- and
// the plan it hands on: slots, term lists, used rows.  Compiled with -fsanitize=address,undefined
// (tests/test_linear_transform_bsgs_args_cpu.py).  Prints "linear_transform_bsgs_args ok" and exits 0, or names the first case that went
// the other way.
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
    std::vector<u64> a(4 * per), b(4 * per), pt(6 * ptw);
    const u64 *pa = a.data(), *po = b.data(), *pp = pt.data();
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;
    const int32_t b3[3] = {0, 1, -2}, g2[2] = {0, 3};
    auto bsgs = [&](const Params &P, int L, u64 n, const u64 *in, const int32_t *bs, u64 nb, const int32_t *gs, u64 ng, const u64 *plain, const uint8_t *mask, const u64 *out) {
        return plan_linear_transform_bsgs(P, L, n, in, bs, nb, gs, ng, plain, mask, out);
    };
    for (int L : {0, Lt + 1, -1}) BAD("level", bsgs(Ck, L, 4, pa, b3, 3, g2, 2, pp, nullptr, po));
    BAD("K < 2", bsgs(*p1, 1, 1, pa, b3, 3, g2, 2, pp, nullptr, po));
    GOOD("CKKS", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, nullptr, po));
    GOOD("NTT-form BFV", bsgs(B, Lt, 4, pa, b3, 3, g2, 2, pp, nullptr, po));
    GOOD("lower level", bsgs(Ck, 1, 4, pa, b3, 3, g2, 2, pp, nullptr, po));
    for (int32_t s : {(int32_t)(N / 2), -(int32_t)(N / 2), (int32_t)0x7fffffff, (int32_t)0x80000000}) {
        const int32_t bad[2] = {1, s};
        BAD("baby step", bsgs(Ck, Lt, 4, pa, bad, 2, g2, 2, pp, nullptr, po));
        BAD("giant step", bsgs(Ck, Lt, 4, pa, b3, 3, bad, 2, pp, nullptr, po));
    }
    {
        const int32_t edge[2] = {(int32_t)(N / 2 - 1), -(int32_t)(N / 2 - 1)};
        GOOD("steps at the edge", bsgs(Ck, Lt, 4, pa, edge, 2, edge, 2, pp, nullptr, po));
    }
    BAD("null baby steps", bsgs(Ck, Lt, 4, pa, nullptr, 3, g2, 2, pp, nullptr, po));
    BAD("null giant steps", bsgs(Ck, Lt, 4, pa, b3, 3, nullptr, 2, pp, nullptr, po));
    BAD("null plaintexts", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, nullptr, nullptr, po));
    BAD("null input", bsgs(Ck, Lt, 4, nullptr, b3, 3, g2, 2, pp, nullptr, po));
    BAD("null output", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, nullptr, nullptr));
    BAD("too many pairs", bsgs(Ck, Lt, 1, pa, b3, ((u64)1 << 10) + 1, g2, (u64)1 << 10, pp, nullptr, po));
    BAD("too many pairs, the product wraps", bsgs(Ck, Lt, 1, pa, b3, (u64)1 << 32, g2, (u64)1 << 32, pp, nullptr, po));
    {
        const uint8_t none[6] = {0, 0, 0, 0, 0, 0};
        BAD("a mask with no term", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, none, po));
        // the bad steps of a masked column are still refused: the step list is checked whole
        const int32_t bad[3] = {0, (int32_t)(N / 2), 1};
        const uint8_t col[6] = {1, 0, 1, 1, 0, 1};
        BAD("a masked bad step", bsgs(Ck, Lt, 4, pa, bad, 3, g2, 2, pp, col, po));
    }
    GOOD("plan", const BsgsPlan pl = bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, nullptr, po);
         if (pl.empty || pl.slots != 3 || pl.keyed_babies != 2 || pl.keyed_rows != 1 || pl.used_rows != 2 || pl.terms.size() != 12 || pl.baby[0] != 1 ||
             pl.baby[1] != Ck.galois_elt_from_step(1) || pl.giant[1] != Ck.galois_elt_from_step(3) || pl.row_first[1] != 3 || pl.row_first[2] != 6)
             throw std::invalid_argument("plan"));
    {
        // row 0 keeps (0, -2), row 1 is dropped whole: baby 1 is not used, the slots close up, giant 3 needs no key
        const uint8_t m[6] = {1, 0, 1, 0, 0, 0};
        GOOD("masked plan", const BsgsPlan pl = bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, m, po);
             if (pl.slots != 2 || pl.keyed_babies != 1 || pl.keyed_rows != 0 || pl.used_rows != 1 || pl.slot[0] != 0 || pl.slot[1] != -1 || pl.slot[2] != 1 ||
                 pl.terms != std::vector<uint32_t>({0, 0, 1, 2}) || pl.row_first[1] != 2 || pl.row_first[2] != 2)
                 throw std::invalid_argument("plan"));
    }
    GOOD("n == 0", const BsgsPlan pl = bsgs(Ck, Lt, 0, nullptr, b3, 3, g2, 2, nullptr, nullptr, nullptr); if (!pl.empty) throw std::invalid_argument("plan"));
    GOOD("n_baby == 0", const BsgsPlan pl = bsgs(Ck, Lt, 4, pa, nullptr, 0, g2, 2, nullptr, nullptr, pa); if (!pl.empty) throw std::invalid_argument("plan"));
    GOOD("n_giant == 0", const BsgsPlan pl = bsgs(Ck, Lt, 4, pa, b3, 3, nullptr, 0, nullptr, nullptr, pa); if (!pl.empty) throw std::invalid_argument("plan"));
    BAD("n == 0, bad level", bsgs(Ck, 0, 0, nullptr, b3, 3, g2, 2, nullptr, nullptr, nullptr));
    BAD("span", bsgs(Ck, Lt, ~(u64)0, low, b3, 3, g2, 2, pp, nullptr, mid));
    BAD("span", bsgs(Ck, Lt, ((u64)1 << 60) / per + 1, low, b3, 3, g2, 2, pp, nullptr, mid));
    GOOD("span", bsgs(Ck, Lt, ((u64)1 << 44) / per, low, b3, 3, g2, 2, pp, nullptr, mid));
    BAD("wraps", bsgs(Ck, Lt, 2, high, b3, 3, g2, 2, pp, nullptr, low));
    BAD("wraps", bsgs(Ck, Lt, 2, low, b3, 3, g2, 2, pp, nullptr, high));
    BAD("plaintexts wrap", bsgs(Ck, Lt, 1, low, b3, 3, g2, 2, high, nullptr, mid));
    BAD("out at in", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, nullptr, pa));
    BAD("out one word inside in", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, nullptr, at(pa, 4 * per - 1)));
    GOOD("out right behind in", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, pp, nullptr, at(pa, 4 * per)));
    BAD("out over the plaintexts", bsgs(Ck, Lt, 1, pa, b3, 3, g2, 2, pp, nullptr, pp));
    BAD("out one word inside the special row of the last plaintext", bsgs(Ck, Lt, 1, pa, b3, 3, g2, 2, pp, nullptr, at(pp, 6 * ptw - 1)));
    GOOD("out right behind the plaintexts", bsgs(Ck, Lt, 1, pa, b3, 3, g2, 2, pp, nullptr, at(pp, 6 * ptw)));
    BAD("plaintexts inside out", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, at(po, 4 * per - 1), nullptr, po));
    GOOD("plaintexts right behind out", bsgs(Ck, Lt, 4, pa, b3, 3, g2, 2, at(po, 4 * per), nullptr, po));
    {
        // a masked plaintext still may not lie under the output: every word of d_plain_qp counts
        const uint8_t m[6] = {1, 1, 1, 1, 1, 0};
        BAD("out inside a masked plaintext", bsgs(Ck, Lt, 1, pa, b3, 3, g2, 2, pp, m, at(pp, 6 * ptw - 1)));
    }
    if (failures) return 1;
    std::printf("linear_transform_bsgs_args ok\n");
    return 0;
}
