// bfv_select_args_main.cpp -- TEST-ONLY, stand-alone.  Runs plan_select of csrc/bfv_pir_args.h (the device-free check of he355_bfv_select, and
// the plan it returns) at accepted and refused edge arguments -- levels, digit widths and counts at and past their ends, count 1, 2, 3 and
// 2^k +- 1 with their level tables read back, strides of 0, strides that collide at the last index pair and one short of it, spans at and past
// 2^60 words and past the end of the address space, strides near 2^64, the grid limit to the pair, overlaps with the leaves and with the
// selectors one word inside and right behind -- compiled with -fsanitize=address,undefined (tests/test_bfv_select_args_cpu.py).  The check
// does arithmetic on counts, strides and addresses the caller chose: none of it may overflow a signed type, shift out of range or form a
// pointer outside its slab before the refusal.  Prints "bfv_select_args ok" and exits 0, or names the first case that went the other way.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/bfv_pir_args.h"
#include "args_main_common.h"

using namespace he355;

// the plan of (n, count) read back against the recursion restated here: c_0 = count, c_(j+1) = ceil(c_j / 2) down to 1; pairs n floor(c_j / 2)
static void check_plan(const BfvSelectPlan &pl, u64 n, u64 count, u32 E, int L)
{
    std::vector<u64> c{count};
    while (c.back() > 1) c.push_back(c.back() - c.back() / 2);
    const int m = (int)c.size() - 1;
    bool ok = pl.depth == m && pl.rows == 2 * E && pl.n == n;
    for (int j = 0; ok && j <= m; ++j) ok = pl.c[j] == c[j];
    for (int j = 0; ok && j < m; ++j) ok = pl.pairs(j) == n * (c[j] / 2);
    if (ok && n && m) {
        u64 pass = kGadgetPassPolys / (2 * E);
        if (pass < 1) pass = 1;
        if (pass > n * (count / 2)) pass = n * (count / 2);
        const u64 nodes = (m >= 2 ? n * c[1] : 0) + (m >= 3 ? n * c[2] : 0);
        ok = pl.pass == pass && pl.slab_polys == pass * (2 * (u64)E + 2) * L && pl.node_cts == nodes && nodes <= (count - count / 2 + (count + 3) / 4) * n;
    } else if (ok) {
        ok = pl.pass == 0 && pl.slab_polys == 0 && pl.node_cts == 0;
    }
    if (!ok) throw std::invalid_argument("plan");
}

int main()
{
    const size_t N = 4096;
    std::unique_ptr<Params> pp(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    const Params &P = *pp;
    const int Lt = (int)P.Ltop, v = 20;
    const size_t per = 2 * (size_t)Lt * N;
    const u32 E = bfv_gadget_table(level_primes(P, Lt).data(), Lt, v).total, E1 = bfv_gadget_table(level_primes(P, 1).data(), 1, 1).total;
    const size_t rg = 2 * (size_t)E * per;
    std::vector<u64> a(24 * per), b(4 * per), s(4 * rg);
    const u64 *pa = a.data(), *pb = b.data(), *ps = s.data();
    // an address `words` words behind a slab's start, formed as an integer: the callers' pointers are only numbers to the check
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull,
              *far = (const u64 *)0x2000000000000000ull;

    for (int L : {0, Lt + 1, -1}) BAD("select", plan_select(P, L, v, 2, 4, pa, 4, 1, ps, 2, 1, pb));
    for (int w : {0, 64, -1}) BAD("select", plan_select(P, Lt, w, 2, 4, pa, 4, 1, ps, 2, 1, pb));
    for (u64 count : {(u64)0, kSelectMaxCount + 1, ~(u64)0}) BAD("select", plan_select(P, Lt, v, 1, count, low, 0, 1, far, 0, 1, mid));
    // the plans: count 1, 2, 3 and 2^k +- 1, one result and three
    for (u64 n : {(u64)1, (u64)3})
        for (u64 count : {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 1023, 1025})
            GOOD("select", check_plan(plan_select(P, Lt, v, n, count, low, count, 1, far, 40, 1, mid), n, count, E, Lt));
    GOOD("select", check_plan(plan_select(P, Lt, v, 1, (u64)1 << 20, low, 0, 1, far, 0, 1, mid), 1, (u64)1 << 20, E, Lt));
    GOOD("select", check_plan(plan_select(P, 1, 1, 1, kSelectMaxCount, low, 0, 1, far, 0, 1, mid), 1, kSelectMaxCount, E1, 1));
    GOOD("select", check_plan(plan_select(P, 1, 1, 1, kSelectMaxCount - 1, low, 0, 1, far, 0, 1, mid), 1, kSelectMaxCount - 1, E1, 1));
    GOOD("select", check_plan(plan_select(P, Lt, v, 0, 5, nullptr, 0, 0, nullptr, 0, 0, nullptr), 0, 5, E, Lt)); // n == 0: nothing to check
    // v = 1 at L = 1: 2E = 120 terms, a pass of 34 pairs; the smallest n at count 2 that needs two passes is 35
    GOOD("select", const BfvSelectPlan pl = plan_select(P, 1, 1, 35, 2, low, 2, 1, far, 1, 1, mid); if (pl.pass != kGadgetPassPolys / (2 * E1) || pl.pairs(0) != 35 || pl.pass >= 35) throw std::invalid_argument("pass"));
    // N = 1024 has no column pass and runs its tail once per level: the sums behind the digits are those of level 0's pairs, not of a pass
    {
        std::unique_ptr<Params> ps(Params::create(kSchemeBFV, 1024, {50, 40, 50}, 20, false));
        const int Ls = (int)ps->Ltop;
        const u32 Es = bfv_gadget_table(level_primes(*ps, Ls).data(), Ls, v).total;
        GOOD("select", const BfvSelectPlan pl = plan_select(*ps, Ls, v, 16, 256, low, 256, 1, far, 0, 1, mid);
                       if (pl.pass != kGadgetPassPolys / (2 * Es) || pl.pairs(0) != 2048 || pl.slab_polys != (pl.pass * 2 * Es + 2048 * 2) * Ls) throw std::invalid_argument("plan"));
    }
    // two leaves at one place
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 4, 0, ps, 2, 1, pb));
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 0, 1, ps, 2, 1, pb));
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 0, 0, ps, 2, 1, pb));
    GOOD("select", plan_select(P, Lt, v, 2, 1, pa, 1, 0, ps, 2, 1, pb)); // count == 1: stride_k moves nothing
    GOOD("select", plan_select(P, Lt, v, 1, 4, pa, 0, 1, ps, 2, 1, pb)); // n == 1: stride_r moves nothing
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 1, 1, ps, 2, 1, pb));
    BAD("select", plan_select(P, Lt, v, 2, 3, pa, 4, 2, ps, 2, 1, pb));  // k = 2, r = 0 and k = 0, r = 1
    BAD("select", plan_select(P, Lt, v, 4, 3, pa, 4, 6, ps, 2, 1, pb));  // k = 2, r = 0 and k = 0, r = 3: the last index pair
    GOOD("select", plan_select(P, Lt, v, 3, 3, low, 4, 6, far, 2, 1, mid)); // one result fewer: no pair left
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 3, 1, ps, 2, 1, pb));
    GOOD("select", plan_select(P, Lt, v, 2, 3, pa, 3, 1, ps, 2, 1, pb));
    GOOD("select", plan_select(P, Lt, v, 2, 2, pa, 2, 3, ps, 1, 1, pb));
    BAD("select", plan_select(P, Lt, v, 3, 3, low, ~(u64)0, ~(u64)0, far, 2, 1, mid));                // equal strides, however large
    BAD("select", plan_select(P, Lt, v, 3, 3, low, ((u64)1 << 63) - 1, ~(u64)0 - 1, far, 2, 1, mid)); // 2 stride_r = stride_k: collides, and far past any span
    // spans
    BAD("select", plan_select(P, Lt, v, 2, 4, low, 1, (u64)1 << 63, far, 2, 1, mid));
    BAD("select", plan_select(P, Lt, v, 2, 4, low, 1, ~(u64)0, far, 2, 1, mid));
    BAD("select", plan_select(P, Lt, v, 2, 2, low, ~(u64)0, 1, far, 1, 1, mid));
    BAD("select", plan_select(P, Lt, v, 3, 1, low, (u64)1 << 63, 0, far, 0, 0, mid));
    BAD("select", plan_select(P, Lt, v, 2, 2, low, (u64)1 << 50, 1, far, 1, 1, mid));             // 2^50 ciphertexts are past 2^60 words
    GOOD("select", plan_select(P, Lt, v, 2, 2, low, 1, ((u64)1 << 45) / per * 2, far, 1, 1, mid)); // 2^46 words: in bounds from a low address
    BAD("select", plan_select(P, Lt, v, 2, 2, high, 1, ((u64)1 << 45) / per * 2, far, 1, 1, low)); // the same span from the top of the address space wraps it
    BAD("select", plan_select(P, Lt, v, 2, 2, low, 2, 1, far, 1, 1, at(high, 0)));                 // the output wraps it
    BAD("select", plan_select(P, Lt, v, 2, 4, low, 4, 1, far, (u64)1 << 50, 1, mid));              // the selectors past 2^60 words
    BAD("select", plan_select(P, Lt, v, 2, 4, low, 4, 1, far, 2, ~(u64)0, mid));
    BAD("select", plan_select(P, Lt, v, 2, 4, low, 4, 1, high, 2, 1, mid));                        // the selectors wrap the address space
    GOOD("select", plan_select(P, Lt, v, 2, 4, low, 4, 1, far, 0, 1, mid));                        // shared bits
    // one launch: n floor(count / 2) 2 L N / 512 blocks
    const u64 lim = 0x7fffffffull / (2 * (u64)Lt * (N / 512));
    BAD("select", plan_select(P, Lt, v, (u64)1 << 31, 2, low, 2, 1, far, 0, 1, mid));
    BAD("select", plan_select(P, Lt, v, lim + 1, 2, low, 2, 1, far, 0, 1, mid)); // one pair too many
    GOOD("select", check_plan(plan_select(P, Lt, v, lim, 2, low, 2, 1, far, 0, 1, mid), lim, 2, E, Lt));
    BAD("select", plan_select(P, Lt, v, lim / 2 + 1, 5, low, 5, 1, far, 0, 1, mid)); // two pairs per result
    GOOD("select", plan_select(P, Lt, v, lim / 2, 5, low, 5, 1, far, 0, 1, mid));
    BAD("select", plan_select(P, Lt, v, lim + 1, 1, low, 1, 0, far, 0, 0, mid)); // count == 1: the copies
    GOOD("select", plan_select(P, Lt, v, lim, 1, low, 1, 0, far, 0, 0, mid));
    BAD("select", plan_select(P, Lt, v, (u64)1 << 12, (u64)1 << 20, low, (u64)1 << 20, 1, far, 0, 1, mid));
    // overlaps
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 4, 1, ps, 2, 1, pa));
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 4, 1, ps, 2, 1, at(pa, 8 * per - 1)));
    GOOD("select", plan_select(P, Lt, v, 2, 4, pa, 4, 1, ps, 2, 1, at(pa, 8 * per)));
    BAD("select", plan_select(P, Lt, v, 2, 4, at(pa, 2 * per - 1), 4, 1, ps, 2, 1, pa)); // the output's last word is the first leaf's first
    GOOD("select", plan_select(P, Lt, v, 2, 4, at(pa, 2 * per), 4, 1, ps, 2, 1, pa));
    BAD("select", plan_select(P, Lt, v, 2, 2, pa, 1, 3, ps, 1, 1, at(pa, 2 * per)));     // in a gap of padded leaves
    BAD("select", plan_select(P, Lt, v, 1, 1, pa, 0, 0, ps, 0, 0, at(pa, N)));           // count == 1 copies: not over itself either
    GOOD("select", plan_select(P, Lt, v, 1, 1, pa, 0, 0, pb, 0, 0, pb));                 // count == 1 reads no selector
    BAD("select", plan_select(P, Lt, v, 2, 4, pa, 4, 1, ps, 2, 1, ps));
    BAD("select", plan_select(P, Lt, v, 1, 4, pa, 0, 1, ps, 0, 1, at(ps, 2 * rg - 1))); // the last word of two bits
    GOOD("select", plan_select(P, Lt, v, 1, 4, pa, 0, 1, ps, 0, 1, at(ps, 2 * rg)));
    BAD("select", plan_select(P, Lt, v, 1, 4, pa, 0, 1, at(ps, per - 1), 0, 1, ps));    // the output's last word is the selectors' first
    if (failures) return 1;
    std::printf("bfv_select_args ok\n");
    return 0;
}
