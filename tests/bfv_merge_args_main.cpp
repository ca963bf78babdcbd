// bfv_merge_args_main.cpp -- TEST-ONLY, stand-alone.  Runs plan_merge of csrc/bfv_pir_args.h (the device-free check of he355_bfv_merge, and
// the plan it returns) at accepted and refused edge arguments -- levels and counts at and past their ends, strides of 0, strides that
// collide at the last index pair and one short of it, spans at and past 2^60 words and past the end of the address space, strides near
// 2^64, grids at 2^31, overlaps one word inside and right behind -- compiled with -fsanitize=address,undefined
// (tests/test_bfv_merge_args_cpu.py).  The check does arithmetic on counts, strides and addresses the caller chose: none of it may overflow a
// signed type, shift out of range or form a pointer outside its slab before the refusal.  Prints "bfv_merge_args ok" and exits 0, or names
// the first case that went the other way.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/bfv_pir_args.h"
#include "args_main_common.h"

using namespace he355;

#define PLAN(d_, half_, scratch_, ...)                                                                                                \
    GOOD("merge", const BfvMergePlan pl = __VA_ARGS__; if (pl.depth != d_ || pl.half != half_ || pl.scratch_cts != scratch_) throw std::invalid_argument("plan"))

int main()
{
    const size_t N = 4096;
    std::unique_ptr<Params> pp(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    const Params &P = *pp;
    const int Lt = (int)P.Ltop;
    const size_t per = 2 * (size_t)Lt * N;
    std::vector<u64> a(24 * per), b(4 * per);
    const u64 *pa = a.data(), *pb = b.data();
    // an address `words` words behind a slab's start, formed as an integer: the callers' pointers are only numbers to the check
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;

    for (int L : {0, Lt + 1, -1}) BAD("merge", plan_merge(P, L, 2, 4, pa, 2, 1, pb));
    for (u64 count : {(u64)0, (u64)N + 1, ~(u64)0}) BAD("merge", plan_merge(P, Lt, 2, count, pa, 2, 1, pb));
    // the plans
    PLAN(0, 0, 0, plan_merge(P, Lt, 2, 1, pa, 0, 1, pb));
    PLAN(1, 2, 4, plan_merge(P, Lt, 2, 2, pa, 2, 1, pb));
    PLAN(2, 4, 12, plan_merge(P, Lt, 2, 3, pa, 2, 1, pb));
    PLAN(2, 4, 12, plan_merge(P, 1, 2, 4, pa, 2, 1, pb));
    PLAN(3, 4, 12, plan_merge(P, Lt, 1, 5, pa, 1, 0, pb));
    PLAN(12, 2048, 6144, plan_merge(P, Lt, 1, N, low, 1, 1, mid));
    PLAN(2, 0, 0, plan_merge(P, Lt, 0, 4, nullptr, 0, 0, nullptr)); // n == 0: nothing to check
    // two inputs at one place
    BAD("merge", plan_merge(P, Lt, 2, 4, pa, 0, 1, pb));
    BAD("merge", plan_merge(P, Lt, 2, 4, pa, 2, 0, pb));
    BAD("merge", plan_merge(P, Lt, 2, 4, pa, 0, 0, pb));
    GOOD("merge", plan_merge(P, Lt, 2, 1, pa, 0, 1, pb)); // count == 1: stride_k moves nothing
    GOOD("merge", plan_merge(P, Lt, 1, 4, pa, 1, 0, pb)); // n == 1: stride_r moves nothing
    BAD("merge", plan_merge(P, Lt, 2, 4, pa, 1, 1, pb));
    BAD("merge", plan_merge(P, Lt, 2, 3, pa, 2, 4, pb));  // k = 2, r = 0 and k = 0, r = 1
    BAD("merge", plan_merge(P, Lt, 4, 3, pa, 6, 4, pb));  // k = 2, r = 0 and k = 0, r = 3: the last index pair
    GOOD("merge", plan_merge(P, Lt, 3, 3, low, 6, 4, mid)); // one result fewer: no pair left
    BAD("merge", plan_merge(P, Lt, 2, 4, pa, 1, 3, pb));
    GOOD("merge", plan_merge(P, Lt, 2, 3, pa, 1, 3, pb));
    GOOD("merge", plan_merge(P, Lt, 2, 2, pa, 3, 2, pb));
    BAD("merge", plan_merge(P, Lt, 3, 3, low, ~(u64)0, ~(u64)0, mid));          // equal strides, however large
    BAD("merge", plan_merge(P, Lt, 3, 3, low, ~(u64)0 - 1, ((u64)1 << 63) - 1, mid)); // 2 stride_r' = stride_k': collides, and far past any span
    // spans
    BAD("merge", plan_merge(P, Lt, 2, 4, low, (u64)1 << 63, 1, mid));
    BAD("merge", plan_merge(P, Lt, 2, 4, low, ~(u64)0, 1, mid));
    BAD("merge", plan_merge(P, Lt, 2, 2, low, 1, ~(u64)0, mid));
    BAD("merge", plan_merge(P, Lt, 3, 1, low, 0, (u64)1 << 63, mid));
    BAD("merge", plan_merge(P, Lt, 2, 2, low, 1, (u64)1 << 50, mid));           // 2^50 ciphertexts are past 2^60 words
    GOOD("merge", plan_merge(P, Lt, 2, 2, low, ((u64)1 << 45) / per * 2, 1, mid)); // 2^46 words: in bounds from a low address
    BAD("merge", plan_merge(P, Lt, 2, 2, high, ((u64)1 << 45) / per * 2, 1, low)); // the same span from the top of the address space wraps it
    BAD("merge", plan_merge(P, Lt, 2, 2, low, 2, 1, at(high, 0)));              // the output wraps it: 2 ciphertexts from 2^64 - 4096
    // one launch
    BAD("merge", plan_merge(P, Lt, (u64)1 << 31, 2, low, (u64)1 << 31, 1, mid));
    BAD("merge", plan_merge(P, Lt, (u64)1 << 19, N, low, (u64)1 << 19, 1, mid));
    BAD("merge", plan_merge(P, Lt, 0x7fffffffull / (2 * Lt * (N / 512)) + 1, 2, low, (u64)1 << 31, 1, mid)); // one pair too many
    GOOD("merge", plan_merge(P, Lt, 0x7fffffffull / (2 * Lt * (N / 512)), 2, low, (u64)1 << 31, 1, mid));
    // overlaps
    BAD("merge", plan_merge(P, Lt, 2, 4, pa, 2, 1, pa));
    BAD("merge", plan_merge(P, Lt, 2, 4, pa, 2, 1, at(pa, 8 * per - 1)));
    GOOD("merge", plan_merge(P, Lt, 2, 4, pa, 2, 1, at(pa, 8 * per)));
    BAD("merge", plan_merge(P, Lt, 2, 4, at(pa, 2 * per - 1), 2, 1, pa));  // the output's last word is the first input's first
    GOOD("merge", plan_merge(P, Lt, 2, 4, at(pa, 2 * per), 2, 1, pa));
    BAD("merge", plan_merge(P, Lt, 2, 2, pa, 3, 1, at(pa, 2 * per)));      // in a gap of padded inputs
    BAD("merge", plan_merge(P, Lt, 1, 1, pa, 0, 0, at(pa, N)));            // count == 1 copies: not over itself either
    if (failures) return 1;
    std::printf("bfv_merge_args ok\n");
    return 0;
}
