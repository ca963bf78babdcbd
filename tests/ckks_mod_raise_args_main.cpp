// ckks_mod_raise_args_main.cpp -- TEST-ONLY, stand-alone.  Runs the device-free checks of he355_ckks_mod_raise and he355_ckks_lift_centred
// (csrc/raise_args.h) at accepted and refused edge arguments -- a BFV context, levels at and past their ends on either side, sizes 0 and 4,
// null pointers with and without work, slabs on an odd word, spans at and past 2^60 words and past the end of the address space, overlaps one word inside and right
// behind (the ignored rows of d_in count), the empty calls -- and the host rule of the small-batch split.  Compiled with
// -fsanitize=address,undefined (tests/test_ckks_mod_raise_args_cpu.py).  Prints "ckks_mod_raise_args ok" and exits 0, or names the first
// case that went the other way.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/raise_args.h"
#include "args_main_common.h"

using namespace he355;

int main()
{
    const size_t N = 4096;
    std::unique_ptr<Params> pb(Params::create(kSchemeBFV, N, {60, 40, 40, 60}, 20, false));
    std::unique_ptr<Params> pc(Params::create(kSchemeCKKS, N, {60, 40, 40, 40, 40, 60}, 0, false));
    std::unique_ptr<Params> p1(Params::create(kSchemeCKKS, N, {60}, 0, false)); // K = 1: one prime, no special prime
    const Params &B = *pb, &Ck = *pc;
    const int Lt = (int)Ck.Ltop; // 5
    std::vector<u64> a(4 * 3 * (size_t)Lt * N), b(4 * 3 * (size_t)Lt * N);
    const u64 *pa = a.data(), *po = b.data();
    auto at = [](const u64 *base, u64 words) { return (const u64 *)((unsigned long long)base + 8 * words); };
    const u64 *low = (const u64 *)0x1000, *high = (const u64 *)0xfffffffffffff000ull, *mid = (const u64 *)0x4000000000000000ull;

    // ---- he355_ckks_mod_raise
    auto up = [&](const Params &P, int L_in, int L_to, int size, u64 n, const u64 *in, const u64 *out) { return plan_mod_raise(P, L_in, L_to, size, n, in, out); };
    GOOD("raise 1 -> top", if (up(Ck, 1, Lt, 2, 4, pa, po)) throw std::invalid_argument("empty"));
    GOOD("raise top -> top", up(Ck, Lt, Lt, 2, 4, pa, po));
    GOOD("raise top -> 1 (the copy alone)", up(Ck, Lt, 1, 3, 4, pa, po));
    GOOD("size 1", up(Ck, 2, 3, 1, 4, pa, po));
    GOOD("one prime", up(*p1, 1, 1, 2, 1, pa, po));
    BAD("BFV", up(B, 1, 2, 2, 4, pa, po));
    BAD("BFV, n == 0", up(B, 1, 2, 2, 0, nullptr, nullptr));
    for (int l : {0, Lt + 1, -1}) {
        BAD("L_in", up(Ck, l, Lt, 2, 4, pa, po));
        BAD("L_to", up(Ck, 1, l, 2, 4, pa, po));
        BAD("L_in, n == 0", up(Ck, l, Lt, 2, 0, nullptr, nullptr));
    }
    BAD("L_to past the one prime", up(*p1, 1, 2, 2, 1, pa, po));
    for (int size : {0, 4, -1}) BAD("size", up(Ck, 1, Lt, size, 4, pa, po));
    BAD("null input", up(Ck, 1, Lt, 2, 4, nullptr, po));
    BAD("null output", up(Ck, 1, Lt, 2, 4, pa, nullptr));
    GOOD("n == 0", if (!up(Ck, 1, Lt, 2, 0, nullptr, nullptr)) throw std::invalid_argument("not empty"));
    BAD("span", up(Ck, 1, Lt, 2, ~(u64)0, low, mid));
    BAD("span of the output", up(Ck, 1, Lt, 2, ((u64)1 << 60) / (2 * Lt * N) + 1, low, mid));
    BAD("span of the ignored rows", up(Ck, Lt, 1, 2, ((u64)1 << 60) / (2 * Lt * N) + 1, low, mid));
    GOOD("span", up(Ck, 1, Lt, 2, ((u64)1 << 44) / (2 * Lt * N), low, mid));
    BAD("in wraps", up(Ck, 1, Lt, 2, 2, high, low));
    BAD("out wraps", up(Ck, 1, Lt, 2, 2, low, high));
    {
        // n = 2, size = 2: d_in at L_in = 1 spans 4 N words, at L_in = 5 it spans 20 N -- rows 1 .. 4 are never read and still count
        const u64 w1 = 2 * 2 * 1 * N, w5 = 2 * 2 * 5 * N, wo = 2 * 2 * 3 * N;
        BAD("out at in", up(Ck, 1, 3, 2, 2, pa, pa));
        BAD("out one word inside in", up(Ck, 1, 3, 2, 2, pa, at(pa, w1 - 1)));
        GOOD("out right behind in", up(Ck, 1, 3, 2, 2, pa, at(pa, w1)));
        BAD("out inside the ignored rows", up(Ck, 5, 3, 2, 2, pa, at(pa, w5 - 1)));
        BAD("out at the first ignored row", up(Ck, 5, 3, 2, 2, pa, at(pa, N)));
        GOOD("out right behind the ignored rows", up(Ck, 5, 3, 2, 2, pa, at(pa, w5)));
        BAD("in one word inside out", up(Ck, 1, 3, 2, 2, at(po, wo - 1), po));
        GOOD("in right behind out", up(Ck, 1, 3, 2, 2, at(po, wo), po));
    }
    BAD("in on an odd word", up(Ck, 1, 3, 2, 2, at(pa, 1), po));
    BAD("out on an odd word", up(Ck, 1, 3, 2, 2, pa, at(po, 1)));
    GOOD("both two words in", up(Ck, 1, 3, 2, 2, at(pa, 2), at(po, 2)));

    // ---- he355_ckks_lift_centred
    auto lift = [&](const Params &P, int L_to, u64 n, const u64 *in, const u64 *out) { return plan_lift_centred(P, L_to, n, in, out); };
    GOOD("lift", if (lift(Ck, Lt, 4, pa, po)) throw std::invalid_argument("empty"));
    GOOD("lift to 1", lift(Ck, 1, 4, pa, po));
    BAD("BFV", lift(B, 2, 4, pa, po));
    for (int l : {0, Lt + 1, -1}) BAD("L_to", lift(Ck, l, 4, pa, po));
    BAD("null input", lift(Ck, Lt, 4, nullptr, po));
    BAD("null output", lift(Ck, Lt, 4, pa, nullptr));
    GOOD("n == 0", if (!lift(Ck, Lt, 0, nullptr, nullptr)) throw std::invalid_argument("not empty"));
    BAD("n == 0, bad level", lift(Ck, 0, 0, nullptr, nullptr));
    BAD("span", lift(Ck, Lt, ~(u64)0, low, mid));
    BAD("span", lift(Ck, Lt, ((u64)1 << 60) / (Lt * N) + 1, low, mid));
    GOOD("span", lift(Ck, Lt, ((u64)1 << 44) / (Lt * N), low, mid));
    BAD("in wraps", lift(Ck, Lt, 2, high, low));
    BAD("out wraps", lift(Ck, Lt, 2, low, high));
    BAD("out at in", lift(Ck, 3, 2, pa, pa));
    BAD("out one word inside in", lift(Ck, 3, 2, pa, at(pa, 2 * N - 1)));
    GOOD("out right behind in", lift(Ck, 3, 2, pa, at(pa, 2 * N)));
    BAD("in one word inside out", lift(Ck, 3, 2, at(po, 2 * 3 * N - 1), po));
    GOOD("in right behind out", lift(Ck, 3, 2, at(po, 2 * 3 * N), po));
    BAD("in on an odd word", lift(Ck, 3, 2, at(pa, 1), po));
    BAD("out on an odd word", lift(Ck, 3, 2, pa, at(po, 3)));
    GOOD("both two words in", lift(Ck, 3, 2, at(pa, 2), at(po, 2)));

    // ---- the split rule: fewer blocks than compute units -> min(L_to - 1, ceil(cus / blocks))
    if (raise_tsplit(1, 16, 256) != 15 || raise_tsplit(2, 6, 256) != 5 || raise_tsplit(63, 6, 256) != 2 || raise_tsplit(64, 6, 256) != 1 || raise_tsplit(1, 2, 256) != 1 ||
        raise_tsplit(1, 1, 256) != 1 || raise_tsplit(0, 6, 256) != 1 || raise_tsplit(~(u64)0 / 4, 6, 256) != 1) {
        std::printf("the split rule\n");
        ++failures;
    }
    if (failures) return 1;
    std::printf("ckks_mod_raise_args ok\n");
    return 0;
}
