// bfv_reply_args_main.cpp -- TEST-ONLY, stand-alone.  Runs plan_reply of csrc/bfv_pir_args.h (the device-free check of
// he355_bfv_reply_compress and he355_bfv_reply_decrypt, and the reply size it returns) at accepted and refused edge arguments -- levels and
// widths at and past their ends, misaligned replies, strides short of a reply and off a multiple of 8, strides near 2^63 and 2^64, spans that
// pass the end of the address space, grids at 2^31, overlaps one byte inside and right behind -- compiled with -fsanitize=address,undefined
// (tests/test_bfv_reply_args_cpu.py).  The check does arithmetic on counts, strides and addresses the caller chose: none of it may overflow a
// signed type, shift out of range or form a pointer outside its slab before the refusal.  Prints "bfv_reply_args ok" and exits 0, or names
// the first case that went the other way.
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
    int k0 = 0, k1 = 0;
    bfv_reply_safe(N, P.plain_modulus, k0, k1);
    if (k0 != 22 || k1 != 34 || !bfv_reply_widths_ok(N, P.primes[0].q, k0, k1)) { std::printf("safe widths\n"); return 1; }
    const u64 B = bfv_reply_size(N, k0, k1);
    if (B != N * 56 / 8) { std::printf("reply size\n"); return 1; }
    std::vector<u64> ct(4 * 2 * (size_t)Lt * N), by(4 * (B / 8 + 3)), st(8);
    const u64 *pc = ct.data();
    const void *pb = by.data();
    const int32_t *s0 = (const int32_t *)st.data(), *s1 = s0 + 4;
    auto at = [](const void *base, u64 bytes) { return (const void *)((unsigned long long)base + bytes); };
    auto wat = [](const void *base, u64 bytes) { return (const u64 *)((unsigned long long)base + bytes); };
    const void *low = (const void *)0x1000, *high = (const void *)0xfffffffffffff000ull;
    const u64 *mid = (const u64 *)0x4000000000000000ull;
    const u64 per = 2 * (u64)Lt * N;
    auto comp = [&](int L, int a, int b, u64 n, const void *bytes, u64 stride, const u64 *c) {
        return plan_reply(P, "he355_bfv_reply_compress", L, a, b, n, bytes, stride, c, 2 * (u64)(L > 0 ? L : 0) * N);
    };
    auto dec = [&](int a, int b, u64 n, const void *bytes, u64 stride, const u64 *pl, const int32_t *x = nullptr, const int32_t *y = nullptr) {
        return plan_reply(P, "he355_bfv_reply_decrypt", 1, a, b, n, bytes, stride, pl, N, true, x, y);
    };
    // the plan
    GOOD("reply", if (comp(Lt, k0, k1, 2, pb, B, pc).bytes != B) throw std::invalid_argument("plan"));
    GOOD("reply", if (dec(2, 2, 2, pb, N / 2, pc).bytes != N / 2) throw std::invalid_argument("plan"));
    // levels
    for (int L : {0, Lt + 1, -1, 1 << 30}) BAD("reply", comp(L, k0, k1, 2, pb, B, pc));
    GOOD("reply", comp(1, k0, k1, 2, pb, B, pc));
    // widths: N 2^(k1 - 1) <= (q_0 - 1) / 2 holds up to k1 = 47 at N = 4096 under a 60-bit prime
    if (!bfv_reply_widths_ok(N, P.primes[0].q, 2, 47) || bfv_reply_widths_ok(N, P.primes[0].q, 2, 48)) { std::printf("width limit\n"); return 1; }
    for (auto w : {std::pair<int, int>{1, 22}, {0, 0}, {-1, 5}, {23, 22}, {2, 48}, {48, 48}, {2, 63}, {2, 64}, {2, 1 << 30}, {-(1 << 30), 2}})
        BAD("reply", comp(Lt, w.first, w.second, 1, low, (u64)1 << 20, mid));
    GOOD("reply", comp(Lt, 2, 47, 1, low, (u64)1 << 20, mid));
    GOOD("reply", comp(Lt, 47, 47, 1, low, (u64)1 << 20, mid));
    GOOD("reply", comp(Lt, 2, 2, 1, low, N / 2, mid));
    // alignment and stride
    BAD("reply", comp(Lt, k0, k1, 2, at(pb, 4), B, pc));
    BAD("reply", comp(Lt, k0, k1, 2, at(pb, 1), B, pc));
    BAD("reply", comp(Lt, k0, k1, 2, pb, B - 8, pc));
    BAD("reply", comp(Lt, k0, k1, 2, pb, B + 4, pc));
    BAD("reply", comp(Lt, k0, k1, 2, pb, 0, pc));
    BAD("reply", comp(Lt, k0, k1, 1, pb, 0, pc)); // n == 1 moves by no stride, but the stride still has to hold a reply
    GOOD("reply", comp(Lt, k0, k1, 2, pb, B + 24, pc));
    GOOD("reply", comp(Lt, k0, k1, 2, at(pb, 8), B, pc));
    // (n - 1) stride + B at and below 2^63, strides near 2^64
    const u64 S62 = (u64)1 << 62;
    BAD("reply", comp(Lt, k0, k1, 3, low, S62, mid));                      // 2 * 2^62 = 2^63
    BAD("reply", comp(Lt, k0, k1, 2, low, (u64)1 << 63, mid));
    BAD("reply", comp(Lt, k0, k1, 2, low, ~(u64)0 - 7, mid));
    BAD("reply", comp(Lt, k0, k1, 2, low, ((u64)1 << 63) - B + 8, mid));   // one word too far
    BAD("reply", comp(Lt, k0, k1, 2, low, ((u64)1 << 63) - B, mid));       // reaches 2^63 exactly
    BAD("reply", comp(Lt, k0, k1, 2, high, ((u64)1 << 63) - B - 8, mid));  // below 2^63, but from the top of the address space it wraps
    BAD("reply", comp(Lt, k0, k1, 2, high, B, mid));                       // two replies from 2^64 - 4096 wrap it
    BAD("reply", comp(Lt, k0, k1, 1, low, B, wat(high, 0)));               // the ciphertexts wrap it
    GOOD("reply", comp(Lt, k0, k1, 2, low, S62, wat(low, S62 + B)));       // 2^62 + B bytes from a low address: in bounds
    GOOD("reply", comp(Lt, k0, k1, 2, low, ((u64)1 << 63) - B - 8 - 0x2000, wat(nullptr, 0xfffffffffffff800ull - 8 * 4 * per)));
    // one launch
    const u64 nmax = 0x7fffffffull / (N / 256);
    BAD("reply", comp(1, 2, 2, nmax + 1, low, N / 2, mid));
    BAD("reply", comp(1, 2, 2, (u64)1 << 40, low, N / 2, mid));
    BAD("reply", comp(1, 2, 2, ~(u64)0, low, N / 2, mid));
    GOOD("reply", comp(1, 2, 2, nmax, low, N / 2, mid));
    // n == 0: nothing to lie anywhere
    GOOD("reply", comp(Lt, k0, k1, 0, nullptr, B, nullptr));
    GOOD("reply", dec(k0, k1, 0, pb, B, wat(pb, 0), (const int32_t *)pb, (const int32_t *)pb));
    // overlaps: compress
    BAD("reply", comp(Lt, k0, k1, 2, pc, B, pc));
    BAD("reply", comp(Lt, k0, k1, 2, at(pc, 8 * 2 * per - 8), B, pc));   // the first reply's first word is the last ciphertext word
    GOOD("reply", comp(Lt, k0, k1, 2, at(pc, 8 * 2 * per), B, pc));
    BAD("reply", comp(Lt, k0, k1, 2, pb, B + 8, wat(pb, 2 * B)));        // the ciphertexts start on the second reply's last word
    GOOD("reply", comp(Lt, k0, k1, 2, pb, B + 8, wat(pb, 2 * B + 8)));
    GOOD("reply", comp(1, k0, k1, 2, at(pc, 8 * 2 * 2 * N), B, pc));     // lower levels read less
    // overlaps: decrypt
    BAD("reply", dec(k0, k1, 2, pb, B, wat(pb, 0)));
    BAD("reply", dec(k0, k1, 2, pb, B, wat(pb, 2 * B - 8)));
    GOOD("reply", dec(k0, k1, 2, pb, B, wat(pb, 2 * B)));
    GOOD("reply", dec(k0, k1, 2, pb, B, pc, s0, s1));
    GOOD("reply", dec(k0, k1, 2, pb, B, pc, nullptr, s1));
    BAD("reply", dec(k0, k1, 2, pb, B, pc, s0, s0));
    BAD("reply", dec(k0, k1, 2, pb, B, pc, s0, s0 + 1));
    GOOD("reply", dec(k0, k1, 2, pb, B, pc, s0, s0 + 2));
    BAD("reply", dec(k0, k1, 2, pb, B, pc, (const int32_t *)pb));
    BAD("reply", dec(k0, k1, 2, pb, B, pc, nullptr, (const int32_t *)at(pb, 2 * B - 4)));
    GOOD("reply", dec(k0, k1, 2, pb, B, pc, nullptr, (const int32_t *)at(pb, 2 * B)));
    BAD("reply", dec(k0, k1, 2, pb, B, pc, (const int32_t *)at(pc, 8 * 2 * N - 4)));
    GOOD("reply", dec(k0, k1, 2, pb, B, pc, (const int32_t *)at(pc, 8 * 2 * N)));
    BAD("reply", dec(k0, k1, 2, pb, B, pc, (const int32_t *)at(high, 0xffc)));  // a budget output that wraps the address space
    if (failures) return 1;
    std::printf("bfv_reply_args ok\n");
    return 0;
}
