// bfv_mac_core.h -- the per-coefficient arithmetic of the NTT-form BFV plaintext inner product (he355_bfv_multiply_plain_accumulate,
// k_bfv_plain_mac in he355_kernels_bfv_ntt.hip): multiply-add into a 128-bit sum, the rule for how many terms such a sum takes, and its
// reduction.  Host-compilable on purpose, like behz_core.h, bfv_level_core.h and bfv_noise_core.h: the HIP kernel and the test-only
// simulator (tests/csim_bfv_mac/sim_bfv_mac.cpp, which holds these very functions to Python integers on the CPU) compile the same text.
//
//   sum    : out = sum_k a_k b_k mod q over canonical residues a_k, b_k <= q - 1.  The products are added UNREDUCED into a 128-bit
//            accumulator (a 64 x 64 -> 128 multiply-add is four v_mad_u64_u32 and their carries; the Barrett reduction is paid once per run)
//   run    : a sum of R terms is at most R (q - 1)^2, so it stays below 2^128 for R <= floor((2^128 - 1) / (q - 1)^2) -- 256 terms for the
//            60-bit primes, 2^28 and more for primes of 50 bits and fewer.  (This is floor(2^128 / (q - 1)^2) unless (q - 1)^2 divides
//            2^128, i.e. q = 2^k + 1; such a q is prime for k = 1, 2, 4, 8, 16 only, where both values lie far above the cap.)  Runs are
//            capped at kBfvMacMaxRun = 2^16 terms: one reduction per 65536 terms is free, and every run length is one a test can walk.
//   fold   : at the end of a run the sum is reduced to its canonical residue (barrett128: exact for ANY 128-bit value, its quotient
//            estimate floor(x floor(2^128 / q) / 2^128) is the true quotient or one below it) and that residue -- at most q - 1, no more
//            than one term -- starts the next run, which therefore takes bfv_mac_run - 1 new terms.
// The result is the canonical residue of the exact integer sum, so it does not depend on where the runs are cut.
#pragma once
#include "device_types.h"

namespace he355 {

constexpr u64 kBfvMacMaxRun = (u64)1 << 16;

// terms one 128-bit sum takes under prime q (host side: a 128-bit division; the kernel gets the value with its arguments)
inline u64 bfv_mac_run(u64 q)
{
    if (q < 3) return kBfvMacMaxRun;
    const u128 m = (u128)(q - 1) * (q - 1);
    const u128 r = ~(u128)0 / m;
    return r > kBfvMacMaxRun ? kBfvMacMaxRun : (u64)r;
}

// acc += a b: a, b canonical; the caller keeps to the run length
HE_HD void bfv_mac_add(u128 &acc, u64 a, u64 b) { acc += (u128)a * b; }
// the canonical residue of a sum
HE_HD u64 bfv_mac_reduce(u128 acc, const ModU64 &m) { return barrett128(acc, m); }
// end of a run that is not the last: the sum's residue becomes the first term of the next run
HE_HD void bfv_mac_fold(u128 &acc, const ModU64 &m) { acc = bfv_mac_reduce(acc, m); }

// One result coefficient, the loop the kernel runs per accumulator: terms a[k * sa], b[k * sb], k < inner, cut into runs of `run` terms
// (run >= 2: the first run takes `run` terms, every later one the carried residue and run - 1 new terms).
HE_HD u64 bfv_mac_dot(const u64 *a, u64 sa, const u64 *b, u64 sb, u64 inner, u64 run, const ModU64 &m)
{
    u128 acc = 0;
    u64 k = 0, take = run;
    while (k < inner) {
        const u64 end = inner - k < take ? inner : k + take;
        for (; k < end; ++k) bfv_mac_add(acc, a[k * sa], b[k * sb]);
        if (k < inner) bfv_mac_fold(acc, m);
        take = run - 1;
    }
    return bfv_mac_reduce(acc, m);
}

} // namespace he355
