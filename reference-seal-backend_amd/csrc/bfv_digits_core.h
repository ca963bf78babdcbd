// bfv_digits_core.h -- the per-coefficient arithmetic of the BFV ciphertext decomposition for recursive (two-dimensional) PIR
// (he355_bfv_decompose, he355_bfv_decompose_ntt, he355_bfv_compose; kernels in he355_kernels_bfv_digits.hip) and the digit table it runs
// on.  Host-compilable on purpose, like bfv_expand_core.h: the HIP kernels and the test-only simulator (tests/csim/sim_bfv_digits.cpp, which
// holds these very functions to Python integers on the CPU) compile the same text.
//
//   table   : w = bitlen(t) - 1 (2^w <= t: every w-bit value is a plaintext coefficient), b_i = bitlen(q_i), D_i = ceil(b_i / w),
//             off_i = sum_{i' < i} D_i', D(L) = off_L.  A ciphertext [size][L][N] becomes F = size D(L) plaintexts; polynomial k, prime i,
//             digit g is plaintext k D(L) + off_i + g.
//   digit   : digit g of a canonical residue x is (x >> (g w)) & (2^w - 1); every shift is below 64 (g w < b_i <= 63).
//   compose : residue = sum_g (digit_g masked) 2^(g w), digits below the top one masked to w bits, the top one to b_i - (D_i - 1) w bits:
//             the sum is below 2^b_i < 2 q_i, one conditional subtraction makes it canonical whatever the digits were.
// The centred lift of a digit under an output prime is bfv_level_core.h's bfv_lift_centred, as for any plaintext coefficient.
#pragma once
#include "device_types.h"

namespace he355 {

// The digit table of a level: small enough to travel as a kernel argument.  D_i <= 63 and D(L) <= 64 * 63.
struct BfvDigitTab {
    int w, L;
    u32 total;                           // D(L)
    unsigned char D[kMaxPrimes];         // digits of prime i
    unsigned char bits[kMaxPrimes];      // b_i
    unsigned short off[kMaxPrimes + 1];  // off_i; off[L] = D(L)
};

HE_HD int bfv_bitlen(u64 x)
{
    int n = 0;
    for (; x; x >>= 1) ++n;
    return n;
}
HE_HD u64 bfv_digit_mask(int bits) { return bits >= 64 ? ~(u64)0 : ((u64)1 << bits) - 1; }
// digit g of x, w bits wide
HE_HD u64 bfv_digit(u64 x, int g, int w) { return (x >> (g * w)) & bfv_digit_mask(w); }
// the bits of digit g that compose keeps: w below the top digit, what is left of b bits at the top
HE_HD int bfv_digit_keep(int g, int D, int b, int w) { return g + 1 < D ? w : b - (D - 1) * w; }
// one term of the composition: (digit masked) 2^(g w)
HE_HD u64 bfv_undigit_term(u64 digit, int g, int D, int b, int w) { return (digit & bfv_digit_mask(bfv_digit_keep(g, D, b, w))) << (g * w); }
// the terms' sum (< 2^b < 2 q) as a canonical residue
HE_HD u64 bfv_undigit_finish(u64 sum, u64 q) { return sum >= q ? sum - q : sum; }
// the prime whose digits hold digit index d < D(L) of a polynomial: off_i <= d < off_(i+1)
HE_HD int bfv_digit_prime(const BfvDigitTab &tab, u32 d)
{
    int i = 0;
    while (i + 1 < tab.L && d >= tab.off[i + 1]) ++i;
    return i;
}

// Plaintext pf = r F + f of a batch, F = size D(L): which residue polynomial of which ciphertext it is cut from, and which digit
struct BfvDigitSrc {
    u64 poly;  // (r size + k) L + i: the residue polynomial of the ciphertext slab [n][size][L][N]
    int prime; // i
    int digit; // g
};
HE_HD BfvDigitSrc bfv_digit_src(const BfvDigitTab &tab, int size, u64 pf)
{
    const u32 F = (u32)size * tab.total, f = (u32)(pf % F);
    const u64 r = pf / F;
    const u32 k = f / tab.total, d = f % tab.total;
    const int i = bfv_digit_prime(tab, d);
    return BfvDigitSrc{(r * size + k) * tab.L + i, i, (int)(d - tab.off[i])};
}

// host side: the table of the first L primes for plain modulus t >= 2 (L <= kMaxPrimes, q_i < 2^63)
inline BfvDigitTab bfv_digit_table(const u64 *q, int L, u64 t)
{
    BfvDigitTab tab;
    tab.w = bfv_bitlen(t) - 1;
    if (tab.w < 1) tab.w = 1; // (t < 2 is refused by the callers)
    tab.L = L;
    unsigned off = 0;
    for (int i = 0; i < kMaxPrimes; ++i) {
        tab.D[i] = tab.bits[i] = 0;
        tab.off[i] = (unsigned short)off;
        if (i >= L) continue;
        const int b = bfv_bitlen(q[i]);
        tab.bits[i] = (unsigned char)b;
        tab.D[i] = (unsigned char)((b + tab.w - 1) / tab.w);
        off += tab.D[i];
    }
    tab.off[kMaxPrimes] = (unsigned short)off;
    tab.total = off;
    return tab;
}

} // namespace he355
