// bfv_bytes_core.h -- the arithmetic of the PIR database codec: packed bytes <-> BFV plaintext coefficients (he355_bfv_bytes_per_plain,
// he355_bfv_unpack_bytes, he355_bfv_unpack_bytes_ntt, he355_bfv_pack_bytes; kernels in he355_kernels_bfv_bytes.hip).  Host-compilable on
// purpose, like bfv_digits_core.h: the HIP kernels, the test-only simulator (tests/csim/sim_bfv_bytes.cpp) and the stand-alone guard
// program (tests/bfv_bytes_guard_main.cpp, run under the address sanitizer) compile the same text.
//
//   definition : w = bitlen(t) - 1 (bfv_digits_core.h's digit width).  The B bytes of a plaintext, 1 <= B <= Bmax = floor(N w / 8), read as ONE
//                little-endian integer v; coefficient e is (v >> (e w)) & (2^w - 1), 0 once e w >= 8 B; the last non-zero field is
//                zero-extended.  The inverse masks every coefficient to w bits, ORs it in at bit e w and keeps the low 8 B bits.
//   extraction : the bytes start at any address a.  The kernels read ALIGNED 64-bit words of base = a & ~7 only; the plaintext's bits are
//                [sh, sh + 8 B) of that word string, sh = 8 (a & 7).  The field at bit p = sh + e w lies in words p >> 6 and (p >> 6) + 1;
//                a funnel shift joins them.  The word that holds byte B - 1 (index `last`) is masked to its valid bits, no word past it is
//                read, and the second word is read only when the field reaches into it.  (Bits below sh in word 0 are never part of a
//                field: every p >= sh.)
//   packing    : output word k of a plaintext holds bits [64 k, 64 k + 64) of v: coefficients floor(64 k / w) .. floor((64 k + 63) / w),
//                the first shifted down when it began in word k - 1.  One owner per word: no atomics, no partial stores.
#pragma once
#include "bfv_digits_core.h"

namespace he355 {

// Where the bytes of one plaintext lie, as the aligned words the kernels read
struct BfvByteSrc {
    const u64 *base; // the aligned word that holds byte 0
    u32 sh;          // 8 (address & 7): the bit of word 0 at which byte 0 starts
    u64 end;         // sh + 8 B: one past the last valid bit
    u64 last;        // (end - 1) >> 6: the word that holds byte B - 1
};
HE_HD BfvByteSrc bfv_bytes_src(const void *bytes, u64 B)
{
    const unsigned long long a = (unsigned long long)bytes;
    BfvByteSrc s;
    s.base = (const u64 *)(a & ~7ull);
    s.sh = (u32)(a & 7) * 8;
    s.end = s.sh + 8 * B;
    s.last = (s.end - 1) >> 6;
    return s;
}
// Bmax: the most bytes N fields of w bits hold
HE_HD u64 bfv_bytes_max(u64 N, int w) { return N * (u64)w / 8; }
// how many coefficients can be non-zero: ceil(8 B / w)
HE_HD u64 bfv_bytes_fields(u64 B, int w) { return (8 * B + (u64)w - 1) / (u64)w; }
// the 64-bit words he355_bfv_pack_bytes writes per plaintext
HE_HD u64 bfv_bytes_words(u64 B) { return (B + 7) / 8; }

// aligned word k of the source with everything at and above bit `end` cleared; 0 (and no read) past the last word
HE_HD u64 bfv_bytes_word(const BfvByteSrc &s, u64 k)
{
    if (k > s.last) return 0;
    const u64 x = s.base[k];
    return k == s.last ? x & bfv_digit_mask((int)(s.end - (s.last << 6))) : x;
}
// coefficient e of the plaintext
HE_HD u64 bfv_bytes_field(const BfvByteSrc &s, u64 e, int w)
{
    const u64 p = s.sh + e * (u64)w;
    if (p >= s.end) return 0;
    const u64 k = p >> 6;
    const int r = (int)(p & 63);
    u64 v = bfv_bytes_word(s, k) >> r;
    if (r + w > 64) v |= bfv_bytes_word(s, k + 1) << (64 - r); // (r >= 2 here: the shift is below 64)
    return v & bfv_digit_mask(w);
}
// output word k < ceil(B / 8) of the plaintext whose N coefficients (any 64-bit words) are coef[]
HE_HD u64 bfv_bytes_pack_word(const u64 *coef, u64 N, u64 k, u64 B, int w)
{
    const u64 lo = 64 * k, e0 = lo / (u64)w;
    u64 e1 = (lo + 63) / (u64)w;
    if (e1 >= N) e1 = N - 1;
    const u64 mask = bfv_digit_mask(w);
    u64 out = 0;
    for (u64 e = e0; e <= e1 && e < N; ++e) {
        const u64 v = coef[e] & mask, p = e * (u64)w;
        out |= p < lo ? v >> (lo - p) : v << (p - lo); // (lo - p < w <= 63, p - lo <= 63)
    }
    const u64 bits = 8 * B;
    return bits - lo >= 64 ? out : out & bfv_digit_mask((int)(bits - lo));
}

} // namespace he355
