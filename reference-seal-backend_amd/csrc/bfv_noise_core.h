// bfv_noise_core.h -- the per-coefficient arithmetic of the BFV invariant noise budget (Decryptor::invariant_noise_budget) and the
// constants it runs on.  Host-compilable on purpose, like bfv_level_core.h and behz_core.h: the HIP kernel (he355_kernels_bfv_noise.hip:
// k_bfv_noise_bits<W>), the host client (client/he_client.cpp: Client::invariant_noise_budget) and the test-only simulator
// (tests/csim_bfv_noise/sim_bfv_noise.cpp, which holds these very functions to Python integers on the CPU, in both forms of the u64
// engine) compile the same text.
//
// Per ciphertext at level L, q_L the product of the first L primes, t the plain modulus:
//   phase = c0 + c1 s (+ c2 s^2) per prime, coefficient form;  every residue times t mod q_i;  CRT-composed to x in [0, q_L);
//   |x| = q_L - x where x >= (q_L + 1) / 2, else x;  noise_bits = bit length of the largest |x| over the N coefficients;
//   budget = max(0, bitlength(q_L) - noise_bits - 1).
// The largest bit length is the bit length of the largest magnitude, so a coefficient yields one small integer and the reduction over
// the polynomial is an integer maximum.
// [UPSTREAM-UNVERIFIED] as SURVEY.md Appendix A: the published SEAL v3.7.2 algorithm (decryptor.cpp, invariant_noise_budget).
#pragma once
#include <vector>

#include "bfv_level_core.h"
#include "client/multiword.h"

namespace he355 {

constexpr int kBfvNoiseMaxL = 16; // data primes a composition keeps in registers (as BFV decryption: he355_decrypt)

// Per level: t folded into the CRT constant, and the bit length of q_L.  Travels as a kernel argument (host side: cached per level).
struct BfvNoiseConst {
    u64 tinv[kBfvNoiseMaxL]; // t (q_L / q_i)^-1 mod q_i: one multiply takes a phase residue to its CRT digit of t * phase
    int q_bits;              // bit length of q_L
    int pad_;
};
// The multiword CRT tables of the first L primes, W = L + 2 words each, little-endian (DeviceContext::crt_tables uploads exactly these)
struct BfvNoiseView {
    const u64 *Q, *halfQ; // [W]: q_L and floor(q_L / 2)
    const u64 *punct;     // [L][W]: q_L / q_i
};

HE_HD int bfv_noise_bitlen64(u64 v) { return v ? 64 - __builtin_clzll(v) : 0; }

// One coefficient: a[i * stride] + b[i * stride] (mod q_i) is residue i of the phase (a: the key-dependent part c1 s (+ c2 s^2), b: c0,
// which never needs a transform; b == nullptr: a alone), i < L = W - 2.  Returns the bit length of |t * phase mod q_L| centred.
// W = L + 2: the word count of the table rows.  Fixed trip counts throughout, so x[] lives in registers (the reason
// k_ckks_decode_compose<W> is a template, he355_kernels_client.hip).
template <int W> HE_HD int bfv_noise_bits(const u64 *a, const u64 *b, u64 stride, const PrimeDev *primes, const BfvNoiseConst &c, const BfvNoiseView &v)
{
    constexpr int L = W - 2;
    static_assert(L >= 1 && L <= kBfvNoiseMaxL, "1 to 16 data primes");
    // The tables are W = L + 2 words wide (the decoders' headroom), but every value formed here is below L q_L < 2^(60 L + 4) <= 2^(64 L)
    // (every prime of a chain is below 2^60, he_params.cpp): L words hold it, the two top words of every table row are zero and no carry
    // leaves word L - 1, so the multiword loops run over L words of the W-word rows.
    u64 x[L];
#pragma unroll
    for (int k = 0; k < L; ++k) x[k] = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) { // x += (q_L / q_i) * ((t phase_i (q_L / q_i)^-1) mod q_i)
        const ModU64 mi = bfv_modu(primes[i]);
        u64 r = a[(u64)i * stride];
        if (b) r = addmod(r, b[(u64)i * stride], mi.q);
        const u64 f = barrett128((u128)r * c.tinv[i], mi);
        const u64 *pu = v.punct + (u64)i * W;
        u64 carry = 0;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const u128 p = (u128)pu[k] * f + x[k] + carry;
            x[k] = (u64)p;
            carry = (u64)(p >> 64);
        }
    }
    auto cmp = [&](const u64 *o) { // mw_cmp(x, o): ascending, the most significant differing word decides last
        int res = 0;
#pragma unroll
        for (int k = 0; k < L; ++k)
            if (x[k] != o[k]) res = x[k] > o[k] ? 1 : -1;
        return res;
    };
    while (cmp(v.Q) >= 0) { // x -= q_L (fewer than L times)
        u64 borrow = 0;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const u128 d = (u128)x[k] - v.Q[k] - borrow;
            x[k] = (u64)d;
            borrow = (u64)(d >> 64) & 1;
        }
    }
    // SEAL's threshold is x >= (q_L + 1) / 2.  q_L is odd, so (q_L + 1) / 2 = floor(q_L / 2) + 1 and the same set is x > halfQ: the
    // halfQ row of the decryption tables serves.
    if (cmp(v.halfQ) > 0) { // |x| = q_L - x
        u64 borrow = 0;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const u128 d = (u128)v.Q[k] - x[k] - borrow;
            x[k] = (u64)d;
            borrow = (u64)(d >> 64) & 1;
        }
    }
    int bits = 0;
#pragma unroll
    for (int k = 0; k < L; ++k)
        if (x[k]) bits = 64 * k + bfv_noise_bitlen64(x[k]);
    return bits;
}
HE_HD int bfv_noise_budget_of(int q_bits, int noise_bits)
{
    const int b = q_bits - noise_bits - 1;
    return b > 0 ? b : 0;
}

// ---- host side: the constants -------------------------------------------------------------------------------------------------------
inline BfvNoiseConst bfv_noise_const(const u64 *q, int L, u64 t)
{
    BfvNoiseConst c;
    for (int i = 0; i < kBfvNoiseMaxL; ++i) c.tinv[i] = 0;
    c.pad_ = 0;
    u64 Q[client::kMwWords];
    client::mw_zero(Q, client::kMwWords);
    Q[0] = 1;
    for (int i = 0; i < L; ++i) client::mw_mul_small(Q, client::kMwWords, q[i]);
    c.q_bits = 0;
    for (int k = 0; k < client::kMwWords; ++k)
        if (Q[k]) c.q_bits = 64 * k + bfv_noise_bitlen64(Q[k]);
    for (int i = 0; i < L; ++i) {
        const u64 qi = q[i];
        u64 pm = 1 % qi;
        for (int k = 0; k < L; ++k)
            if (k != i) pm = (u64)(((u128)pm * (q[k] % qi)) % qi);
        c.tinv[i] = (u64)(((u128)bfv_level_powmod(pm, qi - 2, qi) * (t % qi)) % qi); // q_i is prime
    }
    return c;
}
// the whole table set on the host (the client and the simulator; the device has the multiword part from crt_tables already)
struct BfvNoiseHostTables {
    int L = 0, words = 0;
    std::vector<u64> Q, halfQ, punct;
    BfvNoiseConst c;
    BfvNoiseView view() const { return BfvNoiseView{Q.data(), halfQ.data(), punct.data()}; }
};
inline BfvNoiseHostTables bfv_noise_host_tables(const u64 *q, int L, u64 t)
{
    BfvNoiseHostTables T;
    const int W = L + 2;
    T.L = L; T.words = W;
    T.Q.assign(W, 0); T.halfQ.assign(W, 0); T.punct.assign((size_t)L * W, 0);
    T.Q[0] = 1;
    for (int i = 0; i < L; ++i) client::mw_mul_small(T.Q.data(), W, q[i]);
    for (int k = 0; k < W; ++k) T.halfQ[k] = (T.Q[k] >> 1) | (k + 1 < W ? T.Q[k + 1] << 63 : 0);
    for (int i = 0; i < L; ++i) {
        u64 *p = T.punct.data() + (size_t)i * W;
        p[0] = 1;
        for (int k = 0; k < L; ++k)
            if (k != i) client::mw_mul_small(p, W, q[k]);
    }
    T.c = bfv_noise_const(q, L, t);
    return T;
}
// runtime dispatch over W = L + 2 for host callers
inline int bfv_noise_bits_host(int L, const u64 *a, const u64 *b, u64 stride, const PrimeDev *primes, const BfvNoiseConst &c, const BfvNoiseView &v)
{
    switch (L + 2) {
#define HE355_NOISE_W(W) case W: return bfv_noise_bits<W>(a, b, stride, primes, c, v);
        HE355_NOISE_W(3) HE355_NOISE_W(4) HE355_NOISE_W(5) HE355_NOISE_W(6) HE355_NOISE_W(7) HE355_NOISE_W(8) HE355_NOISE_W(9) HE355_NOISE_W(10)
        HE355_NOISE_W(11) HE355_NOISE_W(12) HE355_NOISE_W(13) HE355_NOISE_W(14) HE355_NOISE_W(15) HE355_NOISE_W(16) HE355_NOISE_W(17) HE355_NOISE_W(18)
#undef HE355_NOISE_W
    default: return -1;
    }
}

} // namespace he355
