// bfv_level_core.h -- the per-coefficient arithmetic of the BFV level operations (modulus switching, plaintext operands) and the
// constants it runs on.  Host-compilable on purpose, like behz_core.h: the HIP kernels (he355_kernels_bfv_level.hip: k_bfv_mod_switch,
// k_bfv_addsub_plain, k_bfv_lift_plain) and the test-only simulator (tests/csim_bfv/sim_bfv_level.cpp, which holds these very
// functions to Python integers on the CPU, in both forms of the u64 engine) compile the same text.
//
//   drop chain : Evaluator::mod_switch_to_next for BFV = RNSTool::divide_and_round_q_last_inplace, once per dropped prime:
//                r = (c_last + floor(q_last / 2)) mod q_last,  out_i = (c_i - (r mod q_i - floor(q_last / 2) mod q_i)) q_last^-1 mod q_i
//   delta      : multiply_add_plain_with_scaling_variant at a level: Delta_L(m) = floor((q_L m + floor((t + 1) / 2)) / t) mod q_i with
//                q_L the product of the first L primes, computed as floor(q_L / t) m + floor(((q_L mod t) m + floor((t + 1) / 2)) / t)
//   lift       : multiply_plain_normal's centred lift of a plaintext coefficient, m or m - t (mod q_i)
// [UPSTREAM-UNVERIFIED] as SURVEY.md Appendix A: the published SEAL v3.7.2 algorithms.
#pragma once
#include <vector>

#include "device_types.h"

namespace he355 {

constexpr int kBfvLevelMaxL = 16; // data primes a drop chain keeps in registers (as BFV decryption: he355_decrypt)

// Constants of dropping prime j, seen from target prime i < j: entry [j * stride + i] of a host-built table.  Both engines' forms of
// q_j^-1 mod q_i travel together (the FC shape ArU64 / ArF64 ::floor_fin2_s take), the prime's owner picks its own.
struct BfvDropConst {
    u64 inv, inv_shoup;  // q_j^-1 mod q_i and the u64 engine's companion word (Shoup quotient, or inv 2^32 mod q_i in the fold build)
    double inv_d, inv_i; // the same for the fp64 engine: value and fl(value / q_i)
    u64 half_mod;        // floor(q_j / 2) mod q_i
    u64 pad_;
};
// Constants of Delta_L: per level (q_L mod t and floor(q_L / t) mod q_i change with L)
struct BfvDeltaConst {
    u64 t, q_mod_t, thr;   // thr = floor((t + 1) / 2)
    u64 qdivt[kMaxPrimes]; // floor(q_L / t) mod q_i, i < L
};

HE_HD ModU64 bfv_modu(const PrimeDev &p)
{
    ModU64 m;
    m.q = p.q; m.cr0 = p.cr0; m.cr1 = p.cr1;
    return m;
}
HE_HD ArU64 bfv_aru(const PrimeDev &p)
{
    ArU64 a;
    a.q = p.q; a.two_q = p.q * 2; a.ninv = p.ninv; a.ninv_q = p.ninv_q; a.cr0 = p.cr0; a.cr1 = p.cr1;
    return a;
}
HE_HD ArF64 bfv_arf(const PrimeDev &p)
{
    ArF64 a;
    a.q = p.qd; a.qinv = p.qinv; a.ninv = p.ninv_d; a.ninv_i = p.ninv_i;
    return a;
}

// ---- drop chain -------------------------------------------------------------------------------------------------------------------
// r = (c_last + floor(q_last / 2)) mod q_last: the rounded source of one step, shared by its targets
HE_HD u64 bfv_drop_source(u64 c_last, u64 q_last) { return addmod(c_last, q_last >> 1, q_last); }
// one target residue of one step, by the engine that owns prime i: (c_i - delta) q_last^-1 with delta = r mod q_i - floor(q_last / 2) mod q_i
template <class Ar> HE_HD u64 bfv_drop_residue(const Ar &ar, const ModU64 &mi, u64 ci, u64 r, u64 q_last, const BfvDropConst &fc)
{
    const u64 ri = q_last > mi.q ? barrett64(r, mi) : r; // r < q_last
    const u64 delta = submod(ri, fc.half_mod, mi.q);
    return ar.floor_fin2_s(ci, ar.from_canon(delta), fc);
}
// One coefficient down the chain: x[0 .. L-1] canonical residues -> x[0 .. L_to-1], primes L-1, L-2, .. L_to dropped one after the other
// (every step reads the residues the step before it left).  ML: the instantiation's register budget, L <= ML.
template <int ML> HE_HD void bfv_drop_chain(const PrimeDev *primes, const BfvDropConst *tab, int stride, int L, int L_to, u64 x[ML])
{
#pragma unroll
    for (int j = ML - 1; j >= 1; --j) {
        if (j >= L || j < L_to) continue;
        const u64 qj = primes[j].q;
        const u64 r = bfv_drop_source(x[j], qj);
#pragma unroll
        for (int i = 0; i < ML - 1; ++i) {
            if (i >= j) continue;
            const PrimeDev &Pi = primes[i];
            const BfvDropConst &fc = tab[j * stride + i];
            const ModU64 mi = bfv_modu(Pi);
            x[i] = Pi.f64 ? bfv_drop_residue(bfv_arf(Pi), mi, x[i], r, qj, fc) : bfv_drop_residue(bfv_aru(Pi), mi, x[i], r, qj, fc);
        }
    }
}

// ---- Delta_L(m) -------------------------------------------------------------------------------------------------------------------
// floor(((q_L mod t) m + floor((t + 1) / 2)) / t): the part of Delta_L(m) every prime shares (m, q_L mod t < t)
HE_HD u64 bfv_delta_fix(u64 m, const BfvDeltaConst &c)
{
    if ((c.t >> 32) == 0) return (m * c.q_mod_t + c.thr) / c.t; // below 2^64: one 64-bit division
    return (u64)(((u128)m * c.q_mod_t + c.thr) / c.t);
}
HE_HD u64 bfv_delta_residue(u64 m, u64 fix, u64 qdivt_i, const ModU64 &mi)
{
    return addmod(barrett128((u128)m * qdivt_i, mi), barrett64(fix, mi), mi.q);
}

// ---- centred lift -----------------------------------------------------------------------------------------------------------------
// m < floor((t + 1) / 2): m, else m - t, as a canonical residue mod q_i (any t, q_i below 2^63)
HE_HD u64 bfv_lift_centred(u64 m, u64 t, const ModU64 &mi)
{
    const bool pos = m < ((t + 1) >> 1);
    const u64 v = pos ? m : t - m;
    const u64 r = v >= mi.q ? barrett64(v, mi) : v;
    return (pos || r == 0) ? r : mi.q - r;
}

// ---- host side: the tables ----------------------------------------------------------------------------------------------------------
inline u64 bfv_level_powmod(u64 a, u64 e, u64 q)
{
    u64 r = 1 % q;
    a %= q;
    for (; e; e >>= 1) {
        if (e & 1) r = (u64)(((u128)r * a) % q);
        a = (u64)(((u128)a * a) % q);
    }
    return r;
}
// [n * n] entries, [j * n + i] filled for i < j.  fold: the context's u64 engine runs the fold build (Params::u64_fold)
inline std::vector<BfvDropConst> bfv_drop_table(const u64 *q, int n, bool fold)
{
    std::vector<BfvDropConst> tab((size_t)n * n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            BfvDropConst &f = tab[(size_t)j * n + i];
            f.inv = f.inv_shoup = f.half_mod = f.pad_ = 0;
            f.inv_d = f.inv_i = 0.0;
            if (i >= j) continue;
            const u64 qi = q[i], qj = q[j];
            f.inv = bfv_level_powmod(qj % qi, qi - 2, qi); // q_i is prime
            f.inv_shoup = pre_word(f.inv, qi, fold);
            f.inv_d = (double)f.inv;
            f.inv_i = (double)f.inv / (double)qi;
            f.half_mod = (qj >> 1) % qi;
        }
    return tab;
}
inline BfvDeltaConst bfv_delta_const(const u64 *q, int L, u64 t)
{
    BfvDeltaConst c;
    c.t = t; c.thr = (t + 1) >> 1; c.q_mod_t = 1 % t;
    for (int i = 0; i < kMaxPrimes; ++i) c.qdivt[i] = 0;
    for (int i = 0; i < L; ++i) c.q_mod_t = (u64)(((u128)c.q_mod_t * (q[i] % t)) % t);
    for (int i = 0; i < L; ++i) { // floor(q_L / t) = (q_L - q_L mod t) / t, and q_L = 0 (mod q_i)
        const u64 qi = q[i], tinv = bfv_level_powmod(t % qi, qi - 2, qi), neg = (c.q_mod_t % qi) ? qi - c.q_mod_t % qi : 0;
        c.qdivt[i] = (u64)(((u128)neg * tinv) % qi);
    }
    return c;
}

} // namespace he355
