// device_tables.h -- the tables a device context uploads when it is made, built on the host: the per-prime block (PrimeDev) with k_k2n's
// lift-class masks, the floor-step constants (FloorConst [K][K]) and the multiword CRT tables of a level.  DeviceContext::init and
// DeviceContext::crt_tables build them here, upload them and wire the device pointers.  Host-only on purpose (no HIP header), in the style
// of rotation_plan.h: tests/csim returns the masks to tests/test_explicit_moduli_cpu.py, tests/floor_forms_host.cpp runs the floor steps on
// floor_const's constants, and tests/shape_rules_main.cpp walks the tables under the sanitizers.
#pragma once
#include <cstring>
#include <vector>

#include "he_params.h"
#include "client/multiword.h"

namespace he355 {

// The device block of one prime of a context over a ring of N coefficients, filled in place; fwd / inv (the device copies of pt.fwd /
// pt.inv) and the k2 masks (k2_lift_masks) are left null / zero for the caller.
inline void prime_dev_fill(PrimeDev &d, const PrimeTables &pt, size_t N)
{
    const ArU64 au = pt.aru();
    const ArF64 af = pt.arf();
    d.q = pt.q; d.cr0 = pt.mod.cr0; d.cr1 = pt.mod.cr1;
    d.ninv = au.ninv; d.ninv_q = au.ninv_q;
    d.qd = af.q; d.qinv = af.qinv; d.ninv_d = af.ninv; d.ninv_i = af.ninv_i;
    d.fwd = nullptr; d.inv = nullptr; d.inv_w0_scaled = pt.inv_w0_scaled;
    d.f64 = pt.f64 ? 1 : 0;
    d.acc_terms = pt.f64 ? floor_direct_terms(pt.q) : 0;
    for (size_t k = 0; k < 64; ++k) d.colw[k] = 0.0;
    if (pt.f64)
        for (size_t k = 0; k < 32 && k < N; ++k) { d.colw[k] = ArF64::tw_w(pt.fwd[k]); d.colw[32 + k] = ArF64::tw_w(pt.inv[k]); }
    d.k2_direct = d.k2_lift = 0;
    d.pow32 = (double)((((u64)1) << 32) % pt.q);
}

// k_k2n's lift class of (digit prime q_j, fp64-engine target prime q_t) -- the same rule the kernel's general path evaluates
enum K2Class { kK2General = 0, kK2Direct = 1, kK2Lift = 2 };
inline K2Class k2_lift_class(u64 qj, u64 qt, int logn1)
{
    const bool df = (qj >> 52) == 0, direct = df && !(qj > 2 * qt);
    double m = df ? (direct ? (double)qj : 0.5 * (double)qt + 1.0) : (double)qt;
    for (int st = 0; st < logn1; ++st) m += (double)qt * (0.5 + m * 4.440892098500626e-16);
    if (!(m * 1.0000001 < 140737488355328.0)) return kK2General;
    return direct ? kK2Direct : kK2Lift;
}
// ... as the masks of the chain's K primes: bit t of pd[j].k2_direct / pd[j].k2_lift (device_types.h)
inline void k2_lift_masks(const Params &P, PrimeDev *pd)
{
    for (size_t j = 0; j < P.K; ++j)
        for (size_t t = 0; t < P.K; ++t) {
            if (!P.primes[t].f64) continue;
            const K2Class c = k2_lift_class(P.primes[j].q, P.primes[t].q, P.logn1);
            if (c == kK2General) continue;
            (c == kK2Direct ? pd[j].k2_direct : pd[j].k2_lift) |= (u64)1 << t;
        }
}

// The floor-step constants of source prime qs seen from target prime qi != qs
inline FloorConst floor_const(u64 qs, u64 qi, bool fold)
{
    FloorConst f;
    std::memset(&f, 0, sizeof(f));
    const u64 inv = Params::invmod(qs % qi, qi);
    f.inv = inv;
    f.inv_shoup = pre_word(inv, qi, fold); // the u64 engine's companion word (Shoup quotient, or inv 2^32 mod q_i)
    f.inv_d = (double)inv;
    f.inv_i = (double)inv / (double)qi;
    f.half_mod = (qs >> 1) % qi;
    f.src_mod = qs % qi;
    return f;
}
// [K * K], entry [s * K + i]; the diagonal is zeros
inline std::vector<FloorConst> floor_const_table(const Params &P)
{
    const size_t K = P.K;
    std::vector<FloorConst> fc(K * K);
    for (size_t s = 0; s < K; ++s)
        for (size_t i = 0; i < K; ++i)
            if (s != i) fc[s * K + i] = floor_const(P.primes[s].q, P.primes[i].q, P.primes[i].fold);
    return fc;
}

// The CRT tables of the first L primes (client/multiword.h CrtView) as one block: Q | floor(Q / 2) | the L punctured products (`words`
// words each) | their inverses mod q_i
struct CrtTablesHost {
    int L = 0, words = 0;
    size_t o_half = 0, o_punct = 0, o_inv = 0;
    std::vector<u64> h;
    double Qd = 0;
};
inline CrtTablesHost crt_tables_host(const Params &P, int L)
{
    CrtTablesHost c;
    const int words = L + 2;
    c.L = L; c.words = words;
    c.o_half = words; c.o_punct = 2 * (size_t)words; c.o_inv = c.o_punct + (size_t)L * words;
    c.h.assign(c.o_inv + L, 0);
    u64 *Q = c.h.data(), *halfQ = Q + c.o_half;
    Q[0] = 1;
    for (int i = 0; i < L; ++i) client::mw_mul_small(Q, words, P.primes[i].q);
    for (int i = 0; i < words; ++i) halfQ[i] = (Q[i] >> 1) | (i + 1 < words ? Q[i + 1] << 63 : 0);
    for (int i = 0; i < L; ++i) {
        u64 *p = c.h.data() + c.o_punct + (size_t)i * words;
        p[0] = 1;
        u64 pm = 1;
        const u64 qi = P.primes[i].q;
        for (int k = 0; k < L; ++k)
            if (k != i) {
                client::mw_mul_small(p, words, P.primes[k].q);
                pm = (u64)(((u128)pm * (P.primes[k].q % qi)) % qi);
            }
        c.h[c.o_inv + i] = Params::invmod(pm, qi);
    }
    c.Qd = client::mw_to_double(Q, words);
    return c;
}

} // namespace he355
