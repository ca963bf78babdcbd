// sim_bfv_level.cpp -- TEST-ONLY.  Runs the product's per-coefficient BFV level arithmetic (csrc/bfv_level_core.h: the very functions the
// HIP kernels k_bfv_mod_switch, k_bfv_addsub_plain and k_bfv_lift_plain compile) on the CPU, on the tables the product uploads
// (bfv_drop_table, bfv_delta_const), so that tests/test_bfv_level_core_cpu.py can hold them to Python integers without a GPU.
// Compiled once per form of the u64 engine into tests/csim/_build; the product never contains it.
#include <cstring>
#include <map>
#include <stdexcept>
#include <vector>

#include "../../reference-seal-backend_amd/csrc/bfv_level_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

namespace {
struct LevelSim {
    Params *p = nullptr;
    std::vector<PrimeDev> pd; // the data primes
    std::vector<u64> q;
    std::vector<BfvDropConst> drop;
    std::map<int, BfvDeltaConst> delta;
};
PrimeDev to_dev(const PrimeTables &pt)
{
    PrimeDev d;
    std::memset(&d, 0, sizeof(d));
    const ArU64 au = pt.aru();
    const ArF64 af = pt.arf();
    d.q = pt.q; d.cr0 = pt.mod.cr0; d.cr1 = pt.mod.cr1;
    d.ninv = au.ninv; d.ninv_q = au.ninv_q;
    d.qd = af.q; d.qinv = af.qinv; d.ninv_d = af.ninv; d.ninv_i = af.ninv_i;
    d.f64 = pt.f64 ? 1 : 0;
    return d;
}
} // namespace

extern "C" {

// the form this library was compiled for: 0 Shoup quotients, 1 fold reduction
int sim_bfvl_form(void) { return HE355_U64_FOLD; }

// null when the parameters are refused, or when this library's form is not the one a context of these primes runs
// (fold build: every u64-engine prime must be 2^60 - c, Params::u64_fold; Shoup build: any chain, with Shoup tables)
void *sim_bfvl_create(size_t N, const int *bits, size_t n_bits, int plain_bits)
{
    try {
        LevelSim *s = new LevelSim();
        s->p = Params::create(kSchemeBFV, N, std::vector<int>(bits, bits + n_bits), plain_bits, false, HE355_U64_FOLD != 0);
        if ((HE355_U64_FOLD != 0) != s->p->u64_fold) {
            delete s->p;
            delete s;
            return nullptr;
        }
        for (size_t i = 0; i < s->p->Ltop; ++i) {
            s->pd.push_back(to_dev(s->p->primes[i]));
            s->q.push_back(s->p->primes[i].q);
        }
        s->drop = bfv_drop_table(s->q.data(), (int)s->p->Ltop, s->p->u64_fold);
        return s;
    } catch (const std::exception &) {
        return nullptr;
    }
}
void sim_bfvl_destroy(void *h)
{
    LevelSim *s = static_cast<LevelSim *>(h);
    if (s) { delete s->p; delete s; }
}
size_t sim_bfvl_levels(void *h) { return static_cast<LevelSim *>(h)->p->Ltop; }
uint64_t sim_bfvl_q(void *h, size_t i) { return static_cast<LevelSim *>(h)->q[i]; }
uint64_t sim_bfvl_t(void *h) { return static_cast<LevelSim *>(h)->p->plain_modulus; }
int sim_bfvl_f64(void *h, size_t i) { return static_cast<LevelSim *>(h)->pd[i].f64; }

// n coefficients down the chain: x [n][L] canonical residues -> out [n][L_to]; the instantiation is the one the product's launcher picks
int sim_bfvl_drop(void *h, int L, int L_to, const uint64_t *x, uint64_t *out, size_t n)
{
    LevelSim *s = static_cast<LevelSim *>(h);
    const int Ltop = (int)s->p->Ltop;
    if (L < 1 || L > Ltop || L > kBfvLevelMaxL || L_to < 1 || L_to > L) return 1;
    for (size_t c = 0; c < n; ++c) {
        u64 v[kBfvLevelMaxL] = {0};
        for (int i = 0; i < L; ++i) v[i] = x[c * L + i];
        if (L <= 4) bfv_drop_chain<4>(s->pd.data(), s->drop.data(), Ltop, L, L_to, v);
        else if (L <= 8) bfv_drop_chain<8>(s->pd.data(), s->drop.data(), Ltop, L, L_to, v);
        else bfv_drop_chain<kBfvLevelMaxL>(s->pd.data(), s->drop.data(), Ltop, L, L_to, v);
        for (int i = 0; i < L_to; ++i) out[c * L_to + i] = v[i];
    }
    return 0;
}
// Delta_L(m) under the first L primes: m [n] mod t -> out [n][L]
int sim_bfvl_delta(void *h, int L, const uint64_t *m, uint64_t *out, size_t n)
{
    LevelSim *s = static_cast<LevelSim *>(h);
    if (L < 1 || L > (int)s->p->Ltop) return 1;
    auto it = s->delta.find(L);
    if (it == s->delta.end()) it = s->delta.emplace(L, bfv_delta_const(s->q.data(), L, s->p->plain_modulus)).first;
    const BfvDeltaConst &dc = it->second;
    for (size_t c = 0; c < n; ++c) {
        const u64 fix = bfv_delta_fix(m[c], dc);
        for (int i = 0; i < L; ++i) out[c * L + i] = bfv_delta_residue(m[c], fix, dc.qdivt[i], bfv_modu(s->pd[i]));
    }
    return 0;
}
// the centred lift under the first L primes: m [n] mod t -> out [n][L]
int sim_bfvl_lift(void *h, int L, const uint64_t *m, uint64_t *out, size_t n)
{
    LevelSim *s = static_cast<LevelSim *>(h);
    if (L < 1 || L > (int)s->p->Ltop) return 1;
    for (size_t c = 0; c < n; ++c)
        for (int i = 0; i < L; ++i) out[c * L + i] = bfv_lift_centred(m[c], s->p->plain_modulus, bfv_modu(s->pd[i]));
    return 0;
}
}
