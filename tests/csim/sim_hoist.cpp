// sim_hoist.cpp -- TEST-ONLY.  Runs the finish arithmetic of the hoisted rotations (csrc/hoist_core.h: the very functions the HIP kernels
// k_hoist_finish_ntt and k_hoist_finish_coeff compile -- the join of c0 with the key switch, the one-source-row permutation, the plain sum's
// term, the signed coefficient gather) on the CPU, over whole polynomials in the kernels' order of operations, so that
// tests/test_rotate_hoisted_core_cpu.py can hold them to Python integers without a GPU.  The permutation and gather tables are the product's
// own (Params).  Built into tests/csim/_build; the product never contains it.
#include <memory>
#include <vector>

#include "../../reference-seal-backend_amd/csrc/he_params.h"
#include "../../reference-seal-backend_amd/csrc/hoist_core.h"

using namespace he355;

extern "C" {

// the product's tables of a ring of N: the NTT-domain permutation (mode 0) or the signed coefficient gather (mode 1) of `elt`
void sim_hoist_table(uint64_t N, uint32_t elt, int mode, uint32_t *out)
{
    std::unique_ptr<Params> p(Params::create(kSchemeCKKS, (size_t)N, {50, 50}, 0, false));
    const std::vector<uint32_t> t = mode ? p->galois_gather_coeff(elt) : p->galois_perm_ntt(elt);
    for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
}
// k_hoist_finish_ntt on one residue polynomial of N: out = the permutation of (u + c0) (poly0) or of u; u null: of c0 alone (the identity's
// term).  plain (optional): out = acc + plain * that, acc = the old `out` unless first.
void sim_hoist_finish_ntt(uint64_t N, uint64_t q, const uint32_t *perm, const uint64_t *u, const uint64_t *c0, int poly0, const uint64_t *plain, int first, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    for (uint64_t a = 0; a < N / 1024; ++a) {
        const uint32_t *pm = perm + a * 1024;
        const uint64_t srow = (uint64_t)hoist_src_row(pm[0]) * 1024; // the ONE source row, as the wave reads it
        uint64_t row[1024];
        for (int e = 0; e < 1024; ++e) row[e] = u ? hoist_join(u[srow + e], c0 ? c0[srow + e] : 0, poly0 != 0, q) : c0[srow + e];
        for (int e = 0; e < 1024; ++e) {
            const uint64_t v = row[hoist_src_elem(pm[e])];
            uint64_t &o = out[a * 1024 + e];
            o = plain ? hoist_plain_term(first ? 0 : o, v, plain[a * 1024 + e], m) : v;
        }
    }
}
// k_hoist_finish_coeff on one residue polynomial
void sim_hoist_finish_coeff(uint64_t N, uint64_t q, const uint32_t *gather, const uint64_t *src, uint64_t *out)
{
    for (uint64_t o = 0; o < N; ++o) out[o] = hoist_gather_sign(src[hoist_gather_src(gather[o])], gather[o], q);
}

} // extern "C"
