// sim_hoist_lazy.cpp -- TEST-ONLY.  Runs the arithmetic of the lazy plain sum and of the plaintext extension (csrc/hoist_core.h: the very
// functions the HIP kernels k_hoist_acc_qp and k_plain_extend compile -- the tile's prime, one term of an accumulator, the constant the
// special prime's forward row pass leaves to take out, the centred reduction of a coefficient) on the CPU, over whole residue polynomials in
// the kernels' order of operations, so that tests/test_rotate_hoisted_lazy_core_cpu.py can hold them to Python integers without a GPU.
// Built into tests/csim/_build; the product never contains it.
#include "../../reference-seal-backend_amd/csrc/he_params.h"
#include "../../reference-seal-backend_amd/csrc/hoist_core.h"

using namespace he355;

extern "C" {

int sim_hoist_qp_prime(int idx, int L, int K) { return hoist_qp_prime(idx, L, K); }
// k_hoist_acc_qp on one residue polynomial of N: acc = (first ? 0 : acc) + plain * (src permuted; perm null: the identity's term, src as it
// lies), the ONE source row of every row read whole as the wave reads it
void sim_hoist_acc_qp(uint64_t N, uint64_t q, const uint32_t *perm, const uint64_t *src, const uint64_t *plain, int first, uint64_t *acc)
{
    const ModU64 m = make_mod(q);
    for (uint64_t a = 0; a < N / 1024; ++a) {
        const uint32_t *pm = perm ? perm + a * 1024 : nullptr;
        const uint64_t srow = pm ? (uint64_t)hoist_src_row(pm[0]) * 1024 : a * 1024;
        for (int e = 0; e < 1024; ++e) {
            const uint64_t v = src[srow + (pm ? hoist_src_elem(pm[e]) : (uint32_t)e)];
            uint64_t &o = acc[a * 1024 + e];
            o = hoist_acc_term(first ? 0 : o, v, plain[a * 1024 + e], m);
        }
    }
}
uint64_t sim_hoist_row_pass_fix(uint64_t q) { return hoist_row_pass_fix(q); }
// what the special-prime wave does to a value the forward row pass returned: times fix
void sim_hoist_sp_unscale(uint64_t n, uint64_t q, uint64_t fix, const uint64_t *in, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    for (uint64_t e = 0; e < n; ++e) out[e] = hoist_sp_unscale(in[e], fix, m);
}
// k_plain_extend on n coefficients under q0: centred into (-q0 / 2, q0 / 2] and reduced mod q
void sim_hoist_centred_mod(uint64_t n, uint64_t q0, uint64_t q, const uint64_t *c, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    for (uint64_t e = 0; e < n; ++e) out[e] = hoist_centred_mod(c[e], q0, q0 >> 1, m);
}

} // extern "C"
